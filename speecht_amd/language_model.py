"""Word n-gram language models for the LM-scored CTC beam search (the reference's `--language-model` decoder,
speech_model.py:84-111).  The model comes from an ARPA file -- the text form every n-gram toolkit writes, KenLM's `lmplz`
included -- parsed by the library into device tables (csrc/lm_tables.h); KenLM's binary format is not read."""
import ctypes
import gzip
import os
import threading

from . import _lib


class UnsupportedLanguageModel(NotImplementedError):
  """The path holds no ARPA model (e.g. a KenLM binary directory with lm.binary / trie)."""


def _find_arpa(path):
  path = os.fspath(path)
  expected = ('expected an ARPA n-gram model: a .arpa or .arpa.gz file, or a directory holding exactly one '
              '(KenLM binary models are not read; `build_binary` has an ARPA source, or write one with `lmplz`)')
  if os.path.isdir(path):
    found = sorted(f for f in os.listdir(path) if f.endswith('.arpa') or f.endswith('.arpa.gz'))
    if len(found) != 1:
      raise UnsupportedLanguageModel('{}: {} ARPA files found; {}'.format(path, len(found), expected))
    return os.path.join(path, found[0])
  if os.path.isfile(path) and (path.endswith('.arpa') or path.endswith('.arpa.gz')):
    return path
  raise UnsupportedLanguageModel('{}: {}'.format(path, expected))


class LanguageModel:
  """An ARPA model parsed into host tables; `device_handle(device)` uploads them (once per device) for the decoder."""

  _cache = {}
  _lock = threading.Lock()

  def __init__(self, path):
    self.path = path
    opener = gzip.open if path.endswith('.gz') else open
    with opener(path, 'rb') as f:
      text = f.read()
    lib = _lib.load()
    handle = ctypes.c_void_p()
    err = ctypes.create_string_buffer(512)
    if lib.st_lm_create_arpa(text, len(text), ctypes.byref(handle), err, len(err)) != 0:
      raise ValueError('{}: {}'.format(path, err.value.decode()))
    self._handle = handle
    self._devices = set()
    order = ctypes.c_int()
    counts = (ctypes.c_int64 * 6)()
    skipped, nodes, dev_bytes = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_size_t()
    _lib.check(lib.st_lm_info(handle, ctypes.byref(order), counts, ctypes.byref(skipped), ctypes.byref(nodes),
                              ctypes.byref(dev_bytes)), 'st_lm_info')
    self.info = dict(order=order.value, words=counts[0], ngrams=[counts[n] for n in range(1, order.value + 1)],
                     skipped_words=skipped.value, trie_nodes=nodes.value, device_bytes=dev_bytes.value)
    self.order = order.value

  @classmethod
  def load(cls, path):
    """The model at `path` (a .arpa / .arpa.gz file or a directory holding one), cached per file; a file saved again since it
    was loaded (another mtime) is loaded anew and the old tables are let go."""
    arpa = os.path.abspath(_find_arpa(path))
    mtime = os.stat(arpa).st_mtime_ns
    with cls._lock:
      cached = cls._cache.get(arpa)
      if cached is None or cached[0] != mtime:
        cls._cache.pop(arpa, None)                    # (freed once no engine or caller holds the old model)
        cached = (mtime, cls(arpa))
        cls._cache[arpa] = cached
      return cached[1]

  def device_handle(self, device=None):
    """The library handle with the tables on `device` (default: the current CUDA device), uploaded there on first use.  The
    decoder reads the copy on the device its stream belongs to."""
    import torch
    device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    index = device.index if device.index is not None else torch.cuda.current_device()
    if index not in self._devices:
      with torch.cuda.device(index):
        stream = torch.cuda.current_stream(index)
        _lib.call('st_lm_upload', self._handle, ctypes.c_void_p(stream.cuda_stream))
      self._devices.add(index)
    return self._handle

  def word_id(self, word):
    i = ctypes.c_int32()
    _lib.call('st_lm_word_id', self._handle, word.encode(), ctypes.byref(i))
    return i.value

  def logp(self, context, word):
    """log10 p(word | context words) with ARPA backoff, through the library's own tables."""
    ids = [self.word_id(w) for w in context]
    ctx = (ctypes.c_int32 * max(len(ids), 1))(*ids)
    out = ctypes.c_float()
    _lib.call('st_lm_query_host', self._handle, ctx, len(ids), self.word_id(word), ctypes.byref(out))
    return out.value

  def score(self, words, bos=True, eos=True):
    """log10 probability of a word sequence (sentence-start context and end token by default)."""
    ctx = ['<s>'] if bos else []
    total = 0.0
    for w in list(words) + (['</s>'] if eos else []):
      total += self.logp(ctx[-(self.order - 1):] if self.order > 1 else [], w)
      ctx.append(w)
    return total

  def trie_lookup(self, prefix):
    """(node or -1, lowest unigram log10 p of the completions, terminal word id or -1) of a letter prefix."""
    node, m, word = ctypes.c_int32(), ctypes.c_float(), ctypes.c_int32()
    _lib.call('st_lm_trie_lookup', self._handle, prefix.encode(), ctypes.byref(node), ctypes.byref(m), ctypes.byref(word))
    return node.value, m.value, word.value

  def __del__(self):
    h = getattr(self, '_handle', None)
    if h is not None and _lib._lib is not None:
      _lib._lib.st_lm_destroy(h)
      self._handle = None
