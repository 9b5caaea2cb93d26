"""Word times and confidences for the finals of live streams, the parts that need no GPU: the C ABI's new symbols against the
header's prototypes, st_stream_keep_rows, what `FinalWords` and `StreamingRecognizer` refuse before anything is allocated, and the
pure-Python job table of a pass's finals (`streaming.final_jobs`) against hand-written finals."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('st_stream_keep_rows', 'st_stream_keep_f32', 'st_ctc_align_ring_f32', 'st_ctc_align_ring_host', 'st_ctc_word_conf_ring_f32',
         'st_ctc_word_conf_ring_host')


def test_abi_symbols_and_prototypes():
  from speecht_amd import _lib
  lib = _lib.load()
  header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'speecht_hip.h')).read(), flags=re.S)
  for name in NAMES:
    m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', header)
    assert m and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    params = [p.strip() for p in m.group(1).split(',')]
    restype, argtypes = _lib._SIGNATURES[name]
    assert len(params) == len(argtypes), (name, params)
    for p, a in zip(params, argtypes):                              # pointers are pointers, ints are ints, sizes are sizes
      kind = 'ptr' if '*' in p else ('size' if p.startswith('size_t') else 'int')
      assert {'c_void_p': 'ptr', 'c_int': 'int', 'c_ulong': 'size', 'c_size_t': 'size'}[a.__name__] == kind, (name, p, a)
  # a device entry point and its host form take the same arguments but the stream
  for dev, host in (('st_ctc_align_ring_f32', 'st_ctc_align_ring_host'), ('st_ctc_word_conf_ring_f32', 'st_ctc_word_conf_ring_host')):
    assert _lib._SIGNATURES[dev][1][:-1] == _lib._SIGNATURES[host][1]
  text = ' '.join(open(os.path.join(ROOT, 'include', 'speecht_hip.h')).read().split())
  assert 'below u0 + M + max_rows - 1 = u0 + cap - 1' in text         # the header argues why M + max_rows rows suffice


def test_keep_rows():
  from speecht_amd import _lib
  lib = _lib.load()
  assert lib.st_stream_keep_rows(9, 10) == 19 and lib.st_stream_keep_rows(1500, 24) == 1524 and lib.st_stream_keep_rows(1, 1) == 2
  for bad in ((0, 4), (4, 0), (-3, 4), (4, -1), (2 ** 31 - 1, 1)):
    assert lib.st_stream_keep_rows(*bad) == 0, bad


class _FakeEngine:
  """What `StreamingRecognizer` looks at before it allocates: the layer list and the class count."""

  class _Layer:
    def __init__(self, width, stride):
      self.width, self.stride = width, stride

  def __init__(self, num_classes):
    self.layers = [self._Layer(48, 2), self._Layer(7, 1)]
    self.num_classes, self.device = num_classes, 'cpu'


def test_refusals_before_anything_is_allocated():
  from speecht_amd.streaming import Endpointing, FinalWords, StreamError, StreamingRecognizer
  with pytest.raises(StreamError, match='neither'):
    FinalWords(timestamps=False, confidence=False)
  w = FinalWords()
  assert w.timestamps and not w.confidence
  with pytest.raises(StreamError, match='endpoint'):
    StreamingRecognizer(_FakeEngine(29), 2, words=FinalWords())
  with pytest.raises(StreamError, match='FinalWords'):
    StreamingRecognizer(_FakeEngine(29), 2, endpoint=Endpointing(), words=True)
  with pytest.raises(StreamError, match='space class'):            # 12 classes: 'auto' names no space
    StreamingRecognizer(_FakeEngine(12), 2, endpoint=Endpointing(), words=FinalWords(confidence=True))
  with pytest.raises(StreamError, match='space class'):
    StreamingRecognizer(_FakeEngine(29), 2, endpoint=Endpointing(space_id=-1), words=FinalWords(confidence=True))
  with pytest.raises(StreamError, match='at most 30 classes'):
    StreamingRecognizer(_FakeEngine(31), 2, endpoint=Endpointing(space_id=27), words=FinalWords(confidence=True))
  with pytest.raises(StreamError, match='2..32 classes'):
    StreamingRecognizer(_FakeEngine(40), 2, endpoint=Endpointing(), words=FinalWords())
  with pytest.raises(StreamError, match="vocabulary's space"):
    StreamingRecognizer(_FakeEngine(29), 2, endpoint=Endpointing(space_id=3), words=FinalWords(confidence=True))
  # what is served passes the check
  FinalWords(confidence=True).check(Endpointing(), 29, 27)
  FinalWords().check(Endpointing(), 32, -1)


def test_the_job_table_of_hand_written_finals():
  from speecht_amd.streaming import final_jobs
  sp = 27
  finals = [(2, 10, 25, [7, 4, sp, sp, 11, 14]),         # two words, a double space
            (0, 0, 9, []),                               # an empty final: no job
            (2, 31, 40, [sp, 0, sp]),                    # the same stream again; leading and trailing spaces
            (1, 100, 700, list(range(20)) * 26),         # 520 ids: too long, no job
            (3, 5, 6, [sp])]                             # only a space: a job without words
  t = final_jobs(finals, sp, 511)
  assert t['index'] == [0, 2, 4]
  assert t['jobs'].dtype == np.int32 and t['jobs'].tolist() == [[2, 10, 15], [2, 31, 9], [3, 5, 1]]
  assert t['ids'].dtype == np.int32 and t['ids'].tolist() == [7, 4, sp, sp, 11, 14, sp, 0, sp, sp]
  assert t['offsets'].dtype == np.int32 and t['offsets'].tolist() == [0, 6, 9, 10]
  assert t['word_spans'].dtype == np.int32 and t['word_spans'].tolist() == [[0, 0, 2], [0, 4, 6], [1, 1, 2]]
  assert t['words'] == [2, 1, 0] and t['max_len'] == 6 and t['max_rows'] == 15
  # without a space class (timestamps alone): the same jobs, no word spans
  t = final_jobs(finals, None, 511)
  assert t['index'] == [0, 2, 4] and t['word_spans'].shape == (0, 3) and t['words'] == [0, 0, 0]
  # the limit is the caller's: 511 ids are a job, 512 are not
  t = final_jobs([(0, 0, 600, [1] * 511), (0, 600, 1200, [1] * 512)], sp, 511)
  assert t['index'] == [0] and t['max_len'] == 511 and t['max_rows'] == 600
  # nothing to do
  t = final_jobs([(0, 0, 9, [])], sp, 511)
  assert t['index'] == [] and t['jobs'].shape == (0, 3) and t['offsets'].tolist() == [0] and t['max_rows'] == 0
