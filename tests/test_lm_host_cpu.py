"""The ARPA tables of the LM-scored beam search through the real library, without a GPU: every listed n-gram and random
unseen tuples against the Python backoff restatement (tests/lm_oracle.py), the character trie, the counts and the format
errors; and what `LanguageModel.load` refuses."""
import gzip
import os

import numpy as np
import pytest

from tests import lm_oracle as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, 'tests', 'golden', 'lm_tiny.arpa')


def _load(path):
  from speecht_amd.language_model import LanguageModel
  return LanguageModel.load(path)


def _check_queries(lm, ref, rng, n_random):
  words = sorted(w[0] for w in ref.prob if len(w) == 1)
  for gram in ref.prob:
    ctx, w = gram[:-1], gram[-1]
    assert abs(lm.logp(ctx, w) - ref.logp(ctx, w)) <= 1e-6 * max(1.0, abs(ref.logp(ctx, w))), gram
  for _ in range(n_random):
    n = int(rng.integers(0, ref.order))
    gram = tuple(words[int(i)] for i in rng.integers(0, len(words), n + 1))
    ctx, w = gram[:-1], gram[-1]
    assert abs(lm.logp(ctx, w) - ref.logp(ctx, w)) <= 1e-6 * max(1.0, abs(ref.logp(ctx, w))), gram


def test_tiny_model_queries_match_the_backoff_restatement():
  lm = _load(TINY)
  ref = L.ArpaModel.load(TINY)
  _check_queries(lm, ref, np.random.default_rng(0), 10000)
  # backoff by hand: "a dog" is not listed -> bo(a) + p(dog)
  assert lm.logp(['a'], 'dog') == pytest.approx(-0.2218 - 2.0, abs=1e-6)
  # trigram listed; unseen trigram backs off through the bigram's backoff
  assert lm.logp(['on', 'the'], 'mat') == pytest.approx(-0.3010, abs=1e-6)
  assert lm.logp(['sat', 'on'], 'dog') == pytest.approx(0.0 + -0.2000 + -2.0, abs=1e-6)
  # unknown words are <unk>, uppercase words are lowercased
  assert lm.logp([], 'zebra') == pytest.approx(-2.5, abs=1e-6)
  assert lm.word_id('HELLO') == lm.word_id('hello') != 0


def test_random_5gram_queries_match_the_backoff_restatement(tmp_path):
  text = L.random_arpa(5, 400, [3000, 3000, 2000, 1000], extra_words=['x1', 'Big'])
  path = tmp_path / 'r5.arpa.gz'
  with gzip.open(str(path), 'wt') as f:
    f.write(text)
  lm = _load(str(path))
  ref = L.ArpaModel(text)
  assert lm.info['order'] == 5 and lm.info['ngrams'] == [405, 3000, 3000, 2000, 1000]
  assert lm.info['skipped_words'] == 1                     # x1 (Big is lowercased and spelled in [a-z'])
  _check_queries(lm, ref, np.random.default_rng(1), 10000)


def test_trie_lowest_unigrams_and_terminal_words():
  lm = _load(TINY)
  ref = L.ArpaModel.load(TINY)
  assert lm.info['order'] == 3 and lm.info['ngrams'] == [22, 14, 6] and lm.info['words'] == 22
  assert lm.info['skipped_words'] == 1                     # b4
  for prefix, m in ref.min_prefix.items():
    node, got, word = lm.trie_lookup(prefix)
    assert node > 0 and got == np.float32(m), prefix
    assert (word >= 0) == (prefix in ref.vocab), prefix
    if word >= 0:
      assert word == lm.word_id(prefix)
  assert lm.trie_lookup('ca')[1] == np.float32(-2.8539)    # cat -1.9031, cab -2.8539: the lowest
  assert lm.trie_lookup("it'")[1] == np.float32(-2.2218) and lm.trie_lookup("it's")[2] == lm.word_id("it's")
  assert lm.trie_lookup('b4')[0] == -1 and lm.trie_lookup('b')[0] == -1
  assert lm.trie_lookup('kat')[0] == -1 and lm.trie_lookup('hello')[2] == lm.word_id('hello')


def _create(text):
  import ctypes
  from speecht_amd import _lib
  lib = _lib.load()
  h = ctypes.c_void_p()
  err = ctypes.create_string_buffer(256)
  data = text.encode()
  rc = lib.st_lm_create_arpa(data, len(data), ctypes.byref(h), err, 256)
  if rc == 0:
    lib.st_lm_destroy(h)
  return rc, err.value.decode()


def test_format_errors_name_the_line():
  text = open(TINY).read()
  assert _create(text) == (0, '')
  cut = text.index('\\3-grams:')
  rc, msg = _create(text[:cut] + '\\3-grams:\n-0.1549\t<s> the cat\n')   # truncated after a line
  assert rc != 0 and msg.startswith('ARPA line ') and 'ends' in msg, msg
  rc, msg = _create(text[:cut + 20])                                     # truncated inside a line
  assert rc != 0 and msg.startswith('ARPA line 49:'), msg
  rc, msg = _create(text.replace('ngram 2=14', 'ngram 2=15'))           # miscounted
  assert rc != 0 and '14 2-grams listed, \\data\\ says 15' in msg and msg.startswith('ARPA line 48:'), msg
  rc, msg = _create(text.replace('ngram 2=14', 'ngram 2=13'))
  assert rc != 0 and 'more 2-grams' in msg, msg
  rc, msg = _create(text.replace('-0.6021\ta cat', '-0.6021\ta zebra'))
  assert rc != 0 and 'missing from the unigrams' in msg, msg
  rc, msg = _create('no model here\n')
  assert rc != 0 and 'data' in msg


def test_data_block_may_run_straight_into_the_first_section():
  text = open(TINY).read()
  tight = text.replace('ngram 3=6\n\n\\1-grams:', 'ngram 3=6\n\\1-grams:')
  assert tight != text
  assert _create(tight) == (0, '')


def test_a_file_saved_again_replaces_its_cached_model(tmp_path):
  from speecht_amd.language_model import LanguageModel
  path = tmp_path / 'm.arpa'
  path.write_text(open(TINY).read())
  first = LanguageModel.load(str(path))
  assert LanguageModel.load(str(path)) is first
  st = os.stat(str(path))
  os.utime(str(path), ns=(st.st_atime_ns, st.st_mtime_ns + 10 ** 9))
  second = LanguageModel.load(str(path))
  assert second is not first and LanguageModel._cache[os.path.abspath(str(path))][1] is second   # the old entry is gone


def test_kenlm_binary_directory_is_refused(tmp_path):
  from speecht_amd.language_model import UnsupportedLanguageModel
  d = tmp_path / 'kenlm-english'
  d.mkdir()
  (d / 'lm.binary').write_bytes(b'mmap lm http://kheafield.com/code format version 5\x00' + bytes(64))
  (d / 'trie').write_bytes(bytes(64))
  with pytest.raises(UnsupportedLanguageModel, match='ARPA'):
    _load(str(d))
  with pytest.raises(NotImplementedError):
    _load(str(d / 'lm.binary'))
  with pytest.raises(NotImplementedError):
    _load(str(tmp_path / 'missing.arpa'))
