"""Hotword biasing without a GPU: the specification's own properties (tests/hotword_oracle.py), the library's tables and scores
(speecht_amd/hotwords.py) against it, the biased restatement of the searches against the unbiased one, the cases and margins of the
GPU comparison (tests/test_gpu_hotwords.py) on the oracle alone, and the exports and the CLI surface."""
import functools
import os

import numpy as np
import pytest

from tests import hotword_oracle as H
from tests import lm_oracle as L
from tests import nbest_oracle as N
from tests import test_nbest_cpu as C

ROOT = C.ROOT
TINY = C.TINY
ids = L.words_to_ids


# ---- the scan -------------------------------------------------------------------------------------------------------------------

def random_phrases(rng, letters=3):
  return [tuple(rng.integers(0, letters, int(rng.integers(1, 6))).tolist()) for _ in range(int(rng.integers(1, 5)))]


def test_scan_properties_on_a_small_alphabet():
  """Final score > 0 iff a phrase occurs in the string; 0 <= score <= w * position at every position; the tables give the string
  scan's score at every position."""
  rng = np.random.default_rng(0)
  hits = 0
  for it in range(3000):
    phrases = random_phrases(rng)
    x = tuple(rng.integers(0, 3, int(rng.integers(0, 14))).tolist())
    w = (1.0, 0.5, 2.5)[it % 3]                                  # exact in float32, so the tables' sums are exact
    during, final = H.scores(phrases, w, x)
    occurs = any(x[i:i + len(p)] == p for p in set(phrases) for i in range(len(x)))
    assert (final > 0) == occurs, (phrases, x, final)
    assert 0 <= final <= w * len(x)
    assert all(0 <= s <= w * (i + 1) for i, s in enumerate(during)), (phrases, x, during)
    assert H.table_scan(H.tables(phrases, w), x) == (during, final), (phrases, x)
    hits += occurs
  assert 300 < hits < 2700


def test_hand_cases():
  s = lambda phrases, text, w=1.0: H.scores(phrases, w, ids(text))
  # nesting: the longer phrase while it lasts, the shorter one when the longer fails or the utterance ends
  assert s(['new', 'new york'], 'new york') == ([1, 2, 3, 4, 5, 6, 7, 8], 8)
  assert s(['new', 'new york'], 'new yorx') == ([1, 2, 3, 4, 5, 6, 7, 3], 3)
  assert s(['new', 'new york'], 'new yo') == ([1, 2, 3, 4, 5, 6], 3)
  # overlap: the first phrase banks at its leaf, the second cannot reuse its characters
  assert s(['abc', 'bcd'], 'abcd') == ([1, 2, 3, 3], 3)
  assert s(['abc', 'bcd'], 'abxbcd') == ([1, 2, 0, 1, 2, 3], 3)
  # a failed match restarts on its own tail: a phrase inside the failed stretch is found
  assert s(['abcd', 'bc'], 'abce') == ([1, 2, 3, 2], 2)
  # self-overlap
  assert s(['aab'], 'aaab') == ([1, 2, 2, 3], 3)
  # leaf banking: back at the root, the phrase can be matched again at once
  assert s(['ab'], 'abab') == ([1, 2, 3, 4], 4)
  # end-of-utterance flush: an open match is forfeited, a completed inner phrase is kept
  assert s(['hello'], 'hell') == ([1, 2, 3, 4], 0)
  assert s(['he', 'hello'], 'hell') == ([1, 2, 3, 4], 2)
  # the weight scales everything; 0 biases nothing
  assert s(['cat'], 'a cat', 0.5) == ([0, 0, 0.5, 1.0, 1.5], 1.5)
  assert s(['cat'], 'a cat', 0.0) == ([0, 0, 0, 0, 0], 0)
  # a label outside the vocabulary neither advances nor breaks a match
  assert H.scores(['ab'], 1.0, [0, 30, 1]) == ([1, 1, 2], 2)


def test_states_are_numbered_breadth_first():
  assert H.states(['ba', 'ab', 'b']) == [(), (0,), (1,), (0, 1), (1, 0)]
  nxt, gain, fin = H.tables(['ba', 'ab', 'b'], 2.0)
  assert nxt.shape == gain.shape == (5, 32) and fin.shape == (5,) and nxt.dtype == np.int32 and gain.dtype == fin.dtype == np.float32
  assert (nxt[:, 28:] == np.arange(5)[:, None]).all() and (gain[:, 28:] == 0).all()
  assert nxt[0, 0] == 1 and nxt[0, 1] == 2 and nxt[1, 1] == 0 and gain[1, 1] == 2.0          # 'ab' banks at its leaf
  assert nxt[2, 0] == 0 and gain[2, 0] == 2.0 and fin[2] == 0.0 and fin[1] == -2.0              # 'b' is kept at the end, 'a' returned


# ---- the library against the oracle -----------------------------------------------------------------------------------------------

def test_library_tables_and_scores_equal_the_oracle():
  from speecht_amd.hotwords import Hotwords
  rng = np.random.default_rng(1)
  sets = [random_phrases(rng) for _ in range(150)]
  sets += [['new', 'new york', 'york'], ['cat', 'cat sat', 'the mat', 'zebra'], ["it's", 'a', 'on the mat', 'on']]
  sets += [[''.join(L.LETTERS[int(c)] if c < 27 else ' ' for c in rng.integers(0, 28, int(rng.integers(1, 9)))) for _ in range(40)]]
  for k, phrases in enumerate(sets):
    w = (1.0, 0.5, 0.7)[k % 3]
    hw = Hotwords([list(p) if not isinstance(p, str) else p for p in phrases], w)
    nxt, gain, fin = H.tables(phrases, w)
    assert hw.n_states == len(nxt)
    assert np.array_equal(hw.next, nxt) and np.array_equal(hw.gain, gain) and np.array_equal(hw.fin, fin), phrases
    assert hw.next.dtype == np.int32 and hw.gain.dtype == np.float32 and hw.fin.dtype == np.float32
    letters = 3 if k < 150 else 28
    for _ in range(5):
      x = rng.integers(0, letters, int(rng.integers(0, 30))).tolist()
      during, final = H.scores(phrases, w, x)
      assert hw.score(x) == pytest.approx((during[-1] if x else 0.0, final), abs=1e-12)
  empty = Hotwords([], 3.0)
  assert empty.n_states == 1 and len(empty) == 0 and not empty.gain.any() and empty.fin.tolist() == [0.0] and empty.score([1, 2]) == (0.0, 0.0)


def test_library_validates_its_phrases():
  from speecht_amd.hotwords import Hotwords, HotwordError, MAX_PHRASES
  hw = Hotwords(['Cat', 'cat', [2, 0, 19], 'the Mat'])
  assert hw.phrases == [tuple(ids('cat')), tuple(ids('the mat'))] and hw.weight == 1.0          # lower-cased, duplicates dropped
  for bad, text in (([''], 'empty'), (['a' * 65], 'too long'), (['café'], 'outside the vocabulary'), ([[1, 28]], '0..27'),
                    ([[]], 'empty'), ('cat', 'list of phrases')):
    with pytest.raises(HotwordError, match=text):
      Hotwords(bad)
  Hotwords(['a' * 64])
  for w in (-1.0, float('nan'), float('inf')):
    with pytest.raises(HotwordError, match='weight'):
      Hotwords(['cat'], w)
  with pytest.raises(HotwordError, match='at most {}'.format(MAX_PHRASES)):
    Hotwords([[i % 28, (i // 28) % 28, i // 784, 1] for i in range(MAX_PHRASES + 1)])
  assert issubclass(HotwordError, ValueError)
  doc = ' '.join(Hotwords.__doc__.split())
  assert 'is a guess' in doc and 'nobody has tuned it' in doc and 'log10' in doc


# ---- the biased restatement of the searches against the unbiased one ----------------------------------------------------------------

@pytest.mark.parametrize('order', [None, 3])
@pytest.mark.parametrize('transform', C.TRANSFORMS)
def test_without_phrases_or_weight_the_oracle_is_the_unbiased_one(order, transform):
  lm = C.oracle_model(order) if order else None
  logits, lens = C.small_case(11)
  for beam in (4, 16):
    want = N.final_sets(logits, lens, beam, input_transform=transform, lm=lm)
    assert H.final_sets(logits, lens, beam, input_transform=transform, lm=lm) == want
    assert H.final_sets(logits, lens, beam, input_transform=transform, lm=lm, hotwords=['on', 'the mat'], hotword_weight=0.0) == want
    assert H.final_sets(logits, lens, beam, input_transform=transform, lm=lm, dtype=np.float32) == \
        N.final_sets(logits, lens, beam, input_transform=transform, lm=lm, dtype=np.float32)


@pytest.mark.parametrize('order', [None, 1, 3, 5])
def test_every_final_total_splits_into_acoustic_lm_and_bias(order):
  lm = C.oracle_model(order) if order else None
  lw, wc, vwc = 1.5, -0.5, 1.0
  phrases, w = ['on', 'on the', 'mat', 'zz'], 1.3
  logits, lens = C.small_case(7 + (order or 0))
  sets = H.final_sets(logits, lens, 16, lm=lm, lm_weight=lw, word_count_weight=wc, valid_word_count_weight=vwc, hotwords=phrases,
                      hotword_weight=w)
  plain = N.final_sets(logits, lens, 16, lm=lm, lm_weight=lw, word_count_weight=wc, valid_word_count_weight=vwc)
  seen = biased = 0
  for entries in sets:
    assert [t for _, t, _ in entries] == sorted((t for _, t, _ in entries), reverse=True)
    for pre, total, acoustic in entries:
      bias = H.scores(phrases, w, pre)[1]
      lm_part = 0.0
      if lm is not None:
        g, nw, nv = N.sentence_score(lm, pre)
        lm_part = lw * (g + wc * nw + vwc * nv)
      assert total == pytest.approx(acoustic + lm_part + bias, abs=1e-9)
      seen, biased = seen + 1, biased + (bias > 0)
  assert seen >= 33 and biased >= 5
  assert [e[0][0] for e in sets] != [e[0][0] for e in plain] or [e[0][1] for e in sets] != [e[0][1] for e in plain]


# ---- the cases of the GPU comparison and their margins, on the oracle alone --------------------------------------------------------

# a nested pair with a space in it ('cat', 'cat sat'), phrases that occur in the sentence row ('the cat sat on the mat') and ones
# that never do ('zebra', 'quiz'); a one-letter phrase banks at every occurrence
PHRASE_SETS = {'cat': ['cat', 'cat sat', 'the mat', 'zebra'], 'on': ['on', 'on the mat', "it's", 'a', 'quiz']}
# beams 4, 16, 32, 64 and 65..128: the five (candidates per lane, entries) shapes of the kernel -- 4, 8, 16, 32 per lane, and wide
# (beam, input transform, phrase set, weight) of the LM-free lists, (beam, ARPA order, input transform, phrase set, weight) of the LM lists
FREE_CASES = [(4, None, 'cat', 1.0), (16, 'log10_softmax', 'on', 0.7), (32, None, 'on', 1.0), (64, 'log10_softmax', 'cat', 1.0),
              (65, None, 'cat', 0.7), (100, 'log10_softmax', 'on', 1.0), (128, None, 'on', 2.0)]
LM_CASES = [(4, 3, 'log10_softmax', 'on', 1.0), (16, 5, None, 'cat', 1.0), (32, 1, 'log10_softmax', 'cat', 0.7),
            (64, 3, None, 'on', 2.0), (65, 1, 'log10_softmax', 'on', 1.0), (100, 3, 'log10_softmax', 'cat', 1.0), (128, 5, None, 'cat', 0.7)]
ALL_CASES = [('free', c) for c in FREE_CASES] + [('lm', c) for c in LM_CASES]
# seeds: 100 * beam + an offset, 1 unless said here -- picked on the oracle alone, for the two conditions tested below
SEED_OFFSET = {}


def case_seed(kind, case):
  return 100 * case[0] + SEED_OFFSET.get((kind, case), 1)


def case_parts(kind, case):
  """-> (beam, ARPA order or None, input transform, phrases, weight, (logits, lens))."""
  beam, order = case[0], (case[1] if kind == 'lm' else None)
  transform, name, weight = case[-3:]
  return beam, order, transform, PHRASE_SETS[name], weight, C.gpu_case(case_seed(kind, case))


@functools.lru_cache(maxsize=None)
def oracle_sets(kind, case, dtype=np.float64):
  """The oracle's ranked final sets of a GPU case (cached: the lists of every n_best are their heads)."""
  beam, order, transform, phrases, weight, (logits, lens) = case_parts(kind, case)
  lm = C.oracle_model(order) if order else None
  return H.final_sets(logits.astype(np.float64), lens, beam, input_transform=transform, lm=lm, dtype=dtype, hotwords=phrases,
                      hotword_weight=weight)


def test_the_cases_cover_the_kernel_shapes_and_the_phrase_kinds():
  per_lane = lambda beam: -(-beam * 29 // 64)
  shapes = {('wide' if c[0] > 64 else next(s for s in (4, 8, 16, 32) if per_lane(c[0]) <= s)) for _, c in ALL_CASES}
  assert shapes == {4, 8, 16, 32, 'wide'}
  assert {c[0] for _, c in ALL_CASES} >= {4, 16, 64, 65, 100, 128}
  assert {c[1] for c in LM_CASES} == {1, 3, 5} and all({c[-3] for c in cases} == set(C.TRANSFORMS) for cases in (FREE_CASES, LM_CASES))
  sentence = 'the cat sat on the mat'
  for phrases in PHRASE_SETS.values():
    assert any(p in sentence for p in phrases) and any(p not in sentence for p in phrases) and any(' ' in p for p in phrases)
    assert any(a != b and b.startswith(a) for a in phrases for b in phrases)


@pytest.mark.parametrize('kind,case', ALL_CASES)
def test_float32_finds_the_same_sets(kind, case):
  """So that the tie rule of the GPU comparison cannot hide a failure (1): the oracle run in float32 returns the same set of first
  n prefixes as in float64, for every case and n; and the bias is at work in every case."""
  beam = case[0]
  sets64, sets32 = oracle_sets(kind, case), oracle_sets(kind, case, np.float32)
  for n in C.n_bests(beam):
    for e64, e32 in zip(sets64, sets32):
      assert {pre for pre, _, _ in e64[:n]} == {pre for pre, _, _ in e32[:n]}, (n, len(e64))
  assert len(sets64[3]) == 1 and sets64[3][0][0] == () and len(sets64[4]) == min(beam, 29)
  _, _, _, phrases, weight, _ = case_parts(kind, case)
  assert sum(H.scores(phrases, weight, pre)[1] > 0 for entries in sets64 for pre, _, _ in entries) >= 3


def test_near_ties_are_rare():
  """(2): over the committed seeds at most 5 % of the adjacent oracle pairs within the first n + 1 lie within tau."""
  close = pairs = 0
  for kind, case in ALL_CASES:
    for n in C.n_bests(case[0]):
      for entries in oracle_sets(kind, case):
        c, p = N.near_tie_share([t for _, t, _ in entries], n, N.TAU)
        close, pairs = close + c, pairs + p
  assert pairs > 2500 and close <= 0.05 * pairs, (close, pairs)


# ---- exports, Python layers, command line ---------------------------------------------------------------------------------------

def test_entry_points_are_exported():
  from speecht_amd import _lib
  lib = _lib.load()
  for name in ('st_ctc_beam_search_decode_bias_nbest', 'st_ctc_beam_search_decode_lm_bias_nbest'):
    assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
  with open(os.path.join(ROOT, 'include', 'speecht_hip.h')) as f:
    header = ' '.join(f.read().split())
  assert 'typedef struct st_bias_tables' in header and 'int st_ctc_beam_search_decode_bias_nbest(' in header
  assert 'int st_ctc_beam_search_decode_lm_bias_nbest(' in header and 'a malformed table gives wrong text' in header


def test_components_split_the_bias_off():
  from speecht_amd import nbest
  from speecht_amd.hotwords import Hotwords
  hw = Hotwords(['cat'], 2.0)
  lists = nbest.components(None, None, [[(ids('a cat'), -1.0), (ids('a cab'), -2.0)], [([], 0.0)]], hotwords=hw)
  assert [h['bias'] for h in lists[0]] == [6.0, 0.0] and [h['acoustic'] for h in lists[0]] == [-7.0, -2.0] and lists[1][0]['bias'] == 0.0

  class Engine:
    def lm_score_prefixes(self, lm, prefixes):
      n = len(prefixes)
      return np.array([-float(len(p)) for p in prefixes]), np.ones(n, np.int32), np.zeros(n, np.int32)

  first = nbest.components(Engine(), object(), [[(ids('cat'), -5.0)]], (2.0, 0.5, 9.0), hotwords=hw)
  assert first[0][0]['acoustic'] == -5.0 - 2.0 * (-3.0 + 0.5) - 6.0 and first[0][0]['bias'] == 6.0
  assert 'bias' not in nbest.components(None, None, [[([1], -1.0)]])[0][0]


def test_command_line_surface(capsys, tmp_path):
  from speecht_amd import hotwords
  cli = C._cli()
  words = tmp_path / 'words.txt'
  words.write_text('# names\nNew York\n\nzebra\nnew york\n')
  _, flags = cli.parse(['transcribe', 'a.flac', '--hotwords', str(words), '--hotword', 'Cat Sat', '--hotword', 'mat', '--hotword-weight', '2.5'])
  assert flags.hotwords == str(words) and flags.hotword == ['Cat Sat', 'mat'] and flags.hotword_weight == 2.5
  hw = hotwords.from_flags(flags)
  assert hw.phrases == [tuple(ids(p)) for p in ('new york', 'zebra', 'cat sat', 'mat')] and hw.weight == 2.5
  _, plain = cli.parse(['transcribe', 'a.flac'])
  assert not hasattr(plain, 'hotwords') and not hasattr(plain, 'hotword') and not hasattr(plain, 'hotword_weight')
  assert hotwords.from_flags(plain) is None

  def refused(args, text):
    with pytest.raises(SystemExit) as e:
      cli.main(['transcribe', 'a.flac'] + args)
    assert e.value.code == 2
    assert text in capsys.readouterr().err

  refused(['--hotword-weight', '2.0'], '--hotword-weight applies with --hotwords or --hotword only')
  refused(['--hotword', 'cat', '--hotword-weight', '-1'], 'hotword weight must be finite and >= 0')
  refused(['--hotword', 'café'], 'outside the vocabulary')
  refused(['--hotword', ''], 'hotword is empty')
  refused(['--hotwords', str(tmp_path / 'missing.txt')], 'cannot read')
  with pytest.raises(SystemExit):
    cli.parse(['transcribe', '--help'])
  text = ' '.join(capsys.readouterr().out.split())
  assert '--hotwords FILE' in text and '--hotword TEXT' in text and '--hotword-weight X' in text and 'nobody has tuned it' in text


def test_transcribe_checks_its_hotwords_before_it_runs():
  from speecht_amd import inference
  from speecht_amd.hotwords import HotwordError
  with pytest.raises(HotwordError, match='outside the vocabulary'):
    inference.transcribe(None, [np.zeros((4, 2))], hotwords=['café'])

  class Engine:
    forward = None

  assert inference.transcribe(Engine(), [], hotwords=['cat']) == ([], [])                    # the lists only when asked for
  assert inference.transcribe(Engine(), [], hotwords=['cat'], nbest=2) == ([], [], [])
