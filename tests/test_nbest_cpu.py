"""N-best lists and second-pass rescoring without a GPU: the float64 specification (tests/nbest_oracle.py) pinned to the two
top-path oracles and to its own score decomposition, the host form of the sentence scores (st_lm_score_prefixes_host) against it,
the margins of the GPU comparison (tests/test_gpu_nbest.py) on the oracle alone, and the exports and the CLI surface."""
import ctypes
import functools
import importlib.machinery
import importlib.util
import os

import numpy as np
import pytest

from oracle import w2l_oracle as O
from tests import lm_oracle as L
from tests import nbest_oracle as N
from tests.test_lm_oracle_cpu import word_logits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, 'tests', 'golden', 'lm_tiny.arpa')
SENTENCE_WORDS = ['the', 'cat', 'sat', 'on', 'mat', 'dog', 'a', "it's"]
TRANSFORMS = (None, 'log10_softmax')


@functools.lru_cache(maxsize=None)
def arpa_text(order, seed=None):
  """order 3: the hand-written model; others: a seeded random model whose vocabulary holds the sentence words."""
  if order == 3 and seed is None:
    with open(TINY) as f:
      return f.read()
  return L.random_arpa(100 + order if seed is None else seed, 150, [400, 300, 200, 100][:order - 1], extra_words=SENTENCE_WORDS)


@functools.lru_cache(maxsize=None)
def oracle_model(order, seed=None):
  return L.ArpaModel(arpa_text(order, seed))


# ---- the new oracle against the two it restates ------------------------------------------------------------------------------

def small_case(seed, C=29):
  rng = np.random.default_rng(seed)
  T, B = 24, 3
  logits = rng.standard_normal((T, B, C)) * 2.0
  if C == 29:
    w = word_logits('on the mat', rng, frames_per_char=2, gap=0)
    logits[:len(w), 1] = w[:T]
  return logits, [T, min(20, T), 0]


@pytest.mark.parametrize('beam', [1, 4, 16, 100])
@pytest.mark.parametrize('transform', TRANSFORMS)
def test_first_hypothesis_is_the_lm_free_top_path(beam, transform):
  logits, lens = small_case(beam)
  ids, score = O.ctc_beam_search_decode(logits, lens, beam, input_transform=transform)
  lists = N.nbest(logits, lens, beam, beam, input_transform=transform)
  assert [l[0][0] for l in lists] == ids
  assert np.array_equal(np.array([[l[0][1]] for l in lists]), score)
  assert len(lists[2]) == 1 and lists[2][0] == ([], 0.0)
  assert all(len(l) <= beam for l in lists) and len(lists[0]) == beam
  for l in lists:
    s = [v for _, v in l]
    assert s == sorted(s, reverse=True) and len({tuple(i) for i, _ in l}) == len(l)


@pytest.mark.parametrize('beam', [1, 4, 16, 100])
@pytest.mark.parametrize('order', [1, 2, 3, 4, 5])
def test_first_hypothesis_is_the_lm_top_path(beam, order):
  lm = oracle_model(order)
  transform = TRANSFORMS[(beam + order) % 2]
  logits, lens = small_case(10 * beam + order)
  ids, score = L.lm_beam_search_decode(logits, lens, lm, beam, transform)
  lists = N.nbest(logits, lens, beam, beam, input_transform=transform, lm=lm)
  assert [l[0][0] for l in lists] == ids
  assert np.array_equal(np.array([[l[0][1]] for l in lists]), score)
  for l in lists:
    s = [v for _, v in l]
    assert s == sorted(s, reverse=True)


@pytest.mark.parametrize('weights', [(0.8, 0.0, 2.3), (1.5, -0.5, 1.0), (-0.4, 1.0, -1.0)])
@pytest.mark.parametrize('order', [1, 3, 5])
def test_every_final_total_splits_into_acoustic_and_sentence_parts(weights, order):
  lm = oracle_model(order)
  lw, wc, vwc = weights
  logits, lens = small_case(7 + order)
  seen = 0
  for entries in N.final_sets(logits, lens, 16, lm=lm, lm_weight=lw, word_count_weight=wc, valid_word_count_weight=vwc):
    sc = L.Scorer(lm, 0.0, 0.0)
    for pre, total, acoustic in entries:
      g, nw, nv = N.sentence_score(lm, pre)
      assert g == pytest.approx(sc.state(pre)[3] + sc.end_delta(pre), rel=1e-12, abs=1e-12)     # the definition: Scorer(lm, 0, 0)
      assert total == pytest.approx(acoustic + lw * (g + wc * nw + vwc * nv), abs=1e-9)
      seen += 1
  assert seen >= 33


# ---- the host form of the sentence scores -------------------------------------------------------------------------------------

def hand_made_prefixes(rng):
  ids = L.words_to_ids
  long = []
  while len(long) < 1500:
    long += ids(SENTENCE_WORDS[int(rng.integers(len(SENTENCE_WORDS)))]) + [L.SPACE]
  return [[], ids(' the cat'), ids('the  cat'), ids('the cat '), ids('the zzgx sat'), ids("it's a cat"), ids("'"), [L.SPACE],
          [L.SPACE, L.SPACE], ids('the cat sat on the mat'), ids('a'), ids('th'), long[:1500]]


def library_model(tmp_path_factory, order, seed=None):
  from speecht_amd.language_model import LanguageModel
  if order == 3 and seed is None:
    return LanguageModel.load(TINY)
  path = os.path.join(str(tmp_path_factory.getbasetemp()), 'nbest_r{}_{}.arpa'.format(order, seed))
  if not os.path.exists(path):
    with open(path, 'w') as f:
      f.write(arpa_text(order, seed))
  return LanguageModel.load(path)


def score_host(lm, prefixes, pitch=None):
  """st_lm_score_prefixes_host on a list of id lists -> (G, n_words, n_valid)."""
  from speecht_amd import _lib
  n = len(prefixes)
  lens = np.array([len(p) for p in prefixes], dtype=np.int32)
  pitch = pitch or max(int(lens.max()) if n else 1, 1)
  ids = np.zeros((max(n, 1), pitch), dtype=np.int32)
  for i, p in enumerate(prefixes):
    ids[i, :len(p)] = p
  g, nw, nv = np.full(n, 7.0), np.full(n, -7, np.int32), np.full(n, -7, np.int32)
  ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
  _lib.call('st_lm_score_prefixes_host', lm._handle, ptr(ids), pitch, ptr(lens), n, ptr(g), ptr(nw), ptr(nv))
  return g, nw, nv


@pytest.mark.parametrize('order', [1, 2, 3, 4, 5])
def test_host_sentence_scores_equal_the_oracle(tmp_path_factory, order):
  lm, ref = library_model(tmp_path_factory, order), oracle_model(order)
  prefixes = hand_made_prefixes(np.random.default_rng(order))
  g, nw, nv = score_host(lm, prefixes, pitch=1600)
  for i, p in enumerate(prefixes):
    rg, rw, rv = N.sentence_score(ref, p)
    assert (nw[i], nv[i]) == (rw, rv), (i, L.ids_to_text(p)[:40])
    assert g[i] == pytest.approx(rg, rel=1e-12), (i, L.ids_to_text(p)[:40])
  assert nw[0] == 0 and nw[1] == 3 and nv[1] == 2 and nw[2] == 3 and nw[3] == 2 and nw[7] == 1 and nw[8] == 2 and nv[8] == 0
  assert nw[4] == 3 and nv[4] == 2 and nw[12] >= 250


def test_host_sentence_scores_refuse_bad_input(tmp_path_factory):
  from speecht_amd import _lib
  lm = library_model(tmp_path_factory, 3)
  g, nw, nv = score_host(lm, [])
  assert len(g) == 0
  for bad in ([0, 28, 1], [-1], [1 << 20]):
    with pytest.raises(_lib.SpeechtHipError, match='outside 0..27'):
      score_host(lm, [[1, 2], bad])


# ---- the margins of the GPU comparison, on the oracle alone --------------------------------------------------------------------

# beams 4, 16, 64, 65, 100, 128: 64 and 65 straddle the kernel's wide instantiation
# (beam, classes, input transform) of the LM-free lists and (beam, ARPA order, input transform) of the LM lists the GPU test decodes
FREE_CASES = [(4, 29, None), (16, 29, 'log10_softmax'), (64, 29, None), (65, 29, 'log10_softmax'), (100, 29, None),
              (128, 29, 'log10_softmax'), (16, 5, None), (100, 5, 'log10_softmax'), (16, 32, 'log10_softmax'), (128, 32, None)]
LM_CASES = [(4, 1, 'log10_softmax'), (4, 3, None), (16, 3, 'log10_softmax'), (16, 5, None), (64, 1, None), (64, 5, 'log10_softmax'),
            (65, 3, None), (65, 1, 'log10_softmax'), (100, 3, 'log10_softmax'), (100, 5, None), (128, 1, 'log10_softmax'),
            (128, 5, None)]
# seeds: 100 * beam + an offset in {1, 2, 3}, 1 unless said here -- picked on the oracle alone, for few near ties (the test below)
SEED_OFFSET = {('free', (4, 29, None)): 2, ('free', (128, 29, 'log10_softmax')): 3}


def case_seed(case, kind='free'):
  return 100 * case[0] + SEED_OFFSET.get((kind, case), 1)


def gpu_case(seed, C=29):
  """The shape of the LM search's GPU test: T = 80, B = 5; a random row, a sentence, a row of mostly blanks, lengths 0 and 1."""
  rng = np.random.default_rng(seed)
  T, B = 80, 5
  logits = rng.standard_normal((T, B, C)) * 2.0
  w = word_logits('the cat sat on the mat', rng, frames_per_char=2, gap=1, noise=1.0, peak=3.0)
  if C == 29:
    logits[:len(w), 1] = w
  logits[:, 2, C - 1] += 3.0
  lens = [80, len(w), 77, 0, 1]
  return logits.astype(np.float32), lens


@functools.lru_cache(maxsize=None)
def oracle_sets(kind, case, dtype=np.float64):
  """The oracle's ranked final sets of a GPU case (cached: the lists of every n_best are their heads)."""
  beam, second, transform = case
  logits, lens = gpu_case(case_seed(case, kind), second if kind == 'free' else 29)
  lm = oracle_model(second) if kind == 'lm' else None
  return N.final_sets(logits.astype(np.float64), lens, beam, input_transform=transform, lm=lm, dtype=dtype)


def n_bests(beam):
  return sorted({1, 2, beam})


ALL_CASES = [('free', c) for c in FREE_CASES] + [('lm', c) for c in LM_CASES]


@pytest.mark.parametrize('kind,case', ALL_CASES)
def test_float32_finds_the_same_sets(kind, case):
  """So that the tie rule of the GPU comparison cannot hide a failure (1): the oracle run in float32 returns the same set of first
  n prefixes as in float64, for every case and n."""
  beam = case[0]
  sets64, sets32 = oracle_sets(kind, case), oracle_sets(kind, case, np.float32)
  for n in n_bests(beam):
    for e64, e32 in zip(sets64, sets32):
      assert {pre for pre, _, _ in e64[:n]} == {pre for pre, _, _ in e32[:n]}, (n, len(e64))
  # the entry counts the header promises: the empty prefix alone for no frames; blank + every label after one frame
  assert len(sets64[3]) == 1 and sets64[3][0][0] == ()
  C = case[1] if kind == 'free' else 29
  assert len(sets64[4]) == min(beam, C)


def test_near_ties_are_rare():
  """(2): over the committed seeds at most 5 % of the adjacent oracle pairs within the first n + 1 lie within tau."""
  close = pairs = 0
  for kind, case in ALL_CASES:
    for n in n_bests(case[0]):
      for entries in oracle_sets(kind, case):
        c, p = N.near_tie_share([t for _, t, _ in entries], n, N.TAU)
        close, pairs = close + c, pairs + p
  assert pairs > 4000 and close <= 0.05 * pairs, (close, pairs)


def test_the_comparison_rule_accepts_near_ties_only():
  entries = [((1,), -1.0, -1.0), ((2,), -2.0, -2.0), ((3,), -2.00005, -2.00005), ((4,), -3.0, -3.0)]
  N.check_list([([1], -1.0), ([3], -2.00005), ([2], -2.00006)], entries, 3)              # a near tie, swapped
  N.check_list([([1], -1.0), ([3], -2.0)], entries, 2)                                   # the near tie at the cut
  for wrong in ([([2], -2.0), ([1], -2.0), ([3], -2.0)],                                # a real gap, swapped (scores made to pass (b))
                [([1], -1.0), ([4], -3.0)],                                              # a real gap at the cut
                [([1], -1.0), ([2], -2.0)][:1],                                          # a hypothesis short
                [([1], -1.0), ([5], -2.0)],                                              # not in the final set
                [([1], -1.0), ([2], -2.001)]):                                           # a wrong score
    with pytest.raises(AssertionError):
      N.check_list(wrong, entries, 2 if len(wrong) < 3 else 3)


# ---- exports, Python layers, command line ---------------------------------------------------------------------------------------

def test_entry_points_are_exported():
  from speecht_amd import _lib
  lib = _lib.load()
  for name in ('st_ctc_beam_search_decode_nbest', 'st_ctc_beam_search_decode_lm_nbest', 'st_lm_score_prefixes_f64',
               'st_lm_score_prefixes_host'):
    assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
  with open(os.path.join(ROOT, 'include', 'speecht_hip.h')) as f:
    header = f.read()
  assert 'final total desc, rank in the set asc' in header and 'total desc, candidate key asc' in header


def test_rescore_breaks_ties_by_first_pass_rank():
  from speecht_amd import nbest

  class Engine:                             # G = -(number of ids): the second pass prefers short hypotheses
    def lm_score_prefixes(self, lm, prefixes):
      n = len(prefixes)
      return np.array([-float(len(p)) for p in prefixes]), np.ones(n, np.int32), np.zeros(n, np.int32)

  lists = nbest.components(None, None, [[([1, 2, 3], -1.0), ([1, 2], -2.0), ([4, 5], -2.0), ([6], -2.5)], [([], 0.0)]])
  assert [h['acoustic'] for h in lists[0]] == [-1.0, -2.0, -2.0, -2.5] and 'lm_log10' not in lists[0][0]
  order, scores = nbest.rescore(lists, Engine(), object(), 1.0, 0.5, 9.0)
  assert order == [[3, 0, 1, 2], [0]]                       # -3.0, then the three at -3.5 in first-pass order
  assert scores[0].tolist() == [-3.0, -3.5, -3.5, -3.5] and scores[1].tolist() == [0.5]
  assert nbest.rerank([1.0, 2.0, 2.0, 0.0]) == N.rerank([1.0, 2.0, 2.0, 0.0]) == [1, 2, 0, 3]
  again = nbest.rescored(lists, Engine(), object(), 1.0, 0.5, 9.0)
  assert [h['first_pass_rank'] for h in again[0]] == [3, 0, 1, 2] and again[0][0]['log_prob'] == -3.0 and again[0][0]['acoustic'] == -2.5
  first = nbest.components(Engine(), object(), [[([1, 2], -5.0)]], (2.0, 0.5, 9.0))
  assert first[0][0]['acoustic'] == -5.0 - 2.0 * (-2.0 + 0.5) and first[0][0]['words'] == 1 and first[0][0]['valid_words'] == 0


def _cli():
  loader = importlib.machinery.SourceFileLoader('speecht_cli_nbest', os.path.join(ROOT, 'speecht-cli'))
  spec = importlib.util.spec_from_loader(loader.name, loader)
  module = importlib.util.module_from_spec(spec)
  loader.exec_module(module)
  return module


def test_command_line_surface(capsys):
  cli = _cli()
  _, flags = cli.parse(['transcribe', 'a.flac', '--beam-width', '16', '--nbest', '4', '--rescore-language-model', TINY,
                        '--rescore-lm-weight', '1.5'])
  assert flags.nbest == 4 and flags.rescore_language_model == TINY and flags.rescore_lm_weight == 1.5
  _, plain = cli.parse(['transcribe', 'a.flac'])
  assert not hasattr(plain, 'nbest') and not hasattr(plain, 'rescore_language_model') and not hasattr(plain, 'rescore_lm_weight')

  def refused(args, text):
    with pytest.raises(SystemExit) as e:
      cli.main(['transcribe', 'a.flac'] + args)
    assert e.value.code == 2
    assert text in capsys.readouterr().err

  refused(['--nbest', '4'], '--nbest needs a beam search (--beam-width or --language-model)')
  refused(['--nbest', '17', '--beam-width', '16'], '--nbest must lie in 1..the beam width (16), got 17')
  refused(['--nbest', '0', '--beam-width', '16'], '--nbest must lie in 1..the beam width (16), got 0')
  refused(['--nbest', '101', '--language-model', TINY], '--nbest must lie in 1..the beam width (100), got 101')
  refused(['--nbest', '4', '--beam-width', '16', '--segment'], 'per-segment lists do not join into file lists')
  refused(['--rescore-language-model', TINY, '--beam-width', '16'], 'apply with --nbest only')
  refused(['--nbest', '4', '--beam-width', '16', '--rescore-lm-weight', '1.0'], 'applies with --rescore-language-model only')
  with pytest.raises(SystemExit):
    cli.parse(['transcribe', '--help'])
  text = ' '.join(capsys.readouterr().out.split())
  assert '--nbest N' in text and '--rescore-language-model PATH' in text and '--rescore-lm-weight X' in text
  assert 'per-segment lists do not join into file lists' in text


def test_transcribe_refuses_lists_without_a_beam_search():
  from speecht_amd import inference, transcription
  with pytest.raises(ValueError, match='needs a beam search'):
    inference.transcribe(None, [np.zeros((4, 2))], nbest=2)
  with pytest.raises(ValueError, match='applies to N-best lists'):
    inference.transcribe(None, [np.zeros((4, 2))], beam_width=4, rescore=dict(language_model=TINY))
  with pytest.raises(ValueError, match='not available with segment'):
    transcription.transcribe_files(None, [], nbest=2, beam_width=4, segment=object())
