"""`speecht-cli search` without a GPU: the CLI surface, the module alias, `Candidate`, the search walk against a restatement of
the reference's loop (speecht/parameter_search.py) with an injected scorer, the candidate scorer's pairing and host path against
`Evaluation.run_step`, and the argument checks of the new C ABI entry points (all made before any launch)."""
import bisect
import ctypes
import importlib.machinery
import importlib.util
import os
import random
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, 'tests', 'golden', 'lm_tiny.arpa')


def _cli():
  loader = importlib.machinery.SourceFileLoader('speecht_cli_search', os.path.join(ROOT, 'speecht-cli'))
  spec = importlib.util.spec_from_loader('speecht_cli_search', loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  return cli


def test_search_help_lists_the_reference_flags_and_the_extensions():
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'speecht-cli'), 'search', '--help'], capture_output=True, text=True,
                     timeout=120)
  assert r.returncode == 0, r.stderr
  for flag in ('--population-size', '--noise-std', '--ui', '--language-model', '--lm-weight', '--word-count-weight',
               '--valid-word-count-weight', '--max-iterations', '--candidates-per-batch', '--seed', '--pair-by-row',
               '--host-scoring'):
    assert flag in r.stdout, flag
  _, flags = _cli().parse(['search', '--language-model', 'x.arpa'])
  assert (flags.population_size, flags.noise_std, flags.use_ui) == (10, 0.5, False)
  assert (flags.max_iterations, flags.candidates_per_batch, flags.language_model) == (0, 1, 'x.arpa')
  with pytest.raises(SystemExit):                                  # --language-model is required
    _cli().parse(['search'])
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'speecht-cli'), 'record'], capture_output=True, text=True, timeout=120)
  assert r.returncode == 2                                          # record stays unprovided


def test_speecht_parameter_search_alias():
  import importlib
  mod = importlib.import_module('speecht.parameter_search')
  assert mod is importlib.import_module('speecht_amd.parameter_search')
  from speecht.parameter_search import Candidate, LanguageModelParameterSearch   # noqa: F401
  from speecht.evaluation import Evaluation
  assert issubclass(LanguageModelParameterSearch, Evaluation)


def _stats(ler, wer):
  return types.SimpleNamespace(global_letter_error_rate=ler, global_word_error_rate=wer)


def test_candidate_ordering_and_format():
  from speecht_amd.parameter_search import Candidate
  a, b = Candidate(1.0, 0.0, 0.0), Candidate(0.5, -1.25, 2.345)
  a.update_score(-0.5, _stats(0.2, 0.3))
  b.update_score(-1.25, _stats(0.5, 0.75))
  assert b < a and a > b and not a < b
  assert str(a) == '-0.50 Candidate (lm_weight=1.00, wc_weight=0.00, valid_wc_weight=0.00) has LER: 0.20 WER: 0.30'
  assert str(b) == '-1.25 Candidate (lm_weight=0.50, wc_weight=-1.25, valid_wc_weight=2.35) has LER: 0.50 WER: 0.75'
  np.random.seed(3)
  c = a.mutate(0.5)
  np.random.seed(3)
  d = np.random.normal(0, 0.5, 3)
  assert (c.lm_weight, c.word_count_weight, c.valid_word_count_weight) == (1.0 + d[0], 0.0 + d[1], 0.0 + d[2])


def _fake_score(c):
  # a deterministic stand-in for a batch's statistics: a function of the weights alone
  ler = abs(c.lm_weight - 2.0) / 4
  wer = abs(c.word_count_weight + 0.5) / 3 + abs(c.valid_word_count_weight - 1.0) / 5
  return ler, wer


def _reference_walk(iterations, population_size, std):
  """The reference's loop (parameter_search.py run_search), restated: the candidate lines it prints and its final population."""
  class C:
    def __init__(self, lm, wc, vwc):
      self.lm, self.wc, self.vwc, self.score = lm, wc, vwc, None

    def __lt__(self, other):
      return self.score < other.score

  def score(c):
    ler, wer = _fake_score(types.SimpleNamespace(lm_weight=c.lm, word_count_weight=c.wc, valid_word_count_weight=c.vwc))
    c.score = -(ler + wer)
  printed = []
  first = C(1.0, 0.0, 0.0)
  score(first)
  population = [first]
  printed.append((first.lm, first.wc, first.vwc, first.score))
  for _ in range(iterations):
    parent = random.choice(population)
    child = C(parent.lm + np.random.normal(0, std), parent.wc + np.random.normal(0, std), parent.vwc + np.random.normal(0, std))
    score(child)
    bisect.insort(population, child)
    if len(population) > population_size:
      del population[0]
    printed.append((child.lm, child.wc, child.vwc, child.score))
  return printed, [(c.lm, c.wc, c.vwc, c.score) for c in population]


def _run_search(k, iterations, population_size=4, std=0.5, seed=11):
  from speecht_amd.evaluation import EvalStatistics
  from speecht_amd.parameter_search import LanguageModelParameterSearch
  search = LanguageModelParameterSearch.__new__(LanguageModelParameterSearch)
  search.flags = types.SimpleNamespace(noise_std=std, population_size=population_size)
  search.candidates, search.num_iterations = [], 0
  calls = []

  def score(cands):
    calls.append(len(cands))
    for c in cands:
      ler, wer = _fake_score(c)
      stats = EvalStatistics()
      stats.track_distances(int(round(ler * 1000)), int(round(wer * 1000)), 1000, 1000)
      c.update_score(-(stats.global_letter_error_rate + stats.global_word_error_rate), stats)
  printed = []
  import builtins
  real_print = builtins.print
  builtins.print = lambda *a, **kw: printed.append(a[0])
  try:
    random.seed(seed)
    np.random.seed(seed)
    search.search(score, max_iterations=iterations, candidates_per_batch=k)
  finally:
    builtins.print = real_print
  return search, printed, calls


def _key(c):
  return (c.lm_weight, c.word_count_weight, c.valid_word_count_weight, c.score)


def test_k1_search_walks_like_the_reference():
  search, printed, calls = _run_search(1, 9)
  random.seed(11)
  np.random.seed(11)
  ref_printed, ref_population = _reference_walk(9, 4, 0.5)
  got = [_key(c) for c in printed]
  assert [g[:3] for g in got] == [r[:3] for r in ref_printed]
  np.testing.assert_allclose([g[3] for g in got], [r[3] for r in ref_printed], atol=1e-3)   # (the stand-in rounds to 1e-3)
  assert [_key(c)[:3] for c in search.candidates] == [r[:3] for r in ref_population]
  assert calls == [1] * 10 and search.num_iterations == 9
  lines = search.population_lines()
  assert lines[0] == 'Current population after 9 iterations' and lines[1] == ''
  assert lines[2:] == [str(c) for c in sorted(search.candidates, reverse=True)]


def test_k3_search_draws_a_generation_from_the_population_as_it_stands():
  """K > 1: K parents drawn (random.choice) from the population before any child is scored, then their mutations in order,
  one scoring call for the K children, insertion and printing in the order drawn; the last generation takes what is left."""
  search, printed, calls = _run_search(3, 7)
  assert calls == [1, 3, 3, 1] and search.num_iterations == 7
  random.seed(11)
  np.random.seed(11)
  first = (1.0, 0.0, 0.0)
  population = [(first, -sum(_fake_score(types.SimpleNamespace(lm_weight=1.0, word_count_weight=0.0, valid_word_count_weight=0.0))))]
  expect = [first]
  done = 0
  while done < 7:
    k = min(3, 7 - done)
    parents = [random.choice(population)[0] for _ in range(k)]
    children = [tuple(p[i] + np.random.normal(0, 0.5) for i in range(3)) for p in parents]
    for ch in children:
      s = -sum(_fake_score(types.SimpleNamespace(lm_weight=ch[0], word_count_weight=ch[1], valid_word_count_weight=ch[2])))
      scores = [q for _, q in population]
      population.insert(bisect.bisect_right(scores, s), (ch, s))
      if len(population) > 4:
        del population[0]
      expect.append(ch)
      done += 1
  assert [_key(c)[:3] for c in printed] == expect
  assert [_key(c)[:3] for c in search.candidates] == [p for p, _ in population]


# ---- the candidate scorer on the host --------------------------------------------------------------------------------------
def _sparse(rows):
  from speecht_amd.speech_input import SparseTensorValue
  idx = [[b, p] for b, r in enumerate(rows) for p in range(len(r))]
  return SparseTensorValue(np.array(idx, dtype=np.int64).reshape(-1, 2), np.array([v for r in rows for v in r], dtype=np.int64),
                           np.array([len(rows), max([len(r) for r in rows] + [0])], dtype=np.int64))


class _FakeDecodes:
  """engine_decode.CandidateDecodes with host arrays (the host path reads ids.shape, lens_host() and host())."""

  def __init__(self, per_candidate, T):
    P, B = len(per_candidate), len(per_candidate[0])
    self.ids = np.zeros((P, B, T), dtype=np.int32)
    self._lens = np.zeros((P, B), dtype=np.int32)
    for p, rows in enumerate(per_candidate):
      for b, r in enumerate(rows):
        self.ids[p, b, :len(r)] = r
        self._lens[p, b] = len(r)
    self._rows = per_candidate

  def lens_host(self):
    return self._lens

  def host(self):
    return [(rows, None) for rows in self._rows]


def _run_step_stats(labels, rows, pair_by_row):
  from speecht_amd.evaluation import EvalStatistics, Evaluation
  model = types.SimpleNamespace(global_step=types.SimpleNamespace(eval=lambda: 0),
                                step=lambda sess, **kw: [np.float32(1.0), [_sparse(rows)], _sparse(labels)])
  ev = Evaluation.__new__(Evaluation)
  ev.flags = types.SimpleNamespace(pair_by_row=pair_by_row)
  stats = EvalStatistics()
  ev.run_step(model, None, stats, save=False, verbose=False)
  return stats


def _fields(s):
  return [s.decodings_counter] + [getattr(s, f) for f in s._FIELDS] + [getattr(s, 'sum_' + f) for f in s._FIELDS]


def test_walk_rows_is_extract_decoded_ids_by_index():
  from speecht_amd.candidate_scoring import walk_rows
  from speecht_amd.evaluation import Evaluation
  rng = np.random.default_rng(5)
  for _ in range(300):
    B = int(rng.integers(1, 7))
    rows = [[int(v) for v in rng.integers(0, 28, int(rng.integers(0, 3)) * int(rng.integers(0, 2)))] for _ in range(B)]
    by_row = Evaluation.rows_by_batch(_sparse(rows))
    want = list(Evaluation.extract_decoded_ids(_sparse(rows)))
    got = [by_row[r] for r in walk_rows([len(r) for r in rows])]
    assert [list(map(int, w)) for w in want] == [list(map(int, g)) for g in got], rows


@pytest.mark.parametrize('pair_by_row', [False, True])
def test_host_scorer_equals_run_step_for_every_candidate(pair_by_row):
  from speecht_amd import vocabulary as V
  from speecht_amd.candidate_scoring import score_candidates
  ids = V.sentence_to_ids
  labels = [ids('the cat sat'), ids("it's a  dog "), ids('on the mat'), ids('x')]
  cands = [[ids('the cat sat'), ids("its a dog"), ids('on the hat'), ids('y')],
           [[], ids('the at'), ids('on the mat'), ids(' x ')],               # row 0 empty: the walk still yields it
           [ids('a'), ids('b c'), [], ids('d')]]                             # a later empty row: the reference walk runs out
  if pair_by_row:
    got = score_candidates(_sparse(labels), _FakeDecodes(cands, 16), pair_by_row=True, device=False)
    for p in range(3):
      assert _fields(got[p]) == _fields(_run_step_stats(labels, cands[p], True))
    return
  with pytest.raises(RuntimeError, match='ran out of decodings'):
    score_candidates(_sparse(labels), _FakeDecodes(cands, 16), device=False)
  with pytest.raises(RuntimeError, match='ran out of decodings'):
    _run_step_stats(labels, cands[2], False)
  got = score_candidates(_sparse(labels), _FakeDecodes(cands[:2], 16), device=False)
  for p in range(2):
    assert _fields(got[p]) == _fields(_run_step_stats(labels, cands[p], False)), p
  # an empty LABEL row shifts the labels as well: the walk pairs what run_step pairs
  labels2 = [ids('ab'), [], ids('cd e'), ids('f')]
  rows2 = [ids('ab'), ids('cd'), [], ids('g')]
  got = score_candidates(_sparse(labels2), _FakeDecodes([rows2], 8), device=False)
  assert _fields(got[0]) == _fields(_run_step_stats(labels2, rows2, False))


# ---- C ABI argument checks (before any launch) ------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
  from speecht_amd import _lib
  return _lib.load()


def test_new_entry_points_are_exported(lib):
  from speecht_amd import _lib
  for name in ('st_ctc_beam_lm_candidates_ws', 'st_ctc_beam_search_decode_lm_candidates', 'st_edit_distance_pairs',
               'st_edit_distance_max_len'):
    assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
  assert lib.st_edit_distance_max_len() >= 2000
  # the workspace: node pools of min(P, 64) x B searches + the shared log-softmax rows; P = 1 is the single search's
  assert lib.st_ctc_beam_lm_candidates_ws(4, 50, 16, 1) == lib.st_ctc_beam_ws(4, 50, 16)
  assert lib.st_ctc_beam_lm_candidates_ws(4, 50, 16, 3) > lib.st_ctc_beam_lm_candidates_ws(4, 50, 16, 2)
  assert lib.st_ctc_beam_lm_candidates_ws(4, 50, 16, 64) == lib.st_ctc_beam_lm_candidates_ws(4, 50, 16, 200)
  assert lib.st_ctc_beam_lm_candidates_ws(4, 50, 16, 0) == 0


def test_candidates_search_rejects_bad_arguments(lib):
  from speecht_amd import _lib
  from speecht_amd.language_model import LanguageModel
  lm = LanguageModel(TINY)
  B, T = 2, 10
  desc = _lib.Tensor3(0x1000, B, T, 29, 0, T, 32)                 # device addresses are never read before a launch
  lens = ctypes.c_void_p(0x2000)
  out = ctypes.c_void_p(0x3000)
  need = lib.st_ctc_beam_lm_candidates_ws(B, T, 8, 2)

  def run(weights, candidates, ws_bytes=need, handle=lm._handle, ptr=desc, wptr=True, oov=-1000.0):
    w = (ctypes.c_float * max(len(weights), 1))(*weights)
    return lib.st_ctc_beam_search_decode_lm_candidates(ctypes.byref(ptr) if ptr is not None else None, lens, 8, 1, handle,
                                                       w if wptr else None, candidates, oov, out, T, out, out,
                                                       ctypes.c_void_p(0x4000), ws_bytes, None)
  ok = [0.8, 0.0, 2.3, 1.0, 0.5, 0.0]
  assert run(ok, 2, ptr=None) == -1 and b'null argument' in lib.st_last_error()
  assert run(ok, 2, handle=None) == -1 and b'null argument' in lib.st_last_error()
  assert run(ok, 2, wptr=False) == -1 and b'null argument' in lib.st_last_error()
  assert run(ok, 0) == -1 and b'candidates' in lib.st_last_error()
  assert run(ok, -3) == -1 and b'candidates' in lib.st_last_error()
  for bad in (float('nan'), float('inf'), -float('inf')):
    w = list(ok)
    w[4] = bad
    assert run(w, 2) == -1 and b'finite (candidate 1)' in lib.st_last_error()
  assert run(ok, 2, oov=float('nan')) == -1 and b'finite' in lib.st_last_error()
  assert run(ok, 2, ws_bytes=need - 1) == -3 and b'workspace' in lib.st_last_error()
  neg = _lib.Tensor3(0x1000, -1, T, 29, 0, T, 32)
  assert run(ok, 2, ptr=neg) == -1 and b'negative' in lib.st_last_error()


def test_edit_distance_rejects_bad_arguments(lib):
  p = ctypes.c_void_p(0x1000)
  call = lambda *a: lib.st_edit_distance_pairs(*a)
  assert call(p, 2, 8, p, p, 2, 8, p, p, -1, p, None) == -1 and b'negative' in lib.st_last_error()
  assert call(p, -2, 8, p, p, 2, 8, p, p, 1, p, None) == -1 and b'negative' in lib.st_last_error()
  assert call(p, 2, -8, p, p, 2, 8, p, p, 1, p, None) == -1 and b'negative' in lib.st_last_error()
  assert call(p, 2, 8, p, p, 2, -1, p, p, 1, p, None) == -1 and b'negative' in lib.st_last_error()
  assert call(None, 2, 8, p, p, 2, 8, p, p, 1, p, None) == -1 and b'null argument' in lib.st_last_error()
  assert call(p, 2, 8, p, p, 2, 8, p, None, 1, p, None) == -1 and b'null argument' in lib.st_last_error()
  assert call(p, 2, 8, p, p, 2, 8, p, p, 1, None, None) == -1 and b'null argument' in lib.st_last_error()
  assert call(None, 0, 0, None, None, 0, 0, None, None, 0, None, None) == 0          # nothing to do
