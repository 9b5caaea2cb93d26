"""Keyword spotting without a GPU: the float64 recursion (tests/spot_oracle.py) against the definition -- an enumeration of all
frame paths over all [s, e) --, its properties, and the host form st_ctc_spot_host against it through every states-per-lane
dispatch and the edge cases.

The host form (and, bit for bit, the kernel: tests/test_gpu_spot.py) is held to EXACT equality with the oracle on the score
bits, the spans, the status and both traces: both sides perform the same IEEE double subtractions, additions and comparisons in
the same order, so there is no tolerance."""
import ctypes
import functools

import numpy as np
import pytest

from tests import align_oracle as AO
from tests import spot_oracle as SO

# keyword lengths at both edges of every states-per-lane dispatch of the lattice (1, 2, 3, 4, 5, 6, 8, 10, 12, 16 states per lane
# hold up to 31, 63, 95, 127, 159, 191, 255, 319, 383, 511 ids)
DISPATCH_LENGTHS = [31, 32, 63, 64, 95, 96, 127, 128, 159, 160, 191, 192, 255, 256, 319, 320, 383, 384, 511]


def _p(a):
  return ctypes.c_void_p(a.ctypes.data)


def csr(keywords):
  offs = np.zeros(len(keywords) + 1, dtype=np.int32)
  offs[1:] = np.cumsum([len(k) for k in keywords])
  return np.array([i for k in keywords for i in k] + [0], dtype=np.int32), offs


def all_jobs(batch, n_keywords):
  return [(b, k) for b in range(batch) for k in range(n_keywords)]


def host_spot(logits, seq_lens, keywords, jobs, max_keyword_len=None, trace=True):
  """st_ctc_spot_host on a dense [B, T, C] batch -> (score [n], span [n, 2], status [n], trace_score [n, T], trace_start [n, T])
  (the traces None without ``trace``)."""
  from speecht_amd import _lib
  lib = _lib.load()
  logits = np.ascontiguousarray(logits, dtype=np.float32)
  B, T, C = logits.shape
  ids, offs = csr(keywords)
  n = len(jobs)
  table = np.array([j for job in jobs for j in job] + [0, 0], dtype=np.int32)
  max_len = max([len(k) for k in keywords] + [1]) if max_keyword_len is None else max_keyword_len
  score = np.full(n + 1, 7.0)
  span = np.full((n + 1, 2), -7, dtype=np.int32)
  status = np.full(n + 1, -7, dtype=np.int32)
  trace_score = np.full((n + 1, T), 7.0)
  trace_start = np.full((n + 1, T), -7, dtype=np.int32)
  need = lib.st_ctc_spot_ws(B, T, max_len, n)
  ws = np.zeros(need // 8 + 1, dtype=np.float64)
  _lib.call('st_ctc_spot_host', _p(logits), B, T, C, _p(np.asarray(seq_lens, dtype=np.int32)), _p(ids), _p(offs), len(keywords),
            max_len, _p(table), n, _p(score), _p(span), _p(trace_score) if trace else None, _p(trace_start) if trace else None,
            _p(status), _p(ws), need)
  assert score[-1] == 7.0 and (span[-1] == -7).all() and status[-1] == -7           # nothing written past the outputs
  assert (trace_score[-1] == 7.0).all() and (trace_start[-1] == -7).all()
  if not trace:
    assert (trace_score == 7.0).all() and (trace_start == -7).all()
    return score[:n], span[:n], status[:n], None, None
  return score[:n], span[:n], status[:n], trace_score[:n], trace_start[:n]


def assert_same_bits(got, want):
  """(score, span, status, trace_score, trace_start) twice: equal bit for bit (the traces may be None on both sides)."""
  assert (got[2] == want[2]).all(), (got[2], want[2])
  assert (got[1] == want[1]).all(), (got[1], want[1])
  assert (np.asarray(got[0]).view(np.int64) == np.asarray(want[0]).view(np.int64)).all(), (got[0], want[0])
  if want[3] is not None:
    assert (np.ascontiguousarray(got[3]).view(np.int64) == np.ascontiguousarray(want[3]).view(np.int64)).all()
    assert (got[4] == want[4]).all()


def random_keyword(rng, L, C, repeat_prob=0.15):
  return AO.random_labels(rng, L, C, repeat_prob=repeat_prob)


@functools.lru_cache(maxsize=None)
def dispatch_case(L, C):
  """One batch for a keyword length: four utterances of min_frames + 0..3 frames (random logits of scale 0.05, 1 and 4 and one
  with the keyword planted), one that is a frame too short, and next to the long keyword a short one; every pair is a job.
  -> (logits [5, T, C], seq_lens, keywords, jobs, the planted keyword's frames)."""
  rng = np.random.default_rng(1000 * C + L)
  kw = random_keyword(rng, L, C)
  need = SO.min_frames(kw)
  xs = [AO.random_logits(rng, need + extra, C, scale) for extra, scale in ((0, 0.05), (1, 1.0), (2, 4.0))]
  x, path = AO.planted_logits(rng, kw, need + 3, C)
  planted = (path.index(1), len(path) - path[::-1].index(2 * L - 1))
  xs += [x, AO.random_logits(rng, need - 1, C, 1.0)]
  logits, lens = AO.pad_batch(xs)
  keywords = [kw, random_keyword(rng, int(rng.integers(1, 8)), C)]
  return logits, lens, keywords, all_jobs(len(xs), 2), planted


# ---- the recursion against the definition ---------------------------------------------------------------------------------------

def _tiny_cases(n):
  rng = np.random.default_rng(3)
  cases = []
  while len(cases) < n:
    C = int(rng.integers(2, 4))
    T = int(rng.integers(1, 7))
    kw = AO.random_labels(rng, int(rng.integers(1, 4)), C, repeat_prob=0.3)
    cases.append((AO.random_logits(rng, T, C, scale=float(rng.choice([0.05, 1.0, 4.0]))), kw))
  return cases


def test_recursion_equals_the_enumeration_of_all_paths():
  worst, finite, none = 0.0, 0, 0
  for x, kw in _tiny_cases(60):
    ref = SO.spot64(x, kw)
    best, ends = SO.enumerate_spot(x, kw)
    for got, want in zip(np.append(ref['trace_score'], ref['score']), np.append(ends, best)):
      if np.isinf(want):
        assert got == want
        none += 1
      else:
        worst = max(worst, abs(got - want))
        finite += 1
    s, e = ref['span']
    if np.isfinite(best):
      assert 0 <= s < e <= x.shape[0] and ref['score'] == ref['trace_score'][e - 1] and ref['trace_start'][e - 1] == s
      assert (ref['trace_score'][e:] < ref['score']).all()              # the latest among equals
    else:
      assert (s, e) == (-1, -1)
  print('recursion against enumeration: {} finite values, {} without an occurrence, largest difference {:.3g}'.format(finite, none, worst))
  assert worst <= 1e-12 and finite > 100 and none > 20


def test_score_is_zero_exactly_when_the_greedy_classes_spell_the_keyword():
  rng = np.random.default_rng(4)
  zeros = 0
  for i in range(3000):
    C = int(rng.integers(2, 4))
    x = AO.random_logits(rng, int(rng.integers(1, 8)), C, scale=float(rng.choice([0.05, 1.0, 4.0])))
    if i % 10 == 0:
      x = np.round(x)                                                   # ties between classes
    kw = AO.random_labels(rng, int(rng.integers(1, 4)), C, repeat_prob=0.3)
    score = SO.spot64(x, kw)['score']
    assert score <= 0.0
    assert (score == 0.0) == SO.greedy_spells_tightly(x, kw), (x, kw)
    zeros += score == 0.0
  assert 300 < zeros < 2700


def planted_case(rng, C=29):
  """A keyword inside a longer label whose alignment is planted -> (logits, keyword, its planted frames (start, end))."""
  before, kw, after = (AO.random_labels(rng, int(rng.integers(lo, hi)), C, repeat_prob=0.2) for lo, hi in ((2, 7), (3, 7), (2, 7)))
  label = before + kw + after
  x, path = AO.planted_logits(rng, label, AO.min_frames(label) + int(rng.integers(0, 30)), C)
  first, last = 2 * len(before) + 1, 2 * (len(before) + len(kw)) - 1
  on_first = [t for t, u in enumerate(path) if u == first]
  on_last = [t for t, u in enumerate(path) if u == last]
  return x, kw, (on_first[0], on_last[-1] + 1)


def test_a_planted_keyword_comes_back_at_its_frames():
  rng = np.random.default_rng(5)
  found = 0
  for _ in range(200):
    x, kw, frames = planted_case(rng)
    r = SO.spot64(x, kw)
    found += r['score'] == 0.0 and tuple(r['span']) == frames
  assert found == 200, found


# ---- the host form against the oracle --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('L', DISPATCH_LENGTHS)
def test_host_form_equals_the_oracle_at_every_dispatch(L):
  logits, lens, keywords, jobs, planted = dispatch_case(L, 29)
  want = SO.spot_batch(logits, lens, keywords, jobs)
  got = host_spot(logits, lens, keywords, jobs)
  assert_same_bits(got, want)
  assert (got[2] == 0).all()
  assert np.isfinite(got[0][0:8:2]).all() and got[0][8] == -np.inf and (got[1][8] == -1).all()      # fits four times, then not
  assert got[0][6] == 0.0 and tuple(got[1][6]) == planted                                            # the planted one
  assert_same_bits(host_spot(logits, lens, keywords, jobs, trace=False), want[:3] + (None, None))


@pytest.mark.parametrize('C', [2, 32])
def test_host_form_equals_the_oracle_at_other_class_counts(C):
  for L in (1, 5, 31, 32, 200):
    logits, lens, keywords, jobs, _ = dispatch_case(L, C)
    assert_same_bits(host_spot(logits, lens, keywords, jobs), SO.spot_batch(logits, lens, keywords, jobs))


def edge_batch():
  """Equal neighbours, a keyword that does not fit, seq_len 0, single -inf classes and all-equal logits (every tie at once)."""
  rng = np.random.default_rng(6)
  C, T = 29, 40
  keywords = [[3, 3, 3], [1, 2, 2, 1], [5], [7, 27, 7, 7], list(range(20)) * 3]
  x = np.stack([AO.random_logits(rng, T, C, 1.0) for _ in range(6)])
  x[1] = 0.0                                              # all-equal logits
  x[2] = np.round(x[2])                                   # many ties
  x[3, ::3, 3] = -np.inf                                  # single -inf classes
  x[3, 1::4, C - 1] = -np.inf
  x[3, 5, 1] = x[3, 6, 2] = -np.inf
  x[4, :, 5] = -np.inf                                    # a class that can never be read
  lens = np.array([T, T, T, T, T, 0], dtype=np.int32)
  x = np.concatenate([x, AO.planted_logits(rng, [9] + keywords[1] + [1, 1], T, C)[0][None]])
  return x, np.append(lens, T).astype(np.int32), keywords, all_jobs(7, len(keywords))


def test_edge_cases_equal_the_oracle():
  x, lens, keywords, jobs = edge_batch()
  want = SO.spot_batch(x, lens, keywords, jobs)
  got = host_spot(x, lens, keywords, jobs)
  assert_same_bits(got, want)
  score = dict(zip(jobs, got[0]))
  span = dict(zip(jobs, got[1].tolist()))
  assert (got[2] == 0).all()
  assert score[(1, 0)] == 0.0 and span[(1, 0)] == [0, 40]               # all equal: everything ties, the longest hit wins
  assert score[(1, 4)] == -np.inf and span[(1, 4)] == [-1, -1]          # 60 ids and 19 repeats on 40 frames
  assert score[(4, 2)] == -np.inf                                       # its only class is impossible
  assert all(score[(5, k)] == -np.inf for k in range(5))                # no frames
  assert np.isfinite(score[(3, 0)]) and score[(6, 1)] == 0.0


def test_refused_jobs_and_arguments():
  from speecht_amd import _lib
  lib = _lib.load()
  rng = np.random.default_rng(7)
  C, T = 29, 20
  x = np.stack([AO.random_logits(rng, T, C) for _ in range(3)])
  keywords = [[1, 2], random_keyword(rng, 40, C, 0.0), [4]]
  jobs = [(0, 0), (3, 0), (-1, 0), (0, 3), (0, -1), (1, 1), (2, 2), (1, 2), (0, 0), (2, 0)]
  for lens in ([T, T, T], [T, T + 1, -1]):
    want = SO.spot_batch(x, lens, keywords, jobs, dispatch_len=31)
    got = host_spot(x, lens, keywords, jobs, max_keyword_len=31)
    assert_same_bits(got, want)
    # outside the tables, and the 40 ids beyond the 31 the call was dispatched for; then the lengths outside 0 .. frames
    assert got[2].tolist() == ([0, 1, 1, 1, 1, 1, 0, 0, 0, 0] if lens[1] == T else [0, 1, 1, 1, 1, 1, 1, 1, 0, 1])
    assert (got[0][got[2] != 0] == -np.inf).all() and (got[1][got[2] != 0] == -1).all()
    assert (got[3][got[2] != 0] == -np.inf).all() and (got[4][got[2] != 0] == -1).all()
  assert_same_bits(host_spot(x, [T, T, T], keywords, jobs), SO.spot_batch(x, [T, T, T], keywords, jobs))
  # an empty keyword is refused, an empty job table is fine
  got = host_spot(x, [T, T, T], [[], [1]], [(0, 0), (0, 1)])
  assert got[2].tolist() == [1, 0]
  assert len(host_spot(x, [T, T, T], keywords, [])[0]) == 0
  assert lib.st_ctc_spot_ws(2, 10, 512, 4) == 0 and lib.st_ctc_spot_ws(2, 10, 0, 4) == 0 and lib.st_ctc_spot_ws(0, 10, 5, 4) == 0
  assert lib.st_ctc_spot_ws(2, 10, 5, -1) == 0 and lib.st_ctc_spot_ws(2, 10, 5, 0) == lib.st_ctc_spot_ws(2, 10, 511, 1 << 20) == 2 * 10 * 256 + 512
  with pytest.raises(_lib.SpeechtHipError):
    host_spot(np.zeros((1, 5, 33), np.float32), [5], [[1]], [(0, 0)])
  with pytest.raises(_lib.SpeechtHipError):
    host_spot(x, [T, T, T], keywords, jobs, max_keyword_len=512)


# ---- pick_hits, the keyword parser, the CLI surface and the error paths ------------------------------------------------------------

def test_pick_hits_equals_its_specification():
  from speecht_amd import spotting
  rng = np.random.default_rng(12)
  total = 0
  for case in range(40):
    kw = AO.random_labels(rng, int(rng.integers(1, 4)), 5, repeat_prob=0.2)
    if case % 2:
      label = [int(i) for _ in range(4) for i in (kw + [int(rng.integers(4))])]
      x = AO.planted_logits(rng, label, AO.min_frames(label) + int(rng.integers(5, 40)), 5, boost=float(rng.choice([1.0, 8.0])))[0]
    else:
      x = AO.random_logits(rng, int(rng.integers(1, 60)), 5, scale=float(rng.choice([0.05, 1.0, 4.0])))
    if case % 5 == 0:
      x = np.round(x)                                                     # equal scores at several ends
    r = SO.spot64(x, kw)
    for threshold in (0.0, -0.1, -0.69, -5.0, -np.inf):
      want = SO.pick_hits(r['trace_score'], r['trace_start'], threshold)
      got = spotting.pick_hits(r['trace_score'], r['trace_start'], threshold)
      assert got == want
      total += len(got)
      assert all(a < b for a, b, _ in got) and all(s / (b - a) >= threshold for a, b, s in got)
      spans = sorted((a, b) for a, b, _ in got)
      assert all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1))          # no two overlap
      if got and threshold == -np.inf:
        assert got[0] == (r['span'][0], r['span'][1], r['score'])                         # the first is the best hit
  assert total > 200
  assert spotting.pick_hits([], [], -1.0) == [] and spotting.pick_hits([-np.inf, -np.inf], [-1, -1], -np.inf) == []


def test_keyword_parsing(tmp_path):
  from speecht_amd import spotting, vocabulary
  from speecht_amd.transcription import TranscriptionError
  assert spotting.keyword_ids("Don't STOP") == vocabulary.sentence_to_ids("don't stop")
  assert spotting.keyword_ids(' a ') == [vocabulary.SPACE_ID, 0, vocabulary.SPACE_ID]
  assert len(spotting.keyword_ids('a' * 511)) == 511 and spotting.MAX_LABELS == 511 and spotting.DEFAULT_THRESHOLD == -0.69
  for bad, what in (('', 'empty'), ('a' * 512, 'too long'), ('route 66', 'outside the vocabulary'), ('café', 'outside the vocabulary')):
    with pytest.raises(TranscriptionError, match=what):
      spotting.keyword_ids(bad)
  f = tmp_path / 'kw.txt'
  f.write_text('# names\nHello\n\n  \nnew york\nhello\n #indented comment\n cat \r\nNew York\n')
  assert spotting.read_keywords(str(f)) == ['hello', 'new york', ' cat ']
  with pytest.raises(OSError):
    spotting.read_keywords(str(tmp_path / 'missing.txt'))


def _cli():
  import importlib.machinery
  import importlib.util
  import os
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  loader = importlib.machinery.SourceFileLoader('speecht_cli_spot', os.path.join(root, 'speecht-cli'))
  spec = importlib.util.spec_from_loader('speecht_cli_spot', loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  return cli, root


def test_cli_surface():
  import subprocess
  import sys
  import os
  cli, root = _cli()
  r = subprocess.run([sys.executable, os.path.join(root, 'speecht-cli'), 'spot', '--help'], capture_output=True, text=True, timeout=120)
  assert r.returncode == 0, r.stderr
  for flag in ('--keywords', '--keyword', '--threshold', '--all', '--batch-size', '--mask-padding', '--sample-rate', '--segment',
               '--segment-threshold', '--min-silence', '--max-segment', '--output', '--run-name', '--train-dir', '--device'):
    assert flag in r.stdout, flag
  text = ' '.join(r.stdout.split())
  for said in ('log-likelihood ratio', 'greedy', 'across a cut is not found', 'not a posterior', 'no trained model', 'ln 0.5'):
    assert said in text, said
  _, flags = cli.parse(['spot', '--keyword', 'hello', '--keyword', 'new york', 'a.flac', 'd'])
  assert (flags.keyword, flags.keywords, flags.paths, flags.batch_size, flags.threshold) == (['hello', 'new york'], None, ['a.flac', 'd'], 1, -0.69)
  assert not flags.all_hits and not flags.segment and not flags.mask_padding and flags.sample_rate == 22050 and flags.output is None
  _, flags = cli.parse(['spot', '--keywords', 'k.txt', '--all', '--threshold', '-1.5', '--segment', '--min-silence', '0.5', '--batch-size', '8',
                        '--mask-padding', '--sample-rate', 'native', '--output', 'o.jsonl', 'a.flac'])
  assert (flags.keywords, flags.keyword, flags.all_hits, flags.threshold, flags.segment, flags.min_silence) == ('k.txt', None, True, -1.5, True, 0.5)
  assert (flags.batch_size, flags.mask_padding, flags.sample_rate, flags.output, flags.max_segment, flags.segment_threshold) == \
      (8, True, 'native', 'o.jsonl', 20.0, 0.03)
  for bad in (['spot', 'a.flac'], ['spot', '--keyword', 'a'], ['spot', '--keyword', 'a', '--keywords', 'k.txt', 'a.flac']):
    with pytest.raises(SystemExit):
      cli.parse(bad)
  _, flags = cli.parse(['train'])
  assert flags.batch_size == 64 and not hasattr(flags, 'keyword')             # the other commands keep their surface
  r = subprocess.run([sys.executable, os.path.join(root, 'speecht-cli'), 'record'], capture_output=True, text=True, timeout=120)
  assert r.returncode == 2


class _NoEngine:
  """An engine nothing may be asked of: the error paths below end before any device work."""
  device = 'cuda:0'

  def __getattr__(self, name):
    raise AssertionError('the engine was used: ' + name)


def test_spot_files_reports_problems_as_entries(tmp_path, capsys):
  import os
  from speecht_amd import spotting
  from speecht_amd.transcription import TranscriptionError
  cli, root = _cli()
  missing = str(tmp_path / 'nothing.flac')
  corrupt = tmp_path / 'corrupt.flac'
  corrupt.write_bytes(b'not a flac stream at all')
  short = tmp_path / 'short.npy'
  np.save(str(short), np.zeros(100, dtype=np.float32))
  paths = [missing, str(corrupt), str(short)]
  res = spotting.spot_files(_NoEngine(), paths, ['hello', 'new york'])
  assert [r['path'] for r in res] == paths and all(r['hits'] is None for r in res)
  assert 'no such file' in res[0]['error'] and 'cannot decode' in res[1]['error'] and 'too short' in res[2]['error']
  assert res[2]['seconds'] == 100 / 16000.0
  # keywords that cannot be searched are refused before any file is read
  with pytest.raises(TranscriptionError, match='outside the vocabulary'):
    spotting.spot_files(_NoEngine(), paths, ['route 66'])
  # no signals, or no keywords: nothing to do, no device
  assert spotting.spot_audio(_NoEngine(), [], [], ['a']) == [] and spotting.spot_audio(_NoEngine(), [np.zeros(9, np.float32)], [16000], []) == [[]]
  # the command line: problems with the keywords end before a model is made
  golden = os.path.join(root, 'tests', 'golden', '1089-134686-0037.flac')
  empty = tmp_path / 'kw.txt'
  empty.write_text('# nothing\n\n')
  for args, said in ((['--keywords', str(empty)], 'no keywords given'), (['--keywords', str(tmp_path / 'none.txt')], 'No such file'),
                     (['--keyword', 'route 66'], 'outside the vocabulary')):
    _, flags = cli.parse(['spot'] + args + [golden])
    assert spotting.run_cli(flags) == 1
    assert said in capsys.readouterr().err
  _, flags = cli.parse(['spot', '--keyword', 'a', str(tmp_path / 'empty_dir_that_is_missing')])
  os.makedirs(flags.paths[0])
  assert spotting.run_cli(flags) == 1 and 'no audio files found' in capsys.readouterr().err
  # the output formats
  entry = dict(path='a.flac', seconds=2.0, error=None,
               hits=[dict(keyword='new york', start=0.1161, end=0.5225, score=-1.25, score_per_frame=-0.0446428)])
  spotting.print_hits(entry)
  assert capsys.readouterr().out == 'a.flac\t0.116\t0.522\tnew york\t-1.2500\t-0.0446\n'
  assert spotting.result_json(entry) == dict(path='a.flac', seconds=2.0, hits=entry['hits'])
