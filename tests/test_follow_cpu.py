"""Following a known script in live streams without a GPU: the float64 oracle (tests/follow_oracle.py) on its own, the host form
st_ctc_follow_stream_host (plain loops over the whole lattice, the arithmetic of csrc/ctc_align_core.h and csrc/ctc_follow_core.h)
against the oracle, against st_ctc_align_long_host and st_ctc_align_host, its independence of how the rows are cut, the edges of K,
the table's semantics, and the surface: exports, argument checks, the Python classes and the CLI flags.

Bound of the host form against the oracle: fit and end_score within 1e-9 absolute -- a few ulps of values up to 32 per row, about
2e-11 over 1 000 rows, with fifty times that in hand; the cursor trace and the events identical, which the oracle's own margin
between best and second-best state (asserted > 1e-9 at every frame; seeds 0-3 give at least 8.1e-5) makes a fair demand."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import align_oracle as AO
from tests import follow_oracle as FO
from tests.align_long_util import host_align_long
from tests.follow_util import Driver, feed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, SPACE = 29, 27


def _same(a, b, tol):
  """|a - b| <= tol where both are finite, equality where one is not."""
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  fin = np.isfinite(a) & np.isfinite(b)
  return bool((np.abs(a[fin] - b[fin]) <= tol).all() and (a[~fin] == b[~fin]).all())


# ---- the oracle alone ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', [0, 1])
def test_oracle_invariants(seed):
  rng = np.random.default_rng(seed)
  T, L, K = 90, 24, 3
  labels = AO.random_labels(rng, L, C)
  starts = FO.word_starts(labels, SPACE)
  x, _ = AO.planted_logits(rng, labels, T, C, boost=4.0)
  r = FO.follow64(x, labels, starts, K)
  assert (np.diff(r.n_reached) >= 0).all() and r.n_reached[-1] == len(r.events)
  assert [w for w, _ in r.events] == list(range(len(r.events)))
  for w, t in r.events:                                       # the first frame with m_t >= a_j + 1, and not before
    assert r.m[t] >= starts[w] + 1 and (r.m[:t] < starts[w] + 1).all()
  assert (r.fit <= 0).all()
  for t in (0, 5, T // 2, T - 1):
    rows = x[:t + 1]
    a = AO.align64(rows, labels)
    if a is None:
      assert r.end_score[t] == -np.inf
    else:
      assert abs(a[2] - r.end_score[t]) <= 1e-9
  assert r.end_score[-1] > -np.inf


@pytest.mark.parametrize('K', [1, 4, 16])
def test_oracle_planted_script(K):
  rng = np.random.default_rng(7)
  labels = FO.script_without_repeats(rng, 120, C, SPACE)
  starts = FO.word_starts(labels, SPACE)
  x = FO.planted_script_logits(rng, labels, C)
  r = FO.follow64(x, labels, starts, K)
  assert (r.c == 2 * np.arange(len(labels)) + 1).all()
  assert r.margin.min() >= 7.0
  assert r.events == [(j, a + K - 1) for j, a in enumerate(starts) if a + K - 1 < len(labels)]


# ---- the host form --------------------------------------------------------------------------------------------------------------------

def _host_whole(x, labels, starts, K, cuts=(64,), max_events=4096):
  d = Driver([labels], [starts], C, max(len(labels), 1), K, max_events=max_events, max_rows=max(cuts) if cuts else 64)
  return feed(d, {0: x}, {0: list(cuts)})[0], d


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_host_form_against_oracle(seed):
  rng = np.random.default_rng(seed)
  T = L = 1000
  labels = AO.random_labels(rng, L, C)
  starts = FO.word_starts(labels, SPACE)
  x = AO.random_logits(rng, T, C)
  K = 3
  r = FO.follow64(x, labels, starts, K)
  assert r.margin.min() > 1e-9, r.margin.min()                # no frame has to be left out
  d = Driver([labels], [starts], C, L, K, max_events=1024, max_rows=100)
  at, trace, events, fit, end = 0, [], [], [], []
  while at < T:
    out = d.step({0: x[at:at + 100]})[0]
    at += 100
    trace += out['trace'].tolist()
    events += out['events']
    fit.append(out['fit'])
    end.append(out['end_score'])
    assert out['lost'] == 0 and out['status'] == 0 and out['frames'] == at and out['c'] == r.c[at - 1]
  assert trace == r.c.tolist()
  assert events == r.events
  assert _same(fit, r.fit[99::100], 1e-9) and _same(end, r.end_score[99::100], 1e-9)


def test_host_form_against_oracle_where_the_script_fits():
  rng = np.random.default_rng(11)
  labels = AO.random_labels(rng, 150, C)
  starts = FO.word_starts(labels, SPACE)
  x, _ = AO.planted_logits(rng, labels, 400, C, boost=5.0)
  r = FO.follow64(x, labels, starts, 2)
  assert r.margin.min() > 1e-9
  got, _ = _host_whole(x, labels, starts, 2, cuts=(37,))
  assert got['trace'] == r.c.tolist() and got['events'] == r.events and r.events
  assert _same(got['last']['fit'], r.fit[-1], 1e-9) and _same(got['last']['end_score'], r.end_score[-1], 1e-9)
  assert np.isfinite(got['last']['end_score'])


@pytest.mark.parametrize('L,T', [(600, 800), (511, 700), (40, 130), (1, 3)])
def test_end_score_is_the_alignment_score(L, T):
  from tests.test_align_cpu import host_align
  rng = np.random.default_rng(L)
  labels = AO.random_labels(rng, L, C)
  x, _ = AO.planted_logits(rng, labels, T, C, boost=3.0)
  got, _ = _host_whole(x, labels, FO.word_starts(labels, SPACE), 1, cuts=(64, 7))
  _, score, status = host_align_long(x, labels)
  assert status == 0
  assert np.float64(got['last']['end_score']).view(np.int64) == np.float64(score).view(np.int64)
  if L <= 511:
    _, _, fscore, fstatus = host_align(x[None], [labels], [T])
    assert fstatus[0] == 0 and np.float32(got['last']['end_score']).view(np.int32) == fscore.view(np.int32)[0]


def _three_streams(seed, T=700):
  rng = np.random.default_rng(seed)
  scripts = [AO.random_labels(rng, L, C) for L in (460, 30, 7)]           # two state blocks, one, one
  starts = [FO.word_starts(s, SPACE) for s in scripts]
  streams = {0: AO.planted_logits(rng, scripts[0], T, C, boost=2.0)[0], 1: AO.random_logits(rng, 211, C),
             2: AO.planted_logits(rng, scripts[2], 97, C, boost=2.0)[0]}
  return scripts, starts, streams


def test_chunk_independence_on_the_host():
  scripts, starts, streams = _three_streams(5)
  K = 4
  ref = None
  big = list(range(65, 131))
  for cut in ([1], [7], [10], [64], big):
    # alone ...
    d = Driver(scripts[:1], starts[:1], C, 460, K, max_rows=130 * 3)
    alone = feed(d, {0: streams[0]}, {0: cut})[0]
    this = (alone['trace'], alone['events'], alone['last']['record'].tolist()[:3] + alone['last']['record'].tolist()[4:], d.state_bytes(0).tobytes())
    if ref is None:
      ref = this
      assert ref[1], 'no event: the case shows nothing'
    assert this[0] == ref[0] and this[1] == ref[1] and this[2] == ref[2]
    assert this[3] == ref[3], 'the state bytes depend on the cut {}'.format(cut[:1])
    # ... and interleaved with two other streams cut their own way
    d = Driver(scripts, starts, C, 460, K, max_rows=130 * 3)
    both = feed(d, streams, {0: cut, 1: [13, 64, 1], 2: [5]})
    rec = both[0]['last']['record'].tolist()
    assert (both[0]['trace'], both[0]['events'], rec[:3] + rec[4:], d.state_bytes(0).tobytes()) == ref
  # the other streams are their own oracle's, too
  d = Driver(scripts, starts, C, 460, K, max_rows=130 * 3)
  both = feed(d, streams, {0: [64], 1: [13, 64, 1], 2: [5]})
  for s in (1, 2):
    r = FO.follow64(streams[s], scripts[s], starts[s], K)
    assert both[s]['trace'] == r.c.tolist() and both[s]['events'] == r.events


@pytest.mark.parametrize('K', [1, 16])
def test_confirm_edges_across_a_step_boundary(K):
  rng = np.random.default_rng(3)
  labels = FO.script_without_repeats(rng, 60, C, SPACE)
  starts = FO.word_starts(labels, SPACE)
  x = FO.planted_script_logits(rng, labels, C)
  r = FO.follow64(x, labels, starts, K)
  assert r.events == [(j, a + K - 1) for j, a in enumerate(starts) if a + K - 1 < 60]
  for cut in ([60], [1], [5], [17, 3]):                       # the window of 16 frames crosses the boundaries of every cut but the first
    got, _ = _host_whole(x, labels, starts, K, cuts=cut)
    assert got['events'] == r.events and got['trace'] == r.c.tolist()


def test_table_semantics_limit_sitting_out_reset_and_reuse():
  rng = np.random.default_rng(9)
  labels = FO.script_without_repeats(rng, 40, C, SPACE)
  starts = FO.word_starts(labels, SPACE)
  x = FO.planted_script_logits(rng, labels, C)
  r = FO.follow64(x, labels, starts, 2)
  # slot 0 has no script, slot 1 follows, slot 2's script is longer than the state was sized for
  d = Driver([[], labels, labels + labels], [[], starts, starts], C, 40, 2, max_rows=200)
  out = d.step({0: x[:10], 1: x[:10], 2: x[:10]}, guard=8)
  assert out[0]['status'] == 2 and out[2]['status'] == 1 and out[0]['c'] == -1 and out[0]['events'] == [] == out[2]['events']
  assert (out[0]['trace'] == -77).all() and (out[2]['trace'] == -77).all()
  assert (d.state_bytes(0) == 0xA5).all() and (d.state_bytes(2) == 0xA5).all()         # neither touches its state
  assert out[1]['trace'].tolist() == r.c[:10].tolist() and out[1]['frames'] == 10
  before = d.state_bytes(1).tobytes()
  # a step in which the stream sits out: its state stays, the record repeats what the header holds, no event
  out2 = d.step({0: x[:3]})
  assert d.state_bytes(1).tobytes() == before
  assert out2[1]['frames'] == 10 and out2[1]['c'] == out[1]['c'] and out2[1]['events'] == [] and out2[1]['fit'] == out[1]['fit']
  # rows at or past the limit are not consumed
  out3 = d.step({1: x[10:30]}, limits={1: 25}, guard=8)
  assert out3[1]['frames'] == 25 and out3[1]['trace'][:15].tolist() == r.c[10:25].tolist() and (out3[1]['trace'][15:] == -77).all()
  assert out[1]['events'] + out3[1]['events'] == [e for e in r.events if e[1] < 25]
  # reset and reuse: the slot starts over on any content, the 128 elements below state 0 become -inf in both columns
  d.reopen(1)
  out4 = d.step({1: x[:40]})
  assert out4[1]['trace'].tolist() == r.c.tolist() and out4[1]['events'] == r.events and out4[1]['frames'] == 40
  fresh = Driver([[], labels, []], [[], starts, []], C, 40, 2, max_rows=200)
  fresh.step({1: x[:40]})
  assert fresh.state_bytes(1).tobytes() == d.state_bytes(1).tobytes()
  cols = d.state_bytes(1)[128:].view(np.float64).reshape(2, -1)
  assert (cols[:, :128] == -np.inf).all()
  # a reset without rows
  d.reopen(1)
  out5 = d.step({1: x[:0]})
  assert out5[1]['frames'] == 0 and out5[1]['c'] == -1 and out5[1]['fit'] == -np.inf and out5[1]['end_score'] == -np.inf


def test_event_overflow_and_lost_rows_on_the_host():
  rng = np.random.default_rng(2)
  labels = FO.script_without_repeats(rng, 50, C, SPACE, word_len=1)
  starts = FO.word_starts(labels, SPACE)
  x = FO.planted_script_logits(rng, labels, C)
  r = FO.follow64(x, labels, starts, 1)
  d = Driver([labels], [starts], C, 50, 1, max_events=1, max_rows=200)
  out = d.step({0: x}, guard=16)[0]
  assert out['events'] == r.events[:1] and out['lost'] == len(r.events) - 1 and out['words'] == len(r.events)
  # a stream with more rows than the caller announced: the surplus is reported, not read
  x3 = np.concatenate([x, x, x])
  d = Driver([labels], [starts], C, 50, 1, max_rows=200)
  out = d.step({0: x3}, max_stream_rows=64)[0]
  assert out['frames'] == 64 and out['status'] == 4


# ---- the surface ----------------------------------------------------------------------------------------------------------------------

def test_exports_and_sizes():
  from speecht_amd import _lib
  lib = _lib.load()
  for name in ('st_ctc_follow_stream_state_bytes', 'st_ctc_follow_stream_ws', 'st_ctc_follow_stream_step', 'st_ctc_follow_stream_host'):
    assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
  nb = lambda L: (2 * L + 1 + 895) // 896
  for L in (1, 447, 448, 895, 896, 16384, 28671):
    assert lib.st_ctc_follow_stream_state_bytes(L) == 128 + 2 * (896 * nb(L) + 128) * 8
    assert lib.st_ctc_follow_stream_ws(300, L, 5) == 300 * 256 + 5 * 64 * nb(L) * 16 + 5 * 32 + 256
  assert [nb(L) for L in (1, 447, 448, 895, 896, 1000)] == [1, 1, 2, 2, 3, 3]
  assert lib.st_ctc_follow_stream_state_bytes(0) == 0 and lib.st_ctc_follow_stream_state_bytes(28672) == 0
  assert lib.st_ctc_follow_stream_ws(0, 10, 1) == 0 and lib.st_ctc_follow_stream_ws(10, 0, 1) == 0 and lib.st_ctc_follow_stream_ws(10, 10, 0) == 0


def test_abi_argument_validation():
  from speecht_amd import _lib
  lib = _lib.load()
  p = lambda a: ctypes.c_void_p(a.ctypes.data)
  x = np.zeros((4, 32), np.float32)
  rows, table = np.zeros((4, 2), np.int32), np.array([[0, 4, -1, 1]], np.int32)
  ids, offs, ws_, woffs = np.array([1, 2], np.int32), np.array([0, 2], np.int32), np.array([0], np.int32), np.array([0, 1], np.int32)
  state = np.zeros(lib.st_ctc_follow_stream_state_bytes(8) // 8, np.float64)
  events, result = np.zeros(8, np.int32), np.zeros(16, np.int32)
  work = np.zeros(lib.st_ctc_follow_stream_ws(4, 8, 1) // 8 + 1, np.float64)
  base = dict(logits=p(x), pitch=32, C=29, rows=p(rows), table=p(table), n_rows=4, max_rows=4, longest=4, S=1, ids=p(ids), offs=p(offs),
              ws=p(ws_), woffs=p(woffs), max_labels=8, K=2, state=p(state), events=p(events), me=4, result=p(result), trace=None,
              work=p(work), nbytes=work.nbytes)
  order = list(base)

  def host(**kw):
    return lib.st_ctc_follow_stream_host(*[dict(base, **kw)[k] for k in order])

  def device(**kw):                                           # refused before anything is launched: no device is touched
    return lib.st_ctc_follow_stream_step(*([dict(base, **kw)[k] for k in order] + [None]))

  assert host() == 0
  bad = [dict(logits=None), dict(rows=None), dict(table=None), dict(ids=None), dict(offs=None), dict(ws=None), dict(woffs=None),
         dict(state=None), dict(events=None), dict(result=None), dict(work=None), dict(C=1), dict(C=33), dict(pitch=28), dict(max_labels=0),
         dict(max_labels=28672), dict(S=0), dict(n_rows=-1), dict(n_rows=5), dict(longest=5), dict(longest=-1), dict(K=0), dict(K=17),
         dict(me=0), dict(nbytes=work.nbytes - 300), dict(state=ctypes.c_void_p(state.ctypes.data + 8)),
         dict(work=ctypes.c_void_p(work.ctypes.data + 4))]
  for kw in bad:
    assert host(**kw) != 0, kw
    assert device(**kw) != 0, kw
    assert b'follow stream' in lib.st_last_error()


def test_script_follower_and_word_helpers():
  from speecht_amd import streaming as S
  f = S.ScriptFollower()
  assert (f.max_labels, f.confirm, f.max_events, f.trace) == (16384, 0.06, 64, False)
  assert f.frames(2) == 3 and f.frames(2, frame_rate=50.0) == 2 and S.ScriptFollower(confirm=0.001).frames(2) == 1
  for kw in (dict(max_labels=0), dict(max_labels=28672), dict(confirm=0), dict(confirm=-1.0), dict(max_events=0), dict(confirm=float('nan'))):
    with pytest.raises(S.StreamError):
      S.ScriptFollower(**kw)
  with pytest.raises(S.StreamError):
    S.ScriptFollower(confirm=1.0).frames(2)                  # more than 16 frames
  ids, starts, words = f.script('Hello  big world', 29)
  assert words == ['hello', 'big', 'world'] and starts == [0, 7, 11] and len(ids) == 16
  assert starts == FO.word_starts(ids, SPACE)
  ids2, starts2, words2 = f.script(ids, 29)
  assert (ids2, starts2) == (ids, starts) and words2 == words
  for bad in ('', '   ', 'café', [28], [-1], []):
    with pytest.raises(S.StreamError):
      f.script(bad, 29)
  with pytest.raises(S.StreamError):
    S.ScriptFollower(max_labels=4).script('hello', 29)
  assert S.WordReached(1, 'big', 40) == S.WordReached(1, 'big', 40) and 'big' in repr(S.WordReached(1, 'big', 40))


def test_cli_flags():
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'speecht-cli'), 'stream', '--help'], capture_output=True, text=True)
  assert r.returncode == 0, r.stderr
  for flag in ('--script', '--script-text', '--follow-confirm'):
    assert flag in r.stdout
  from speecht_amd import streaming as S

  class Flags:
    script, script_text, follow_confirm = None, None, 0.06
  assert S.follower_of(Flags) == (None, None)
  Flags.script_text = 'a b'
  f, text = S.follower_of(Flags)
  assert isinstance(f, S.ScriptFollower) and text == 'a b'
  Flags.script = 'x.txt'
  with pytest.raises(S.StreamError):
    S.follower_of(Flags)
  assert S.reached_line('a.wav', S.WordReached(2, 'world', 50), 2, 160, 16000.0) == 'a.wav\treached\t2\tworld\t1.000'
