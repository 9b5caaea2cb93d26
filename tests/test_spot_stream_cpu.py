"""Keyword spotting in live streams on the host: st_ctc_spot_stream_host against the float64 specification
(tests/spot_stream_oracle.py) bit for bit, however the rows are cut; its events against the offline host trace; the plans' layout
and validation.  Needs no GPU."""
import numpy as np
import pytest

from tests import spot_stream_cases as SC
from tests import spot_stream_oracle as SO

KW29 = [[2, 0, 19], [0], [7, 7], [19, 7, 4, 27, 2, 0, 19], [4, 4, 4, 11]]          # "cat", "a", "hh", "the cat", "eeel"
KW5 = [[0, 1], [2], [3, 3], [1, 0, 2, 3]]
NEG_INF = float('-inf')


def _stream(C, T, seed, keywords):
  """Noise with tight readings of some keywords planted in it (one of them twice, back to back)."""
  x = SC.noise(T, C, seed, scale=1.5)
  at = 5
  for n, k in enumerate(keywords + keywords[:1]):
    if at + 3 * len(k) + 4 >= T:
      break
    at = SC.plant(x, at, k, C - 1, stay=1 + n % 2) + (n % 3)
  return x


def _oracle_by_step(x, keywords, threshold, hold, bounds, finish):
  """The oracle's events of rows x, grouped by the step that emits them: bounds = the rows consumed after each step."""
  ev = SO.stream_events(x, keywords, threshold, hold, finish)
  steps, lo = [], 0
  for hi in bounds:
    steps.append(SO.as_set((k, a, e, kind, sc) for k, a, e, kind, sc, fr in ev if kind == 0 and lo <= fr < hi))
    lo = hi
  return steps, SO.as_set((k, a, e, kind, sc) for k, a, e, kind, sc, fr in ev if kind == 1)


def _run_cuts(keywords, C, x, sizes, threshold, hold, pack=1):
  """One stream fed in pieces of the given sizes, then finished: every step's events are the oracle's of those frames."""
  r = SC.Runner(keywords, C, 2, threshold, hold, pack=pack, max_events=256)
  bounds = np.cumsum(sizes).tolist()
  assert bounds[-1] == len(x)
  want, flushed = _oracle_by_step(x, keywords, threshold, hold, bounds, True)
  lo, seen = 0, set()
  for i, hi in enumerate(bounds):
    got = r.step({1: (x[lo:hi], -1, i == 0)})
    assert got[1] == (want[i], len(want[i])), (i, lo, hi)
    assert got[0] == (set(), 0)
    seen |= got[1][0]
    lo = hi
  got = r.step({1: (x[:0], len(x), False)})
  assert got[1] == (flushed, len(flushed))
  return seen | flushed, r


@pytest.mark.parametrize('threshold', [0.0, -0.69, NEG_INF])
@pytest.mark.parametrize('hold', [1, 4])
@pytest.mark.parametrize('C,keywords', [(29, KW29), (5, KW5)])
def test_every_cut_gives_the_specification(C, keywords, hold, threshold):
  T = 90
  x = _stream(C, T, 11 * C + hold, keywords)
  whole, _ = _run_cuts(keywords, C, x, [T], threshold, hold)
  assert whole, 'the case holds no hit'
  one, _ = _run_cuts(keywords, C, x, [1] * T, threshold, hold)
  rng = np.random.RandomState(C + hold)
  cuts = []
  while sum(cuts) < T:
    cuts.append(min(int(rng.randint(0, 12)), T - sum(cuts)))          # (steps without rows among them)
  rand, _ = _run_cuts(keywords, C, x, cuts, threshold, hold)
  assert whole == one == rand
  if threshold == 0.0:
    assert all(np.int64(bits).view(np.float64) == 0.0 for *_, bits in whole)


def test_cuts_at_the_frame_a_held_hit_leaves():
  C, hold = 29, 5
  x = _stream(C, 60, 3, KW29[:1])
  ev = [e for e in SO.stream_events(x, KW29[:1], -0.69, hold) if e[3] == 0]
  assert ev
  k, a, end, kind, score, frame = ev[0]
  if frame == end + hold - 1:                                             # it left by rule 4
    for consumed in (end + hold - 1, end + hold):
      _run_cuts(KW29[:1], C, x, [consumed, len(x) - consumed], -0.69, hold)
  # and with the planted reading alone: it stays pending for exactly `hold` frames
  y = np.zeros((30, C), np.float32)
  y[:, C - 1] = 5.0
  stop = SC.plant(y, 4, [2, 0, 19], C - 1)
  r = SC.Runner([[2, 0, 19]], C, 1, 0.0, hold)
  assert r.step({0: (y[:stop + hold - 1], -1, True)})[0] == (set(), 0)
  got = r.step({0: (y[stop + hold - 1:stop + hold], -1, False)})[0]
  assert got == (SO.as_set([(0, 4, stop, 0, 0.0)]), 1)


@pytest.mark.parametrize('C,keywords', [(29, KW29), (5, KW5), (29, [[i % 28 for i in range(40)], [3], [5, 5]])])
def test_pack_0_and_pack_1_agree(C, keywords):
  x = _stream(C, 70, 17, keywords)
  a, ra = _run_cuts(keywords, C, x, [7] * 10, NEG_INF, 3, pack=0)
  b, rb = _run_cuts(keywords, C, x, [7] * 10, NEG_INF, 3, pack=1)
  assert a == b and a
  assert ra.n_waves == len(keywords) and rb.n_waves < ra.n_waves


def test_idle_streams_resets_limits_and_finishes():
  C, kws = 5, KW5
  x, y = _stream(C, 64, 1, kws), _stream(C, 50, 2, kws)
  r = SC.Runner(kws, C, 3, NEG_INF, 2, max_events=256)
  want_x = SO.as_set(e[:5] for e in SO.stream_events(x, kws, NEG_INF, 2))
  got_x, got_y = set(), set()
  got = r.step({0: (x[:20], -1, True), 2: (y[:9], -1, True)})
  got_x |= got[0][0]
  before = r.state_words()
  got = r.step({0: (x[20:31], -1, False)})                              # stream 2 sits out: its record keeps its bits
  per = r.state_bytes // 4
  assert np.array_equal(before[2 * per:3 * per], r.state_words()[2 * per:3 * per]) and got[2] == (set(), 0) and got[1] == (set(), 0)
  got_x |= got[0][0]
  got = r.step({0: (x[31:], -1, False), 2: (y[:30], -1, True)})         # stream 2 starts again from frame 0 in mid-stream
  got_x |= got[0][0]
  got_y |= got[2][0]
  # stream 0 finishes on a limit that leaves its last 4 rows of the step unconsumed; stream 2 goes on
  z = np.concatenate([x, _stream(C, 10, 9, kws)])
  got = r.step({0: (z[64:74], 70, False), 2: (y[30:], -1, False)})
  got_x |= got[0][0]
  got_y |= got[2][0]
  assert got_x == SO.as_set(e[:5] for e in SO.stream_events(z[:70], kws, NEG_INF, 2)) != want_x
  got_y |= r.step({2: (y[:0], 50, False)})[2][0]
  assert got_y == SO.as_set(e[:5] for e in SO.stream_events(y, kws, NEG_INF, 2))
  assert any(kind == 1 for _, _, _, kind, _ in got_y | got_x)
  # a finish with nothing pending flushes nothing: a stream of blanks
  r = SC.Runner(kws, C, 1, -0.69, 2)
  blanks = np.zeros((12, C), np.float32)
  blanks[:, C - 1] = 9.0
  assert r.step({0: (blanks, 12, True)})[0] == (set(), 0)
  # a step without rows, reset or limit changes nothing and reports nothing
  before = r.state_words()
  assert r.step({})[0] == (set(), 0) and np.array_equal(before, r.state_words())


def test_more_events_than_the_buffer_holds():
  C, kws = 5, KW5
  x = _stream(C, 80, 4, kws)
  want = SO.as_set(e[:5] for e in SO.stream_events(x, kws, NEG_INF, 1, finish=False))
  assert len(want) > 4
  r = SC.Runner(kws, C, 2, NEG_INF, 1, max_events=1)
  garbage = r.events.copy()
  ev, count = r.step({0: (x, -1, True)})[0]
  assert count == len(want) and len(ev) == 1 and ev <= want
  assert np.array_equal(r.events[16 + 8:], garbage[16 + 8:])           # beyond slot 0 of stream 0 nothing was written


def _offline_traces(x, keywords, C):
  lib = SC.lib()
  ids, offs = SC.csr(keywords)
  T, K = len(x), len(keywords)
  longest = max(len(k) for k in keywords)
  jobs = np.asarray([(0, k) for k in range(K)], dtype=np.int32)
  score, span, status = np.zeros(K), np.zeros((K, 2), np.int32), np.zeros(K, np.int32)
  trv, trs = np.zeros((K, T)), np.zeros((K, T), np.int32)
  need = int(lib.st_ctc_spot_ws(1, T, longest, K))
  ws = np.zeros(need // 8 + 2, dtype=np.float64)
  p = SC._p
  assert lib.st_ctc_spot_host(p(np.ascontiguousarray(x)), 1, T, C, p(np.asarray([T], np.int32)), p(ids), p(offs), K, longest, p(jobs), K,
                              p(score), p(span), p(trv), p(trs), p(status), p(ws), need) == 0
  return trv, trs


@pytest.mark.parametrize('threshold', [-0.69, NEG_INF])
@pytest.mark.parametrize('C,keywords', [(29, KW29), (5, KW5)])
def test_events_lie_on_the_offline_trace_and_do_not_overlap(C, keywords, threshold):
  x = _stream(C, 120, 23, keywords)
  got = SC.feed_in_cuts(SC.Runner(keywords, C, 1, threshold, 3, max_events=512), {0: x}, [13, 1, 40])[0]
  assert got == SO.as_set(e[:5] for e in SO.stream_events(x, keywords, threshold, 3))
  trv, trs = _offline_traces(x, keywords, C)
  for k in range(len(keywords)):
    mine = sorted((a, e) for kk, a, e, _, _ in got if kk == k)
    assert all(p[1] <= q[0] for p, q in zip(mine, mine[1:])), (k, mine)
  for k, a, e, kind, bits in got:
    assert np.float64(trv[k, e - 1]).view(np.int64) == bits and trs[k, e - 1] == a and 0 <= a < e


def test_a_planted_keyword_scores_exactly_zero_on_its_span():
  C = 29
  x = SC.noise(50, C, 8)
  stop = SC.plant(x, 12, [19, 7, 4], C - 1, stay=2)
  x[stop:stop + 6, C - 1] = 30.0
  got = SC.feed_in_cuts(SC.Runner([[19, 7, 4]], C, 1, 0.0, 2), {0: x}, [9])[0]
  assert got == SO.as_set([(0, 12, stop, 0, 0.0)])


def test_plan_validation():
  assert SC.make_plan([[28]], 29, 1) is None                               # an id >= C - 1
  assert SC.make_plan([[-1]], 29, 1) is None
  assert SC.make_plan([[1], []], 29, 1) is None                            # L = 0
  assert SC.make_plan([[1] * 512], 29, 1) is None                          # L = 512
  assert SC.make_plan([[1] * 511], 29, 1) is not None
  assert SC.make_plan([[1, 2], [3]], 29, 1, offsets=[0, 2, 1]) is None      # offsets not monotone
  assert SC.make_plan([[1, 2]], 29, 1, offsets=[-1, 1]) is None
  assert SC.make_plan([[1]], 33, 1) is None and SC.make_plan([[0]], 1, 1) is None and SC.make_plan([[1]], 29, 2) is None
  assert SC.make_plan([], 29, 1) is None
  assert SC.lib().st_ctc_spot_stream_state_bytes(SC._p(np.zeros(64, np.int32))) == 0


def _states(plan):
  """-> per wave the descriptor of every state in state order, and the keyword at every lane."""
  places, kpl, nw = SC.layout(plan)
  waves = plan[16:16 + nw * (kpl + 1) * 64].reshape(nw, kpl + 1, 64)
  return [w[:kpl].T.reshape(-1) for w in waves], [w[kpl] for w in waves], places, kpl


@pytest.mark.parametrize('keywords,kpl,places', [
    ([[1] * 31], 1, [(0, 0, 31)]),                                         # one wave of 63 states
    ([[1] * 31, [2]], 1, [(0, 0, 31), (1, 0, 1)]),                         # 63 + 3 lanes: the second spills
    ([list(range(28)) + [0, 1, 2, 3]], 2, [(0, 0, 32)]),                   # 65 states: two per lane
    ([[k % 28] for k in range(21)], 1, [(0, 3 * k, 1) for k in range(21)]),
    ([[0, 0]], 1, [(0, 0, 2)]),                                            # "aa"
    ([[3, 4, 5], [6]], 1, [(0, 0, 3), (0, 7, 1)]),
    ([[i % 28 for i in range(100)], [1, 2], [3]], 4, [(0, 0, 100), (0, 204, 2), (0, 212, 1)]),   # 51 lanes, then 5 states on 2 lanes, 3 on 1
])
def test_the_packed_layout(keywords, kpl, places):
  C = 29
  plan, nw = SC.make_plan(keywords, C, 1)
  desc, end_kw, got_places, got_kpl = _states(plan)
  assert got_kpl == kpl and got_places == places and nw == max(p[0] for p in places) + 1
  live_seen = [np.zeros(kpl * 64, bool) for _ in range(nw)]
  for k, (kw, (w, g0, L)) in enumerate(zip(keywords, places)):
    assert g0 % kpl == 0 and g0 + 2 * L + 1 <= kpl * 64
    d = desc[w][g0:g0 + 2 * L + 1]
    assert d[0] == C - 1 and d[-1] == C - 1                                # the two dead outer states
    for u in range(1, 2 * L):
      cls = kw[u // 2] if u & 1 else C - 1
      skip = bool(u & 1) and u >= 3 and kw[u // 2] != kw[u // 2 - 1]
      assert d[u] == cls | 64 | (32 if skip else 0) | (128 if u == 1 else 0) | (256 if u == 2 * L - 1 else 0), (k, u)
    live_seen[w][g0:g0 + 2 * L + 1] = True
    assert end_kw[w][(g0 + 2 * L - 1) // kpl] == k
  for w in range(nw):
    assert (desc[w][~live_seen[w]] == C - 1).all()                          # padding is dead
    assert sorted(end_kw[w][end_kw[w] >= 0].tolist()) == [k for k, p in enumerate(places) if p[0] == w]
  unpacked, nw0 = SC.make_plan(keywords, C, 0)
  assert nw0 == len(keywords) and all(p[:2] == (k, 0) for k, p in enumerate(SC.layout(unpacked)[0]))


def test_step_validation_on_the_host():
  r = SC.Runner(KW5, 5, 1, -0.69, 2)
  x = SC.noise(4, 5, 1)
  r.step({0: (x, -1, True)}, threshold=float('nan'), want=-1)
  r.step({0: (x, -1, True)}, threshold=0.5, want=-1)
  r.step({0: (x, -1, True)}, hold=0, want=-1)
  bad = r.plan.copy()
  good, r.plan = r.plan, bad
  bad[0] ^= 1
  r.step({0: (x, -1, True)}, want=-1)
  bad[0] ^= 1
  bad[4] = 7                                                              # a KPL no lattice has
  r.step({0: (x, -1, True)}, want=-1)
  r.plan = good
  other = SC.Runner(KW5, 6, 1, -0.69, 2)
  other.C = 5
  other.step({0: (x, -1, True)}, want=-1)                                  # a plan for other classes
  assert r.step({0: (x, -1, True)})[0][1] >= 0
