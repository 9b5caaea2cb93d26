"""Inputs and harnesses shared by the tests of keyword spotting in live streams (test_spot_stream_cpu.py, test_gpu_spot_stream.py):
synthetic logits with planted readings, plans through the C ABI, and a runner that feeds streams in steps -- on host memory through
st_ctc_spot_stream_host, or, given a torch device, on device memory through st_ctc_spot_stream_step.  Both runners put guard words
around the state, the events and the counts, start every buffer as garbage and hold poison in the pitch columns of the logits."""
import ctypes

import numpy as np

GUARD = 0x5A5A5A5A
PITCH_EXTRA = 3                        # columns beyond the classes, full of NaN


def lib():
  from speecht_amd import _lib
  return _lib.load()


def csr(keywords):
  ids = np.asarray([i for k in keywords for i in k] + [0], dtype=np.int32)       # (never empty: ctypes wants a pointer)
  offs = np.cumsum([0] + [len(k) for k in keywords]).astype(np.int32)
  return ids, offs


def _p(a):
  return a.ctypes.data_as(ctypes.c_void_p)


def make_plan(keywords, C, pack, offsets=None):
  """-> (plan int32 array, n_waves) or None when the plan functions refuse (both must)."""
  ids, offs = csr(keywords)
  if offsets is not None:
    offs = np.asarray(offsets, dtype=np.int32)
  n = len(offs) - 1
  size = int(lib().st_ctc_spot_stream_plan_bytes(_p(ids), _p(offs), n, C, pack))
  plan = np.zeros(max(size // 4, 1 << 12), dtype=np.int32)
  nw = ctypes.c_int(-1)
  code = lib().st_ctc_spot_stream_plan(_p(ids), _p(offs), n, C, pack, _p(plan), ctypes.byref(nw))
  assert (code == 0) == (size > 0), (code, size)
  if code != 0:
    return None
  assert size % 4 == 0 and plan[1] * 4 == size and not plan[size // 4:].any()
  return plan[:size // 4].copy(), nw.value


def layout(plan):
  """The places of the keywords a plan holds: [(wave, first state, L)], KPL, n_waves."""
  kpl, nw, nk, at = int(plan[4]), int(plan[5]), int(plan[2]), int(plan[7])
  return [tuple(int(v) for v in plan[at + 4 * k:at + 4 * k + 3]) for k in range(nk)], kpl, nw


def noise(T, C, seed, scale=3.0):
  rng = np.random.RandomState(seed)
  return (rng.standard_normal((T, C)) * scale).astype(np.float32)


def plant(x, at, keyword, blank, height=30.0, stay=1):
  """Make the arg-max of rows at .. spell ``keyword`` tightly (``stay`` rows per label, a blank between equal neighbours);
  returns the row behind the reading."""
  t = at
  for i, k in enumerate(keyword):
    if i and keyword[i - 1] == k:
      x[t, blank] = height
      t += 1
    for _ in range(stay):
      x[t, k] = height
      t += 1
  return t


class Runner:
  """S streams in steps.  ``step({stream: (rows [n, C], limit or -1, reset)})`` -> {stream: (events as a set, count)}; streams it
  does not name sit the step out.  ``device``: a torch device for st_ctc_spot_stream_step, None for st_ctc_spot_stream_host."""

  def __init__(self, keywords, C, S, threshold, hold, pack=1, max_events=16, device=None):
    self.C, self.S, self.max_events, self.device = C, S, max_events, device
    self.threshold, self.hold = float(threshold), int(hold)
    self.plan, self.n_waves = make_plan(keywords, C, pack)
    self.state_bytes = int(lib().st_ctc_spot_stream_state_bytes(_p(self.plan)))
    assert self.state_bytes > 0 and self.state_bytes % 8 == 0
    self.frames = np.zeros(S, dtype=np.int64)
    rng = np.random.RandomState(5)
    # [guard 16 | payload | guard 16] int32 words each, payloads garbage
    self.state = self._guarded(S * self.state_bytes // 4, rng)
    self.events = self._guarded(S * max_events * 8, rng)
    self.counts = self._guarded(S, rng)
    if device is not None:
      import torch
      self.torch = torch
      self.d_state, self.d_events, self.d_counts = (torch.from_numpy(a.copy()).to(device) for a in (self.state, self.events, self.counts))
      self.d_plan = torch.from_numpy(self.plan).to(device)
      assert lib().st_ctc_spot_stream_plan_bind(_p(self.plan), ctypes.c_void_p(self.d_plan.data_ptr())) == 0

  @staticmethod
  def _guarded(words, rng):
    a = rng.randint(-2 ** 31, 2 ** 31 - 1, size=words + 32, dtype=np.int64).astype(np.int32)
    a[:16] = a[-16:] = GUARD
    return a

  def tables(self, feeds):
    """-> logits [n_rows, pitch] (NaN beyond the classes), rows [n_rows, 2], table [S, 4]."""
    pitch = self.C + PITCH_EXTRA
    table = np.zeros((self.S, 4), dtype=np.int32)
    table[:, 2] = -1
    blocks, rows, at = [], [], 0
    for s in sorted(feeds):
      x, limit, reset = feeds[s]
      x = np.asarray(x, dtype=np.float32).reshape(-1, self.C)
      if reset:
        self.frames[s] = 0
      table[s] = (at, len(x), limit, int(bool(reset)))
      block = np.full((len(x), pitch), np.nan, dtype=np.float32)
      block[:, :self.C] = x
      blocks.append(block)
      rows += [(s, self.frames[s] + i) for i in range(len(x))]
      at += len(x)
      self.frames[s] += len(x)
    logits = np.concatenate(blocks) if blocks else np.zeros((0, pitch), np.float32)
    if not len(logits):
      logits = np.full((1, pitch), np.nan, dtype=np.float32)                  # (a pointer that is not null)
      n_rows = 0
    else:
      n_rows = len(logits)
    rows = np.asarray(rows + [(0, 0)], dtype=np.int32)
    return np.ascontiguousarray(logits), rows, table, n_rows, pitch

  def step(self, feeds, threshold=None, hold=None, want=0):
    logits, rows, table, n_rows, pitch = self.tables(feeds)
    thr = ctypes.c_double(self.threshold if threshold is None else threshold)
    hold = self.hold if hold is None else hold
    if self.device is None:
      code = lib().st_ctc_spot_stream_host(_p(logits), pitch, self.C, _p(rows), _p(table), n_rows, self.S, _p(self.plan), thr, hold,
                                           _p(self.state[16:]), _p(self.events[16:]), self.max_events, _p(self.counts[16:]))
      state, events, counts = self.state, self.events, self.counts
    else:
      torch = self.torch
      d = lambda a: torch.from_numpy(a).to(self.device)
      d_logits, d_rows, d_table = d(logits), d(rows), d(table)
      at = lambda t: ctypes.c_void_p(t.data_ptr() + 64)
      stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
      code = lib().st_ctc_spot_stream_step(ctypes.c_void_p(d_logits.data_ptr()), pitch, self.C, ctypes.c_void_p(d_rows.data_ptr()),
                                           ctypes.c_void_p(d_table.data_ptr()), n_rows, self.S, _p(self.plan), thr, hold, at(self.d_state),
                                           at(self.d_events), self.max_events, at(self.d_counts), stream)
      state, events, counts = (t.cpu().numpy() for t in (self.d_state, self.d_events, self.d_counts))
      self.state = state
    assert code == want, (code, lib().st_last_error().decode())
    for a in (state, events, counts):
      assert (a[:16] == GUARD).all() and (a[-16:] == GUARD).all()
    if code != 0:
      return None
    counts = counts[16:-16]
    events = events[16:-16].reshape(self.S, self.max_events, 8)
    out = {}
    for s in range(self.S):
      kept = events[s, :min(int(counts[s]), self.max_events)]
      assert not kept[:, 6:].any() and np.isin(kept[:, 3], (0, 1)).all()
      out[s] = ({(int(e[0]), int(e[1]), int(e[2]), int(e[3]), int(e[4:6].copy().view(np.int64)[0])) for e in kept}, int(counts[s]))
      assert len(out[s][0]) == len(kept)
    self.last_events = events.copy()
    return out

  def state_words(self):
    return self.state[16:-16].copy()


def feed_in_cuts(runner, streams, cuts, finish=True):
  """``streams``: {s: logits [T, C]}; every stream is fed in pieces of the sizes ``cuts`` cycles through (all streams the same
  sizes), reset on its first step and, with ``finish``, finished by a last step without rows.  -> {s: set of all events}."""
  got = {s: set() for s in streams}
  T = max(len(x) for x in streams.values())
  at, i = 0, 0
  first = True
  while at < T:
    n = cuts[i % len(cuts)]
    feeds = {s: (x[at:at + n], -1, first) for s, x in streams.items() if at < len(x) or first}
    for s, (ev, count) in runner.step(feeds).items():
      assert count == len(ev)
      if s in got:
        assert not (got[s] & ev)
        got[s] |= ev
      else:
        assert count == 0
    at, i, first = at + n, i + 1, False
  if finish:
    for s, (ev, count) in runner.step({s: (np.zeros((0, runner.C), np.float32), len(x), False) for s, x in streams.items()}).items():
      assert count == len(ev)
      if s in got:
        got[s] |= ev
  return got
