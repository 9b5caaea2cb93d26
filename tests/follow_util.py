"""Drives st_ctc_follow_stream_host (numpy buffers) or st_ctc_follow_stream_step (torch buffers on a device) step by step, with the
tables a recogniser would build: what tests/test_follow_host.py and tests/test_gpu_follow.py share."""
import ctypes

import numpy as np

from speecht_amd import _lib

FILL = 0xA5          # what a state holds before its first step: any content


class Driver:
  """``scripts``: per slot a list of ids ([]: the slot is not followed), ``starts``: per slot the word starts.  `step` feeds rows and
  returns per slot what the entry point left; `state_bytes(slot)` the slot's state."""

  def __init__(self, scripts, starts, C, max_labels, confirm, max_events=64, max_rows=256, device=None, state_labels=None):
    self.lib = _lib.load()
    self.S, self.C, self.K, self.max_events, self.max_rows, self.max_labels = len(scripts), C, confirm, max_events, max_rows, max_labels
    self.device = device
    self.scripts = scripts
    ids = np.asarray([i for s in scripts for i in s] + [0], dtype=np.int32)
    offs = np.cumsum([0] + [len(s) for s in scripts]).astype(np.int32)
    ws = np.asarray([i for s in starts for i in s] + [0], dtype=np.int32)
    woffs = np.cumsum([0] + [len(s) for s in starts]).astype(np.int32)
    self.sb = int(self.lib.st_ctc_follow_stream_state_bytes(state_labels or max_labels))
    self.wsb = int(self.lib.st_ctc_follow_stream_ws(max_rows, max_labels, self.S))
    assert self.sb and self.wsb
    self.tables = [self._put(a) for a in (ids, offs, ws, woffs)]
    self.state = self._put(np.full(self.S * self.sb, FILL, dtype=np.uint8))
    self.work = self._put(np.zeros(self.wsb, dtype=np.uint8))
    self.frames = [0] * self.S
    self.fresh = [True] * self.S

  def _put(self, a):
    if self.device is None:
      return a
    import torch
    return torch.from_numpy(a).to(self.device)

  def _ptr(self, a):
    if a is None:
      return None
    return ctypes.c_void_p(a.ctypes.data if self.device is None else a.data_ptr())

  def _get(self, a):
    return a if self.device is None else a.cpu().numpy()

  def reopen(self, slot):
    self.frames[slot], self.fresh[slot] = 0, True

  def step(self, feeds, limits=None, max_stream_rows=None, pitch=None, guard=0):
    """``feeds``: {slot: rows [n, C]}; ``limits``: {slot: limit}.  -> {slot: dict(record, events, lost, trace)} for every slot."""
    limits = limits or {}
    C, S = self.C, self.S
    pitch = pitch or C
    named = sorted(feeds)
    table = np.zeros((S, 4), dtype=np.int32)
    table[:, 2] = -1
    rows, chunks, at = [], [], 0
    for s in named:
      x = np.asarray(feeds[s], dtype=np.float32).reshape(-1, C)
      table[s] = (at, len(x), limits.get(s, -1), int(self.fresh[s]))
      rows += [(s, self.frames[s] + i) for i in range(len(x))]
      chunks.append(x)
      at += len(x)
    for s, lim in limits.items():
      if s not in feeds:
        table[s, 2] = lim
    n_rows = at
    logits = np.zeros((max(n_rows, 1), pitch), dtype=np.float32)
    if n_rows:
      logits[:n_rows, :C] = np.concatenate(chunks)
    rows_a = np.asarray(rows + [(0, 0)], dtype=np.int32)
    longest = max([len(c) for c in chunks] + [0]) if max_stream_rows is None else max_stream_rows
    me = self.max_events
    # (guard words behind the events and the trace: nothing may be written there)
    events = np.full(S * me * 2 + guard, -77, dtype=np.int32)
    result = np.full(S * 16, -77, dtype=np.int32)
    trace = np.full(max(n_rows, 1) + guard, -77, dtype=np.int32)
    d = [self._put(a) for a in (logits, rows_a, table, events, result, trace)]
    args = [self._ptr(d[0]), pitch, C, self._ptr(d[1]), self._ptr(d[2]), n_rows, self.max_rows, longest, S] + \
           [self._ptr(t) for t in self.tables] + [self.max_labels, self.K, self._ptr(self.state), self._ptr(d[3]), me, self._ptr(d[4]),
                                                  self._ptr(d[5]), self._ptr(self.work), self.wsb]
    if self.device is None:
      _lib.call('st_ctc_follow_stream_host', *args)
    else:
      import torch
      _lib.call('st_ctc_follow_stream_step', *(args + [ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)]))
    events, result, trace = (self._get(a) for a in d[3:])
    if guard:
      assert (events[S * me * 2:] == -77).all() and (trace[max(n_rows, 1):] == -77).all()
    out = {}
    for s in range(S):
      rec = result[16 * s:16 * s + 16]
      count = int(rec[3])
      ev = events[s * me * 2:(s + 1) * me * 2].reshape(me, 2)[:min(count, me)]
      t0, n = int(table[s, 0]), int(table[s, 1])
      out[s] = dict(record=rec.copy(), events=[tuple(e) for e in ev.tolist()], lost=max(count - me, 0), trace=trace[t0:t0 + n].copy(),
                    frames=int(rec[0]), c=int(rec[1]), status=int(rec[2]), fit=float(rec[4:6].view(np.float64)[0]),
                    end_score=float(rec[6:8].view(np.float64)[0]), words=int(rec[8]))
    for s in named:
      took = len(feeds[s]) if limits.get(s, -1) < 0 else max(min(limits[s] - self.frames[s], len(feeds[s])), 0)
      self.frames[s] += took
      self.fresh[s] = False
    return out

  def state_bytes(self, slot):
    return self._get(self.state)[slot * self.sb:(slot + 1) * self.sb].copy()


def feed(driver, streams, cuts, limits_at_end=False):
  """Feeds ``streams`` {slot: logits [T, C]} in steps whose sizes ``cuts`` {slot: [sizes, cycled]} give, all slots in every step.
  -> {slot: dict(trace [T], events, lost, last: the last step's entry)}."""
  at = {s: 0 for s in streams}
  acc = {s: dict(trace=[], events=[], lost=0, last=None) for s in streams}
  k = 0
  while any(at[s] < len(streams[s]) for s in streams):
    feeds = {}
    for s, x in streams.items():
      if at[s] < len(x):
        n = cuts[s][k % len(cuts[s])]
        feeds[s] = x[at[s]:at[s] + n]
        at[s] += len(feeds[s])
    out = driver.step(feeds)
    for s in feeds:
      acc[s]['trace'] += out[s]['trace'].tolist()
      acc[s]['events'] += out[s]['events']
      acc[s]['lost'] += out[s]['lost']
      acc[s]['last'] = out[s]
    k += 1
  return acc
