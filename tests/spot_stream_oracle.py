"""Float64 specification of keyword spotting in live streams (st_ctc_spot_stream_step / st_ctc_spot_stream_host;
include/speecht_hip.h).

The lattice is `spot_oracle.spot64`'s: its trace gives, for every absolute frame t of the stream, e = end_t and a = s_t(2L-1).  A
(stream, keyword) pair keeps a pending hit or none and ``last_end`` (0 at first).  After frame t:

  1. cand = e > -inf and a >= last_end and e >= threshold * float64(t + 1 - a)        (one IEEE multiply)
  2. pending, cand and a >= pending.end: emit pending, last_end = pending.end, nothing pending
  3. cand and (nothing pending or e >= pending.score): pending = (e, a, t + 1)          (the later frame wins among equals)
  4. pending and t + 1 - pending.end >= hold: emit it, last_end = pending.end, nothing pending

and when the stream finishes what is pending is emitted with kind 1 (flushed).  The rule only ever looks at frames up to t, so the
events a step reports are those whose emitting frame lies among the step's rows: `events_by_frame` names that frame."""
import numpy as np

from tests import spot_oracle


def run_rule(trace_score, trace_start, threshold, hold, finish=True):
  """-> [(start, end, score, kind, frame)]: the hits of one keyword in emission order, ``frame`` the frame whose update emitted the
  hit (the number of frames for a flushed one)."""
  assert hold >= 1 and not np.isnan(threshold) and threshold <= 0
  pending, last_end, out = None, 0, []
  T = len(trace_score)
  for t in range(T):
    e, a = float(trace_score[t]), int(trace_start[t])
    with np.errstate(invalid='ignore'):
      cand = e > -np.inf and a >= last_end and e >= np.float64(threshold) * np.float64(t + 1 - a)
    if pending is not None and cand and a >= pending[1]:
      out.append(pending + (0, t))
      last_end, pending = pending[1], None
    if cand and (pending is None or e >= pending[2]):
      pending = (a, t + 1, e)
    if pending is not None and t + 1 - pending[1] >= hold:
      out.append(pending + (0, t))
      last_end, pending = pending[1], None
  if finish and pending is not None:
    out.append(pending + (1, T))
  return out


def stream_events(logits, keywords, threshold, hold, finish=True):
  """All events of one stream's rows ``logits`` [T, C] -> [(keyword index, start, end, kind, score, frame)]."""
  out = []
  for k, kw in enumerate(keywords):
    r = spot_oracle.spot64(logits, kw)
    out += [(k, a, e, kind, score, frame) for a, e, score, kind, frame in run_rule(r['trace_score'], r['trace_start'], threshold, hold, finish)]
  return out


def as_set(events):
  """Events as the tests compare them: {(keyword, start, end, kind, score bits)}."""
  return {(int(k), int(a), int(e), int(kind), int(np.float64(score).view(np.int64))) for k, a, e, kind, score in events}
