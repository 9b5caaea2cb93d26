"""Float64 specification of keyword spotting (st_ctc_spot_f32 / st_ctc_spot_host; include/speecht_hip.h).

One utterance ``logits`` [T, C], blank = C-1, one keyword k of L >= 1 ids in 0 .. C-2.  Per frame
d_t(c) = float64(x_t(c)) - float64(max_c x_t(c)): <= 0, exactly 0 for the greedy class, the log of the ratio between the
class's softmax probability and the greedy class's (the normaliser cancels: no exp, no log).

An OCCURRENCE over frames [s, e) is a frame path that is a CTC alignment of k which begins on k_0 and ends on k_{L-1}: no
leading or trailing blank, blanks optional between labels and compulsory between equal neighbours, repeats collapse.  Its score
is the sum of d_t(class at t).  The spot score is the maximum over all s < e <= T and all such paths (`enumerate_spot` is this
definition, literally); `spot64` is the recursion that computes it:

  v_t(u) = best + d_t(class(u)) for the states u = 1 .. 2L-1 of the 2L+1 CTC states (0 and 2L are dead), v_{-1} = -inf,
  best over -- in this order, replaced only by a strictly larger value -- stay v_{t-1}(u), advance v_{t-1}(u-1), skip
  v_{t-1}(u-2) (a label that differs from the previous label) and, for u = 1, enter = 0.0 with start t;
  s_t(u) = the start of the predecessor taken (t for enter, -1 when best is -inf);  end_t = v_t(2L-1) with start s_t(2L-1).

The answer is the largest finite end_t, the LATEST t among equals: score = end_t, span = (s_t(2L-1), t+1); without a finite
end_t it is -inf and (-1, -1).  Every operation is one IEEE double addition or comparison in a fixed order, so an
implementation that follows the recursion returns these very bits.

`pick_hits` is the specification of `speecht_amd.spotting.pick_hits`: several hits from the trace (end_t and its start for
every frame)."""
import itertools

import numpy as np


def ratio64(logits):
  x = np.asarray(logits, dtype=np.float32).astype(np.float64)
  return x - x.max(axis=-1, keepdims=True) if x.shape[0] else x


def min_frames(keyword):
  keyword = list(keyword)
  return len(keyword) + sum(keyword[i] == keyword[i - 1] for i in range(1, len(keyword)))


def spot64(logits, keyword):
  """-> dict(score, span (start, end), trace_score [T] float64, trace_start [T] int32)."""
  kw = [int(k) for k in keyword]
  d = ratio64(logits)
  T, C = d.shape
  L, blank = len(kw), C - 1
  assert L >= 1
  U = 2 * L + 1
  cls = np.array([kw[u // 2] if u & 1 else blank for u in range(U)])
  skip_ok = np.array([bool(u & 1) and u >= 3 and kw[u // 2] != kw[u // 2 - 1] for u in range(U)])
  live = np.array([1 <= u <= 2 * L - 1 for u in range(U)])
  ninf = -np.inf
  v = np.full(U, ninf)
  s = np.full(U, -1, dtype=np.int64)
  trace_score = np.full(T, ninf)
  trace_start = np.full(T, -1, dtype=np.int32)
  best_score, best_span = ninf, (-1, -1)
  with np.errstate(invalid='ignore'):
    for t in range(T):
      best, start = v.copy(), s.copy()
      adv, adv_s = np.concatenate(([ninf], v[:-1])), np.concatenate(([-1], s[:-1]))
      take = adv > best
      best[take], start[take] = adv[take], adv_s[take]
      skp, skp_s = np.concatenate(([ninf, ninf], v[:-2])), np.concatenate(([-1, -1], s[:-2]))
      take = skip_ok & (skp > best)
      best[take], start[take] = skp[take], skp_s[take]
      if 0.0 > best[1]:
        best[1], start[1] = 0.0, t
      start[best == ninf] = -1
      v = np.where(live, best + d[t, cls], ninf)
      s = np.where(live, start, -1)
      end, end_start = float(v[U - 2]), int(s[U - 2])
      trace_score[t], trace_start[t] = end, end_start
      if end > ninf and end >= best_score:
        best_score, best_span = end, (end_start, t + 1)
  return dict(score=best_score, span=best_span, trace_score=trace_score, trace_start=trace_start)


def is_occurrence(classes, keyword, blank):
  """Whether the per-frame ``classes`` are a CTC alignment of ``keyword`` that begins and ends on a label."""
  classes = [int(c) for c in classes]
  if not classes or classes[0] == blank or classes[-1] == blank:
    return False
  merged = [c for i, c in enumerate(classes) if i == 0 or c != classes[i - 1]]
  return [c for c in merged if c != blank] == [int(k) for k in keyword]


def enumerate_spot(logits, keyword):
  """The definition: every class sequence over every [s, e) -> (best score, best score of the occurrences that end at each frame
  [T]); -inf where there is none.  For tiny T and C only."""
  d = ratio64(logits)
  T, C = d.shape
  ends = np.full(T, -np.inf)
  for s in range(T):
    for e in range(s + 1, T + 1):
      for path in itertools.product(range(C), repeat=e - s):
        if is_occurrence(path, keyword, C - 1):
          ends[e - 1] = max(ends[e - 1], float(sum(d[s + i, c] for i, c in enumerate(path))))
  return (float(ends.max()) if T else -np.inf), ends


def greedy_spells_tightly(logits, keyword):
  """Whether, on some [s, e), a choice of one maximal class per frame is an occurrence of the keyword."""
  d = ratio64(logits)
  T, C = d.shape
  tops = [np.flatnonzero(d[t] == 0.0).tolist() for t in range(T)]
  for s in range(T):
    for e in range(s + 1, T + 1):
      if any(is_occurrence(path, keyword, C - 1) for path in itertools.product(*tops[s:e])):
        return True
  return False


def pick_hits(trace_score, trace_start, threshold):
  """Non-overlapping hits from one (utterance, keyword) trace -> [(start, end, score)] in order of acceptance: the candidates are
  the frames with a finite end_t, by score descending, then end descending; a candidate is a hit if its [start, end) overlaps
  no accepted hit and score / (end - start) >= threshold."""
  cands = [(float(v), t + 1, int(trace_start[t])) for t, v in enumerate(trace_score) if np.isfinite(v)]
  cands.sort(key=lambda c: (-c[0], -c[1]))
  hits = []
  for score, end, start in cands:
    if all(end <= a or start >= b for a, b, _ in hits) and score / (end - start) >= threshold:
      hits.append((start, end, score))
  return hits


def spot_batch(logits, seq_lens, keywords, jobs, dispatch_len=None):
  """What the entry points return for a dense [B, T, C] batch and a job table [(utterance, keyword)] ->
  (score [n], span [n, 2], status [n], trace_score [n, T], trace_start [n, T]).  ``dispatch_len``: max_keyword_len of the call
  (the keywords beyond the lattice it picks are refused); default: the longest keyword."""
  B, T, _ = logits.shape
  n = len(jobs)
  score, span, status = np.full(n, -np.inf), np.full((n, 2), -1, dtype=np.int32), np.zeros(n, dtype=np.int32)
  trace_score, trace_start = np.full((n, T), -np.inf), np.full((n, T), -1, dtype=np.int32)
  longest = max([len(k) for k in keywords] + [1]) if dispatch_len is None else dispatch_len
  states = next(k * 64 for k in (1, 2, 3, 4, 5, 6, 8, 10, 12, 16) if k * 64 >= 2 * longest + 1)
  for i, (b, k) in enumerate(jobs):
    ok = 0 <= b < B and 0 <= k < len(keywords)
    ok = ok and 1 <= len(keywords[k]) and 2 * len(keywords[k]) + 1 <= states and 0 <= seq_lens[b] <= T
    if not ok:
      status[i] = 1
      continue
    Tb = int(seq_lens[b])
    r = spot64(logits[b, :Tb], keywords[k])
    score[i], span[i] = r['score'], r['span']
    trace_score[i, :Tb], trace_start[i, :Tb] = r['trace_score'], r['trace_start']
  return score, span, status, trace_score, trace_start
