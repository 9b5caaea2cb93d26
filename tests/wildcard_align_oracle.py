"""Float64 specification of the forced alignment with a wildcard label and of the per-label fit (st_ctc_align_wild_f32 /
st_ctc_align_long_wild_f32 and their host forms; include/speecht_hip.h).  It builds on tests/align_oracle.py: the lattice, the
moves, the ties (stay, advance, skip), the end rule, the score and the spans are the ones specified there.

The wildcard W.  ``labels`` may hold, besides ids in [0, C-1), the id ``wild_id(C)`` = C, one past the blank.  W is a label
state like any other: it occupies at least one frame, counts as one label in the fit rule T >= L + adjacent repeats, and its
class differs from every id, so the skip over the blank into it and out of it is allowed.  Its emission at frame t is the
largest of the row's C log-softmax values -- the blank included -- plus ``bias``:  ly_t(W) = max_c ly_t(c) + bias, with a
finite bias <= 0.  Two adjacent wildcards are refused as a bad argument (ValueError).  The span of a wildcard is the stretch
of audio the transcript leaves out.

The fit.  The best path gives label k of class c_k the frames [a, b);  fit_k = sum_{t = a .. b-1} ly_t(c_k) - max_c ly_t(c):
0 exactly where the greedy reading spells the label on every one of its frames, negative otherwise.  For a wildcard it is
bias * (b - a), one product.  Blank frames belong to no label.
"""
import numpy as np

from tests import align_oracle as AO


def wild_id(C):
  return int(C)


def check_labels(labels, C, bias):
  labels = [int(l) for l in labels]
  W = wild_id(C)
  if not (np.isfinite(bias) and bias <= 0.0):
    raise ValueError('the wildcard bias must be finite and <= 0')
  if any(not (0 <= l < C - 1 or l == W) for l in labels):
    raise ValueError('label ids must lie in [0, C-1) or be the wildcard')
  if any(a == W and b == W for a, b in zip(labels, labels[1:])):
    raise ValueError('two adjacent wildcards')
  return labels


def emissions64(logits, bias):
  """[T, C+1]: the log-softmax rows of align_oracle, and in column C the wildcard's emission."""
  ly = AO.log_softmax64(logits)
  return np.concatenate([ly, ly.max(axis=1, keepdims=True) + np.float64(bias)], axis=1)


def align_wild64(logits, labels, bias):
  """-> (states [T], spans [L, 2], score), or None when the label does not fit: align_oracle.align64 on the emissions above."""
  T, C = np.asarray(logits).shape
  labels = check_labels(labels, C, bias)
  ly = emissions64(logits, bias)
  L, blank = len(labels), C - 1
  U = 2 * L + 1
  if T < AO.min_frames(labels):
    return None
  if T == 0:
    return np.zeros(0, dtype=np.int64), np.zeros((0, 2), dtype=np.int64), 0.0
  cls = np.array([labels[u // 2] if u & 1 else blank for u in range(U)])
  skip_ok = np.array([bool(u & 1) and u >= 3 and labels[u // 2] != labels[u // 2 - 1] for u in range(U)])
  ninf = -np.inf
  v = np.full(U, ninf)
  v[:2] = ly[0, cls[:2]]
  bp = np.zeros((T, U), dtype=np.int8)
  for t in range(1, T):
    adv = np.concatenate(([ninf], v[:-1]))
    skp = np.where(skip_ok, np.concatenate(([ninf, ninf], v[:-2]))[:U], ninf)
    best, move = v.copy(), np.zeros(U, dtype=np.int8)
    take = adv > best
    best[take], move[take] = adv[take], 1
    take = skp > best
    best[take], move[take] = skp[take], 2
    v = best + ly[t, cls]
    bp[t] = move
  u = U - 2 if U > 1 and v[U - 2] >= v[U - 1] else U - 1
  score = float(v[u])
  states = np.empty(T, dtype=np.int64)
  for t in range(T - 1, -1, -1):
    states[t] = u // 2 if u & 1 else -1
    u -= int(bp[t, u])
  return states, AO.spans_from_states(states, L), score


def path_score_wild64(logits, states, labels, bias):
  """sum_t of the emission of the class of states[t] (label indices, -1 = blank), the wildcard's included."""
  ly = emissions64(logits, bias)
  blank = ly.shape[1] - 2
  cls = [labels[s] if s >= 0 else blank for s in states]
  return float(ly[np.arange(len(cls)), cls].sum()) if len(cls) else 0.0


def fit64(logits, labels, spans, bias):
  """[L] float64: the fit of every label on the path given by ``spans``."""
  ly = AO.log_softmax64(logits)
  C = ly.shape[1]
  gap = ly - ly.max(axis=1, keepdims=True)
  out = np.zeros(len(labels))
  for k, (c, (a, b)) in enumerate(zip(labels, np.asarray(spans))):
    out[k] = np.float64(bias) * float(b - a) if c == wild_id(C) else gap[a:b, c].sum()
  return out


def brute_force(logits, labels, bias):
  """The best alignment by enumeration of every monotone state sequence (tiny lattices only) -> (score, number of state
  sequences that reach it), or None when there is none."""
  T, C = np.asarray(logits).shape
  labels = check_labels(labels, C, bias)
  ly = emissions64(logits, bias)
  L, blank = len(labels), C - 1
  U = 2 * L + 1
  cls = [labels[u // 2] if u & 1 else blank for u in range(U)]
  skip_ok = [bool(u & 1) and u >= 3 and labels[u // 2] != labels[u // 2 - 1] for u in range(U)]
  best, count = None, 0

  def walk(t, u, s):
    nonlocal best, count
    s = s + ly[t, cls[u]]
    if t == T - 1:
      if u >= U - 2:
        if best is None or s > best + 1e-12 * max(abs(best), 1.0):
          best, count = s, 1
        elif abs(s - best) <= 1e-12 * max(abs(best), 1.0):
          count += 1
      return
    for d in (0, 1, 2):
      n = u + d
      if n < U and (d < 2 or skip_ok[n]):
        walk(t + 1, n, s)

  if T == 0:
    return (0.0, 1) if L == 0 else None
  for u0 in range(min(2, U)):
    walk(0, u0, 0.0)
  return None if best is None else (float(best), count)


def planted_gap_case(rng, C=29, part_labels=12, part_frames=40, gap_labels=15, gap_frames=50, boost=8.0):
  """The experiment of the wildcard's purpose: ``part_labels`` labels over ``part_frames`` frames, then ``gap_frames`` frames
  spelling ``gap_labels`` OTHER labels the transcript leaves out, then a second transcribed part.
  -> (logits [T, C], labels of part 1, labels of part 2, first frame of the left-out stretch, one past its last)."""
  lab1, lab2 = AO.random_labels(rng, part_labels, C), AO.random_labels(rng, part_labels, C)
  mid = AO.random_labels(rng, gap_labels, C)
  x1, _ = AO.planted_logits(rng, lab1, part_frames, C, boost)
  xm, _ = AO.planted_logits(rng, mid, gap_frames, C, boost)
  x2, _ = AO.planted_logits(rng, lab2, part_frames, C, boost)
  return np.concatenate([x1, xm, x2]), lab1, lab2, part_frames, part_frames + gap_frames
