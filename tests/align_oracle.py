"""Float64 specification of the forced alignment (st_ctc_align_f32 / st_ctc_align_host; include/speecht_hip.h).

The best-path (Viterbi) CTC alignment of ``labels`` against ``logits`` [T, C], blank = C-1.  The lattice has U = 2L+1 states,
even states are blanks, odd state u is label (u-1)//2.  A path gives every frame one state; it

  * starts in state 0 or 1 and ends in state U-1 or U-2,
  * moves by 0 (stay), 1 (advance) or 2 (skip) states per frame, the skip only between DIFFERENT labels,
  * and maximises sum_t ln softmax(logits[t])[class of the state at t].

Ties go to the smaller move: stay, then advance, then skip (decided at the later frame over the best scores of the three
predecessors); a tie at the end goes to the last label state.  L = 0 is valid: every frame is blank and there are no spans.
A label does not fit when T < L + (adjacent repeats).

``states`` [T] holds the label index of each frame, -1 for a blank; ``spans`` [L, 2] the first frame and one past the last
frame spent in each label's state.
"""
import numpy as np


def log_softmax64(logits):
  x = np.asarray(logits, dtype=np.float64)
  m = x.max(axis=-1, keepdims=True)
  return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def min_frames(labels):
  labels = list(labels)
  return len(labels) + sum(labels[i] == labels[i - 1] for i in range(1, len(labels)))


def spans_from_states(states, n_labels):
  """[L, 2] first frame / one past the last frame of each label index in ``states`` (-1, -1 for an index that is absent)."""
  spans = np.full((n_labels, 2), -1, dtype=np.int64)
  for t, s in enumerate(states):
    if s >= 0:
      if spans[s, 0] < 0:
        spans[s, 0] = t
      spans[s, 1] = t + 1
  return spans


def align64(logits, labels, dtype=np.float64):
  """-> (states [T], spans [L, 2], score), or None when the label does not fit.  ``dtype``: the number format the lattice
  (log-softmax rows and running scores) is kept in; float64 is the specification, float32 shows what an fp32 lattice gives."""
  labels = [int(l) for l in labels]
  ly = log_softmax64(logits).astype(dtype)
  T, C = ly.shape
  L, blank = len(labels), C - 1
  U = 2 * L + 1
  if T < min_frames(labels):
    return None
  if T == 0:
    return np.zeros(0, dtype=np.int64), np.zeros((0, 2), dtype=np.int64), 0.0
  cls = np.array([labels[u // 2] if u & 1 else blank for u in range(U)])
  skip_ok = np.array([bool(u & 1) and u >= 3 and labels[u // 2] != labels[u // 2 - 1] for u in range(U)])
  ninf = dtype(-np.inf)
  v = np.full(U, ninf, dtype=dtype)
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
    v = (best + ly[t, cls]).astype(dtype)
    bp[t] = move
  u = U - 2 if U > 1 and v[U - 2] >= v[U - 1] else U - 1
  score = float(v[u])
  states = np.empty(T, dtype=np.int64)
  for t in range(T - 1, -1, -1):
    states[t] = u // 2 if u & 1 else -1
    u -= int(bp[t, u])
  return states, spans_from_states(states, L), score


def path_score64(logits, states, labels):
  """sum_t ln softmax(logits[t])[class of states[t]] in float64 (``states``: label indices, -1 = blank)."""
  ly = log_softmax64(logits)
  blank = ly.shape[1] - 1
  cls = [labels[s] if s >= 0 else blank for s in states]
  return float(ly[np.arange(len(cls)), cls].sum()) if len(cls) else 0.0


def is_valid_alignment(states, labels):
  """Whether ``states`` (label indices, -1 = blank) is a CTC alignment of ``labels``: the indices 0 .. L-1 appear in order,
  each as one run, and two equal neighbouring labels have a blank between their runs."""
  labels = list(labels)
  runs = []            # (label index, preceded by a blank)
  prev = None
  for s in states:
    s = int(s)
    if s < -1 or s >= len(labels):
      return False
    if s >= 0 and s != prev:
      runs.append((s, prev == -1))
    prev = s
  if [r[0] for r in runs] != list(range(len(labels))):
    return False
  return all(after_blank or k == 0 or labels[k] != labels[k - 1] for k, after_blank in runs)


def accuracy_ratios(logits, labels, states, score, s_star):
  """The two sides of the accuracy condition as (ratio of path loss to its bound, ratio of score error to its bound):
       S* - path_score64(P)        <= 2 T 2^-24 |S*|
       |score - path_score64(P)|   <= T 2^-24 |S*| + 2^-23 |S*|
  both ratios must be <= 1 (a zero bound with a zero left side counts as 0)."""
  T = len(states)
  p = path_score64(logits, states, labels)
  b1 = 2.0 * T * 2.0 ** -24 * abs(s_star)
  b2 = T * 2.0 ** -24 * abs(s_star) + 2.0 ** -23 * abs(s_star)
  ratio = lambda x, b: 0.0 if x <= 0.0 else (x / b if b > 0.0 else np.inf)
  return ratio(s_star - p, b1), ratio(abs(score - p), b2)


def states_from_classes(classes, blank):
  """Label indices (-1 = blank) of a per-frame class sequence, and the label sequence it collapses to."""
  states, labels, prev = [], [], None
  for c in classes:
    if c == blank:
      states.append(-1)
    else:
      if c != prev:
        labels.append(int(c))
      states.append(len(labels) - 1)
    prev = c
  return states, labels


def random_alignment(rng, labels, T):
  """A random valid alignment of ``labels`` over T >= min_frames(labels) frames -> per-frame lattice states u."""
  labels = list(labels)
  L = len(labels)
  # mandatory units: each label one frame, a blank between equal neighbours; the spare frames go to random runs
  units = []
  for k in range(L):
    if k > 0 and labels[k] == labels[k - 1]:
      units.append(2 * k)
    units.append(2 * k + 1)
  optional = [u for u in range(0, 2 * L + 1, 2) if u not in units]
  spare = T - len(units)
  assert spare >= 0
  chosen = sorted(set(units) | {u for u in optional if rng.random() < 0.5}) if spare else sorted(units)
  while len(chosen) > T:                          # too many optional blanks: drop some
    drop = [u for u in chosen if u not in units]
    chosen.remove(drop[int(rng.integers(len(drop)))])
  if not chosen:
    chosen = [0]
  extra = rng.multinomial(T - len(chosen), np.ones(len(chosen)) / len(chosen))
  out = []
  for u, e in zip(chosen, extra):
    out += [u] * (1 + int(e))
  return out


def random_labels(rng, L, C, repeat_prob=0.3):
  """L ids in [0, C-1) with adjacent repeats drawn at ``repeat_prob`` (C = 2 has one label class: all repeats)."""
  out = []
  for k in range(L):
    if k and rng.random() < repeat_prob:
      out.append(out[-1])
    else:
      out.append(int(rng.integers(C - 1)))
  return out


def random_logits(rng, T, C, scale=3.0):
  return (rng.standard_normal((T, C)) * scale).astype(np.float32)


def planted_logits(rng, labels, T, C, boost=8.0):
  """N(0, 1) noise with ``boost`` added to the class of a random valid alignment on every frame -> (logits, lattice states)."""
  path = random_alignment(rng, labels, T)
  x = rng.standard_normal((T, C)).astype(np.float32)
  for t, u in enumerate(path):
    x[t, labels[u // 2] if u & 1 else C - 1] += np.float32(boost)
  return x, path


def pad_batch(logit_list, frames=None):
  """Utterances [T_b, C] -> (dense [B, frames, C] float32 zero beyond each utterance's frames, seq_lens)."""
  frames = frames or max(max(x.shape[0] for x in logit_list), 1)
  C = logit_list[0].shape[1]
  out = np.zeros((len(logit_list), frames, C), dtype=np.float32)
  for b, x in enumerate(logit_list):
    out[b, :x.shape[0]] = x
  return out, np.array([x.shape[0] for x in logit_list], dtype=np.int32)
