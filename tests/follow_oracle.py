"""Float64 specification of following a known script in a live stream (st_ctc_follow_stream_step / st_ctc_follow_stream_host;
include/speecht_hip.h).

The lattice is the forced alignment's (tests/align_oracle.py) for the script's L ids over the stream's rows, without back-pointers.
After frame t: b_t the best state's value and c_t the LOWEST state attaining it (-1 if none is finite); pos_t = (c_t + 1) >> 1; g_t
the running sum of the rows' largest ln-softmax values and fit_t = b_t - g_t; m_t the minimum of the last K positions (frames before
0 count as 0); word j, beginning at label a_j, is reached at the first frame with m_t >= a_j + 1; end_score_t the value of the end
state, the score `align64` gives the rows 0 .. t.
"""
import numpy as np

from tests import align_oracle


def word_starts(ids, space_id):
  """The first label index of every maximal run of ids other than ``space_id`` (None / -1: no space, one word)."""
  out, inside = [], False
  for i, l in enumerate(ids):
    if space_id is not None and l == space_id:
      inside = False
    elif not inside:
      out.append(i)
      inside = True
  return out


def lattice_columns(logits, labels):
  """-> v [T, U] float64, the whole lattice (row t the column after frame t), and ly [T, C]."""
  labels = [int(l) for l in labels]
  ly = align_oracle.log_softmax64(logits)
  T, C = ly.shape
  L, blank = len(labels), C - 1
  U = 2 * L + 1
  cls = np.array([labels[u // 2] if u & 1 else blank for u in range(U)])
  skip_ok = np.array([bool(u & 1) and u >= 3 and labels[u // 2] != labels[u // 2 - 1] for u in range(U)])
  ninf = -np.inf
  out = np.full((T, U), ninf)
  v = np.full(U, ninf)
  for t in range(T):
    if t == 0:
      v[:2] = ly[0, cls[:2]]
    else:
      adv = np.concatenate(([ninf], v[:-1]))
      skp = np.where(skip_ok, np.concatenate(([ninf, ninf], v[:-2]))[:U], ninf)
      v = np.maximum(np.maximum(v, adv), skp) + ly[t, cls]
    out[t] = v
  return out, ly


class Followed:
  """``c`` [T] the cursor trace, ``pos``, ``m``, ``b``, ``g``, ``fit``, ``end_score`` [T], ``margin`` [T] (best minus second-best
  state value, inf with one finite state), ``events`` [(word, frame)], ``n_reached`` [T] the words reached up to each frame."""


def follow64(logits, labels, starts, confirm):
  v, ly = lattice_columns(logits, labels)
  T, U = v.shape
  r = Followed()
  r.b = v.max(axis=1) if T else np.zeros(0)
  r.c = np.where(np.isfinite(r.b), v.argmax(axis=1), -1) if T else np.zeros(0, dtype=np.int64)     # argmax: the first maximum
  srt = np.sort(v, axis=1)
  with np.errstate(invalid='ignore'):
    r.margin = np.where(np.isfinite(srt[:, -2]), srt[:, -1] - srt[:, -2], np.inf)
  r.pos = np.where(r.c <= 0, 0, (r.c + 1) >> 1)
  r.g = np.zeros(T)
  acc = 0.0
  for t in range(T):
    acc = acc + ly[t].max()
    r.g[t] = acc
  r.fit = r.b - r.g
  padded = np.concatenate((np.zeros(confirm - 1, dtype=np.int64), r.pos))
  r.m = np.array([padded[t:t + confirm].min() for t in range(T)], dtype=np.int64)
  r.events, r.n_reached, nw = [], np.zeros(T, dtype=np.int64), 0
  for t in range(T):
    while nw < len(starts) and r.m[t] >= starts[nw] + 1:
      r.events.append((nw, t))
      nw += 1
    r.n_reached[t] = nw
  end = np.where(v[:, U - 2] >= v[:, U - 1], U - 2, U - 1)
  r.end_score = v[np.arange(T), end]
  return r


def planted_script_logits(rng, labels, C, boost=12.0):
  """One frame per label: N(0, 1) noise with ``boost`` added to label t's class at frame t (a script without adjacent repeats: the
  best path takes a new label every frame, the cursor is 2t + 1)."""
  assert all(labels[i] != labels[i - 1] for i in range(1, len(labels)))
  x = rng.standard_normal((len(labels), C)).astype(np.float32)
  x[np.arange(len(labels)), labels] += np.float32(boost)
  return x


def script_without_repeats(rng, L, C, space_id=None, word_len=5):
  """L ids in [0, C-1) without adjacent repeats; with ``space_id`` a space after every ``word_len`` other ids."""
  out = []
  while len(out) < L:
    if space_id is not None and len(out) % (word_len + 1) == word_len:
      out.append(space_id)
      continue
    l = int(rng.integers(C - 1))
    if l == space_id or (out and l == out[-1]):
      continue
    out.append(l)
  return out
