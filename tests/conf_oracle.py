"""Float64 specification of the CTC word confidences (st_ctc_word_conf_f32 / st_ctc_word_conf_host; include/speecht_hip.h).

``logits`` [T, C], blank = C-1, ``labels`` a list of ids, ``space_id`` the id that separates words, p_t = softmax(logits[t]).

  * The words of a label are its maximal runs of ids other than ``space_id`` (`split_words`).
  * P(l) is the CTC probability of the label: the sum over all alignments.
  * P(l*j): word j's ids are replaced by ONE pseudo-label * and the standard lattice (2L'+1 states, blanks between labels, a
    skip only between different labels) is run with two changes: the * state emits sum_{c != space} p_t(c), the blank
    included, and the two blank states beside * are impossible.  * differs from its neighbours (spaces, or the label's ends).
  * log_prob = ln P(l); log_conf[j] = min(0, ln P(l) - ln P(l*j)); P(l) = 0 gives log_conf = -inf.

Everything here is in log space.  `brute_force` is the definition itself, by enumeration of all C^T frame paths.
"""
import functools

import numpy as np

from tests.align_oracle import log_softmax64, min_frames


def split_words(ids, space_id):
  """-> list of (first, one past last) of the maximal runs of ids other than ``space_id``."""
  out, start = [], None
  for k, i in enumerate(list(ids) + [space_id]):
    if i != space_id:
      if start is None:
        start = k
    elif start is not None:
      out.append((start, k))
      start = None
  return out


def _lse3(a, b, c):
  m = np.maximum(np.maximum(a, b), c)
  ms = np.where(np.isfinite(m), m, 0.0)
  with np.errstate(divide='ignore'):
    return ms + np.log(np.exp(a - ms) + np.exp(b - ms) + np.exp(c - ms))


def _lattices(ly, space_id, jobs, live_blanks=False):
  """ln P of several lattices over the same rows.  ``jobs``: label lists in which the pseudo-label is the id -1."""
  T, C = ly.shape
  blank = C - 1
  STAR, DEAD = C, C + 1
  with np.errstate(divide='ignore'):
    star = np.log(np.exp(ly[:, [c for c in range(C) if c != space_id]]).sum(axis=1))
  ext = np.concatenate([ly, star[:, None], np.full((T, 1), -np.inf)], axis=1)
  J, U = len(jobs), max(2 * len(l) + 1 for l in jobs)
  cls = np.full((J, U), DEAD)
  skip = np.zeros((J, U), dtype=bool)
  for j, lab in enumerate(jobs):
    lab = [STAR if i < 0 else i for i in lab]
    for u in range(2 * len(lab) + 1):
      if u & 1:
        cls[j, u] = lab[u // 2]
        skip[j, u] = u >= 3 and lab[u // 2] != lab[u // 2 - 1]
      else:
        k = u // 2
        beside = (k > 0 and lab[k - 1] == STAR) or (k < len(lab) and lab[k] == STAR)
        cls[j, u] = DEAD if beside and not live_blanks else blank
  ninf = np.full((J, 1), -np.inf)
  a = np.full((J, U), -np.inf)
  a[:, :2] = ext[0][cls[:, :2]]
  for t in range(1, T):
    adv = np.concatenate([ninf, a[:, :-1]], axis=1)
    skp = np.where(skip, np.concatenate([ninf, ninf, a[:, :-2]], axis=1)[:, :U], -np.inf)
    a = _lse3(a, adv, skp) + ext[t][cls]
  out = np.empty(J)
  for j, lab in enumerate(jobs):
    u = 2 * len(lab)
    out[j] = np.logaddexp(a[j, u], a[j, u - 1]) if u > 0 else a[j, u]
  return out


def word_conf64(logits, labels, space_id, live_blanks=False):
  """-> dict(log_prob, log_conf [words], ln_star [words] = ln P(l*j), words = split_words), or None when the label does not
  fit its frames.  ``live_blanks``: the WRONG lattice, with the blanks beside * left alive (counts paths twice)."""
  labels = [int(i) for i in labels]
  x = np.asarray(logits, dtype=np.float64)
  T = x.shape[0]
  if T < min_frames(labels):
    return None
  words = split_words(labels, space_id)
  if T == 0:
    return dict(log_prob=0.0, log_conf=np.zeros(0), ln_star=np.zeros(0), words=words)
  with np.errstate(invalid='ignore'):
    ly = log_softmax64(x)
  jobs = [labels] + [labels[:a] + [-1] + labels[b:] for a, b in words]
  ln = _lattices(ly, space_id, jobs, live_blanks)
  lp, ls = float(ln[0]), ln[1:]
  with np.errstate(invalid='ignore'):
    conf = np.full(len(words), -np.inf) if lp == -np.inf else np.minimum(0.0, lp - ls)
  return dict(log_prob=lp, log_conf=conf, ln_star=ls, words=words)


# ---- the definition by enumeration -------------------------------------------------------------------------------------------

def _collapse(classes, blank):
  out, prev = [], None
  for c in classes:
    if c != blank and c != prev:
      out.append(c)
    prev = c
  return tuple(out)


@functools.lru_cache(maxsize=None)
def _collapse_table(n, C):
  """The collapsed label of every class sequence of n frames, indexed by the sequence read as a base-C number (frame 0 the
  most significant digit), and the sequences' first and last classes."""
  seqs = [tuple((q // C ** (n - 1 - t)) % C for t in range(n)) for q in range(C ** n)]
  return [_collapse(s, C - 1) for s in seqs], [s[0] if s else None for s in seqs], [s[-1] if s else None for s in seqs]


def brute_force(logits, labels, space_id, word=None):
  """ln of the probability, summed over all C^T frame paths, that the path reads ``labels`` (``word`` None), or that it splits
  into [an alignment of the ids before the word that ends on a space frame (no frames when there are none)] [one or more
  frames of any class but the space] [an alignment of the ids after the word that starts on a space frame (no frames when
  there are none)].  Asserts that no path splits in two ways."""
  labels = tuple(int(i) for i in labels)
  p = np.exp(log_softmax64(np.asarray(logits, dtype=np.float64)))
  T, C = p.shape
  n = np.arange(C ** T)
  D = (n[:, None] // C ** (T - 1 - np.arange(T))[None, :]) % C
  prob = p[np.arange(T)[None, :], D].prod(axis=1)
  if word is None:
    ok = np.array([s == labels for s in _collapse_table(T, C)[0]])
    with np.errstate(divide='ignore'):
      return float(np.log(prob[ok].sum()))
  a, b = word
  prefix, suffix = labels[:a], labels[b:]
  nospace = D != space_id
  count = np.zeros(C ** T, dtype=np.int64)
  for i in range(0, T):
    if (i == 0) != (len(prefix) == 0):
      continue
    col, _, last = _collapse_table(i, C)
    pre_ok = np.array([s == prefix and (i == 0 or l == space_id) for s, l in zip(col, last)])[n // C ** (T - i)]
    for k in range(i + 1, T + 1):
      if (k == T) != (len(suffix) == 0):
        continue
      col, first, _ = _collapse_table(T - k, C)
      suf_ok = np.array([s == suffix and (k == T or f == space_id) for s, f in zip(col, first)])[n % C ** (T - k)]
      count += pre_ok & suf_ok & nospace[:, i:k].all(axis=1)
  assert count.max() <= 1
  with np.errstate(divide='ignore'):
    return float(np.log(prob[count > 0].sum()))


# ---- inputs ------------------------------------------------------------------------------------------------------------------

def random_word_labels(rng, L, C, space_id, word_len=(1, 8), repeat_prob=0.15, edge_space_prob=0.0, double_space_prob=0.0):
  """L ids in [0, C-1): words of ``word_len`` letters (adjacent repeats at ``repeat_prob``) separated by ``space_id``; leading,
  trailing and double spaces at the given probabilities."""
  letters = [c for c in range(C - 1) if c != space_id]
  out = [space_id] if rng.random() < edge_space_prob else []
  while len(out) < L:
    n = int(rng.integers(word_len[0], word_len[1] + 1))
    for k in range(n):
      out.append(out[-1] if k and rng.random() < repeat_prob else letters[int(rng.integers(len(letters)))])
    out.append(space_id)
    if rng.random() < double_space_prob:
      out.append(space_id)
  out = out[:L]
  if out and out[-1] == space_id and rng.random() >= edge_space_prob:
    out[-1] = letters[int(rng.integers(len(letters)))]
  return out


def csr(labels):
  lens = [len(l) for l in labels]
  offs = np.zeros(len(labels) + 1, dtype=np.int32)
  offs[1:] = np.cumsum(lens)
  return np.array([i for l in labels for i in l] + [0], dtype=np.int32), offs


def batch_spans(labels, space_id):
  """The word_spans argument of the entry points: [n_words, 3] int32 = utterance, first label, one past the last."""
  rows = [(b, a, e) for b, lab in enumerate(labels) for a, e in split_words(lab, space_id)]
  return np.array(rows, dtype=np.int32).reshape(-1, 3)
