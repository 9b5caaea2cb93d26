"""The case table of the wildcard CTC loss tests (tests/test_wild_ctc_cpu.py keeps it honest on the CPU,
tests/test_gpu_wild_ctc.py runs it through st_ctc_loss_grad_wild_f32).  Pure numpy.  The dispatch geometry -- states per lane,
the longest label of a dispatch, which label indices sit on lane boundaries, chunk-edge frame counts -- is tests/ctc_cases.py's.

One batch per states-per-lane dispatch k, the smallest shapes that reach every instantiation of the recursion and of the
wildcard gradient kernel.  Labels hold WILDCARD (-1) where the transcript leaves audio out:

  long     the longest label the dispatch holds (32k - 1), wildcards PLACED on label indices of both sets of boundary_indices
           (the state's skip neighbours live in the next lane / it sits in the last slots of its lane) and on others, every
           frame of the batch, N(0,1)*2 logits
  ends     about half the dispatch with a wildcard at both ends, frames at a 64-frame chunk edge
  w1       the label [wildcard] alone over one frame
  wedge    the label [wildcard] alone over a chunk-edge frame count
  masked   peaked logits around a planted alignment; on a window in the middle every label class is -inf, so only blanks can
           cover it: the wildcard's emission is 0 there, and the planted path (blank through the window) remains
  plain_a  no wildcard, N(0,1)*2 logits
  plain_b  no wildcard, peaked logits
  short    a label with wildcards one frame short, the wildcard counted as a label: refused

The dense frame count of a batch ends at 64m - 1, 64m or 64m + 1 (rotating over the batches).  The same kinds at 2, 3 and 31
classes (the most the wildcard's slot allows) for k = 1 and k = 3.  Logits are float32 (the oracle widens them)."""
import functools
from collections import namedtuple

import numpy as np

from tests import align_oracle as AO
from tests import ctc_cases as CC
from tests import wild_ctc_oracle as WO

W = WO.WILDCARD
BIAS = WO.WILDCARD_BIAS
KINDS = ('long', 'ends', 'w1', 'wedge', 'masked', 'plain_a', 'plain_b', 'short')

Utterance = namedtuple('Utterance', 'kind label logits feasible wild')      # logits [Tb, C] float32
Batch = namedtuple('Batch', 'name k C frames utterances')


def with_wildcards_at(label, indices):
  out = list(label)
  for i in indices:
    out[i] = W
  assert not any(a == W and b == W for a, b in zip(out, out[1:]))
  return out


def spread(rng, indices, n, taken):
  """Up to n of ``indices``, from its low, middle and high part in turn, none next to one already taken."""
  indices = sorted(indices)
  out = []
  for part in range(n):
    third = indices[part % 3 * len(indices) // 3:(part % 3 + 1) * len(indices) // 3] or indices
    free = [i for i in third if not ({i - 1, i, i + 1} & (taken | set(out)))]
    if free:
      out.append(free[int(rng.integers(len(free)))])
  return out


def long_label(rng, L, k, C):
  """The longest label with wildcards on three indices of each set of boundary_indices and on two others (index 0 and, where
  there is one, an index of neither set) -> (label, indices on crossing, on last slots, others)."""
  base = AO.random_labels(rng, L, C, repeat_prob=0.15)
  crossing, last_slots = CC.boundary_indices(L, k)
  taken = {0}
  on_cross = spread(rng, crossing, 3, taken)
  taken |= set(on_cross)
  on_last = spread(rng, [i for i in last_slots if i not in on_cross], 3, taken)
  taken |= set(on_last)
  neither = [i for i in range(1, L) if i not in crossing and i not in last_slots]
  others = [0] + spread(rng, neither, 1, taken)
  return with_wildcards_at(base, on_cross + on_last + others), on_cross, on_last, others


def planted(rng, label, path, C, boost=8.0):
  """N(0, 1) noise with ``boost`` on the class of lattice state path[t] (a wildcard state: on a label class drawn per frame;
  with one label class and no wildcard the draw is that class)."""
  x = rng.standard_normal((len(path), C)).astype(np.float32)
  for t, u in enumerate(path):
    c = C - 1 if not u & 1 else (label[u // 2] if label[u // 2] != W else int(rng.integers(C - 1)))
    x[t, c] += np.float32(boost)
  return x


def masked_utterance(rng, L, C, frames):
  """The first part of the label over the first frames, a window of blanks, the rest -- which opens with a wildcard -- over the
  others; then -inf on every label class in the window.  Another wildcard sits in the first part."""
  s = L // 2
  label = with_wildcards_at(AO.random_labels(rng, L, C, repeat_prob=0.15), sorted({max(s - 3, 0), s}))
  window = 5
  t0 = WO.min_frames(label[:s]) + (frames - window - WO.min_frames(label)) // 2
  head = AO.random_alignment(rng, label[:s], t0)
  tail = AO.random_alignment(rng, label[s:], frames - window - t0)
  path = head + [2 * s] * window + [u + 2 * s for u in tail]
  x = planted(rng, label, path, C)
  x[t0:t0 + window, :C - 1] = -np.inf
  return Utterance('masked', label, x, True, True), (t0, t0 + window)


def make_batch(name, k, C, rot, seed):
  rng = np.random.default_rng(seed)
  l_max = CC.largest_label(k)
  lab_long = long_label(rng, l_max, k, C)[0]
  l_half = max(4, 16 * k)
  lab_ends = with_wildcards_at(AO.random_labels(rng, l_half, C, repeat_prob=0.15), [0, l_half - 1])
  t_ends = CC.chunk_edge_frames(CC.CHUNK_EDGES[rot % 5], WO.min_frames(lab_ends) + 4)
  t_wedge = CC.CHUNK_EDGES[(rot + 1) % 5]
  t_mask = CC.chunk_edge_frames(CC.CHUNK_EDGES[(rot + 2) % 5], 2 * l_half + 12)
  need = max(WO.min_frames(lab_long) + 6, t_ends, t_wedge, t_mask)
  frames = 64 * ((need + 1 + 63) // 64) + (-1, 0, 1)[rot % 3]
  assert frames >= need
  normal = lambda t: AO.random_logits(rng, t, C, scale=2.0)
  lab_a = AO.random_labels(rng, l_half, C, repeat_prob=0.15)
  lab_b = AO.random_labels(rng, max(2, l_half // 2), C, repeat_prob=0.15)
  t_b = WO.min_frames(lab_b) + 9
  n_short = min(l_max, 40)
  lab_short = with_wildcards_at(AO.random_labels(rng, n_short, C, repeat_prob=0.5), [0, n_short // 2, n_short - 1][:n_short])
  utts = [Utterance('long', lab_long, normal(frames), True, True),
          Utterance('ends', lab_ends, normal(t_ends), True, True),
          Utterance('w1', [W], normal(1), True, True),
          Utterance('wedge', [W], normal(t_wedge), True, True),
          masked_utterance(rng, l_half, C, t_mask)[0],
          Utterance('plain_a', lab_a, normal(frames - (rot % 2) * 2), True, False),
          Utterance('plain_b', lab_b, planted(rng, lab_b, AO.random_alignment(rng, lab_b, t_b), C), True, False),
          Utterance('short', lab_short, normal(WO.min_frames(lab_short) - 1), False, True)]
  assert [u.kind for u in utts] == list(KINDS) and all(u.logits.shape[0] <= frames for u in utts)
  assert CC.dispatch_of(max(len(u.label) for u in utts)) == k
  return Batch(name, k, C, frames, utts)


@functools.lru_cache(maxsize=None)
def dispatch_batches():
  """One 29-class batch per dispatch."""
  return tuple(make_batch('wk{}'.format(k), k, 29, i, 3000 + k) for i, k in enumerate(CC.KPLS))


@functools.lru_cache(maxsize=None)
def class_count_batches():
  """2, 3 and 31 classes at one and at three states per lane."""
  return tuple(make_batch('wk{}-C{}'.format(k, C), k, C, i, 4000 + 40 * k + C)
               for i, (k, C) in enumerate((k, C) for k in (1, 3) for C in (2, 3, 31)))


def all_batches():
  return dispatch_batches() + class_count_batches()


BATCH_NAMES = tuple(['wk{}'.format(k) for k in CC.KPLS] + ['wk{}-C{}'.format(k, C) for k in (1, 3) for C in (2, 3, 31)])


def batch_by_name(name):
  return next(b for b in all_batches() if b.name == name)


@functools.lru_cache(maxsize=None)
def oracle_results(name):
  """(loss, grad [Tb, C]) of every utterance of a batch from tests/wild_ctc_oracle.py at BIAS, None for the refused one; computed
  once per process and shared (do not modify)."""
  out = []
  for u in batch_by_name(name).utterances:
    if not u.feasible:
      out.append(None)
      continue
    loss, grad = WO.ctc_loss_and_grad(u.logits, u.label, BIAS)
    grad.setflags(write=False)
    out.append((loss, grad))
  return tuple(out)
