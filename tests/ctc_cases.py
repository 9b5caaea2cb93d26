"""The case table of the CTC loss / gradient lattice tests (tests/test_ctc_cases_cpu.py keeps it honest on the CPU,
tests/test_gpu_ctc_lattice.py runs it through st_ctc_loss_grad_hilo_f32).  Pure numpy.

csrc/ctc.hip deals the U = 2L+1 lattice states k-contiguous per lane of one wave, k = the smallest of 1, 2, 3, 4, 5, 6, 8, 10,
12, 16 with 64k >= U, and instantiates the recursion and the gradient kernel once per k.  One batch per k:

  a        the longest label the dispatch holds (32k - 1), repeats drawn at 0.15, every frame of the batch, N(0,1)*2 logits
  b        the shortest label that needs the dispatch, exactly min_frames(label) frames: one path exists
  c        the longest length again with repeats PLACED on the transitions that cross a lane boundary (the u-2 / u+2 neighbour
           lives in the next lane) and on the last slots of lanes, and non-repeats on others of them, see boundary_indices
  d        about half the dispatch, frames at a 64-frame chunk edge, peaked logits around a planted alignment
  d_masked the same kind with classes masked to -inf: unused ones throughout, a used one for a while, the blank at the start
  e        the empty label over 0, 1 or 3 frames
  f        one label, one frame
  g        a label that is one frame short: refused

The dense frame count of a batch ends at 64m - 1, 64m or 64m + 1 (rotating over the batches) and is only as large as its longest
label needs.  The same kinds at 2, 3 and 32 classes for k = 1 and k = 3.  Logits are float32 (the oracle widens them: it
gets exactly what the device gets)."""
import functools
from collections import namedtuple

import numpy as np

from tests import align_oracle as AO

KPLS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16)
CHUNK_EDGES = (63, 64, 65, 128, 129)
KINDS = ('a', 'b', 'c', 'd', 'd_masked', 'e', 'f', 'g')

# Bounds of the device test.  Loss: 1e-5 relative, the bound of test_ctc_loss_grad.  The lattice's rounding is RELATIVE in p, so
# absolute in -log p, whatever the loss: a float32 recursion cannot hold 1e-5 relative on the near-zero losses of peaked rows
# with 2 or 3 classes.  The float32 restatement of the recursion (scaled_alpha_loss) is 2.95e-5 relative = 4.29e-7 absolute off
# on a loss of 0.0145 (k1-C2, utterance d); over the cases on which it misses a quarter of 1e-5 relative its worst absolute
# error is MODEL_WORST_ABS = 8.55e-7 (k3-C3, d, loss 0.112); on every loss above 0.35 it is within 2.6e-7 relative.  The floor
# is 4 x that error: below a loss of 0.342 the bound is 3.42e-6 absolute, above it 1e-5 relative as before.  On the CPU the
# model is held to a quarter of the relative part and to HALF the floor (a quarter of it is the model's own worst case by
# construction and would leave no room for another libm's rounding).
LOSS_RTOL = 1e-5
MODEL_WORST_ABS = 8.55e-7
LOSS_FLOOR = 4 * MODEL_WORST_ABS
PAIR_ATOL = 2e-5          # |hi + lo - ref|, the bound of the masked-class test
GRAD_ATOL = 5e-5          # max |g - scale * ref| / scale, the bound of test_ctc_loss_grad


def loss_bound(ref):
  return max(LOSS_RTOL * abs(ref), LOSS_FLOOR)


def model_loss_bound(ref):
  """What the float32 model has to reach on the CPU."""
  return max(0.25 * LOSS_RTOL * abs(ref), 0.5 * LOSS_FLOOR)


def states_per_lane_from_ws(ws_bytes, batch, frames):
  """The k that st_ctc_ws sized the workspace for: rows * 32 floats * 3 (log-softmax, emission pairs) + two lattices of
  rows * 64k (mantissa, exponent) records + 512 bytes."""
  rows = batch * frames
  k, rest = divmod(ws_bytes - 512 - rows * 32 * 4 * 3, rows * 64 * 4 * 4)
  assert ws_bytes > 0 and rest == 0
  return k


Utterance = namedtuple('Utterance', 'kind label logits feasible masked')      # logits [Tb, C] float32
Batch = namedtuple('Batch', 'name k C frames utterances')


def dispatch_of(max_label_len):
  """States per lane that a label of this length is run with: the smallest k with 64k >= 2L+1."""
  return next(k for k in KPLS if 64 * k >= 2 * max_label_len + 1)


def largest_label(k):
  return 32 * k - 1


def smallest_label(k):
  """The shortest label that needs dispatch k (1 for the first: the empty label is utterance e)."""
  i = KPLS.index(k)
  return largest_label(KPLS[i - 1]) + 1 if i else 1


def boundary_indices(L, k):
  """Two sets of label indices i >= 1 (label state u = 2i+1, lane u // k, slot u % k) for dispatch k -> (crossing, last slots).
  Crossing, u % k in {0, 1}: the transition 2i-1 -> 2i+1 that a repeat at i forbids crosses a lane boundary, so alpha's skip
  predecessor u-2 comes from the previous lane AND beta's skip successor of state 2i-1 from the next one: this one set puts
  both directions' cross-lane moves under a repeat or a non-repeat.  Last slots, u % k in {k-2, k-1}: the state sits in the
  last two slots of its lane, where beta takes its u+1 / u+2 from the neighbour lane; the repeat at i itself governs a
  transition inside the lane for k >= 4 (the in-lane counterpart).  With one state per lane every transition crosses lanes."""
  if k == 1:
    every = list(range(1, L))
    return every, every
  crossing = [i for i in range(1, L) if (2 * i + 1) % k in (0, 1)]
  last_slots = [i for i in range(1, L) if (2 * i + 1) % k in (k - 2, k - 1)]
  return crossing, last_slots


def repeat_indices(label):
  return {i for i in range(1, len(label)) if label[i] == label[i - 1]}


def lane_thirds(indices, L, k):
  """Which thirds (0 low, 1 middle, 2 high) of the lanes in use hold the label states of ``indices``."""
  lanes = (2 * L + 1 + k - 1) // k
  return {min(2, 3 * ((2 * i + 1) // k) // lanes) for i in indices}


def labels_with_repeats_at(rng, L, C, repeats):
  """L ids in [0, C-1), equal to their predecessor exactly at the indices in ``repeats`` (C = 2 has one label class: every
  index repeats)."""
  out = []
  for i in range(L):
    if i and (i in repeats or C == 2):
      out.append(out[-1])
    else:
      v = int(rng.integers(C - 1))
      while i and v == out[-1]:
        v = int(rng.integers(C - 1))
      out.append(v)
  return out


def boundary_label(rng, L, k, C):
  """Utterance c: a coin per index of the two sets of boundary_indices decides between a repeat and a non-repeat, redrawn until
  each set has four of both in low, middle and high lanes."""
  crossing, last_slots = boundary_indices(L, k)
  union = sorted(set(crossing) | set(last_slots))
  for _ in range(100):
    chosen = {i for i in union if rng.random() < 0.5}
    label = labels_with_repeats_at(rng, L, C, chosen)
    rep = repeat_indices(label)
    ok = True
    for side in (crossing, last_slots):
      yes, no = [i for i in side if i in rep], [i for i in side if i not in rep]
      ok = ok and len(yes) >= 4 and lane_thirds(yes, L, k) == {0, 1, 2}
      ok = ok and (C == 2 or (len(no) >= 4 and lane_thirds(no, L, k) == {0, 1, 2}))
    if ok:
      return label
  raise AssertionError('no boundary label for L={} k={} C={}'.format(L, k, C))


def chunk_edge_frames(edge, need):
  """``edge`` (63, 64, 65, 128 or 129) moved up by whole 64-frame chunks until ``need`` frames fit."""
  while edge < need:
    edge += 64
  return edge


def masked_utterance(rng, L, C, frames):
  """Peaked logits around a planted alignment, then -inf over: every class the label leaves unused (the label avoids the upper
  eight where there are that many), the blank on the first two frames (the path must open with the first label), and the class
  of the label three quarters in for up to twenty frames from frame 2 on, while most of its states cannot be reached yet.  A
  path remains: hold the first label (or the blank after it, should that be the masked class) through the window; the frames
  allow for the window on top of min_frames."""
  unused = 8 if C - 1 >= 16 else 0
  label = AO.random_labels(rng, L, C - unused, repeat_prob=0.15)
  x, _ = AO.planted_logits(rng, label, frames, C, boost=8.0)
  x[:, C - 1 - unused:C - 1] = -np.inf
  window = min(20, frames - AO.min_frames(label) - 3)
  assert window >= 1
  x[:2, C - 1] = -np.inf
  x[2:2 + window, label[(3 * L) // 4]] = -np.inf
  return Utterance('d_masked', label, x, True, True)


def make_batch(name, k, C, rot, seed):
  rng = np.random.default_rng(seed)
  l_max, l_lo = largest_label(k), smallest_label(k)
  lab_a = AO.random_labels(rng, l_max, C, repeat_prob=0.15)
  lab_b = AO.random_labels(rng, l_lo, C, repeat_prob=0.15)
  lab_c = boundary_label(rng, l_max, k, C)
  l_half = max(2, 16 * k)
  lab_d = AO.random_labels(rng, l_half, C, repeat_prob=0.15)
  t_d = chunk_edge_frames(CHUNK_EDGES[rot % 5], AO.min_frames(lab_d) + 4)
  t_m = chunk_edge_frames(CHUNK_EDGES[(rot + 2) % 5], 2 * l_half + 26)           # (min_frames <= 2L - 1)
  need = max(AO.min_frames(lab_a), AO.min_frames(lab_c) + 2, t_d, t_m) + 6
  frames = 64 * ((need + 1 + 63) // 64) + (-1, 0, 1)[rot % 3]
  assert frames >= need
  normal = lambda t: AO.random_logits(rng, t, C, scale=2.0)
  utts = [Utterance('a', lab_a, normal(frames), True, False),
          Utterance('b', lab_b, normal(AO.min_frames(lab_b)), True, False),
          Utterance('c', lab_c, normal(frames - (rot % 2) * 2), True, False),
          Utterance('d', lab_d, AO.planted_logits(rng, lab_d, t_d, C, boost=8.0)[0], True, False),
          masked_utterance(rng, l_half, C, t_m),
          Utterance('e', [], normal((0, 1, 3)[rot % 3]), True, False),
          Utterance('f', [int(rng.integers(C - 1))], normal(1), True, False)]
  lab_g = AO.random_labels(rng, min(l_max, 40), C, repeat_prob=0.5)
  utts.append(Utterance('g', lab_g, normal(AO.min_frames(lab_g) - 1), False, False))
  assert [u.kind for u in utts] == list(KINDS) and all(u.logits.shape[0] <= frames for u in utts)
  assert dispatch_of(max(len(u.label) for u in utts)) == k
  return Batch(name, k, C, frames, utts)


@functools.lru_cache(maxsize=None)
def dispatch_batches():
  """One 29-class batch per dispatch."""
  return tuple(make_batch('k{}'.format(k), k, 29, i, 1000 + k) for i, k in enumerate(KPLS))


@functools.lru_cache(maxsize=None)
def class_count_batches():
  """2, 3 and 32 classes at one and at three states per lane."""
  return tuple(make_batch('k{}-C{}'.format(k, C), k, C, i, 2000 + 40 * k + C)
               for i, (k, C) in enumerate((k, C) for k in (1, 3) for C in (2, 3, 32)))


def all_batches():
  return dispatch_batches() + class_count_batches()


def batch_by_name(name):
  return next(b for b in all_batches() if b.name == name)


BATCH_NAMES = tuple(['k{}'.format(k) for k in KPLS] + ['k{}-C{}'.format(k, C) for k in (1, 3) for C in (2, 3, 32)])


@functools.lru_cache(maxsize=None)
def oracle_results(name):
  """(loss, grad [Tb, C]) of every utterance of a batch from the float64 oracle, None for the refused one; computed once per
  process and shared (do not modify)."""
  from oracle import w2l_oracle as O
  out = []
  for u in batch_by_name(name).utterances:
    if not u.feasible:
      out.append(None)
      continue
    with np.errstate(invalid='ignore', divide='ignore'):
      loss, grad = O.ctc_loss_and_grad(u.logits.astype(np.float64)[:, None, :], [u.label], [u.logits.shape[0]])
    grad = grad[:, 0, :]
    grad.setflags(write=False)
    out.append((float(loss[0]), grad))
  return tuple(out)
