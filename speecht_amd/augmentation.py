"""SpecAugment (Park et al. 2019) for training batches: a time warp, frequency masks and time masks drawn anew for every utterance
at every step, applied on the device while ``Wav2LetterEngine.load_batch`` copies the batch into the network's input tensor
(st_spec_augment_f32, csrc/spec_augment.hip) -- no extra pass over the batch.  The specification is DESIGN.md "SpecAugment"; the
arithmetic lives once in csrc/spec_augment_core.h, shared by the kernel and the host form this module binds (``plan_host``,
``apply_host``: no GPU needed).

Masked elements become 0: ``preprocessing.normalize`` makes every utterance's features zero-mean, so 0 is the utterance's mean
value, the mask value of the paper.

Randomness is counter-based (Philox4x32-10): an utterance's draws are a function of (seed, draw id) alone, not of its row, its
batch or the padded length.  ``draw_ids`` gives the ids a training step uses."""
import collections
import ctypes

import numpy as np

from . import _lib

MAX_MASKS = 8
ROWS_PER_WORKGROUP = 32        # of the kernel (csrc/spec_augment.hip SA_ROWS): tests pick shapes around it


class SpecAugmentPolicy(collections.namedtuple('SpecAugmentPolicy', 'time_warp freq_width freq_masks time_width time_masks time_ratio')):
  """W, F, mF, T, mT, p: the largest time-warp displacement (frames), the largest frequency-mask width and the number of
  frequency masks, the largest time-mask width, the number of time masks and the largest share of an utterance's own length one
  time mask may take."""
  __slots__ = ()

  def __new__(cls, time_warp=0, freq_width=0, freq_masks=0, time_width=0, time_masks=0, time_ratio=1.0):
    p = super().__new__(cls, int(time_warp), int(freq_width), int(freq_masks), int(time_width), int(time_masks), float(time_ratio))
    if min(p.time_warp, p.freq_width, p.time_width) < 0:
      raise ValueError('SpecAugment: negative time warp or mask width in {}'.format(p))
    if not (0 <= p.freq_masks <= MAX_MASKS and 0 <= p.time_masks <= MAX_MASKS):
      raise ValueError('SpecAugment: 0 .. {} masks of each kind, got {} and {}'.format(MAX_MASKS, p.freq_masks, p.time_masks))
    if not 0.0 <= p.time_ratio <= 1.0:
      raise ValueError('SpecAugment: the time-mask ratio must lie in 0 .. 1, got {}'.format(p.time_ratio))
    return p

  @property
  def time_ratio_q16(self):
    """p as the 16.16 fixed-point integer host and device evaluate floor(p L) with: (q16 * L) >> 16."""
    return int(round(self.time_ratio * 65536))

  @property
  def is_identity(self):
    return self.time_warp == 0 and self.freq_masks == 0 and self.time_masks == 0

  @property
  def plan_words(self):
    return 2 + 2 * (self.freq_masks + self.time_masks)

  def c_args(self):
    return (self.time_warp, self.freq_width, self.freq_masks, self.time_width, self.time_masks, self.time_ratio_q16)

  def describe(self):
    if self.is_identity:
      return 'none'
    return 'time warp {} frames, {} frequency mask(s) of up to {} channels, {} time mask(s) of up to {} frames and {:g} of the utterance'.format(
        self.time_warp, self.freq_masks, self.freq_width, self.time_masks, self.time_width, self.time_ratio)


IDENTITY = SpecAugmentPolicy()
# the paper's LibriSpeech policies (Park et al. 2019, table 1), valid for 80 mel channels at a 10 ms hop
POLICIES = {'none': IDENTITY,
            'LB': SpecAugmentPolicy(80, 27, 1, 100, 1, 1.0),
            'LD': SpecAugmentPolicy(80, 27, 2, 100, 2, 1.0)}


def draw_ids(global_step, batch, world=1, rank=0):
  """The draw ids of one rank's rows at one step: global_step * (batch * world) + rank * batch + row -- the id the same utterance
  would get in ONE process that sees the whole global batch (InputBatchLoader keeps rows [rank B, (rank + 1) B) of each)."""
  return (np.int64(global_step) * np.int64(batch * world) + np.int64(rank * batch) + np.arange(batch, dtype=np.int64))


class SpecAugment:
  """What ``load_batch(..., augment=...)`` takes: a policy, the 64-bit augmentation seed and one draw id per batch row."""

  def __init__(self, policy, seed=0, draw_ids=None):
    self.policy = POLICIES[policy] if isinstance(policy, str) else SpecAugmentPolicy(*policy)
    self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    self.draw_ids = None if draw_ids is None else np.ascontiguousarray(draw_ids, dtype=np.int64)

  def at(self, ids):
    """The same policy and seed with these draw ids."""
    return SpecAugment(self.policy, self.seed, ids)

  def for_step(self, global_step, batch, world=1, rank=0):
    return self.at(draw_ids(global_step, batch, world, rank))

  def __repr__(self):
    return 'SpecAugment({}, seed={})'.format(self.policy.describe(), self.seed)


def _p(a):
  return a.ctypes.data_as(ctypes.c_void_p)


def _lens_ids(seq_lens, ids):
  lens = np.ascontiguousarray(seq_lens, dtype=np.int32)
  ids = np.ascontiguousarray(ids, dtype=np.int64)
  if lens.ndim != 1 or ids.shape != lens.shape:
    raise ValueError('SpecAugment: {} lengths but draw ids of shape {}'.format(lens.shape, ids.shape))
  return lens, ids


def plan_host(augment, seq_lens, channels):
  """The plans st_spec_augment_f32 would draw, [B, 2 + 2 (mF + mT)] int32: {c, w, (f0, f) per frequency mask, (t0, t) per time
  mask} (st_spec_augment_plan_host)."""
  lens, ids = _lens_ids(seq_lens, augment.draw_ids)
  plan = np.zeros((len(lens), augment.policy.plan_words), dtype=np.int32)
  _lib.call('st_spec_augment_plan_host', _p(lens), _p(ids), len(lens), int(channels), augment.seed, *augment.policy.c_args(), _p(plan))
  return plan


def apply_host(augment, x, seq_lens, out=None, halo=0):
  """The host form (st_spec_augment_host): x [B, T, C] float32 -> (augmented batch, plans).  ``out``: a float32 buffer
  [B, t_pitch, c_pitch] to write the interior rows (from row ``halo`` of each utterance) and valid channels of, as the kernel
  writes the engine's input tensor; default a fresh [B, T, C] array."""
  x = np.ascontiguousarray(x, dtype=np.float32)
  B, T, C = x.shape
  lens, ids = _lens_ids(seq_lens, augment.draw_ids)
  if len(lens) != B:
    raise ValueError('SpecAugment: batch of {} with {} lengths'.format(B, len(lens)))
  if out is None:
    out = np.zeros((B, T, -(-C // 16) * 16), dtype=np.float32)
    result = out[:, :, :C]
  else:
    assert out.dtype == np.float32 and out.flags.c_contiguous and out.ndim == 3 and out.shape[0] == B, 'apply_host: bad output buffer'
    result = out[:, halo:halo + T, :C]
  dst = _lib.Tensor3(out.ctypes.data, B, T, C, halo, out.shape[1], out.shape[2])
  plan = np.zeros((B, augment.policy.plan_words), dtype=np.int32)
  _lib.call('st_spec_augment_host', _p(x), B, T, C, _p(lens), _p(ids), augment.seed, *augment.policy.c_args(), ctypes.byref(dst), _p(plan))
  return result, plan


def add_arguments(parser):
  """The `speecht-cli train` flags."""
  parser.add_argument('--spec-augment', dest='spec_augment', choices=['none', 'LB', 'LD'], default='none',
                      help='(extension) SpecAugment on the device as every training batch is loaded: a time warp, frequency masks '
                           'and time masks drawn anew per utterance and step.  LB / LD: the paper\'s LibriSpeech policies (for 80 '
                           'mel channels at a 10 ms hop); the flags below override single values.  Evaluation steps never augment.')
  parser.add_argument('--time-warp', dest='time_warp', type=int, default=None, metavar='W', help='largest time-warp displacement in frames')
  parser.add_argument('--freq-masks', dest='freq_masks', type=int, default=None, metavar='N', help='number of frequency masks (0 .. 8)')
  parser.add_argument('--freq-mask-width', dest='freq_mask_width', type=int, default=None, metavar='F', help='largest frequency-mask width in channels')
  parser.add_argument('--time-masks', dest='time_masks', type=int, default=None, metavar='N', help='number of time masks (0 .. 8)')
  parser.add_argument('--time-mask-width', dest='time_mask_width', type=int, default=None, metavar='T', help='largest time-mask width in frames')
  parser.add_argument('--time-mask-ratio', dest='time_mask_ratio', type=float, default=None, metavar='P',
                      help='largest share of an utterance\'s own length one time mask may take (0 .. 1)')
  parser.add_argument('--augment-seed', dest='augment_seed', type=int, default=None,
                      help='seed of the augmentation draws (default: --seed if given, else 0); the draws are a function of it, the '
                           'training step and the utterance\'s row in the global batch, so a resumed run continues the same sequence')


def from_flags(flags):
  """The SpecAugment the train flags ask for (no draw ids yet), or None when nothing is switched on."""
  base = POLICIES[getattr(flags, 'spec_augment', None) or 'none']
  names = dict(time_warp='time_warp', freq_masks='freq_masks', freq_width='freq_mask_width', time_masks='time_masks',
               time_width='time_mask_width', time_ratio='time_mask_ratio')
  given = {field: getattr(flags, flag) for field, flag in names.items() if getattr(flags, flag, None) is not None}
  policy = SpecAugmentPolicy(**dict(base._asdict(), **given))
  if policy.is_identity:
    return None
  seed = getattr(flags, 'augment_seed', None)
  if seed is None:
    seed = getattr(flags, 'seed', None) or 0
  return SpecAugment(policy, seed)
