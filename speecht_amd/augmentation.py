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
import fractions
import os

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


# ---- waveform augmentation: speed perturbation and noise mixing (DESIGN.md "Waveform augmentation") ----------------------------------
#
# Both act on the waveform before the features: st_wave_augment_f32 (csrc/wave_augment.hip) on the device, st_wave_augment_host
# and st_wave_augment_plan_host on the host, all three on the arithmetic of csrc/wave_augment_core.h.  The plan (which speed, how
# many samples come out, whether noise is mixed, which clip from where at which SNR) is always made on the host: the caller needs
# every output length before it can size a buffer.

MAX_SPEED_TERM = 32
MAX_SPEEDS = 8
KAISER_FAST = dict(zeros=16, rolloff=0.85, beta=8.555504641634386)        # resampy's kaiser_fast
TILE = 256                       # positions per tile of the power sums (csrc/wave_augment_core.h WA_TILE)
PLAN_DTYPE = np.dtype([('M', '<i8'), ('offset', '<i8'), ('lin', '<f8'), ('speed', '<i4'), ('noisy', '<i4'), ('clip', '<i4'),
                       ('snr_centi', '<i4')])                              # st::WavePlan, 40 bytes


def _as_speed(value):
  """(num, den) of a pair or of a number such as 0.9 (-> 9/10), reduced; refuses what the kernels do not take."""
  if isinstance(value, (tuple, list)) and len(value) == 2:
    f = fractions.Fraction(int(value[0]), int(value[1]))
  else:
    f = fractions.Fraction(str(value))
  num, den = f.numerator, f.denominator
  if not (1 <= num <= MAX_SPEED_TERM and 1 <= den <= MAX_SPEED_TERM and den <= 2 * num and num <= 2 * den):
    raise ValueError('speed {}: a speed is a fraction of terms 1 .. {} between 1/2 and 2'.format(value, MAX_SPEED_TERM))
  return num, den


def half_width(num, den):
  """H: the filter reaches H input samples to either side."""
  return 16 if num <= den else -(-16 * num // den)


def out_len(n, num, den):
  """M = ceil(n den / num): what n samples become at the speed num/den."""
  return -(-int(n) * den // num)


def speed_table(num, den):
  """The phase table [den][2H] (float32) of the speed num/den: the Kaiser-windowed sinc of resampy's kaiser_fast (16 zero crossings,
  rolloff 0.85) with cutoff 0.85 min(1, den/num), tap j = -H+1 .. H of phase phi at tau = j - phi/den, every row divided by its own
  sum in float64 and then rounded.  The kernels and the host form read it; neither evaluates a sinc or a Bessel function."""
  num, den = _as_speed((num, den))
  H = half_width(num, den)
  fc = KAISER_FAST['rolloff'] * min(1.0, den / num)
  tau = np.arange(-H + 1, H + 1, dtype=np.float64)[None, :] - np.arange(den, dtype=np.float64)[:, None] / den
  r = tau / H
  window = np.where(np.abs(r) < 1.0, np.i0(KAISER_FAST['beta'] * np.sqrt(np.maximum(0.0, 1.0 - r * r))) / np.i0(KAISER_FAST['beta']), 0.0)
  h = fc * np.sinc(fc * tau) * window
  return (h / h.sum(axis=1, keepdims=True)).astype(np.float32)


class WavePolicy(collections.namedtuple('WavePolicy', 'speeds noise_prob snr_db')):
  """speeds: the fractions one is drawn from per utterance and step (pairs, or numbers such as 0.9 -> 9/10; default Kaldi's 0.9 /
  1.0 / 1.1); noise_prob: the share of utterances that get a noise clip mixed in; snr_db: the range (lo, hi) the signal-to-noise
  ratio is drawn from, in hundredths of a dB.  The default range 10 .. 30 dB is a guess, not tuned on data."""
  __slots__ = ()

  def __new__(cls, speeds=((9, 10), (1, 1), (11, 10)), noise_prob=0.0, snr_db=(10.0, 30.0)):
    speeds = tuple(_as_speed(s) for s in speeds)
    if not 1 <= len(speeds) <= MAX_SPEEDS:
      raise ValueError('WavePolicy: 1 .. {} speeds, got {}'.format(MAX_SPEEDS, len(speeds)))
    noise_prob = float(noise_prob)
    if not 0.0 <= noise_prob <= 1.0:
      raise ValueError('WavePolicy: the noise probability must lie in 0 .. 1, got {}'.format(noise_prob))
    lo, hi = float(snr_db[0]), float(snr_db[1])
    if not -100.0 <= lo <= hi <= 100.0:
      raise ValueError('WavePolicy: the SNR range must be ordered and within -100 .. 100 dB, got {} .. {}'.format(lo, hi))
    return super().__new__(cls, speeds, noise_prob, (lo, hi))

  @property
  def noise_prob_q16(self):
    return int(round(self.noise_prob * 65536))

  @property
  def snr_centi(self):
    return int(round(self.snr_db[0] * 100)), int(round(self.snr_db[1] * 100))

  @property
  def is_identity(self):
    return self.noise_prob == 0.0 and all(num == den for num, den in self.speeds)

  def c_speeds(self):
    return np.ascontiguousarray(self.speeds, dtype=np.int32).reshape(-1, 2)

  def tables(self):
    """The speeds' tables one after the other, as the entry points take them."""
    return np.concatenate([speed_table(num, den).reshape(-1) for num, den in self.speeds])

  def describe(self):
    if self.is_identity:
      return 'none'
    text = 'speeds ' + ' '.join('{}/{}'.format(*s) for s in self.speeds)
    if self.noise_prob > 0:
      text += ', noise on {:g} of the utterances at {:g} .. {:g} dB SNR (a range that is a guess, not tuned on data)'.format(
          self.noise_prob, *self.snr_db)
    return text


class NoiseBank:
  """Noise clips at the model's sample rate, one float32 array and the clips' offsets in it; every clip has at least one sample."""

  def __init__(self, samples, offsets, rate):
    self.samples = np.ascontiguousarray(samples, dtype=np.float32)
    self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    self.rate = int(rate)
    lens = np.diff(self.offsets)
    if len(lens) < 1 or self.offsets[0] != 0 or self.offsets[-1] != len(self.samples) or lens.min() < 1 or lens.max() >= 2 ** 31:
      raise ValueError('NoiseBank: clips of 1 .. 2^31 - 1 samples stored one after the other, got offsets {}'.format(self.offsets))
    self._device = {}

  @property
  def lengths(self):
    return np.diff(self.offsets)

  def __len__(self):
    return len(self.offsets) - 1

  @classmethod
  def from_arrays(cls, clips, rate):
    clips = [np.asarray(c, dtype=np.float32).reshape(-1) for c in clips]
    return cls(np.concatenate(clips) if clips else np.zeros(0, np.float32), np.concatenate([[0], np.cumsum([len(c) for c in clips])]), rate)

  @classmethod
  def from_directory(cls, path, rate, device='cuda:0'):
    """Every audio file under `path` that the bundled decoders read (transcription.load_native: WAV, FLAC, .npy), resampled to
    `rate` with the device resampler (audio_io.resample_kaiser_best_device), once, at start-up."""
    from . import audio_io, transcription
    files = sorted(os.path.join(root, f) for root, _, names in os.walk(path) for f in names
                   if f.lower().endswith(('.wav', '.flac', '.npy')))
    if not files:
      raise ValueError('NoiseBank: no .wav, .flac or .npy file under {}'.format(path))
    loaded = [transcription.load_native(f) for f in files]
    clips = [np.asarray(a, dtype=np.float32) for a, r in loaded if r == rate]
    other = [(a, r) for a, r in loaded if r != rate]
    if other:
      audio, offsets = audio_io.resample_kaiser_best_device([a for a, _ in other], [r for _, r in other], rate, device=device)
      host = audio.cpu().numpy()
      clips += [host[offsets[i]:offsets[i + 1]] for i in range(len(other))]
    return cls.from_arrays([c for c in clips if len(c) >= 1], rate)

  def device_arrays(self, device):
    """(samples, offsets) as device tensors, uploaded once per device."""
    import torch
    key = str(device)
    if key not in self._device:
      self._device[key] = (torch.as_tensor(self.samples).to(device), torch.as_tensor(self.offsets).to(device))
    return self._device[key]


class WaveAugment:
  """What ``engine.load_wave_batch(..., wave=...)`` takes: a policy, the 64-bit augmentation seed, the noise bank and one draw id per
  row of the GLOBAL batch (every rank plans every row: the padded length is the global batch's)."""

  def __init__(self, policy=None, seed=0, noise=None, draw_ids=None):
    self.policy = policy if isinstance(policy, WavePolicy) else WavePolicy(*(policy or ()))
    if self.policy.noise_prob > 0 and noise is None:
      raise ValueError('WaveAugment: a noise probability needs a noise bank')
    self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    self.noise = noise
    self.draw_ids = None if draw_ids is None else np.ascontiguousarray(draw_ids, dtype=np.int64)
    self._tables = None
    self._device_tables = {}

  def at(self, ids):
    other = WaveAugment(self.policy, self.seed, self.noise, ids)
    other._tables, other._device_tables = self.tables, self._device_tables
    return other

  def for_step(self, global_step, batch, world=1, rank=0):
    """The draw ids of the whole global batch at this step (``rank`` only names the caller: its rows are
    [rank batch, (rank + 1) batch) of the plan)."""
    return self.at(draw_ids(global_step, batch * world, 1, 0))

  @property
  def tables(self):
    if self._tables is None:
      self._tables = self.policy.tables()
    return self._tables

  def device_tables(self, device):
    import torch
    key = str(device)
    if key not in self._device_tables:
      self._device_tables[key] = torch.as_tensor(self.tables).to(device)
    return self._device_tables[key]

  def __repr__(self):
    return 'WaveAugment({}, seed={}, {} noise clips)'.format(self.policy.describe(), self.seed, 0 if self.noise is None else len(self.noise))


def plan_wave_host(augment, lengths, min_samples=0):
  """The plans of utterances of `lengths` samples (st_wave_augment_plan_host): a PLAN_DTYPE record each -- M output samples, the
  speed index (-1: the drawn speed would leave M <= min_samples, the utterance stays as it is), and for a noisy one the clip, the
  offset into it, the SNR in hundredths of a dB and lin = 10^(snr/10)."""
  lens = np.ascontiguousarray(lengths, dtype=np.int64).reshape(-1)
  ids = np.ascontiguousarray(augment.draw_ids, dtype=np.int64).reshape(-1)
  if ids.shape != lens.shape:
    raise ValueError('WaveAugment: {} lengths but {} draw ids'.format(len(lens), len(ids)))
  pol = augment.policy
  plan = np.zeros(len(lens), dtype=PLAN_DTYPE)
  speeds = pol.c_speeds()
  clip_lens = None if augment.noise is None else np.ascontiguousarray(augment.noise.lengths, dtype=np.int64)
  lo, hi = pol.snr_centi
  _lib.call('st_wave_augment_plan_host', _p(lens), _p(ids), len(lens), augment.seed, _p(speeds), len(speeds), pol.noise_prob_q16, lo, hi,
            None if clip_lens is None else _p(clip_lens), 0 if clip_lens is None else len(clip_lens), int(min_samples), _p(plan))
  return plan


def _cat(waves):
  waves = [np.ascontiguousarray(w, dtype=np.float32).reshape(-1) for w in waves]
  offsets = np.concatenate([[0], np.cumsum([len(w) for w in waves])]).astype(np.int64)
  return (np.concatenate(waves) if waves else np.zeros(0, np.float32)), offsets


def out_offsets_of(plan, align=4):
  """Where each utterance's output starts: one after the other, every start a multiple of `align` samples (16-byte stores)."""
  M = np.asarray(plan['M'], dtype=np.int64)
  starts = np.concatenate([[0], np.cumsum(-(-M // align) * align)]).astype(np.int64)
  return starts


def apply_wave_host(augment, waves, plan=None, min_samples=0, return_sums=False):
  """The host form (st_wave_augment_host): a list of waveforms -> (list of augmented waveforms, plans[, the two sums of squares
  [n, 2] of the noisy ones])."""
  x, in_off = _cat(waves)
  if plan is None:
    plan = plan_wave_host(augment, np.diff(in_off), min_samples)
  plan = np.ascontiguousarray(plan, dtype=PLAN_DTYPE)
  out_off = out_offsets_of(plan)
  out = np.zeros(max(1, int(out_off[-1])), dtype=np.float32)
  sums = np.zeros((len(plan), 2), dtype=np.float64)
  speeds, bank = augment.policy.c_speeds(), augment.noise
  x = x if len(x) else np.zeros(1, np.float32)
  _lib.call('st_wave_augment_host', _p(x), _p(in_off), len(plan), _p(plan), _p(speeds), len(speeds), _p(augment.tables),
            None if bank is None else _p(bank.samples), None if bank is None else _p(bank.offsets), 0 if bank is None else len(bank),
            _p(out), _p(out_off), _p(sums))
  result = [out[out_off[u]:out_off[u] + plan['M'][u]] for u in range(len(plan))]
  return (result, plan, sums) if return_sums else (result, plan)


def apply_wave_device(augment, audio, in_offsets, plan, stream=None, align=4):
  """st_wave_augment_f32 on waveforms already in HBM: ``audio`` a float32 device tensor of utterances one after the other,
  ``in_offsets`` their host int64 offsets, ``plan`` the host plans of exactly these utterances.  Returns (device tensor, host
  offsets): utterance u is out[offsets[u] : offsets[u] + plan['M'][u]]; ``align`` = 1 packs the outputs as the feature kernels
  read them (utterance u ends where u + 1 starts)."""
  import torch
  dev = audio.device
  plan = np.ascontiguousarray(plan, dtype=PLAN_DTYPE)
  in_off = np.ascontiguousarray(in_offsets, dtype=np.int64)
  n = len(plan)
  if len(in_off) != n + 1 or audio.dtype != torch.float32 or not audio.is_contiguous() or int(in_off[-1]) > audio.numel():
    raise ValueError('apply_wave_device: {} plans for offsets {} into {} float32 samples'.format(n, in_off.shape, audio.numel()))
  out_off = out_offsets_of(plan, align)
  max_out = int(plan['M'].max())
  bank = augment.noise
  lib = _lib.load()
  ws_bytes = lib.st_wave_augment_ws(n, max_out) if bank is not None else 0
  # one upload: {in offsets | out offsets | plans}, all 8-byte words
  words = np.concatenate([in_off.view(np.uint8), out_off.view(np.uint8), plan.view(np.uint8)])
  stream = stream if stream is not None else torch.cuda.current_stream(dev)
  with torch.cuda.stream(stream):
    table = torch.as_tensor(words).to(dev, non_blocking=False)
    out = torch.empty(max(1, int(out_off[-1])), dtype=torch.float32, device=dev)
    ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.float64, device=dev)
    tables = augment.device_tables(dev)
    noise, clip_off = bank.device_arrays(dev) if bank is not None else (None, None)
  base = table.data_ptr()
  P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
  speeds = augment.policy.c_speeds()
  _lib.call('st_wave_augment_f32', P(audio), ctypes.c_void_p(base), n, audio.numel(), ctypes.c_void_p(base + 16 * (n + 1)), _p(speeds),
            len(speeds), P(tables), P(noise), P(clip_off), 0 if bank is None else len(bank), P(out), ctypes.c_void_p(base + 8 * (n + 1)),
            out.numel(), max_out, P(ws), ws_bytes, ctypes.c_void_p(stream.cuda_stream))
  return out, out_off


def add_wave_arguments(parser):
  """The waveform flags of `speecht-cli train`."""
  parser.add_argument('--waveforms', dest='waveforms', action='store_true',
                      help='(extension) train from the waveform cache `speecht-cli preprocess --waveforms` wrote: the features are '
                           'computed on the device inside the step, which is what the waveform augmentations below need')
  parser.add_argument('--speed-perturb', dest='speed_perturb', default=None, metavar='S,S,..',
                      help='speeds one is drawn from per utterance and step, e.g. 0.9,1.0,1.1 (needs --waveforms)')
  parser.add_argument('--noise-dir', dest='noise_dir', default=None, metavar='DIR', help='directory of noise recordings to mix in (needs --waveforms)')
  parser.add_argument('--noise-prob', dest='noise_prob', type=float, default=None, metavar='P',
                      help='share of the utterances that get noise (default 0.5 when --noise-dir is given)')
  parser.add_argument('--noise-snr', dest='noise_snr', default=None, metavar='LO,HI',
                      help='range of the signal-to-noise ratio in dB (default 10,30: a guess, not tuned on data)')


def check_wave_flags(flags):
  """Either waveform-augmentation flag without --waveforms is an error that names --waveforms."""
  asked = [name for name, attr in (('--speed-perturb', 'speed_perturb'), ('--noise-dir', 'noise_dir'), ('--noise-prob', 'noise_prob'),
                                   ('--noise-snr', 'noise_snr')) if getattr(flags, attr, None) is not None]
  if asked and not getattr(flags, 'waveforms', False):
    raise ValueError('{} needs --waveforms: the waveform augmentations act before the features, and training from the feature cache '
                     'has no waveform'.format(', '.join(asked)))


def wave_from_flags(flags, rate=None, device='cuda:0', bank=None):
  """The WaveAugment the train flags ask for, or None for the identity policy.  Either augmentation flag without --waveforms is an
  error.  ``bank``: a NoiseBank to use instead of reading --noise-dir."""
  check_wave_flags(flags)
  speeds, noise_dir = getattr(flags, 'speed_perturb', None), getattr(flags, 'noise_dir', None)
  prob = getattr(flags, 'noise_prob', None)
  if noise_dir is None and bank is None:
    if prob:
      raise ValueError('--noise-prob needs --noise-dir')
    prob = 0.0
  elif prob is None:
    prob = 0.5
  snr = getattr(flags, 'noise_snr', None)
  policy = WavePolicy(tuple(float(s) for s in speeds.split(',')) if speeds else ((1, 1),), prob,
                      tuple(float(s) for s in snr.split(',')) if snr else (10.0, 30.0))
  if policy.is_identity:
    return None
  if policy.noise_prob > 0 and bank is None:
    bank = NoiseBank.from_directory(noise_dir, rate, device)
  seed = getattr(flags, 'augment_seed', None)
  if seed is None:
    seed = getattr(flags, 'seed', None) or 0
  return WaveAugment(policy, seed, bank if policy.noise_prob > 0 else None)
