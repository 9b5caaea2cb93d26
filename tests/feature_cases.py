"""The case table of the feature front end tests (tests/test_feature_cases_cpu.py keeps it honest on the CPU,
tests/test_gpu_features.py runs it through csrc/melspec.hip).  Pure numpy; float32 signals, every one seeded by its name.

What the lengths sit on (hop 160; frames = 1 + n // hop, pairs = (frames + 1) // 2, a wave of mel_pair_kernel owns 4 pairs, a
workgroup 16, an utterance wave_slots() slots of maxima and sums; pair 0 always reflects, a later pair is loaded straight once
j0 = 2 p hop - 256 >= 0 and j0 + hop + 512 <= n):

  257            2 frames   the shortest legal utterance: one pair, both ends reflect into the same frame
  319 / 320      2 -> 3     a half-empty last pair appears
  479 / 480      3 -> 4
  735 / 736                 pair 1 reflects / is the first straight load
  1119/1120/1280 7 / 8 / 9  one wave exactly, then a second wave holding a single half pair
  4959/4960/5120 31/32/33   one workgroup exactly, then a second workgroup holding a single half pair
  81919 / 81920  512 / 513  64 -> 68 slots: the second pass of utterance_stats() / utterance_max()'s lane-strided loop
  192077         1201       152 slots (three passes), 12 s of audio: the longest input of the table

Signal kinds (KINDS): what each promises about power_to_db's amin = 1e-10 clamp and its -80 dB floor is PROMISES, checked at
80 mels / 16 kHz by the CPU test.  'pair75' / 'pair85' are the same tone and the same noise, the noise scaled so that the
weakest mel value of the clip lies about 75 dB / 85 dB under the strongest: the first is unfloored (closed-form statistics), the
second is not (statistics pass), on almost the same data.  'zeros' is the all-zero utterance: its reference is 0/0, it is only
ever a neighbour."""
import functools
import zlib
from collections import namedtuple

import numpy as np

NFFT = 512
PAIRS_PER_WAVE = 4
MEL_TOL = 1e-3            # the project's tolerance on z-normalised mel features (tests/test_gpu_parity.py)
MFCC_TOL = 2e-3           # ... and on the three MFCC blocks

# length -> frames at hop 160
LENGTHS = {257: 2, 319: 2, 320: 3, 479: 3, 480: 4, 735: 5, 736: 5, 1119: 7, 1120: 8, 1280: 9, 4959: 31, 4960: 32, 5120: 33,
           81919: 512, 81920: 513, 192077: 1201}
LONGEST = 192077

KINDS = ('noise', 'noise_zeros', 'zeros_noise', 'tone', 'chirp', 'impulse', 'dc', 'speech', 'int16', 'quiet1e-5', 'quiet3e-6',
         'pair75', 'pair85')
# kind -> (share of mel powers under amin, share of dB values on the floor): 'none' = 0, 'some' = strictly between 0 and 1
PROMISES = {'noise': ('none', 'none'), 'noise_zeros': ('some', 'some'), 'zeros_noise': ('some', 'some'),
            'tone': ('some', 'some'), 'chirp': ('some', 'some'), 'impulse': ('some', 'some'), 'dc': ('some', 'some'),
            'speech': ('some', 'some'), 'int16': ('none', 'none'), 'quiet1e-5': ('some', 'none'),
            'quiet3e-6': ('some', 'none'), 'pair75': ('none', 'none'), 'pair85': ('none', 'some')}
MFCC_KINDS = tuple(k for k in KINDS if k != 'dc')      # DC's deltas are rounding noise: float32 is 5.5 off float64 on it

N_MELS = (1, 13, 40, 80, 128, 256)
RATES = (8000, 16000, 22050, 48000)
HOPS = (80, 128, 160, 200)
N_MFCC = (1, 13, 20, 32)
MFCC_DIRECT = ((40, 32), (13, 13))                     # (n_mels, n_mfcc) through st_mfcc_f32 itself

PAIR_TONE = 0.5
PAIR_NOISE = {'pair75': 4e-3, 'pair85': 4e-3 * 10.0 ** -0.5}     # the second 10 dB under the first

Clip = namedtuple('Clip', 'name kind audio')
MelBatch = namedtuple('MelBatch', 'name n_mels sr hop clips')
MfccBatch = namedtuple('MfccBatch', 'name n_mels n_mfcc sr hop clips direct')


# ---- the kernel's launch geometry, restated ---------------------------------------------------------------------------------

def frames_of(n, hop=160):
  return 1 + n // hop


def pairs_of(n, hop=160):
  return (frames_of(n, hop) + 1) // 2


def wave_slots(max_frames):
  """melspec.hip's wave_slots(): 4 per workgroup of 16 pairs."""
  return ((max_frames + 1) // 2 + 4 * PAIRS_PER_WAVE - 1) // (4 * PAIRS_PER_WAVE) * 4


def straight_pairs(n, hop=160):
  """The frame pairs that load_pair() reads without reflection."""
  return [p for p in range(pairs_of(n, hop)) if 2 * p * hop - NFFT // 2 >= 0 and 2 * p * hop - NFFT // 2 + hop + NFFT <= n]


def first_straight_length(hop):
  """The shortest utterance in which some pair is loaded straight."""
  p = -(-(NFFT // 2) // (2 * hop))
  return 2 * p * hop - NFFT // 2 + hop + NFFT


# ---- signals ----------------------------------------------------------------------------------------------------------------

def _rng(name):
  return np.random.default_rng(zlib.crc32(name.encode()))


def _make(kind, n, sr, rng):
  t = np.arange(n, dtype=np.float64)
  noise = lambda sigma: sigma * rng.standard_normal(n)
  if kind == 'noise':
    return noise(0.1)
  if kind == 'zeros':
    return np.zeros(n)
  if kind in ('noise_zeros', 'zeros_noise'):
    y = noise(0.1)
    cut = n // 2 + 3
    if kind == 'noise_zeros':
      y[cut:] = 0.0
    else:
      y[:cut] = 0.0
    return y
  if kind == 'tone':
    return 0.8 * np.sin(2 * np.pi * 1000.0 * t / sr)
  if kind == 'chirp':                                     # linear, 100 Hz -> sr / 2 over the clip
    f0, f1 = 100.0, sr / 2.0
    return 0.5 * np.sin(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / n) / sr)
  if kind == 'impulse':
    y = np.zeros(n)
    y[(2 * n) // 3] = 1.0
    return y
  if kind == 'dc':
    return np.full(n, 0.5)
  if kind == 'speech':                                    # bursts of harmonics with exact-zero pauses between them
    y = np.zeros(n)
    burst = max(64, n // 7)
    for i, start in enumerate(range(burst // 2, n - burst, 2 * burst)):
      f0 = 110.0 + 35.0 * i
      seg = t[:burst]
      env = np.sin(np.pi * (seg + 0.5) / burst) ** 2
      y[start:start + burst] = env * sum(0.3 / h * np.sin(2 * np.pi * h * f0 * seg / sr + h) for h in range(1, 9))
    return y
  if kind == 'int16':
    return 8000.0 * noise(0.1)
  if kind == 'quiet1e-5':
    return noise(1e-5)
  if kind == 'quiet3e-6':
    return noise(3e-6)
  if kind in PAIR_NOISE:
    g = np.random.default_rng(75).standard_normal(n)      # the SAME noise in both clips of the pair
    return PAIR_TONE * np.sin(2 * np.pi * 1000.0 * t / sr) + PAIR_NOISE[kind] * g
  raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def clip(kind, n, sr=16000):
  name = '{}-{}'.format(kind, n) + ('' if sr == 16000 else '@{}'.format(sr))
  audio = np.ascontiguousarray(_make(kind, n, sr, _rng(name)), dtype=np.float32)
  audio.setflags(write=False)
  return Clip(name, kind, audio)


# ---- mel batches ------------------------------------------------------------------------------------------------------------

def _hop_lengths(hop):
  n = first_straight_length(hop)
  return (257, n - 1, n, 8 * hop - 1, 8 * hop, 32 * hop)


@functools.lru_cache(maxsize=None)
def mel_batches():
  c = clip
  out = [
      MelBatch('short-edges', 80, 16000, 160,
               tuple(c('noise', n) for n in (257, 319, 320, 479, 480, 735, 736, 1119, 1120, 1280))),
      MelBatch('workgroup-edges', 80, 16000, 160, (c('noise', 4959), c('noise_zeros', 4960), c('noise', 5120), c('int16', 257),
                                                  c('noise', 4960), c('zeros_noise', 5120))),
      # the shortest clip first / last beside the longest: idle workgroups, idle slots, frame_off even / odd
      MelBatch('slots-shortest-first', 80, 16000, 160,
               (c('noise', 257), c('noise', LONGEST), c('noise_zeros', 81919), c('noise', 81920))),
      MelBatch('slots-shortest-last', 128, 16000, 160,
               (c('chirp', 81920), c('zeros_noise', 81920), c('speech', LONGEST), c('noise', 257))),
      MelBatch('kinds', 80, 16000, 160,
               tuple(c(k, n) for k, n in zip(KINDS, (4960, 5120, 4959, 1280, 5120, 1119, 736, 4960, 480, 4959, 5120, 4000, 4000)))),
      # 13 mels: frame_off * n_mels is a multiple of 4 only for every fourth offset -- floored clips on the scalar path
      MelBatch('unaligned-13', 13, 16000, 160, (c('noise', 257), c('noise_zeros', 5120), c('zeros_noise', 4959), c('speech', 1280),
                                                c('dc', 320), c('noise', 1119), c('tone', 736))),
      MelBatch('branch-pair', 80, 16000, 160, (c('pair75', 4000), c('noise', 257), c('pair85', 4000))),
      MelBatch('silent-neighbour', 80, 16000, 160, (c('noise', 1280), c('zeros', 1120), c('tone', 4960))),
      MelBatch('silent-neighbour-without', 80, 16000, 160, (c('noise', 1280), c('tone', 4960))),
  ]
  for n_mels in N_MELS:
    for sr in RATES:
      out.append(MelBatch('bank-{}-{}'.format(n_mels, sr), n_mels, sr, 160,
                          (c('chirp', 4959, sr), c('noise', 1120, sr), c('noise_zeros', 1280, sr), c('noise', 257, sr))))
  for hop in HOPS:
    if hop != 160:
      kinds = ('noise', 'noise', 'noise', 'noise_zeros', 'noise', 'chirp')
      out.append(MelBatch('hop-{}'.format(hop), 80, 16000, hop, tuple(c(k, n) for k, n in zip(kinds, _hop_lengths(hop)))))
  return tuple(out)


MEL_BATCH_NAMES = tuple(['short-edges', 'workgroup-edges', 'slots-shortest-first', 'slots-shortest-last', 'kinds', 'unaligned-13',
                         'branch-pair', 'silent-neighbour', 'silent-neighbour-without'] +
                        ['bank-{}-{}'.format(m, sr) for m in N_MELS for sr in RATES] +
                        ['hop-{}'.format(h) for h in HOPS if h != 160])


def mel_batch(name):
  return next(b for b in mel_batches() if b.name == name)


# ---- MFCC batches -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mfcc_clips():
  """2, 3, 8, 9, 10 and 33 frames -- shorter than, as long as and just longer than the 9-tap delta window and the 9-frame edge
  pad -- then a floored clip, the quiet and the int16-scale ones, and the other kinds (not DC)."""
  c = clip
  return (c('noise', 257), c('noise', 320), c('noise', 1120), c('noise', 1280), c('noise', 1440), c('noise', 5120),
          c('noise_zeros', 4960), c('quiet1e-5', 4959), c('quiet3e-6', 5120), c('int16', 1280), c('zeros_noise', 1440),
          c('tone', 1120), c('chirp', 4960), c('impulse', 1280), c('speech', 4959), c('pair75', 4000), c('pair85', 4000))


@functools.lru_cache(maxsize=None)
def mfcc_batches():
  # one coefficient over two frames: the delta of the two frames is the same number twice, the reference's deviation is 0 and
  # its delta block 0/0 -- the 2-frame clip is left out of the n_mfcc = 1 batch (3 frames are its shortest)
  clips = lambda k: tuple(c for c in mfcc_clips() if k > 1 or len(c.audio) >= 320)
  out = [MfccBatch('mfcc-128-{}'.format(k), 128, k, 16000, 160, clips(k), False) for k in N_MFCC]
  out += [MfccBatch('mfcc-{}-{}'.format(m, k), m, k, 16000, 160, mfcc_clips(), True) for m, k in MFCC_DIRECT]
  return tuple(out)


MFCC_BATCH_NAMES = tuple(['mfcc-128-{}'.format(k) for k in N_MFCC] + ['mfcc-{}-{}'.format(m, k) for m, k in MFCC_DIRECT])


def mfcc_batch(name):
  return next(b for b in mfcc_batches() if b.name == name)


# ---- the float64 references, computed once per process and shared (do not modify) -------------------------------------------

@functools.lru_cache(maxsize=None)
def mel_reference(kind, n, clip_sr, n_mels, hop):
  from oracle import w2l_oracle as O
  with np.errstate(invalid='ignore', divide='ignore'):
    ref = O.calc_power_spectrogram(clip(kind, n, clip_sr).audio, clip_sr, n_mels=n_mels, hop_length=hop)
  ref.setflags(write=False)
  return ref


def mel_references(batch):
  """[frames, n_mels] float64 of every clip of a mel batch (NaN throughout for the all-zero utterance)."""
  return tuple(mel_reference(c.kind, len(c.audio), batch.sr, batch.n_mels, batch.hop) for c in batch.clips)


@functools.lru_cache(maxsize=None)
def mfcc_references(name):
  from oracle import w2l_oracle as O
  b = mfcc_batch(name)
  out = []
  for c in b.clips:
    ref = O.calc_mfccs(c.audio, b.sr, n_mfcc=b.n_mfcc, hop_length=b.hop, n_mels=b.n_mels)
    ref.setflags(write=False)
    out.append(ref)
  return tuple(out)


def mel_shares(audio, sr=16000, n_mels=80, hop=160):
  """(share of mel powers under amin, share of dB values on the -80 floor, smallest dB value) in the float64 oracle."""
  from oracle import w2l_oracle as O
  S = O.mel_filterbank(sr, NFFT, n_mels) @ O.stft_power(audio, NFFT, hop)
  db = O.power_to_db(S)
  return float(np.mean(S < 1e-10)), float(np.mean(db <= db.max() - 80.0)), float(db.min() - db.max())
