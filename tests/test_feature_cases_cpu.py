"""Keeps the case table of the feature front end tests (tests/feature_cases.py) honest, and shows on the CPU that the tolerances
the GPU test (tests/test_gpu_features.py) asserts are reachable in float32 before any kernel is involved: a numpy float32
restatement of the chain (float32 frames through scipy.fft.rfft, which stays in complex64; mel product, log2, dB and the three
MFCC blocks in float32; mean and deviation in double and rounded once, as the kernels do) has to land within a QUARTER of the
tolerance against the float64 oracle on every case.

Floors measured here (worst float32-model error against float64, per group; printed by the last two tests):
  mel, bound 2.5e-4:  1.1e-4 on the 513-frame chirp at 128 mels, 6.4e-5 speech-like, 5.3e-5 the -85 dB clip of the pair,
                      3.9e-5 noise (128 mels), 1.4e-5 quiet (sigma = 3e-6), <= 3.7e-6 on every edge length at 80 mels,
                      <= 5.7e-5 over the 24 filterbanks, <= 4.7e-5 at hops 80 / 128 / 200
  MFCC, bound 5e-4:   2.0e-4 on the sigma = 3e-6 clip (its delta block: c0 = -1 131 is worth 1.2e-4 per float32 ulp against a
                      deviation of 0.15), 3.3e-5 sigma = 1e-5, 2.2e-5 int16 scale, <= 9.1e-6 on every other kind
The model sums the cosine projection in mfcc_dct_kernel's order (a BLAS product's blocking moved the quiet clip's c0 by an ulp
from 33 frames on: 9e-4).  One coefficient over two frames has a constant delta (deviation 0, 0/0 in the reference): the
2-frame clip is not in the n_mfcc = 1 batch.  DC is no MFCC case: its deltas are pure rounding noise and this model differs from float64 by 5.5 on it."""
import numpy as np
import pytest
import scipy.fft

from oracle import w2l_oracle as O
from tests import feature_cases as FC


# ---- the lengths ------------------------------------------------------------------------------------------------------------

def _slots(max_frames):
  """wave_slots() of melspec.hip, restated on its own: 16 pairs per workgroup, 4 slots per workgroup."""
  pairs = (max_frames + 1) // 2
  return 4 * ((pairs + 15) // 16)


def _straight(p, n, hop):
  """load_pair()'s wave-uniform condition for the straight path."""
  j0 = 2 * p * hop - 256
  return j0 >= 0 and j0 + hop + 512 <= n


def test_lengths_sit_on_the_frame_pair_wave_and_workgroup_edges():
  geometry = {}
  for n, frames in FC.LENGTHS.items():
    assert n > 256 and 1 + n // 160 == frames == FC.frames_of(n)
    pairs = (frames + 1) // 2
    waves, groups = -(-pairs // 4), -(-pairs // 16)
    assert FC.pairs_of(n) == pairs and FC.wave_slots(frames) == _slots(frames) == 4 * groups
    assert FC.straight_pairs(n) == [p for p in range(pairs) if _straight(p, n, 160)]
    geometry[n] = (frames, pairs, waves, groups, _slots(frames), frames % 2 == 1)
  #                 frames pairs waves groups slots half-empty last pair
  assert geometry == {257: (2, 1, 1, 1, 4, False), 319: (2, 1, 1, 1, 4, False), 320: (3, 2, 1, 1, 4, True),
                      479: (3, 2, 1, 1, 4, True), 480: (4, 2, 1, 1, 4, False), 735: (5, 3, 1, 1, 4, True),
                      736: (5, 3, 1, 1, 4, True), 1119: (7, 4, 1, 1, 4, True), 1120: (8, 4, 1, 1, 4, False),
                      1280: (9, 5, 2, 1, 4, True), 4959: (31, 16, 4, 1, 4, True), 4960: (32, 16, 4, 1, 4, False),
                      5120: (33, 17, 5, 2, 8, True), 81919: (512, 256, 64, 16, 64, False),
                      81920: (513, 257, 65, 17, 68, True), 192077: (1201, 601, 151, 38, 152, True)}
  # (the issue counts 304 slots for 1 201 frames; wave_slots() gives 4 per 16 pairs = 152: more than two passes of the
  # 64-lane loop either way)
  assert _slots(1201) > 2 * 64 and _slots(513) > 64 >= _slots(512)
  # pair 1 is the first that can be loaded straight, and only from 736 samples on; pair 0 never is
  assert FC.straight_pairs(735) == [] and FC.straight_pairs(736) == [1] and FC.first_straight_length(160) == 736
  assert all(0 not in FC.straight_pairs(n) for n in FC.LENGTHS)
  # the last pair always reflects (its second frame, or its empty partner, ends past the utterance)
  assert all(FC.pairs_of(n) - 1 not in FC.straight_pairs(n) for n in FC.LENGTHS)
  # 257 samples: frame 0 reflects at the start, frame 1 at the end -- and frame 0's window reaches the end as well
  assert 0 - 256 < 0 and 0 + 255 < 257 <= 160 + 255


def test_every_length_kind_filterbank_and_hop_is_in_a_batch():
  batches = FC.mel_batches()
  assert tuple(b.name for b in batches) == FC.MEL_BATCH_NAMES
  base = [b for b in batches if b.hop == 160 and b.sr == 16000]
  assert {len(c.audio) for b in base for c in b.clips} >= set(FC.LENGTHS)
  assert {c.kind for b in base for c in b.clips} >= set(FC.KINDS)
  assert {(b.n_mels, b.sr) for b in batches} >= {(m, sr) for m in FC.N_MELS for sr in FC.RATES}
  assert {b.hop for b in batches} == set(FC.HOPS) == {80, 128, 160, 200}
  for b in batches:
    lens = [len(c.audio) for c in b.clips]
    assert len(set(lens)) > 1 and min(lens) > 256, b.name                           # ragged, and legal
    assert all(c.audio.dtype == np.float32 and not c.audio.flags.writeable for c in b.clips)
    assert max(lens) <= FC.LONGEST == 192077                                        # 12 s at 16 kHz
  # the other hops sit on their own first straight load, on one wave exactly and on a second workgroup
  for hop in (80, 128, 200):
    b = FC.mel_batch('hop-{}'.format(hop))
    lens = [len(c.audio) for c in b.clips]
    n = FC.first_straight_length(hop)
    assert FC.straight_pairs(n - 1, hop) == [] and len(FC.straight_pairs(n, hop)) == 1 and {257, n - 1, n} <= set(lens)
    assert {FC.frames_of(x, hop) for x in lens} >= {8, 9, 33}


def test_batch_positions():
  first, last = FC.mel_batch('slots-shortest-first'), FC.mel_batch('slots-shortest-last')
  for b, at in ((first, 0), (last, len(last.clips) - 1)):
    lens = [len(c.audio) for c in b.clips]
    assert lens[at] == 257 and max(lens) == FC.LONGEST
    # idle workgroups and idle slots: the batch's grid has 38 workgroups per utterance, the short clip fills one wave of one
    assert _slots(FC.frames_of(max(lens))) // 4 == 38 and FC.pairs_of(257) == 1
  off = lambda b, at: sum(FC.frames_of(len(c.audio)) for c in b.clips[:at])
  assert off(first, 0) % 2 == 0 and off(last, len(last.clips) - 1) % 2 == 1          # both parities of frame_off
  # more than 64 slots with a floored clip in the batch: the statistics pass runs behind a two-pass slot walk
  assert any(c.kind in ('noise_zeros', 'zeros_noise') and len(c.audio) >= 81919 for c in first.clips)
  # 13 mels: floored clips whose rows start off a 16-byte boundary
  b = FC.mel_batch('unaligned-13')
  unaligned = [c for i, c in enumerate(b.clips) if (off(b, i) * 13) % 4 != 0 and FC.PROMISES[c.kind][1] == 'some']
  assert b.n_mels == 13 and len(unaligned) >= 2 and {(off(b, i) * 13) % 4 for i in range(len(b.clips))} >= {1, 2, 3}
  # the all-zero utterance between two ordinary ones, and the same two without it
  b, w = FC.mel_batch('silent-neighbour'), FC.mel_batch('silent-neighbour-without')
  assert not b.clips[1].audio.any() and b.clips[0].audio.any() and b.clips[2].audio.any()
  assert (b.clips[0], b.clips[2]) == w.clips
  pair = FC.mel_batch('branch-pair')
  assert [c.kind for c in pair.clips][::2] == ['pair75', 'pair85'] and len(pair.clips[0].audio) == len(pair.clips[2].audio)


def test_mfcc_table():
  assert tuple(b.name for b in FC.mfcc_batches()) == FC.MFCC_BATCH_NAMES
  assert {(b.n_mels, b.n_mfcc) for b in FC.mfcc_batches() if not b.direct} == {(128, k) for k in (1, 13, 20, 32)}
  assert {(b.n_mels, b.n_mfcc) for b in FC.mfcc_batches() if b.direct} == {(40, 32), (13, 13)}
  clips = FC.mfcc_clips()
  for b in FC.mfcc_batches():                  # one coefficient over two frames has a constant delta: 0/0 in the reference
    assert b.clips == (clips if b.n_mfcc > 1 else tuple(c for c in clips if len(c.audio) != 257))
  assert {FC.frames_of(len(c.audio)) for c in clips} >= {2, 3, 8, 9, 10, 33}
  assert {c.kind for c in clips} == set(FC.MFCC_KINDS) == set(FC.KINDS) - {'dc'}
  assert len({len(c.audio) for c in clips}) > 1
  # the top_db floor of the MFCC's power_to_db (ref = 1.0) is active on the floored clip, and amin on the quiet ones
  for c in clips:
    S = O.mel_filterbank(16000, 512, 128) @ O.stft_power(c.audio, 512, 160)
    db = 10.0 * np.log10(np.maximum(1e-10, S))
    if c.kind in ('noise_zeros', 'zeros_noise', 'speech'):
      assert 0 < np.mean(db < db.max() - 80.0) < 1
    if c.kind.startswith('quiet'):
      assert 0 < np.mean(S < 1e-10) < 1


# ---- the kinds --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', FC.KINDS)
def test_kind_keeps_its_promise_about_amin_and_the_floor(kind):
  """At 80 mels / 16 kHz, on every clip of the kind in the hop-160 batches."""
  seen = 0
  for b in FC.mel_batches():
    if (b.n_mels, b.sr, b.hop) != (80, 16000, 160):
      continue
    for c in b.clips:
      if c.kind != kind:
        continue
      seen += 1
      under_amin, on_floor, lowest = FC.mel_shares(c.audio)
      for share, promise in zip((under_amin, on_floor), FC.PROMISES[kind]):
        assert (share == 0.0) if promise == 'none' else (0.0 < share < 1.0), (c.name, under_amin, on_floor, lowest)
      if FC.PROMISES[kind][1] == 'none':
        assert lowest > -79.0, (c.name, lowest)                # clear of the floor: float32 takes the same branch
      print('{}: {:.1%} of the mel powers under amin, {:.1%} of the dB values on the floor, lowest {:.1f} dB'.format(
          c.name, under_amin, on_floor, lowest))
  assert seen


def test_the_branch_pair_falls_on_either_side_of_the_floor():
  a, _, b = FC.mel_batch('branch-pair').clips
  (_, floor_a, low_a), (_, floor_b, low_b) = FC.mel_shares(a.audio), FC.mel_shares(b.audio)
  assert floor_a == 0.0 and -78.0 < low_a < -72.0                     # about -75 dB: every element above the floor
  assert 0.0 < floor_b < 0.1 and low_b == -80.0                       # about -85 dB: a few elements on it
  ref_a, _, ref_b = FC.mel_references(FC.mel_batch('branch-pair'))
  assert 0 < np.max(np.abs(ref_a - ref_b)) < 1.0                      # almost the same data
  print('pair: lowest {:.2f} dB / floored share {:.2%}; references differ by {:.3f}'.format(
      low_a, floor_b, np.max(np.abs(ref_a - ref_b))))


def test_quiet_shares():
  """The issue's figures at 80 mels: about 4 % and 88 % of the mel powers under amin."""
  a = FC.mel_shares(FC.clip('quiet1e-5', 4959).audio)[0]
  b = FC.mel_shares(FC.clip('quiet3e-6', 5120).audio)[0]
  assert 0.01 < a < 0.15 and 0.7 < b < 0.97, (a, b)


# ---- the filterbanks --------------------------------------------------------------------------------------------------------

def test_filterbanks_have_empty_rows_and_rows_of_more_than_three_pieces():
  widest = {}
  for n_mels in FC.N_MELS:
    for sr in FC.RATES:
      fb = O.mel_filterbank(sr, 512, n_mels).astype(np.float32)
      nz = fb != 0
      empty = int((~nz.any(axis=1)).sum())
      widest[n_mels, sr] = (empty, int(nz.sum(axis=1).max()))
  assert widest[256, 48000][0] > 0 and widest[256, 16000][0] > 0          # all-zero rows: a piece of no bins, log2(0)
  assert all(widest[m, sr][0] == 0 for m in (1, 13, 40, 80) for sr in FC.RATES)
  assert widest[13, 16000][1] > 48 and widest[1, 16000][1] > 48           # 4 plan pieces and more
  assert max(w for _, w in widest.values()) <= 257


# ---- reachability of the tolerance ------------------------------------------------------------------------------------------

def _log_mel32(audio, sr, n_mels, hop):
  """float32: log2(max(amin, mel power)) [n_mels, frames], as mel_pair_kernel leaves it."""
  f = np.float32
  y = np.pad(np.asarray(audio, dtype=f), 256, mode='reflect')
  frames = 1 + (len(y) - 512) // hop
  idx = np.arange(512)[None, :] + hop * np.arange(frames)[:, None]
  win = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(512) / 512)).astype(f)
  spec = scipy.fft.rfft(y[idx] * win[None, :], axis=1)
  assert spec.dtype == np.complex64
  power = (spec.real * spec.real + spec.imag * spec.imag).T
  S = O.mel_filterbank(sr, 512, n_mels).astype(f) @ power
  assert S.dtype == f
  return np.log2(np.maximum(S, f(1e-10)))


def _normalize32(x):
  """Mean and deviation in double, rounded once; the normalisation itself in float32."""
  d = x.astype(np.float64)
  mean = d.mean()
  inv = np.float32(1.0 / np.sqrt(max((d * d).mean() - mean * mean, 0.0)))
  return (x - np.float32(mean)) * inv


def mel_model32(audio, sr, n_mels, hop):
  f = np.float32
  l2 = _log_mel32(audio, sr, n_mels, hop)
  db = np.maximum(f(3.0102999566398120) * (l2 - l2.max()), f(-80.0))
  out = _normalize32(db).T
  assert out.dtype == f
  return out


def mfcc_model32(audio, sr, n_mels, n_mfcc, hop):
  f = np.float32
  l2 = _log_mel32(audio, sr, n_mels, hop)
  db = f(3.0102999566398120) * l2
  db = np.maximum(db, db.max() - f(80.0))
  # the cosine projection as mfcc_dct_kernel sums it: lane l takes mels l, l + 64, ... in turn, then a binary tree over the lanes
  # (a BLAS product's order is its own, and c0 = -1 131 on a quiet clip is worth 1.2e-4 per float32 ulp)
  prod = np.zeros((n_mfcc, 256, db.shape[1]), dtype=f)
  prod[:, :n_mels] = O.dct_basis(n_mfcc, n_mels).astype(f)[:, :, None] * db[None, :, :]
  lanes = prod[:, 0:64] + prod[:, 64:128] + prod[:, 128:192] + prod[:, 192:256]
  for o in (32, 16, 8, 4, 2, 1):
    lanes = lanes[:, :o] + lanes[:, o:2 * o]
  coef = lanes[:, 0]
  w = (np.arange(4.0, -5.0, -1.0) / 60.0).astype(f)

  def delta(x):                                             # one causal pass from rest over the padded axis
    y = np.zeros_like(x)
    for k, wk in enumerate(w):
      y[:, k:] += wk * x[:, :x.shape[1] - k]
    return y

  T = coef.shape[1]
  pad = np.pad(coef, [(0, 0), (9, 9)], mode='edge')
  d1 = delta(pad)
  d2 = delta(d1)
  cut = slice(pad.shape[1] - 5 - T, pad.shape[1] - 5)
  out = np.concatenate([_normalize32(coef), _normalize32(d1[:, cut]), _normalize32(d2[:, cut])], axis=0).T
  assert out.dtype == f
  return out


@pytest.mark.parametrize('name', FC.MEL_BATCH_NAMES)
def test_mel_references_are_finite_and_the_float32_model_reaches_a_quarter_of_the_tolerance(name):
  batch = FC.mel_batch(name)
  worst = {}
  for c, ref in zip(batch.clips, FC.mel_references(batch)):
    assert ref.shape == (1 + len(c.audio) // batch.hop, batch.n_mels) and ref.dtype == np.float64
    if c.kind == 'zeros':
      assert np.isnan(ref).all()                             # 0/0: only ever a neighbour
      continue
    assert np.isfinite(ref).all(), c.name
    err = float(np.max(np.abs(mel_model32(c.audio, batch.sr, batch.n_mels, batch.hop) - ref)))
    worst[c.kind] = max(worst.get(c.kind, 0.0), err)
    assert err <= 0.25 * FC.MEL_TOL, (c.name, err)
  print('{}: float32 model against float64, worst {}'.format(name, ', '.join('{} {:.1e}'.format(k, v) for k, v in worst.items())))


@pytest.mark.parametrize('name', FC.MFCC_BATCH_NAMES)
def test_mfcc_references_are_finite_and_the_float32_model_reaches_a_quarter_of_the_tolerance(name):
  batch = FC.mfcc_batch(name)
  worst = {}
  for c, ref in zip(batch.clips, FC.mfcc_references(name)):
    assert ref.shape == (1 + len(c.audio) // batch.hop, 3 * batch.n_mfcc) and np.isfinite(ref).all(), c.name
    err = float(np.max(np.abs(mfcc_model32(c.audio, batch.sr, batch.n_mels, batch.n_mfcc, batch.hop) - ref)))
    worst[c.kind] = max(worst.get(c.kind, 0.0), err)
    assert err <= 0.25 * FC.MFCC_TOL, (c.name, err)
  print('{}: float32 model against float64, worst {}'.format(name, ', '.join('{} {:.1e}'.format(k, v) for k, v in worst.items())))
