"""The whole-utterance feature kernels of csrc/melspec.hip (st_melspec_f32, st_mfcc_f32) against the float64 oracle on the case
table of tests/feature_cases.py (checked on the CPU by tests/test_feature_cases_cpu.py): clips on every frame, pair, wave,
workgroup and slot boundary of mel_pair_kernel, both load paths, floored and amin-clamped signals on aligned and unaligned
rows, six filterbank widths at four sample rates, four hops, four MFCC widths, clips shorter than the delta window -- and every
utterance of every batch again on its own.

Bounds: 1e-3 on the z-normalised mel features, 2e-3 on the three MFCC blocks (the project's tolerances); bit-identity between
an utterance in a batch and alone, except for n_mels % 4 != 0 on floored clips, where the statistics pass sums 16-byte chunks
or single floats depending on the row offset: there 4 float32 ulp of max(|x|, 1).

Worst device errors measured (MI355X; every test prints its own):
  mel, bound 1e-3:   1.0e-4 on the 513-frame chirp at 128 mels, 4.4e-5 speech-like (1 201 frames), 3.9e-5 noise, 3.8e-5 / 2.0e-5
                     the -85 / -75 dB pair, 2.7e-5 quiet (sigma = 3e-6), <= 7.6e-6 on every edge length at 80 mels, <= 5.9e-6
                     at 13 mels, <= 6.8e-5 over the 24 filterbanks, <= 5.1e-5 at hops 80 / 128 / 200
  MFCC, bound 2e-3:  1.9e-4 on the sigma = 3e-6 clip (40 mels, 32 coefficients), 3.8e-5 sigma = 1e-5, 1.7e-5 int16 scale,
                     <= 1.1e-5 on every other kind; the first three delta-delta frames <= 1.3e-5
Every bit-identity asserted below held."""
import ctypes

import numpy as np
import pytest
import torch

from tests import feature_cases as FC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


# ---- device calls -----------------------------------------------------------------------------------------------------------

def _offsets(audio_list, hop):
  lens = np.array([len(a) for a in audio_list], dtype=np.int64)
  s_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
  f_off = np.concatenate([[0], np.cumsum(1 + lens // hop)]).astype(np.int64)
  return lens, s_off, f_off


def direct_call(dev, entry, audio_list, sr, n_mels, hop, n_mfcc=None):
  """st_melspec_f32 (n_mfcc None) or st_mfcc_f32 through ctypes -> list of [frames, width] float32 arrays.  The output buffer
  carries a sentinel row behind the last frame."""
  from speecht_amd import _lib
  from speecht_amd.preprocessing import mel_filterbank
  assert entry == ('st_melspec_f32' if n_mfcc is None else 'st_mfcc_f32')
  lib = _lib.load()
  lens, s_off, f_off = _offsets(audio_list, hop)
  total, width = int(f_off[-1]), n_mels if n_mfcc is None else 3 * n_mfcc
  d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
  x, so, fo = d(np.concatenate(audio_list)), d(s_off), d(f_off)
  basis = d(mel_filterbank(float(sr), 512, n_mels).astype(np.float32))
  need = lib.st_melspec_ws(len(lens), total, n_mels) if n_mfcc is None else lib.st_mfcc_ws(len(lens), total, n_mels, n_mfcc)
  ws = torch.empty(need // 4 + 64, dtype=torch.float32, device=dev)
  out = torch.full(((total + 1) * width,), -777.25, dtype=torch.float32, device=dev)
  P = lambda t: ctypes.c_void_p(t.data_ptr())
  head = (P(x), P(so), len(lens), int(lens.max()), P(basis), n_mels)
  tail = (512, hop, P(fo), total, P(out), P(ws), ws.numel() * 4, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
  _lib.call(entry, *(head + (() if n_mfcc is None else (n_mfcc,)) + tail))
  host = out.view(total + 1, width).cpu().numpy()
  assert (host[total] == -777.25).all()                    # nothing behind the last frame
  return [host[f_off[i]:f_off[i + 1]] for i in range(len(lens))]


def device_mel(dev, clips, sr, n_mels, hop):
  from speecht_amd.preprocessing import calc_power_spectrogram_batch
  return calc_power_spectrogram_batch([c.audio for c in clips], sr, n_mels=n_mels, hop_length=hop, device=dev)


def device_mfcc(dev, batch, clips):
  from speecht_amd.preprocessing import calc_mfccs_batch
  audio = [c.audio for c in clips]
  if batch.direct:
    return direct_call(dev, 'st_mfcc_f32', audio, batch.sr, batch.n_mels, batch.hop, batch.n_mfcc)
  assert batch.n_mels == 128                                # what calc_mfccs_batch computes
  return calc_mfccs_batch(audio, batch.sr, n_mfcc=batch.n_mfcc, hop_length=batch.hop, device=dev)


_SOLO = {}


def solo_mel(dev, c, sr, n_mels, hop):
  """The clip's features from a batch of its own, computed once per (clip, filterbank, hop)."""
  key = (c.name, sr, n_mels, hop)
  if key not in _SOLO:
    _SOLO[key] = device_mel(dev, [c], sr, n_mels, hop)[0]
  return _SOLO[key]


def same_bits(a, b):
  return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def within_ulps(a, b, ulps):
  scale = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.float32(1.0))
  return a.shape == b.shape and bool(np.all(np.abs(a.astype(np.float64) - b) <= ulps * np.spacing(scale).astype(np.float64)))


def _report(name, worst):
  print('{}: worst error against float64: {}'.format(name, ', '.join('{} {:.2e}'.format(k, v) for k, v in worst.items())))


# ---- mel --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', FC.MEL_BATCH_NAMES)
def test_mel_against_the_oracle_and_every_utterance_alone(dev, name):
  batch = FC.mel_batch(name)
  refs = FC.mel_references(batch)
  feats = device_mel(dev, batch.clips, batch.sr, batch.n_mels, batch.hop)
  assert len(feats) == len(batch.clips)
  worst = {}
  for i, (c, f, ref) in enumerate(zip(batch.clips, feats, refs)):
    assert f.shape == ref.shape == (1 + len(c.audio) // batch.hop, batch.n_mels) and f.dtype == np.float32, c.name
    if c.kind == 'zeros':                                   # 0/0 in the reference: only a neighbour
      continue
    assert np.isfinite(f).all(), c.name
    err = float(np.max(np.abs(f - ref)))
    worst[c.kind] = max(worst.get(c.kind, 0.0), err)
    assert err < FC.MEL_TOL, (name, i, c.name, err, np.unravel_index(np.argmax(np.abs(f - ref)), f.shape))
  _report(name, worst)
  # every utterance alone: another grid, other slot counts, other row offsets
  for i, (c, f) in enumerate(zip(batch.clips, feats)):
    if c.kind == 'zeros':
      continue
    alone = solo_mel(dev, c, batch.sr, batch.n_mels, batch.hop)
    lowest = FC.mel_shares(c.audio, batch.sr, batch.n_mels, batch.hop)[2] if batch.n_mels % 4 else 0.0
    if batch.n_mels % 4 == 0 or lowest > -79.0:             # aligned rows, or the closed form of an unfloored clip
      assert same_bits(f, alone), (name, i, c.name, float(np.max(np.abs(f - alone))))
    else:
      assert within_ulps(f, alone, 4), (name, i, c.name, float(np.max(np.abs(f - alone))))


def test_mel_direct_entry_point_equals_the_python_one(dev):
  """st_melspec_f32 through the shared ctypes helper, at a hop other than 160 and at 13 mels."""
  for name in ('hop-200', 'unaligned-13'):
    batch = FC.mel_batch(name)
    direct = direct_call(dev, 'st_melspec_f32', [c.audio for c in batch.clips], batch.sr, batch.n_mels, batch.hop)
    for a, b in zip(direct, device_mel(dev, batch.clips, batch.sr, batch.n_mels, batch.hop)):
      assert same_bits(a, b)


def test_the_silent_neighbour_changes_nothing(dev):
  """An all-zero utterance (every mel power on amin, deviation 0) between two ordinary ones: theirs are the bits of the batch
  without it.  Its own rows (0/0) are not compared."""
  b, w = FC.mel_batch('silent-neighbour'), FC.mel_batch('silent-neighbour-without')
  with_it = device_mel(dev, b.clips, b.sr, b.n_mels, b.hop)
  without = device_mel(dev, w.clips, w.sr, w.n_mels, w.hop)
  assert same_bits(with_it[0], without[0]) and same_bits(with_it[2], without[1])
  assert with_it[1].shape == (1 + len(b.clips[1].audio) // b.hop, b.n_mels)
  for f, ref in zip(without, FC.mel_references(w)):
    assert np.max(np.abs(f - ref)) < FC.MEL_TOL


def test_no_jump_between_the_closed_form_and_the_statistics_pass(dev):
  """The -75 / -85 dB pair: the first takes the closed-form statistics, the second the statistics pass, on almost the same
  data; both within tolerance, and no further apart than their references plus twice the tolerance."""
  batch = FC.mel_batch('branch-pair')
  ref_a, _, ref_b = FC.mel_references(batch)
  a, _, b = device_mel(dev, batch.clips, batch.sr, batch.n_mels, batch.hop)
  err_a, err_b = float(np.max(np.abs(a - ref_a))), float(np.max(np.abs(b - ref_b)))
  gap, ref_gap = float(np.max(np.abs(a - b))), float(np.max(np.abs(ref_a - ref_b)))
  print('branch pair: errors {:.2e} / {:.2e}, apart {:.4f} (references {:.4f})'.format(err_a, err_b, gap, ref_gap))
  assert err_a < FC.MEL_TOL and err_b < FC.MEL_TOL
  assert gap <= ref_gap + 2 * FC.MEL_TOL
  assert np.all(np.abs(a - b) <= np.abs(ref_a - ref_b) + 2 * FC.MEL_TOL)


# ---- MFCC -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', FC.MFCC_BATCH_NAMES)
def test_mfcc_against_the_oracle_and_every_utterance_alone(dev, name):
  batch = FC.mfcc_batch(name)
  refs = FC.mfcc_references(name)
  feats = device_mfcc(dev, batch, batch.clips)
  k = batch.n_mfcc
  worst, worst_leak = {}, 0.0
  for i, (c, f, ref) in enumerate(zip(batch.clips, feats, refs)):
    assert f.shape == ref.shape == (1 + len(c.audio) // batch.hop, 3 * k) and f.dtype == np.float32, c.name
    assert np.isfinite(f).all(), c.name
    # the delta-delta's start-up leak (the filter at rest reaches into its first three frames) on its own
    leak = float(np.max(np.abs(f[:3, 2 * k:] - ref[:3, 2 * k:])))
    worst_leak = max(worst_leak, leak)
    assert leak < FC.MFCC_TOL, (name, i, c.name, 'first three delta-delta frames', leak)
    for block, what in enumerate(('mfcc', 'delta', 'delta-delta')):
      err = float(np.max(np.abs(f[:, block * k:(block + 1) * k] - ref[:, block * k:(block + 1) * k])))
      worst[c.kind] = max(worst.get(c.kind, 0.0), err)
      assert err < FC.MFCC_TOL, (name, i, c.name, what, err)
  _report(name, worst)
  print('{}: first three delta-delta frames {:.2e}'.format(name, worst_leak))
  for i, (c, f) in enumerate(zip(batch.clips, feats)):
    alone = device_mfcc(dev, batch, [c])[0]
    assert same_bits(f, alone), (name, i, c.name, float(np.max(np.abs(f - alone))))
