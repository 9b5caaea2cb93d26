"""`speecht-cli transcribe` without a GPU: the library exports, the CLI surface, the resampling length planner against the
inline float64 expressions of the host path, the shared tap selection of csrc/resample_map.h through the host form of the
kernel (st_resample_kaiser_host) against audio_io.resample_kaiser_best + fix_length, and the path handling."""
import ctypes
import importlib.machinery
import importlib.util
import math
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_FLAC = os.path.join(ROOT, 'tests', 'golden', '1089-134686-0037.flac')
RATE_PAIRS = [(8000, 22050), (16000, 22050), (22050, 22050), (44100, 22050), (48000, 22050), (22050, 16000)]


def _cli():
  loader = importlib.machinery.SourceFileLoader('speecht_cli_transcribe', os.path.join(ROOT, 'speecht-cli'))
  spec = importlib.util.spec_from_loader('speecht_cli_transcribe', loader)
  cli = importlib.util.module_from_spec(spec)
  loader.exec_module(cli)
  return cli


def test_library_exports_the_resampler():
  from speecht_amd import _lib
  lib = _lib.load()
  assert hasattr(lib, 'st_resample_kaiser_f32')
  assert hasattr(lib, 'st_resample_kaiser_host')


def test_transcribe_help_and_defaults():
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'speecht-cli'), 'transcribe', '--help'], capture_output=True,
                     text=True, timeout=120)
  assert r.returncode == 0, r.stderr
  for flag in ('--sample-rate', '--output', '--language-model', '--beam-width', '--beam-input', '--lm-weight', '--mfcc',
               '--power', '--run-name', '--train-dir', '--device', '--batch-size'):
    assert flag in r.stdout, flag
  assert 'masked' in r.stdout                                      # the batch-size caveat is stated
  cli = _cli()
  _, flags = cli.parse(['transcribe', 'a.flac'])
  assert (flags.batch_size, flags.sample_rate, flags.paths, flags.feature_type) == (1, 22050, ['a.flac'], 'power')
  _, flags = cli.parse(['transcribe', '--sample-rate', 'native', '--batch-size', '8', 'a.flac', 'd'])
  assert (flags.batch_size, flags.sample_rate, flags.paths) == (8, 'native', ['a.flac', 'd'])
  _, flags = cli.parse(['train'])
  assert flags.batch_size == 64                                    # the other commands keep their default
  _, flags = cli.parse(['preprocess', '--device-resample'])
  assert flags.device_resample
  with pytest.raises(SystemExit):
    cli.parse(['transcribe', '--sample-rate', 'fast', 'a.flac'])
  with pytest.raises(SystemExit):
    cli.parse(['transcribe'])                                      # PATH is required


def test_record_still_not_provided():
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'speecht-cli'), 'record'], capture_output=True, text=True, timeout=120)
  assert r.returncode == 2


def test_length_planner_matches_the_inline_expressions():
  from speecht_amd.audio_io import plan_resample, resample_lengths
  ns = list(range(1, 5001)) + list(range(320, 10 ** 7 + 1, 320)) + list(range(441, 10 ** 7 + 1, 441))
  for sr_orig, sr_new in RATE_PAIRS:
    ratio = float(sr_new) / float(sr_orig)
    for n in ns:
      want = (n, n) if sr_orig == sr_new else (int(n * ratio), int(math.ceil(n * float(sr_new) / sr_orig)))
      assert resample_lengths(n, sr_orig, sr_new) == want, (n, sr_orig, sr_new)
  lens = [5, 1000, 441, 3]
  rates = [16000, 44100, 22050, 8000]
  offsets, valid = plan_resample(lens, rates, 22050)
  plans = [resample_lengths(n, r, 22050) for n, r in zip(lens, rates)]
  assert offsets.tolist() == [0] + np.cumsum([t for _, t in plans]).tolist()
  assert valid.tolist() == [min(a, t) for a, t in plans]


def _host_resample(signals, rates, sr_new):
  from speecht_amd import _lib
  from speecht_amd.audio_io import _kaiser_best_filter, plan_resample
  lens = np.array([len(s) for s in signals], dtype=np.int64)
  in_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
  out_off, valid = plan_resample(lens, rates, sr_new)
  audio = np.ascontiguousarray(np.concatenate([np.asarray(s, np.float32) for s in signals]))
  r32 = np.asarray(rates, dtype=np.int32)
  win = np.ascontiguousarray(_kaiser_best_filter()[0], dtype=np.float64)
  out = np.zeros(max(int(out_off[-1]), 1), dtype=np.float64)
  P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
  _lib.call('st_resample_kaiser_host', P(audio), P(in_off), len(signals), P(r32), int(sr_new), P(out_off), P(valid), P(win),
            win.shape[0], P(out))
  return [out[out_off[i]:out_off[i + 1]] for i in range(len(signals))]


def _reference(y, sr_orig, sr_new):
  """audio_io.librosa_load's resampling of a float32 signal, before its cast to float32."""
  from speecht_amd.audio_io import resample_kaiser_best
  y = np.asarray(y, np.float32).astype(np.float64)
  if sr_orig == sr_new:
    return y
  target = int(math.ceil(y.shape[0] * float(sr_new) / sr_orig))
  z = resample_kaiser_best(y, sr_orig, sr_new)
  return np.concatenate([z, np.zeros(max(0, target - z.shape[0]))])[:target]


def _signals():
  rng = np.random.default_rng(7)
  sig = [rng.uniform(-1, 1, n).astype(np.float32) for n in (1, 2, 63, 64, 65, 321)]
  t = np.arange(3 * 16000) / 16000.0
  sig.append((0.6 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * 3100.0 * t)).astype(np.float32))
  return sig


def test_host_form_matches_the_host_resampler():
  from speecht_amd.audio_io import librosa_load
  golden, golden_rate = librosa_load(GOLDEN_FLAC, sr=None)
  worst = 0.0
  for sr_orig, sr_new in RATE_PAIRS + [(44100, 16000)]:
    signals = _signals()
    rates = [sr_orig] * len(signals)
    if (sr_orig, sr_new) == (16000, 22050):
      signals.append(golden)
      rates.append(golden_rate)
    got = _host_resample(signals, rates, sr_new)
    for y, r, g in zip(signals, rates, got):
      ref = _reference(y, r, sr_new)
      assert g.shape == ref.shape, (len(y), r, sr_new)
      if sr_orig == sr_new:
        assert np.array_equal(g, ref)                               # equal rates: copied exactly
      elif g.size:
        worst = max(worst, float(np.max(np.abs(g - ref))))
        assert np.max(np.abs(g - ref)) <= 1e-12, (len(y), r, sr_new)
  print('max |host form - resample_kaiser_best| = {:.3e}'.format(worst))


def test_host_form_mixed_rates_in_one_call():
  signals = _signals()
  rates = [8000, 16000, 22050, 44100, 48000, 16000, 44100]
  got = _host_resample(signals, rates, 22050)
  for y, r, g in zip(signals, rates, got):
    ref = _reference(y, r, 22050)
    assert g.shape == ref.shape
    assert np.max(np.abs(g - ref), initial=0.0) <= 1e-12


def test_host_form_selects_the_host_taps():
  """The taps of resample_map.h are those of resample_kaiser_best: a unit impulse at every source position reads back the
  weight the host applies to it, bit for bit -- a shifted tap, a dropped tap or another table entry would show."""
  n = 65
  for sr_orig, sr_new in [(16000, 22050), (22050, 16000), (44100, 22050)]:
    signals = [np.eye(n, dtype=np.float32)[k] for k in (0, 1, 31, 63, 64)]
    got = _host_resample(signals, [sr_orig] * len(signals), sr_new)
    for y, g in zip(signals, got):
      ref = _reference(y, sr_orig, sr_new)
      assert g.shape == ref.shape
      assert np.array_equal(g != 0, ref != 0)                        # same support: same taps selected
      assert np.array_equal(g, ref)                                  # one tap per output: its weight, exactly


def test_expand_paths_orders_directories(tmp_path):
  from speecht_amd.transcription import expand_paths
  d = tmp_path / 'corpus'
  (d / 'b').mkdir(parents=True)
  (d / 'a').mkdir()
  for rel in ('b/2.flac', 'a/9.wav', 'a/1.flac', 'z.WAV', 'notes.txt', 'a/x.npy'):
    (d / rel).write_bytes(b'')
  single = tmp_path / 'one.npy'
  single.write_bytes(b'')
  got = expand_paths([str(single), str(d)])
  want = [str(single)] + sorted(str(d / rel) for rel in ('a/1.flac', 'a/9.wav', 'b/2.flac', 'z.WAV'))
  assert got == want


def test_unsupported_or_missing_file_is_reported_with_its_path(tmp_path):
  from speecht_amd.transcription import TranscriptionError, check_length, load_native
  bad = tmp_path / 'clip.mp3'
  bad.write_bytes(b'ID3')
  with pytest.raises(TranscriptionError, match=r'clip\.mp3: unsupported audio file type \.mp3'):
    load_native(str(bad))
  with pytest.raises(TranscriptionError, match='no such file'):
    load_native(str(tmp_path / 'missing.flac'))
  corrupt = tmp_path / 'corrupt.flac'
  corrupt.write_bytes(b'not a flac stream at all')
  with pytest.raises(TranscriptionError, match=r'corrupt\.flac: cannot decode'):
    load_native(str(corrupt))
  w = tmp_path / 'tone.wav'
  with wave.open(str(w), 'wb') as f:
    f.setnchannels(1); f.setsampwidth(2); f.setframerate(8000)
    f.writeframes(np.zeros(800, '<i2').tobytes())
  y, rate = load_native(str(w))
  assert (y.shape, rate) == ((800,), 8000)
  check_length(187, 8000, 22050)                                    # ceil(187 * 22050 / 8000) = 516 > 256
  with pytest.raises(TranscriptionError, match='too short'):
    check_length(92, 8000, 22050)                                   # 254 samples after resampling
  with pytest.raises(TranscriptionError, match='too short'):
    check_length(256, 22050, 'native')
