"""Audio files to text on the GPU: the kaiser_best resampling kernel against its host float64 form, the device feature path
against the host one on the golden FLAC, transcribe_audio against inference.transcribe and SpeechModel.step, `speecht-cli
transcribe` end to end, and `preprocess --device-resample` against the default preprocess."""
import argparse
import ctypes
import json
import os
import shutil
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
GOLDEN_FLAC = os.path.join(GOLDEN, '1089-134686-0037.flac')
TINY_LM = os.path.join(GOLDEN, 'lm_tiny.arpa')
RATE_PAIRS = [(8000, 22050), (16000, 22050), (22050, 22050), (44100, 22050), (48000, 22050), (22050, 16000)]


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def _host_form(signals, rates, sr_new):
  """st_resample_kaiser_host: the float64 host form of the kernel (pinned to audio_io.resample_kaiser_best by the CPU tests)."""
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


def _ragged(rng):
  from speecht_amd.audio_io import librosa_load
  sig = [rng.uniform(-1, 1, n).astype(np.float32) for n in (1, 2, 63, 64, 65, 321)]
  sig.append(librosa_load(GOLDEN_FLAC, sr=None)[0])
  t = np.arange(3 * 16000) / 16000.0
  sig.append((0.7 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32))
  sig.append(rng.uniform(-1, 1, 15 * 48000).astype(np.float32))
  sig.append(np.clip(rng.normal(0, 0.3, 60 * 48000), -1, 1).astype(np.float32))
  return sig


def test_device_resampler_matches_the_host_form(dev):
  from speecht_amd.audio_io import resample_kaiser_best_batch
  rng = np.random.default_rng(11)
  signals = _ragged(rng)
  worst = 0.0
  batches = [([sr_orig] * len(signals), sr_new) for sr_orig, sr_new in RATE_PAIRS]
  batches.append(([8000, 16000, 22050, 44100, 48000, 16000, 16000, 8000, 44100, 48000], 22050))   # mixed rates, one launch
  for rates, sr_new in batches:
    got = resample_kaiser_best_batch(signals, rates, sr_new, dev)
    want = _host_form(signals, rates, sr_new)
    for y, r, g, w in zip(signals, rates, got, want):
      assert g.dtype == np.float32 and g.shape == w.shape, (len(y), r, sr_new)
      if r == sr_new:
        assert np.array_equal(g, y)                                  # equal rates: the samples, bit for bit
      elif g.size:
        err = float(np.max(np.abs(g.astype(np.float64) - w)))
        worst = max(worst, err)
        assert err <= 1e-6, (len(y), r, sr_new, err)
  print('max |device - host float64| = {:.3e}'.format(worst))


def test_golden_flac_device_features_match_the_host_path(dev):
  from speecht_amd import preprocessing
  from speecht_amd.transcription import device_features, load_native
  y, rate = load_native(GOLDEN_FLAC)
  host_audio, host_rate = preprocessing.load_audio(GOLDEN_FLAC)
  for kind, fn in (('power', preprocessing.calc_power_spectrogram), ('mfcc', preprocessing.calc_mfccs)):
    got, = device_features([y], [rate], kind, 22050, dev)
    want = fn(host_audio, host_rate)
    assert got.shape == want.shape
    err = float(np.max(np.abs(got - want)))
    print('{}: max |device path - host path| = {:.3e}'.format(kind, err))
    assert err < 1e-3


def _wav(path, samples, rate):
  with wave.open(str(path), 'wb') as w:
    w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
    w.writeframes((np.clip(samples, -1, 1) * 32767).astype('<i2').tobytes())


def _tone(rate, seconds, f0):
  t = np.arange(int(rate * seconds)) / float(rate)
  return 0.5 * np.sin(2 * np.pi * f0 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3.0 * t))


def _model(tmp_path, input_size=128, seed=1234):
  from speecht_amd.speech_input import SingleInputLoader
  from speecht_amd.speech_model import Wav2LetterModel
  loader = SingleInputLoader(input_size)
  model = Wav2LetterModel(loader, input_size, 29)
  model.add_training_ops()
  model.add_decoding_ops()
  model.finalize(str(tmp_path / 'log'), 'r', 'record')
  model.init_seed = seed
  return model, loader


def test_transcribe_audio_plumbing(dev, tmp_path):
  from speecht_amd import inference
  from speecht_amd.speech_model import Session
  from speecht_amd.transcription import device_features, load_native, transcribe_audio
  y, rate = load_native(GOLDEN_FLAC)
  signals = [y, _tone(8000, 2.0, 300.0).astype(np.float32), _tone(44100, 1.5, 900.0).astype(np.float32)]
  rates = [rate, 8000, 44100]
  model, loader = _model(tmp_path)
  with Session(dev) as sess:
    model.init_session(sess)
    eng = model.engine
    feats = device_features(signals, rates, 'power', 22050, dev)
    for decode in ({}, dict(beam_width=16), dict(language_model=TINY_LM, lm_options=dict(lm_weight=0.8))):
      ids, texts = transcribe_audio(eng, signals, rates, **decode)
      want_ids, want_texts = inference.transcribe(eng, feats, batch_size=1, **decode)
      assert ids == want_ids and texts == want_texts, decode
    ids, _ = transcribe_audio(eng, signals, rates)
    for f, i in zip(feats, ids):
      loader.set_input(f)
      decoded, = model.step(sess, loss=False, update=False, decode=True)
      assert decoded[0].values.tolist() == list(i)
    ids4, _ = transcribe_audio(eng, signals, rates, batch_size=4)     # opt-in: one padded batch -- runs, same count
    assert len(ids4) == len(signals)


def _cli(args, cwd):
  return subprocess.run([sys.executable, os.path.join(ROOT, 'speecht-cli'), 'transcribe'] + args, cwd=str(cwd),
                        capture_output=True, text=True, timeout=600)


def test_cli_transcribe_end_to_end(dev, tmp_path):
  from speecht_amd.speech_model import Session
  from speecht_amd.transcription import transcribe_files
  train = tmp_path / 'train'
  model, _ = _model(tmp_path)
  audio = tmp_path / 'audio'
  (audio / 'sub').mkdir(parents=True)
  shutil.copy(GOLDEN_FLAC, str(audio / 'a.flac'))
  _wav(audio / 'sub' / 'b8k.wav', _tone(8000, 2.0, 300.0), 8000)
  _wav(audio / 'c44k.wav', _tone(44100, 1.5, 900.0), 44100)
  files = [str(audio / 'a.flac'), str(audio / 'c44k.wav'), str(audio / 'sub' / 'b8k.wav')]   # the directory's sorted order
  (train / 'run').mkdir(parents=True)
  with Session(dev) as sess:
    model.init_session(sess)
    model.saver.save(sess, str(train / 'run' / 'speechT'), global_step=model.global_step)
    want = {r['path']: r['text'] for r in transcribe_files(model.engine, files)}
  cwd = tmp_path / 'cwd'
  cwd.mkdir()
  out = tmp_path / 'out.jsonl'
  base = ['--train-dir', str(train), '--run-name', 'run', '--device', dev]
  r = _cli(base + ['--output', str(out), GOLDEN_FLAC, str(audio / 'sub' / 'b8k.wav'), str(audio)], cwd)
  assert r.returncode == 0, r.stderr
  lines = r.stdout.splitlines()
  paths = [GOLDEN_FLAC, str(audio / 'sub' / 'b8k.wav')] + files
  assert [l.split('\t')[0] for l in lines] == paths
  for line, p in zip(lines, paths):
    assert line.split('\t', 1)[1] == want[os.path.join(str(audio), 'a.flac') if p == GOLDEN_FLAC else p]
  records = [json.loads(l) for l in out.read_text().splitlines()]
  assert [x['path'] for x in records] == paths
  assert [x['text'] for x in records] == [l.split('\t', 1)[1] for l in lines]
  assert abs(records[1]['seconds'] - 2.0) < 1e-9
  assert sorted(os.listdir(str(cwd))) == []                           # no train / data / log directory made
  # a corrupt file: reported with its path, exit status 1, the other files still transcribed
  bad = audio / 'bad.flac'
  bad.write_bytes(b'fLaC-but-not-really')
  r = _cli(base + [str(bad), str(audio / 'c44k.wav')], cwd)
  assert r.returncode == 1
  assert str(bad) in r.stderr
  assert r.stdout.splitlines() == ['{}\t{}'.format(audio / 'c44k.wav', want[str(audio / 'c44k.wav')])]
  # no checkpoint: fails as evaluate does
  r = _cli(['--train-dir', str(train), '--run-name', 'missing', '--device', dev, GOLDEN_FLAC], cwd)
  assert r.returncode != 0
  assert 'No checkpoint for evaluation found' in r.stderr
  assert not (train / 'missing').exists()


def test_preprocess_device_resample_matches_default(dev, tmp_path):
  from speecht_amd.preprocessing import Preprocessing
  results = {}
  for mode in (False, True):
    data = tmp_path / ('data_dev' if mode else 'data_host')
    (data / 'train').mkdir(parents=True)
    text = 'THE GOLDEN UTTERANCE'
    for uid in ('1089-134686-0037', '1089-134686-0099'):
      shutil.copy(GOLDEN_FLAC, str(data / 'train' / (uid + '.flac')))
    (data / 'train' / '1089-134686.trans.txt').write_text('1089-134686-0037 {}\n1089-134686-0099 {}\n'.format(text, text))
    for kind in ('power', 'mfcc'):
      flags = argparse.Namespace(data_dir=str(data), feature_type=kind, train_only=True, test_only=False, dev_only=False,
                                 device_resample=mode, device=dev)
      Preprocessing(flags).run()
      sub = 'preprocessed-power' if kind == 'power' else 'preprocessed'
      for uid in ('1089-134686-0037', '1089-134686-0099'):
        with np.load(str(data / sub / 'train' / (uid + '.npz'))) as z:
          results[(mode, kind, uid)] = (z['audio_fragments'], z['transcript'])
  for kind in ('power', 'mfcc'):
    for uid in ('1089-134686-0037', '1089-134686-0099'):
      host, device = results[(False, kind, uid)], results[(True, kind, uid)]
      assert device[0].shape == host[0].shape
      assert float(np.max(np.abs(device[0] - host[0]))) < 1e-3
      assert np.array_equal(device[1], host[1])
