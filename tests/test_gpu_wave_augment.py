"""Waveform augmentation on the GPU (st_wave_augment_f32, behind ``augmentation.apply_wave_device`` and
``engine.load_wave_batch``) against its host form (st_wave_augment_host: the two share csrc/wave_augment_core.h, so every
comparison is bit for bit).  The host form itself is held against the float64 specification in tests/test_wave_augment_cpu.py."""
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

LENGTHS = [1, 255, 256, 257, 300, 513, 1000, 3001, 3001, 4097, 70000, 70001]     # 70 000: more than 256 tiles of the power sums
THREE = ((9, 10), (1, 1), (11, 10))
RATE = 16000


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def A():
  from speecht_amd import augmentation
  return augmentation


def same_bits(a, b):
  a, b = np.asarray(a), np.asarray(b)
  return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


_CACHE = {}


def waves():
  if 'waves' not in _CACHE:
    rng = np.random.default_rng(21)
    _CACHE['waves'] = [rng.standard_normal(n).astype(np.float32) * 0.3 for n in LENGTHS]
  return _CACHE['waves']


def bank():
  """Clips of 1, 700 and 50 000 samples: the wrap extreme, one shorter than most utterances, one longer than most."""
  if 'bank' not in _CACHE:
    rng = np.random.default_rng(22)
    _CACHE['bank'] = A().NoiseBank.from_arrays([rng.standard_normal(1), rng.standard_normal(700), rng.standard_normal(50000)], RATE)
  return _CACHE['bank']


def on_device(dev, aug, batch, plan, align=4):
  """The kernels' outputs as host arrays.  align = 4: every output starts on a 16-byte boundary; 1: packed, as training lays them
  out for the feature kernels (odd starts: the scalar branches of the copy and the mix)."""
  x = np.concatenate(batch)
  offsets = np.concatenate([[0], np.cumsum([len(w) for w in batch])]).astype(np.int64)
  out, out_off = A().apply_wave_device(aug, torch.as_tensor(x).to(dev), offsets, plan, align=align)
  torch.cuda.synchronize()
  host = out.cpu().numpy()
  return [host[out_off[u]:out_off[u] + plan['M'][u]] for u in range(len(plan))]


@pytest.mark.parametrize('speeds', [((11, 10),), ((9, 10),), ((32, 31),), ((2, 1),), ((1, 2),), THREE], ids=lambda s: '_'.join('%d-%d' % p for p in s))
@pytest.mark.parametrize('noise_prob', [0.0, 1.0, 0.5])
@pytest.mark.parametrize('min_samples,align', [(0, 4), (0, 1), (256, 4)], ids=['all_resampled', 'packed', 'short_ones_replaced'])
def test_kernels_equal_the_host_form_bit_for_bit(dev, speeds, noise_prob, min_samples, align):
  """min_samples = 0: every utterance is resampled at a forced speed, the 1-sample one included (its windows lie almost wholly
  outside the utterance); 256: the rule of feasibility sends the short ones through the copy."""
  aug = A().WaveAugment(A().WavePolicy(speeds, noise_prob, (5.0, 25.0)), seed=17, noise=bank()).at(np.arange(12) + 1000)
  want, plan = A().apply_wave_host(aug, waves(), min_samples=min_samples)
  assert noise_prob in (0.0, 1.0) or 0 < plan['noisy'].sum() < 12
  if min_samples == 0:
    assert (plan['speed'] >= 0).all()
  elif len(speeds) == 1:
    (num, den), = speeds
    assert plan['speed'].tolist() == [-1 if -(-n * den // num) <= 256 else 0 for n in LENGTHS] and plan['speed'][0] == -1
  got = on_device(dev, aug, waves(), plan, align)
  for u, (g, w) in enumerate(zip(got, want)):
    assert same_bits(g, w), (u, plan[u], int((g.view(np.int32) != w.view(np.int32)).sum()))


def test_an_utterance_does_not_depend_on_its_row_or_its_batch(dev):
  aug = A().WaveAugment(A().WavePolicy(THREE, 1.0, (5.0, 25.0)), seed=3, noise=bank())
  x = waves()[9]
  rng = np.random.default_rng(23)
  others = [rng.standard_normal(n).astype(np.float32) for n in LENGTHS]
  results = []
  for batch, row in (([x], 0), ([x] + waves()[1:], 0), (waves()[:11] + [x], 11), ([x] + others[1:], 0)):
    ids = np.arange(len(batch)) + 500
    ids[row] = 77
    plan = A().plan_wave_host(aug.at(ids), [len(w) for w in batch], min_samples=256)
    results.append((on_device(dev, aug, batch, plan)[row], plan[row]))
  assert results[0][1]['noisy'] and results[0][1]['speed'] in (0, 2), results[0][1]       # (id 77 draws a speed change and noise)
  for out, plan in results[1:]:
    assert plan == results[0][1] and same_bits(out, results[0][0])


# ---- through the engine and the training step ------------------------------------------------------------------------------------

SAMPLES = [16000, 6400, 11111, 9000]                 # 0.4 .. 1.0 s at 16 kHz


def speech(seed=31):
  rng = np.random.default_rng(seed)
  return [(rng.standard_normal(n) * 0.1 * np.sin(np.arange(n) / 300.0)).astype(np.float32) for n in SAMPLES]


def engine_of(dev, channels):
  from speecht_amd.engine import Wav2LetterEngine
  from tests import workloads as WL
  key = ('engine', channels)
  if key not in _CACHE:
    _CACHE[key] = Wav2LetterEngine(WL.w2l_layers(channels, width=24, fc=40), device=dev)
  return _CACHE[key]


def input_tensor(eng):
  X0 = eng.shape.X[0]
  torch.cuda.synchronize()
  return X0.buf.cpu().numpy().reshape(X0.batch, X0.t_pitch, X0.c_pitch).copy()


@pytest.mark.parametrize('feature_type,channels', [('power', 16), ('mfcc', 39)])
def test_waveform_batch_without_augmentation_fills_the_input_tensor_like_the_feature_batch(dev, feature_type, channels):
  from speecht_amd import preprocessing as P
  audio = speech()
  if feature_type == 'power':
    feats = P.calc_power_spectrogram_batch(audio, RATE, n_mels=channels, device=dev)
  else:
    feats = P.calc_mfccs_batch(audio, RATE, n_mfcc=channels // 3, device=dev)
  frames = np.array([len(f) for f in feats])
  assert frames.tolist() == [1 + n // 160 for n in SAMPLES]
  padded = np.zeros((4, frames.max(), channels), dtype=np.float32)
  for row, f in zip(padded, feats):
    row[:len(f)] = f
  eng = engine_of(dev, channels)
  eng.load_batch(padded, frames)
  want = input_tensor(eng)
  eng.shape.X[0].buf.zero_()
  lens = np.array(SAMPLES)
  eng.load_wave_batch(np.concatenate(audio), lens, lens, feature_type, RATE)
  assert eng.wave_plan is None and np.array_equal(eng.wave_frames, frames) and np.array_equal(eng.seq_lens_host, frames)
  assert same_bits(input_tensor(eng), want)


def test_each_rank_pads_to_the_global_batch(dev):
  """Two ranks with two rows each get the max_T one process with all four rows gets, and the rows it gets."""
  aug = A().WaveAugment(A().WavePolicy(THREE, 0.5, (5.0, 25.0)), seed=8, noise=bank())
  audio, lens = speech(), np.array(SAMPLES)
  eng = engine_of(dev, 16)
  wave = aug.for_step(3, 2, world=2, rank=0)
  assert wave.draw_ids.tolist() == [12, 13, 14, 15] and aug.for_step(3, 4).draw_ids.tolist() == [12, 13, 14, 15]
  eng.load_wave_batch(np.concatenate(audio), lens, lens, 'power', RATE, wave=wave)
  whole, T = input_tensor(eng), eng.shape.X[0].frames
  plan = A().plan_wave_host(wave, lens, min_samples=256)
  assert np.array_equal(eng.wave_plan, plan) and T == (1 + plan['M'] // 160).max() and len(set(plan['speed'])) > 1
  assert np.array_equal(eng.seq_lens_host, 1 + plan['M'] // 160)
  for rank in (0, 1):
    rows = slice(2 * rank, 2 * rank + 2)
    eng.load_wave_batch(np.concatenate(audio[rows]), lens[rows], lens, 'power', RATE, wave=aug.for_step(3, 2, world=2, rank=rank), rank=rank)
    assert eng.shape.X[0].frames == T and np.array_equal(eng.wave_plan, plan[rows])
    assert same_bits(input_tensor(eng), whole[rows])


def wave_model(tmp_path, name, wave_augment, spec_augment):
  from speecht_amd.speech_input import Coordinator, InputBatchLoader
  from speecht_amd.speech_model import Wav2LetterModel
  from tests import workloads as WL
  audio = speech()
  labels = [WL.make_labels(i, 4 + i, 10) for i in range(4)]

  def gen():
    while True:
      for i in range(4):
        yield audio[i], labels[i]
  loader = InputBatchLoader(16, 4, gen, wave=dict(feature_type='power', rate=RATE))
  coord = Coordinator()
  loader.start_threads(None, coord)
  model = Wav2LetterModel(loader, 16, 29)
  model.add_training_ops(learning_rate=1e-3, spec_augment=spec_augment, wave_augment=wave_augment)
  model.add_decoding_ops()
  model.finalize(str(tmp_path / 'log'), name, 'train')
  model.init_seed = 11
  return model, coord


def test_training_steps_augment_and_a_restored_model_draws_the_same(dev, tmp_path):
  from speecht_amd.speech_model import Session
  wave = A().WaveAugment(A().WavePolicy(THREE, 0.5, (5.0, 25.0)), seed=13, noise=bank())
  spec = A().SpecAugment((4, 5, 2, 6, 2, 1.0), seed=13)
  model, coord = wave_model(tmp_path, 'a', wave, spec)
  other, coord2 = wave_model(tmp_path, 'b', wave, spec)
  lens = np.array(SAMPLES)
  try:
    with Session(dev) as sess:
      model.init_session(sess)
      # an evaluation-style step sees the clean features
      assert np.isfinite(model.step(sess, update=False)[0])
      assert model.engine.wave_plan is None and model.engine.wave_frames.tolist() == [1 + n // 160 for n in SAMPLES]
      first = model.step(sess)[0]
      plan0 = A().plan_wave_host(wave.for_step(0, 4), lens, min_samples=256)
      assert np.isfinite(first) and np.array_equal(model.engine.wave_plan, plan0)
      assert np.array_equal(model.engine.seq_lens_host, 1 + plan0['M'] // 160)
      ck = str(tmp_path / 'run')
      os.makedirs(ck)
      model.saver.save(sess, ck + '/speechT.ckpt', global_step=model.global_step)
      second = model.step(sess)[0]
      plan1 = A().plan_wave_host(wave.for_step(1, 4), lens, min_samples=256)
      assert np.isfinite(second) and np.array_equal(model.engine.wave_plan, plan1) and not np.array_equal(plan0, plan1)
      weights = model.engine.get_weights()[0][0].copy()
      # the restored model makes step 2 with the same bits
      other.init_session(sess)
      other.restore(sess, ck)
      assert other.global_step.eval() == 1
      again = other.step(sess)[0]
      assert np.array_equal(other.engine.wave_plan, plan1)
      assert np.float32(again).tobytes() == np.float32(second).tobytes(), (again, second)
      assert same_bits(other.engine.get_weights()[0][0], weights)
  finally:
    coord.request_stop()
    coord2.request_stop()


def test_cli_preprocess_waveforms_then_train_and_resume(dev, tmp_path, capsys):
  """`preprocess --waveforms` then `train --waveforms` with both augmentations, through the executor, the feeder and stager threads
  and the staged form of the waveform batch; the noise directory holds a clip at another rate, which the device resampler
  brings to the cache's; a second run resumes from the checkpoint."""
  import importlib.machinery
  import importlib.util
  import wave
  loader = importlib.machinery.SourceFileLoader('speecht_cli_wave_train', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'speecht-cli'))
  cli = importlib.util.module_from_spec(importlib.util.spec_from_loader(loader.name, loader))
  loader.exec_module(cli)
  data, noise = tmp_path / 'data', tmp_path / 'noise'
  (data / 'train').mkdir(parents=True)
  noise.mkdir()
  rng = np.random.default_rng(41)
  lines = []
  for i, n in enumerate((16000, 21000, 18000, 24000)):
    np.save(str(data / 'train' / 'u-{}.npy'.format(i)), (rng.standard_normal(n) * 0.1).astype(np.float32))
    lines.append('u-{} HELLO WORLD {}'.format(i, 'AB' * i))
  (data / 'train' / 'u.trans.txt').write_text('\n'.join(lines) + '\n')
  np.save(str(noise / 'hiss.npy'), rng.standard_normal(5000).astype(np.float32))
  with wave.open(str(noise / 'hum.wav'), 'wb') as w:                   # 8 kHz: resampled to the cache's 16 kHz at start-up
    w.setnchannels(1)
    w.setsampwidth(2)
    w.setframerate(8000)
    w.writeframes((np.sin(np.arange(4000) / 5.0) * 8000).astype('<i2').tobytes())
  common = ['--data-dir', str(data), '--train-dir', str(tmp_path / 'train'), '--log-dir', str(tmp_path / 'log'), '--run-name', 'w']
  assert cli.main(['preprocess', '--waveforms', '--train-only'] + common) == 0
  train = ['train', '--waveforms', '--speed-perturb', '0.9,1.0,1.1', '--noise-dir', str(noise), '--noise-prob', '0.5', '--batch-size', '2',
           '--steps-per-checkpoint', '2', '--seed', '3'] + common
  capsys.readouterr()
  assert cli.main(train + ['--max-steps', '2']) == 0
  out = capsys.readouterr().out
  assert 'Training from waveforms at 16000 Hz' in out and 'Waveform augmentation: speeds 9/10 1/1 11/10' in out and 'guess' in out
  assert 'global step 2 ' in out and 'Model saved' in out and np.isfinite(float(out.split('average loss ')[1].split()[0]))
  assert os.path.exists(str(tmp_path / 'train' / 'w' / 'speechT.ckpt-2.npz'))
  assert cli.main(train + ['--max-steps', '2']) == 0
  out = capsys.readouterr().out
  assert 'global step 4 ' in out and os.path.exists(str(tmp_path / 'train' / 'w' / 'speechT.ckpt-4.npz'))
  # an augmentation flag without --waveforms is refused, and names the flag that is missing
  with pytest.raises(ValueError, match='--waveforms'):
    cli.main(['train', '--speed-perturb', '0.9,1.1', '--max-steps', '1'] + common)
