"""Waveform augmentation without a GPU: the float64 specification tests/wave_augment_oracle.py against itself (tones come out as
tones), and the host form of the library (st_wave_augment_host / st_wave_augment_plan_host through ctypes: the arithmetic the
kernels share, csrc/wave_augment_core.h) against it -- the derived float32 bound, identity, lengths, the achieved SNR, the wrap,
silence, the fixed order of the power sums, the draws, and the surface (exports, argument checks)."""
import os
import re

import numpy as np
import pytest

from tests import spec_augment_oracle as SO
from tests import wave_augment_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEEDS = [(11, 10), (9, 10), (32, 31), (7, 8), (2, 1), (1, 2)]
RATE = 16000


def A():
  from speecht_amd import augmentation
  return augmentation


def same_bits(a, b):
  a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
  return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def one_speed(num, den):
  return A().WaveAugment(A().WavePolicy(speeds=((num, den),)), seed=5)


def bank3(seed=11):
  rng = np.random.default_rng(seed)
  return A().NoiseBank.from_arrays([rng.standard_normal(1), rng.standard_normal(700), rng.standard_normal(50000)], RATE)


# ---- the specification against itself --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('num,den', SPEEDS)
def test_oracle_turns_tones_into_tones(num, den):
  """A tone below 0.9 x the cutoff comes out as the tone at f num/den within 1e-3 away from the ends (measured: at most 3.2e-5 at
  these tones, 1.9e-4 up to 5 000 Hz; a wrong phase or an off-by-one tap gives errors of order 0.1)."""
  H = O.half_width(num, den)
  for f in (100.0, 1000.0, 3000.0):
    if (num, den) == (2, 1) and f == 3000.0:
      continue                                         # above 0.9 x the cutoff 0.85 x 4 000 Hz
    x = np.sin(2 * np.pi * f * np.arange(4000) / RATE)
    y, _ = O.resample(x, num, den)
    assert len(y) == O.out_len(4000, num, den)
    want = np.sin(2 * np.pi * f * (np.arange(len(y)) * num / den) / RATE)
    err = np.abs(y - want)[2 * H:len(y) - 2 * H].max()
    print('speed {}/{} tone {} Hz: {:.3g}'.format(num, den, f, err))
    assert err <= 1e-3


@pytest.mark.parametrize('num,den', SPEEDS + [(1, 1)])
def test_table_rows_sum_to_one_and_match_the_oracle(num, den):
  h = O.table(num, den)
  assert h.shape == (den, 2 * O.half_width(num, den))
  assert np.abs(h.sum(axis=1) - 1.0).max() <= 1e-15
  assert same_bits(A().speed_table(num, den), h.astype(np.float32))


def test_table_against_a_scalar_evaluation_of_the_formula():
  """The oracle's table and ``speed_table`` are the same lines of numpy, so their bit equality says nothing about either.  Here
  every tap is evaluated on its own with math.sin and the power series of I0, sum_k ((x/2)^k / k!)^2: agreement to 1e-13."""
  import math

  def i0(x):
    term, total, k = 1.0, 1.0, 0
    while term > 1e-20 * total:
      k += 1
      term *= (x / 2.0) ** 2 / (k * k)
      total += term
    return total

  for num, den in SPEEDS:
    H = 16 if num <= den else -(-16 * num // den)
    fc = 0.85 * min(1.0, den / num)
    h = O.table(num, den)
    for phi in range(den):
      row = []
      for j in range(-H + 1, H + 1):
        tau = j - phi / den
        r = tau / H
        sinc = 1.0 if tau == 0 else math.sin(math.pi * fc * tau) / (math.pi * fc * tau)
        row.append(fc * sinc * i0(8.555504641634386 * math.sqrt(1.0 - r * r)) / i0(8.555504641634386) if abs(r) < 1 else 0.0)
      total = math.fsum(row)
      assert max(abs(v / total - g) for v, g in zip(row, h[phi])) <= 1e-13, (num, den, phi)


# ---- the host form against the specification --------------------------------------------------------------------------------------

def lengths_for(num, den):
  return [1, 2, 2 * O.half_width(num, den) - 1, 255, 256, 257, 513, 3001]


@pytest.mark.parametrize('num,den', SPEEDS)
def test_host_form_meets_the_derived_bound(num, den):
  """|y - y64| <= (2H + 1) 2^-24 sum_k |h_phi[k] x_k|: 2H fmaf roundings of partial sums that never exceed the sum of magnitudes, and
  one for slack; h is the float32 table on both sides.  Measured worst case: 0.18 of the bound (at 7/8)."""
  rng = np.random.default_rng(num * 100 + den)
  waves = [rng.standard_normal(n).astype(np.float32) for n in lengths_for(num, den)]
  aug = one_speed(num, den).at(np.arange(len(waves)))
  out, plan = A().apply_wave_host(aug, waves)
  h32, H = A().speed_table(num, den), O.half_width(num, den)
  worst = 0.0
  for x, y, p in zip(waves, out, plan):
    assert p['speed'] == 0 and p['M'] == len(y) == O.out_len(len(x), num, den)
    y64, mag = O.resample(x, num, den, h=h32)
    bound = (2 * H + 1) * 2.0 ** -24 * mag
    err = np.abs(y.astype(np.float64) - y64)
    assert (err <= bound).all()
    worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
  print('speed {}/{}: worst error {:.3g} of the bound'.format(num, den, worst))


def test_speed_one_returns_the_inputs_bits():
  rng = np.random.default_rng(1)
  waves = [rng.standard_normal(n).astype(np.float32) for n in (1, 2, 255, 256, 257, 3001)]
  waves[1][0] = -0.0
  out, plan = A().apply_wave_host(one_speed(1, 1).at(np.arange(6)), waves)
  for x, y in zip(waves, out):
    assert same_bits(x, y)


# ---- noise ----------------------------------------------------------------------------------------------------------------------

def noisy_and_clean(num, den, waves, bank, plan_edit=None):
  """(clean outputs, noisy outputs, plans, sums): the same speed with noise_prob 0 and 1."""
  ids = np.arange(len(waves)) + 40
  clean, _ = A().apply_wave_host(one_speed(num, den).at(ids), waves)
  aug = A().WaveAugment(A().WavePolicy(speeds=((num, den),), noise_prob=1.0, snr_db=(5.0, 25.0)), seed=5, noise=bank).at(ids)
  plan = A().plan_wave_host(aug, [len(w) for w in waves])
  if plan_edit:
    plan_edit(plan)
  noisy, plan, sums = A().apply_wave_host(aug, waves, plan=plan, return_sums=True)
  return clean, noisy, plan, sums


def test_noise_reaches_the_drawn_snr_and_is_one_fmaf():
  bank = bank3()
  rng = np.random.default_rng(2)
  waves = [rng.standard_normal(n).astype(np.float32) * 0.1 for n in (1, 300, 1000, 3001, 60000)]
  for num, den in ((9, 10), (1, 1)):
    clean, noisy, plan, sums = noisy_and_clean(num, den, waves, bank)
    assert plan['noisy'].all()
    for s, y, p, (ss, sz) in zip(clean, noisy, plan, sums):
      z = O.noise_of(bank.samples, bank.offsets, p['clip'], p['offset'], p['M'])
      a = O.gain(ss, sz, int(p['M']), float(p['lin']))
      ps, pn = (s.astype(np.float64) ** 2).mean(), (z.astype(np.float64) ** 2).mean()
      achieved = 10 * np.log10(ps / (a * a * pn))
      assert abs(achieved - p['snr_centi'] / 100.0) <= 1e-9
      assert 500 <= p['snr_centi'] <= 2500
      assert same_bits(y, O.fmaf32(np.float32(a), z, s))


def test_short_clip_and_offset_at_its_last_sample_wrap():
  bank = bank3()
  waves = [np.random.default_rng(3).standard_normal(900).astype(np.float32)]

  def last(plan):
    plan['clip'], plan['offset'] = 1, 699

  clean, noisy, plan, sums = noisy_and_clean(9, 10, waves, bank, last)     # 1 000 outputs meet the 700-sample clip
  z = O.noise_of(bank.samples, bank.offsets, 1, 699, 1000)
  assert z[0] == bank.samples[1 + 699] and z[1] == bank.samples[1] and z[701] == bank.samples[1]
  a = O.gain(sums[0, 0], sums[0, 1], 1000, float(plan['lin'][0]))
  assert a > 0 and same_bits(noisy[0], O.fmaf32(np.float32(a), z, clean[0]))


def test_silence_on_either_side_mixes_nothing():
  silent_bank = A().NoiseBank.from_arrays([np.zeros(300)], RATE)
  x = np.random.default_rng(4).standard_normal(1000).astype(np.float32)
  clean, noisy, plan, sums = noisy_and_clean(11, 10, [x], silent_bank)
  assert plan['noisy'][0] and sums[0, 1] == 0.0 and same_bits(clean[0], noisy[0])
  clean, noisy, plan, sums = noisy_and_clean(11, 10, [np.zeros(1000, np.float32)], bank3())
  assert plan['noisy'][0] and sums[0, 0] == 0.0 and sums[0, 1] > 0 and same_bits(clean[0], noisy[0])


def test_power_sums_follow_the_fixed_order():
  """The host form's two sums equal the tile-tree evaluation bit for bit; 70 000 samples are more than 256 tiles."""
  bank = A().NoiseBank.from_arrays([np.random.default_rng(5).standard_normal(50000)], RATE)
  rng = np.random.default_rng(6)
  waves = [rng.standard_normal(n).astype(np.float32) for n in (1, 255, 256, 257, 70000)]
  clean, noisy, plan, sums = noisy_and_clean(1, 1, waves, bank)
  for s, p, (ss, sz) in zip(clean, plan, sums):
    z = O.noise_of(bank.samples, bank.offsets, 0, p['offset'], p['M'])
    assert ss == O.sum_squares(s) and sz == O.sum_squares(z)


# ---- draws ------------------------------------------------------------------------------------------------------------------------

def test_plans_depend_on_seed_id_and_length_alone_and_match_the_oracle():
  bank = bank3()
  pol = A().WavePolicy(noise_prob=0.5, snr_db=(10.0, 30.0))
  lens = np.array([1, 255, 256, 257, 300, 513, 1000, 3001, 3001, 4097, 70000, 70001])
  ids = np.arange(12) * 7 + 2 ** 33
  aug = A().WaveAugment(pol, seed=0x1234567890abcdef, noise=bank)
  plans = A().plan_wave_host(aug.at(ids), lens, min_samples=256)
  perm = np.random.default_rng(7).permutation(12)
  assert np.array_equal(A().plan_wave_host(aug.at(ids[perm]), lens[perm], min_samples=256), plans[perm])
  for u in range(12):
    assert np.array_equal(A().plan_wave_host(aug.at(ids[u:u + 1]), lens[u:u + 1], min_samples=256), plans[u:u + 1])
    want = O.plan(pol.speeds, pol.noise_prob_q16, pol.snr_centi, aug.seed, int(ids[u]), int(lens[u]), bank.lengths, 256)
    for name in ('speed', 'M', 'noisy', 'clip', 'offset', 'snr_centi'):
      assert plans[u][name] == want[name], (u, name)
    assert abs(plans[u]['lin'] - want['lin']) <= 2.3e-16 * want['lin']
  assert plans['noisy'].min() == 0 and plans['noisy'].max() == 1
  other = A().plan_wave_host(A().WaveAugment(pol, seed=1, noise=bank).at(ids), lens, min_samples=256)
  assert not np.array_equal(other, plans)


def test_noise_probability_zero_and_one_and_uniform_draws():
  bank = bank3()
  ids = np.arange(20000)
  lens = np.full(20000, 5000)
  never = A().plan_wave_host(A().WaveAugment(A().WavePolicy(noise_prob=0.0), 9, bank).at(ids), lens)
  always = A().plan_wave_host(A().WaveAugment(A().WavePolicy(noise_prob=1.0), 9, bank).at(ids), lens)
  assert not never['noisy'].any() and always['noisy'].all()
  assert np.array_equal(never['speed'], always['speed'])
  sigma = np.sqrt(20000 * (1 / 3) * (2 / 3))
  for field in ('speed', 'clip'):
    counts = np.bincount(always[field], minlength=3)
    assert len(counts) == 3 and np.abs(counts - 20000 / 3).max() <= 4 * sigma, counts
  for k in range(3):
    at = always['offset'][always['clip'] == k]
    assert at.min() >= 0 and at.max() < bank.lengths[k]
  half = A().plan_wave_host(A().WaveAugment(A().WavePolicy(noise_prob=0.5), 9, bank).at(ids), lens)
  assert abs(int(half['noisy'].sum()) - 10000) <= 4 * np.sqrt(20000 * 0.25)


def test_min_samples_rule_replaces_the_speed_exactly_when_it_should():
  aug = one_speed(11, 10).at(np.zeros(8, dtype=np.int64))
  lens = np.arange(278, 286)
  plans = A().plan_wave_host(aug, lens, min_samples=256)
  for n, p in zip(lens, plans):
    M = O.out_len(int(n), 11, 10)
    assert (p['speed'], p['M']) == ((-1, n) if M <= 256 else (0, M))
  assert {-1, 0} == set(plans['speed'])


def test_draws_differ_from_spec_augments():
  for seed, draw_id in ((0, 0), (5, 77), (2 ** 63 + 1, 2 ** 40)):
    assert O.block(seed, draw_id, 0) != SO.block(seed, draw_id, 0)
  # the library's speed draw is the word of the stream whose counter ends in 1, not of SpecAugment's
  ids = np.arange(64)
  plans = A().plan_wave_host(A().WaveAugment(A().WavePolicy(), 3).at(ids), np.full(64, 9000))
  assert [SO.uniform(O.block(3, i, 0)[0], 2) for i in ids] == list(plans['speed'])
  assert [SO.uniform(SO.block(3, i, 0)[0], 2) for i in ids] != list(plans['speed'])


# ---- surface ------------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_exported_and_declared():
  from speecht_amd import _lib
  lib = _lib.load()
  header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'speecht_hip.h')).read(), flags=re.S)
  for name in ('st_wave_augment_plan_host', 'st_wave_augment_ws', 'st_wave_augment_f32', 'st_wave_augment_host'):
    assert re.search(r'\b' + name + r'\s*\(', header) and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_bad_arguments_are_refused():
  from speecht_amd import _lib
  with pytest.raises(ValueError):
    A().WavePolicy(speeds=((33, 32),))
  with pytest.raises(ValueError):
    A().WavePolicy(speeds=(2.5,))
  with pytest.raises(ValueError):
    A().WaveAugment(A().WavePolicy(noise_prob=0.5))
  assert A().WavePolicy(speeds=(0.9, 1.0, 1.1)).speeds == ((9, 10), (1, 1), (11, 10))
  aug = one_speed(9, 10).at(np.arange(1))
  plan = A().plan_wave_host(aug, [100])
  plan['M'] = 5000                                     # more than 100 samples make at 9/10: refused before anything is written
  with pytest.raises(_lib.SpeechtHipError, match='plans 5000 outputs'):
    A().apply_wave_host(aug, [np.zeros(100, np.float32)], plan=plan)


# ---- flags, the waveform cache, the loader -------------------------------------------------------------------------------------------

def load_cli():
  import importlib.machinery
  import importlib.util
  loader = importlib.machinery.SourceFileLoader('speecht_cli_wave_augment', os.path.join(ROOT, 'speecht-cli'))
  cli = importlib.util.module_from_spec(importlib.util.spec_from_loader(loader.name, loader))
  loader.exec_module(cli)
  return cli


def test_cli_flags_build_the_policy_and_need_waveforms(tmp_path):
  cli = load_cli()
  noise_dir = tmp_path / 'noise'
  noise_dir.mkdir()
  np.save(str(noise_dir / 'hum.npy'), np.sin(np.arange(5000) / 7.0).astype(np.float32))
  np.save(str(noise_dir / 'hiss.npy'), np.random.default_rng(0).standard_normal(300).astype(np.float32))
  _, flags = cli.parse(['train', '--waveforms', '--speed-perturb', '0.9,1.0,1.1', '--noise-dir', str(noise_dir), '--noise-prob', '0.25',
                        '--noise-snr', '5,15', '--augment-seed', '9'])
  aug = A().wave_from_flags(flags, rate=16000)          # (.npy clips are at 16 kHz: nothing to resample, no GPU needed)
  assert aug.policy == (((9, 10), (1, 1), (11, 10)), 0.25, (5.0, 15.0)) and aug.seed == 9
  assert len(aug.noise) == 2 and sorted(aug.noise.lengths) == [300, 5000]
  assert 'guess' in aug.policy.describe()
  _, flags = cli.parse(['train', '--waveforms', '--speed-perturb', '0.9,1.1', '--seed', '4'])
  aug = A().wave_from_flags(flags)
  assert aug.policy.speeds == ((9, 10), (11, 10)) and aug.policy.noise_prob == 0.0 and aug.noise is None and aug.seed == 4
  _, flags = cli.parse(['train', '--waveforms', '--noise-dir', str(noise_dir)])
  assert A().wave_from_flags(flags, rate=16000).policy.noise_prob == 0.5
  # no augmentation: --waveforms alone works, and the identity policy is None
  _, flags = cli.parse(['train', '--waveforms'])
  assert flags.waveforms and A().wave_from_flags(flags) is None
  _, flags = cli.parse(['train', '--waveforms', '--speed-perturb', '1.0'])
  assert A().wave_from_flags(flags) is None
  _, flags = cli.parse(['train'])
  assert not flags.waveforms and A().wave_from_flags(flags) is None
  for extra in (['--speed-perturb', '0.9,1.1'], ['--noise-dir', str(noise_dir)], ['--noise-prob', '0.5'], ['--noise-snr', '0,10']):
    _, flags = cli.parse(['train'] + extra)
    with pytest.raises(ValueError, match='--waveforms'):
      A().wave_from_flags(flags)
  _, flags = cli.parse(['preprocess', '--waveforms'])
  assert flags.waveforms


def test_preprocess_waveforms_writes_the_cache_and_load_samples_reads_it(tmp_path):
  from speecht_amd import preprocessing as P
  data = tmp_path / 'data'
  (data / 'train').mkdir(parents=True)
  rng = np.random.default_rng(3)
  audio = {'a-1': rng.standard_normal(4000).astype(np.float32), 'a-2': rng.standard_normal(9000).astype(np.float32)}
  for name, x in audio.items():
    np.save(str(data / 'train' / (name + '.npy')), x)
  (data / 'train' / 'a.trans.txt').write_text('a-1 HELLO WORLD\na-2 GOOD DAY\n')
  cli = load_cli()
  _, flags = cli.parse(['preprocess', '--waveforms', '--train-only', '--data-dir', str(data)])
  P.Preprocessing(flags).run()
  assert sorted(os.listdir(str(data / 'preprocessed-wave' / 'train'))) == ['a-1.npz', 'a-2.npz']
  reader = P.SpeechCorpusReader(str(data))
  assert reader.wave_rate('train') == 16000
  got = sorted(reader.load_samples('train', feature_type='wave', shuffle_seed=1), key=lambda s: len(s[0]))
  assert len(got) == 2
  for (x, transcript), name in zip(got, ('a-1', 'a-2')):
    assert x.dtype == np.float32 and same_bits(x, audio[name])
  from speecht_amd import vocabulary
  assert list(got[0][1]) == list(vocabulary.sentence_to_ids('HELLO WORLD'))
  # max_size applies to the unperturbed frame count 1 + len // hop: 26 and 57 frames
  assert [len(x) for x, _ in reader.load_samples('train', feature_type='wave', max_size=56)] == [4000]
  assert len(list(reader.load_samples('train', feature_type='wave', max_size=57))) == 2


def test_a_waveform_cache_holds_one_rate(tmp_path):
  """Files at different rates in one corpus are refused when the cache is written, and a cache that holds two rates when it is
  read: the step builds one mel basis for the whole cache."""
  from speecht_amd import preprocessing as P
  data = tmp_path / 'data'
  (data / 'train').mkdir(parents=True)
  np.save(str(data / 'train' / 'a-1.npy'), np.zeros(4000, np.float32))
  np.save(str(data / 'train' / 'a-2.npy'), np.zeros(5000, np.float32))
  (data / 'train' / 'a.trans.txt').write_text('a-1 HELLO\na-2 WORLD\n')
  reader = P.SpeechCorpusReader(str(data))
  rates = {'a-1': 16000, 'a-2': 22050}
  with pytest.raises(ValueError, match='holds one rate'):
    reader.store_waveforms('train', audio_loader=lambda path: (np.load(path), rates[os.path.basename(path)[:3]]))
  assert reader.store_waveforms('train') == 2
  with np.load(str(data / 'preprocessed-wave' / 'train' / 'a-2.npz')) as f:
    np.savez(str(data / 'preprocessed-wave' / 'train' / 'a-2'), audio=f['audio'], rate=np.int64(8000), transcript=f['transcript'])
  with pytest.raises(ValueError, match='holds one rate'):
    list(reader.load_samples('train', feature_type='wave', shuffle_seed=1))


def test_loader_waveform_item_carries_the_global_lengths_and_this_ranks_rows():
  from speecht_amd.speech_input import InputBatchLoader, WaveBatch
  rng = np.random.default_rng(4)
  waves = [rng.standard_normal(n).astype(np.float32) for n in (700, 900, 500, 1100)]
  samples = tuple((w, [1, 2, 3][:1 + i % 3]) for i, w in enumerate(waves))
  whole = InputBatchLoader(16, 4, None, wave=dict(feature_type='power', rate=16000))
  item, lens, labels = whole._feed_item(samples)
  assert isinstance(item, WaveBatch) and item.rank == 0 and item.feature_type == 'power' and item.rate == 16000
  assert lens.tolist() == item.global_lengths.tolist() == [700, 900, 500, 1100] and same_bits(item.audio, np.concatenate(waves))
  assert labels.dense_shape.tolist() == [4, 1 + 1100 // 160]
  shard = InputBatchLoader(16, 2, None, wave=dict(feature_type='power', rate=16000), shard=(1, 2))
  item, lens, labels = shard._feed_item(samples)
  assert item.rank == 1 and lens.tolist() == item.lengths.tolist() == [500, 1100] and item.global_lengths.tolist() == [700, 900, 500, 1100]
  assert same_bits(item.audio, np.concatenate(waves[2:])) and labels.dense_shape.tolist() == [2, 1 + 1100 // 160]
  assert labels.values.tolist() == [1, 2, 3, 1]
