#!/usr/bin/env python
"""Measures the waveform augmentation on the GPU and writes profiles/wave_augment.json (or --out).

What it times, at 32 x 10 s and 64 x 15 s of 22 050 Hz audio:
  * the augment call (augmentation.apply_wave_device: plan upload, st_wave_augment_f32's launches) for the identity policy, speeds
    only (0.9 / 1.0 / 1.1), noise only (every utterance) and both -- host clock around calls that end in a synchronise;
  * the two kernels' own times from the library's timed launch trace, per output sample;
  * st_resample_kaiser_f32 (the float64 kaiser_best resampler) making as many outputs, from the same trace, for the comparison the
    design rests on (22 050 -> 20 045 Hz is the speed 11/10);
  * the same for a batch in which every utterance is resampled at 11/10 (in the three-speed batch a third is copied);
  * a device ``copy_`` of the output's bytes, the floor of the noise mix, between device events like the kernel times.
With ``--parent DIR`` (a checkout of the parent commit with its library built) it also runs, in processes of their own that
alternate between the two builds, ``--rounds`` times each:
  * the fp32 training step at the headline shape (32 x 10 s at 16 kHz, 80 mel channels) fed features by the parent's build and fed
    waveforms (no augmentation) by this one -- the difference is what features-in-the-step cost -- and fed features by this one;
  * the waveform-fed step with the full policy (three speeds, noise on half the utterances), as a rate in utterances/s;
  * bench.py, load_batch with SpecAugment (LD) and st_melspec_f32 on both builds.
Results of the pairs are ratios of medians with both builds' own min - max."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RATE = 22050


def timed(fn, reps, torch):
  fn()
  torch.cuda.synchronize()
  times = []
  for _ in range(reps):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    times.append((time.perf_counter() - t0) * 1e3)
  return dict(min_ms=min(times), median_ms=float(np.median(times)), max_ms=max(times), reps=reps)


def kernel_ms(lines, name):
  return [float(re.search(r' ms=([0-9.eE+-]+)', l).group(1)) for l in lines if name in l and ' ms=' in l]


def event_us(fn, reps, torch):
  """Device time of fn's work on the current stream, between two events: (min, median, max) in microseconds."""
  fn()
  torch.cuda.synchronize()
  times = []
  for _ in range(reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    times.append(start.elapsed_time(stop) * 1e3)
  return dict(min_us=min(times), median_us=float(np.median(times)), max_us=max(times), reps=reps)


HEADLINE = dict(batch=32, rate=16000, samples=160000, frames=1001, mels=80)


def child_step(args):
  """A training loop at the headline shape through the loader (stager thread and all): features or waveforms in."""
  import torch
  from speecht_amd.speech_input import Coordinator, InputBatchLoader
  from speecht_amd.speech_model import Session, Wav2LetterModel
  H, rng = HEADLINE, np.random.default_rng(0)
  labels = [rng.integers(0, 28, 120).tolist() for _ in range(H['batch'])]
  if args.feed == 'features':
    pool = [rng.standard_normal((H['frames'], H['mels'])).astype(np.float32) for _ in range(H['batch'])]
    kw = {}
  else:
    pool = [(rng.standard_normal(H['samples']) * 0.1).astype(np.float32) for _ in range(H['batch'])]
    kw = dict(wave=dict(feature_type='power', rate=H['rate']))

  def gen():
    while True:
      for x, l in zip(pool, labels):
        yield x, l
  loader = InputBatchLoader(H['mels'], H['batch'], gen, **kw)
  model = Wav2LetterModel(loader, H['mels'], 29)
  train = {}
  if args.policy == 'full':
    from speecht_amd import augmentation as A
    bank = A.NoiseBank.from_arrays([rng.standard_normal(n).astype(np.float32) for n in (48000, 320000, 112000)], H['rate'])
    train = dict(wave_augment=A.WaveAugment(A.WavePolicy(noise_prob=0.5), seed=1, noise=bank))
  model.add_training_ops(learning_rate=1e-4, **train)
  model.add_decoding_ops()
  model.finalize(tempfile.mkdtemp(), 'bench', 'train')
  model.init_seed = 1
  coord = Coordinator()
  with Session('cuda:0') as sess:
    model.init_session(sess)
    loader.start_threads(sess, coord)
    try:
      for _ in range(args.warmup):
        model.step(sess)
      torch.cuda.synchronize()
      each, began = [], time.perf_counter()
      for _ in range(args.steps):
        t0 = time.perf_counter()
        model.step(sess)
        each.append((time.perf_counter() - t0) * 1e3)
      torch.cuda.synchronize()
      total = (time.perf_counter() - began) * 1e3
    finally:
      coord.request_stop()
  ms = total / args.steps
  return dict(ms_per_step=ms, utterances_per_s=H['batch'] * 1e3 / ms, host_ms_min=min(each), host_ms_median=float(np.median(each)),
              host_ms_max=max(each), steps=args.steps)


def child_specaug(args):
  import torch
  from speecht_amd import augmentation as A
  from speecht_amd.engine import Wav2LetterEngine
  from tests import workloads as WL
  H = HEADLINE
  eng = Wav2LetterEngine(WL.w2l_layers(H['mels']), device='cuda:0')
  x = torch.randn(H['batch'], H['frames'], H['mels'], device='cuda:0')
  lens = np.full(H['batch'], H['frames'])
  aug = A.SpecAugment('LD', 1, np.arange(H['batch']))
  return event_us(lambda: eng.load_batch(x, lens, augment=aug), args.steps, torch)


def child_melspec(args):
  import ctypes
  import torch
  from speecht_amd import _lib, preprocessing
  H, dev = HEADLINE, torch.device('cuda:0')
  audio = torch.randn(H['batch'] * H['samples'], device=dev) * 0.1
  s_off = np.arange(H['batch'] + 1, dtype=np.int64) * H['samples']
  f_off = np.arange(H['batch'] + 1, dtype=np.int64) * H['frames']
  total = int(f_off[-1])
  basis = torch.as_tensor(preprocessing.mel_filterbank(float(H['rate']), 512, H['mels']).astype(np.float32)).contiguous().to(dev)
  d_soff, d_foff = torch.as_tensor(s_off).to(dev), torch.as_tensor(f_off).to(dev)
  out = torch.empty(total * H['mels'], dtype=torch.float32, device=dev)
  ws = torch.empty(_lib.load().st_melspec_ws(H['batch'], total, H['mels']) // 4 + 64, dtype=torch.float32, device=dev)
  P = lambda t: ctypes.c_void_p(t.data_ptr())
  stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
  call = lambda: _lib.call('st_melspec_f32', P(audio), P(d_soff), H['batch'], H['samples'], P(basis), H['mels'], 512, 160, P(d_foff), total,
                           P(out), P(ws), ws.numel() * 4, stream)
  return event_us(call, args.steps, torch)


def run_child(root, mode, extra=(), limit=240):
  """One measurement in a process of its own on the build under `root`; a failure ends the whole run."""
  if mode == 'bench':
    cmd = [sys.executable, 'bench.py', '--gpus', '1', '--steps', '30', '--warmup', '10']
  else:
    cmd = [sys.executable, os.path.abspath(__file__), '--child', mode, '--root', root] + list(extra)
  r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=limit)
  if r.returncode != 0:
    raise SystemExit('{} on {} ended with status {}:\n{}'.format(mode, root, r.returncode, (r.stdout + r.stderr)[-3000:]))
  record = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
  if mode == 'bench':
    record = dict(ms_per_step=record['ms_per_step'], ms_per_step_median=record['ms_per_step_median'])
  return record


def spread(records, key):
  values = [r[key] for r in records]
  return dict(min=min(values), median=float(np.median(values)), max=max(values), runs=len(values))


def against_parent(parent, rounds):
  jobs = [('step_features', 'step', ['--feed', 'features'], 'ms_per_step', (parent, ROOT)),
          ('step_waveforms_identity', 'step', ['--feed', 'wave'], 'ms_per_step', (ROOT,)),
          ('step_waveforms_full_policy', 'step', ['--feed', 'wave', '--policy', 'full'], 'utterances_per_s', (ROOT,)),
          ('bench_py', 'bench', [], 'ms_per_step_median', (parent, ROOT)),
          ('load_batch_spec_augment_LD', 'specaug', ['--steps', '200'], 'median_us', (parent, ROOT)),
          ('st_melspec_f32', 'melspec', ['--steps', '200'], 'median_us', (parent, ROOT))]
  runs = {name: {} for name, *_ in jobs}
  for _ in range(rounds):
    for name, mode, extra, key, roots in jobs:
      for root in roots:                               # the builds alternate
        runs[name].setdefault('parent' if root == parent else 'this', []).append(run_child(root, mode, extra))
  out = {}
  for name, mode, extra, key, roots in jobs:
    entry = dict(unit=key, **{build: spread(records, key) for build, records in runs[name].items()})
    if 'parent' in entry:
      entry['ratio_this_over_parent'] = entry['this']['median'] / entry['parent']['median']
    out[name] = entry
  out['step_waveforms_identity']['ratio_over_parent_feature_step'] = (out['step_waveforms_identity']['this']['median'] /
                                                                      out['step_features']['parent']['median'])
  out['step_waveforms_identity']['ms_over_parent_feature_step'] = (out['step_waveforms_identity']['this']['median'] -
                                                                   out['step_features']['parent']['median'])
  return out


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wave_augment.json'))
  parser.add_argument('--reps', type=int, default=30)
  parser.add_argument('--parent', default=None, help='a checkout of the parent commit with its library built')
  parser.add_argument('--rounds', type=int, default=2)
  parser.add_argument('--child', default=None, choices=['step', 'specaug', 'melspec'])
  parser.add_argument('--root', default=ROOT)
  parser.add_argument('--feed', default='features', choices=['features', 'wave'])
  parser.add_argument('--policy', default='none', choices=['none', 'full'])
  parser.add_argument('--steps', type=int, default=60)
  parser.add_argument('--warmup', type=int, default=15)
  args = parser.parse_args()
  sys.path.insert(0, os.path.abspath(args.root))
  if args.child:
    print(json.dumps(dict(step=child_step, specaug=child_specaug, melspec=child_melspec)[args.child](args)))
    return
  import torch
  from speecht_amd import _lib, audio_io
  from speecht_amd import augmentation as A
  assert torch.cuda.is_available(), 'this measurement needs a GPU'
  dev = torch.device('cuda:0')
  rng = np.random.default_rng(0)
  bank = A.NoiseBank.from_arrays([rng.standard_normal(n).astype(np.float32) for n in (RATE * 3, RATE * 20, RATE * 7)], RATE)
  policies = dict(identity=A.WavePolicy(((1, 1),), 0.0), speeds=A.WavePolicy(noise_prob=0.0), noise=A.WavePolicy(((1, 1),), 1.0),
                  both=A.WavePolicy(noise_prob=1.0), one_speed_11_10=A.WavePolicy(((11, 10),), 0.0))
  result = dict(device=torch.cuda.get_device_name(0), rate=RATE, shapes={})
  for batch, seconds in ((32, 10), (64, 15)):
    n = RATE * seconds
    waves = rng.standard_normal((batch, n)).astype(np.float32) * 0.1
    audio = torch.as_tensor(waves.reshape(-1)).to(dev)
    offsets = np.arange(batch + 1, dtype=np.int64) * n
    shape = dict(samples_in=batch * n)
    for name, policy in policies.items():
      aug = A.WaveAugment(policy, seed=1, noise=bank).at(np.arange(batch))
      plan = A.plan_wave_host(aug, np.full(batch, n), min_samples=256)
      call = lambda: A.apply_wave_device(aug, audio, offsets, plan, align=1)
      entry = dict(samples_out=int(plan['M'].sum()), call=timed(call, args.reps, torch))
      with _lib.launch_trace(timed=True) as tr:
        for _ in range(args.reps):
          call()
        torch.cuda.synchronize()
      for kernel in ('wave_speed', 'wave_mix'):
        ms = kernel_ms(tr.lines, kernel)
        if ms:
          entry[kernel] = dict(min_ms=min(ms), max_ms=max(ms), ns_per_output=min(ms) * 1e6 / entry['samples_out'])
      shape[name] = entry
    # the float64 kaiser_best resampler on as many outputs as the speed 11/10 makes: 22 050 -> 20 045 Hz (= 22 050 x 10 / 11, rounded)
    signals = [waves[i] for i in range(batch)]
    with _lib.launch_trace(timed=True) as tr:
      for _ in range(3):
        audio_io.resample_kaiser_best_device(signals, [RATE] * batch, 20045, device='cuda:0')
      torch.cuda.synchronize()
    ms = kernel_ms(tr.lines, 'resample_kaiser')
    outs = [int(re.search(r'out=(\d+)', l).group(1)) for l in tr.lines if 'resample_kaiser' in l]
    shape['resample_kaiser_f32'] = dict(samples_out=outs[0], min_ms=min(ms), max_ms=max(ms), ns_per_output=min(ms) * 1e6 / outs[0])
    dst = torch.empty_like(audio)
    shape['copy_same_bytes'] = event_us(lambda: dst.copy_(audio), args.reps, torch)
    result['shapes']['{}x{}s'.format(batch, seconds)] = shape
  del audio, dst
  torch.cuda.empty_cache()
  if args.parent:
    result['against_parent'] = against_parent(os.path.abspath(args.parent), args.rounds)
  else:
    result['not_measured'] = ['everything that needs the parent build (--parent): the training steps, bench.py, load_batch with SpecAugment, '
                              'st_melspec_f32']
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write('\n')
  print(json.dumps(result, sort_keys=True))


if __name__ == '__main__':
  main()
