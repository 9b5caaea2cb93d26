#!/usr/bin/env python3
"""Audio to text (`speecht-cli transcribe`): the kaiser_best resampling kernel against the host resampler, and where the time
of transcribe_files goes.

* Resampling: a batch of 64 utterances of 15 s at 16 kHz and at 44.1 kHz, both to 22.05 kHz.  Device time: HIP events around
  the st_resample_kaiser_f32 launch on buffers already on the device, after a warm-up, median over the repeats.  Host time:
  audio_io.resample_kaiser_best (float64 numpy, what load_audio runs for FLAC) on --host-utts of the utterances, in the same
  run, scaled to the batch.  The work the kernel needs is counted from the shapes (taps from the planner's own formulas):
  multiply-adds, float64 operations and the least HBM traffic, against the peaks.
* End to end: transcribe_files on --files copies of the golden LibriSpeech FLAC (5.2 s, 16 kHz) with a fresh full-size
  model, greedy, batch_size 1: host decoding, device resampling + features, then the forward passes and the decoder timed
  apart over the same features.
* --kernel-only: just the resampling launches (for a `rocprofv3 --kernel-trace --stats` run of its own); --merge-stats adds
  such a run's kernel times to the JSON record.
Writes a JSON record (default profiles/transcribe.json)."""
import argparse
import ctypes
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speecht_amd import _lib, audio_io  # noqa: E402

PEAK_FP64_TFLOPS = 78.6          # MI355X FP64 vector, spec
PEAK_HBM_TBS = 8.0               # spec
GOLDEN_FLAC = os.path.join(ROOT, 'tests', 'golden', '1089-134686-0037.flac')


def taps_per_output(n, sr_orig, sr_new):
  """Taps (both wings) of every interpolated output of an n-sample signal: the expressions of csrc/resample_map.h."""
  ratio = float(sr_new) / float(sr_orig)
  scale = min(1.0, ratio)
  step = int(scale * 512)
  nwin = 512 * 64 + 1
  n_out, _ = audio_io.resample_lengths(n, sr_orig, sr_new)
  t = np.arange(n_out, dtype=np.float64) / ratio
  base = t.astype(np.int64)
  total = 0
  for wing in (0, 1):
    frac = scale * (t - base)
    if wing:
      frac = scale - frac
    offset = (frac * 512).astype(np.int64)
    avail = base + 1 if wing == 0 else n - base - 1
    total += int(np.maximum(np.minimum((nwin - offset) // step, avail), 0).sum())
  return total


class DeviceBatch:
  """A resampling batch staged on the device once, launched repeatedly."""

  def __init__(self, signals, rates, sr_new, dev):
    import torch
    self.torch = torch
    lens = np.array([len(s) for s in signals], dtype=np.int64)
    self.out_off, valid = audio_io.plan_resample(lens, rates, sr_new)
    in_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    self.audio = torch.as_tensor(np.concatenate(signals).astype(np.float32)).to(dev)
    self.meta = [torch.as_tensor(a).to(dev) for a in (in_off, self.out_off, valid)]
    self.rates = torch.as_tensor(np.asarray(rates, np.int32)).to(dev)
    self.total = int(self.out_off[-1])
    self.out = torch.empty(self.total, dtype=torch.float32, device=dev)
    self.win = audio_io._device_filter(torch.device(dev))
    self.n, self.sr_new, self.dev = len(signals), sr_new, dev

  def launch(self):
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.call('st_resample_kaiser_f32', P(self.audio), P(self.meta[0]), self.n, P(self.rates), self.sr_new, P(self.meta[1]),
              P(self.meta[2]), self.total, P(self.win), self.win.numel(), P(self.out),
              ctypes.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream))

  def time_ms(self, warmup, repeats):
    torch = self.torch
    for _ in range(warmup):
      self.launch()
    times = []
    for _ in range(repeats):
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      self.launch()
      b.record()
      b.synchronize()
      times.append(a.elapsed_time(b))
    return times


def resample_case(sr_orig, args, dev, rng):
  n = int(args.seconds * sr_orig)
  signals = [np.clip(rng.normal(0, 0.3, n), -1, 1).astype(np.float32) for _ in range(args.batch)]
  batch = DeviceBatch(signals, [sr_orig] * args.batch, 22050, dev)
  times = batch.time_ms(args.warmup, args.repeats)
  ms = float(np.median(times))
  host_t = []
  for s in signals[:args.host_utts]:
    t0 = time.perf_counter()
    audio_io.resample_kaiser_best(s.astype(np.float64), sr_orig, 22050)
    host_t.append(time.perf_counter() - t0)
  taps = taps_per_output(n, sr_orig, 22050) * args.batch
  flops_per_tap = 5 if sr_orig < 22050 else 7       # weight (sub, mul, add; two scaling multiplies when down-sampling) + mul + add
  bytes_min = 4 * n * args.batch + 4 * batch.total + 8 * (512 * 64 + 1)
  t_flops = taps * flops_per_tap / (PEAK_FP64_TFLOPS * 1e12)
  t_bytes = bytes_min / (PEAK_HBM_TBS * 1e12)
  return dict(
      source_rate=sr_orig, target_rate=22050, utterances=args.batch, seconds_each=args.seconds, input_samples=n * args.batch,
      output_samples=batch.total, device_ms_median=ms, device_ms_min=float(np.min(times)), device_ms_max=float(np.max(times)),
      repeats=args.repeats, host_s_per_utterance=float(np.mean(host_t)), host_utterances_timed=len(host_t),
      host_s_batch_scaled=float(np.mean(host_t)) * args.batch, speedup=float(np.mean(host_t)) * args.batch / (ms * 1e-3),
      multiply_adds=taps, fp64_flops=taps * flops_per_tap, hbm_bytes_min=bytes_min,
      bound='fp64' if t_flops > t_bytes else 'hbm', share_of_peak=max(t_flops, t_bytes) / (ms * 1e-3))


def end_to_end(args, dev):
  import torch
  from speecht_amd.speech_input import SingleInputLoader
  from speecht_amd.speech_model import Session, Wav2LetterModel
  from speecht_amd.transcription import device_features, load_native, transcribe_files
  tmp = tempfile.mkdtemp()
  try:
    paths = []
    for i in range(args.files):
      paths.append(os.path.join(tmp, 'utt{:03d}.flac'.format(i)))
      shutil.copy(GOLDEN_FLAC, paths[-1])
    model = Wav2LetterModel(SingleInputLoader(128), 128, 29)
    model.add_training_ops()
    model.add_decoding_ops()
    model.finalize(tmp, 'bench', 'record')
    model.init_seed = 1
    with Session(dev) as sess:
      model.init_session(sess)
      eng = model.engine
      transcribe_files(eng, paths[:2])                             # warm-up: code objects, filter table, allocator
      timings = {}
      t0 = time.perf_counter()
      res = transcribe_files(eng, paths, timings=timings)
      total = time.perf_counter() - t0
      assert all(r['error'] is None for r in res)
      # the network and the decoder apart, over the same features (serial: a synchronise after each stage)
      y, rate = load_native(paths[0])
      feats = device_features([y] * args.files, [rate] * args.files, 'power', 22050, dev)
      fwd = dec = 0.0
      for f in feats:
        eng.load_batch(f[None], [f.shape[0]])
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        eng.forward()
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        eng.greedy_decode()
        torch.cuda.synchronize(dev)
        fwd += t2 - t1
        dec += time.perf_counter() - t2
    audio_s = sum(r['seconds'] for r in res)
    return dict(files=args.files, audio_seconds=audio_s, total_s=total, host_decode_s=timings['decode_host'],
                device_resample_features_s=timings['features'], forward_and_decode_s=timings['transcribe'],
                forward_s_serial=fwd, decode_s_serial=dec, realtime_factor=audio_s / total)
  finally:
    shutil.rmtree(tmp, ignore_errors=True)


def merge_stats(path, out):
  """Kernel times of a `rocprofv3 --kernel-trace` run of --kernel-only (its SQLite results file): the resampling dispatches
  in launch order -- 6 of the 16 kHz batch (1 warm-up + 5), then 6 of the 44.1 kHz batch."""
  import sqlite3
  db = sqlite3.connect(path)
  rows = db.execute("SELECT name, duration FROM kernels WHERE name LIKE '%resample%' ORDER BY start").fetchall()
  per = len(rows) // 2
  stats = {}
  for label, part in (('16000_to_22050', rows[:per]), ('44100_to_22050', rows[per:])):
    ns = np.array([d for _, d in part[1:]], dtype=np.float64)          # without the warm-up launch
    stats[label] = dict(kernel=part[0][0], launches=len(ns), median_ms=float(np.median(ns)) / 1e6,
                        min_ms=float(ns.min()) / 1e6, max_ms=float(ns.max()) / 1e6)
  rec = json.load(open(out))
  rec['rocprof_kernel_trace'] = stats
  with open(out, 'w') as f:
    json.dump(rec, f, indent=1)
  print(json.dumps(stats, indent=1))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=64)
  ap.add_argument('--seconds', type=float, default=15.0)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--repeats', type=int, default=20)
  ap.add_argument('--host-utts', type=int, default=2, help='utterances the host resampler is timed on (scaled to --batch)')
  ap.add_argument('--files', type=int, default=32)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'transcribe.json'))
  ap.add_argument('--kernel-only', action='store_true')
  ap.add_argument('--merge-stats', default=None, help='results database of a rocprofv3 --kernel-trace run of --kernel-only, added to --out')
  args = ap.parse_args()
  if args.merge_stats:
    merge_stats(args.merge_stats, args.out)
    return
  import torch
  assert torch.cuda.is_available(), 'bench_transcribe needs a GPU'
  dev = 'cuda:0'
  rng = np.random.default_rng(0)
  if args.kernel_only:
    for sr in (16000, 44100):
      n = int(args.seconds * sr)
      DeviceBatch([rng.uniform(-1, 1, n).astype(np.float32) for _ in range(args.batch)], [sr] * args.batch, 22050,
                  dev).time_ms(1, 5)
    torch.cuda.synchronize()
    return
  rec = dict(device=torch.cuda.get_device_name(0), resample=[resample_case(sr, args, dev, rng) for sr in (16000, 44100)],
             end_to_end=end_to_end(args, dev))
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(rec, f, indent=1)
  print(json.dumps(rec, indent=1))


if __name__ == '__main__':
  main()
