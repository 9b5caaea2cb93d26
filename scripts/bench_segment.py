#!/usr/bin/env python3
"""Long recordings, two measurements, written to profiles/segment.json (--output); neither is a gate.

1. Segmentation: one hour of 16 kHz audio (synthetic speech-like bursts: noise under a syllable-rate envelope, 0.5-8 s long, pauses
   of 0.2-2 s, a few bursts longer than max_segment) segmented and gathered on the device (segmentation.segment_device on audio
   already in HBM: four kernels and the read-back of the small tables; wall clock with a device synchronisation, median of 5)
   against the numpy specification tests/segment_oracle.py on the host (one run), and whether the two agree bit for bit.
2. Masking cost: engine.forward(mask_padding=True) against engine.forward() at the configs[2] inference shape -- batches of 64
   utterances of 2-15 s, bucketed by length, 128 mel bands, the full model in fp32 (HIP events around the forward passes of all
   buckets, median of 5): the lost hand-off of the frequency-domain chain plus ten small launches per pass."""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speecht_amd import inference, segmentation
from speecht_amd.engine import Wav2LetterEngine
from tests import segment_oracle, workloads

ap = argparse.ArgumentParser()
ap.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'segment.json'))
ap.add_argument('--seconds', type=float, default=3600.0, help='length of the synthetic recording')
ap.add_argument('--utterances', type=int, default=512, help='utterances of the masking measurement')
ap.add_argument('--skip-oracle', action='store_true', help='do not run the numpy specification (minutes for an hour of audio)')
a = ap.parse_args()
dev = torch.device('cuda:0')


def recording(seconds, rate=16000, seed=0):
  rng = np.random.default_rng(seed)
  parts, n = [], 0
  while n < seconds * rate:
    long_one = rng.random() < 0.02
    burst = int(rate * (rng.uniform(21.0, 30.0) if long_one else rng.uniform(0.5, 8.0)))
    t = np.arange(burst) / rate
    envelope = (0.55 + 0.45 * np.sin(2 * np.pi * rng.uniform(2.0, 5.0) * t)) * rng.uniform(0.2, 0.9)
    parts.append(rng.standard_normal(burst) * 0.3 * envelope)
    parts.append(rng.standard_normal(int(rate * rng.uniform(0.2, 2.0))) * 1e-3)
    n += len(parts[-2]) + len(parts[-1])
  return np.clip(np.concatenate(parts)[:int(seconds * rate)], -1, 1).astype(np.float32), rate


def median(values):
  return sorted(values)[len(values) // 2]


# ---- 1. segmentation --------------------------------------------------------------------------------------------------------
x, rate = recording(a.seconds)
opts = segmentation.SegmentOptions()
audio = torch.as_tensor(np.concatenate([x, np.zeros(4, np.float32)])).to(dev)
offsets = np.array([0, len(x)], dtype=np.int64)
times = []
for _ in range(6):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  table, gathered, out_offsets = segmentation.segment_device(audio, offsets, [rate], opts)
  torch.cuda.synchronize()
  times.append((time.perf_counter() - t0) * 1e3)
seg = dict(seconds_of_audio=a.seconds, rate=rate, segments=int(len(table)), gathered_seconds=round(float(out_offsets[-1]) / rate, 1),
           longest_segment_seconds=round(float((table[:, 2] - table[:, 1]).max()) / rate, 2) if len(table) else 0.0,
           device_ms=round(median(times[1:]), 3), device_ms_all=[round(t, 3) for t in times[1:]])
if not a.skip_oracle:
  t0 = time.perf_counter()
  want, _ = segment_oracle.segment([x], [rate], opts.threshold, opts.min_silence, opts.max_segment)
  utts, _ = segment_oracle.gather([x], [rate], want, opts.pad)
  seg['oracle_host_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
  flat = np.concatenate(utts + [np.zeros(0, np.float32)])
  seg['device_equals_oracle'] = bool(table.tolist() == want.tolist() and
                                     np.array_equal(gathered.cpu().numpy().view(np.uint32), flat.view(np.uint32)))
  seg['oracle_over_device'] = round(seg['oracle_host_ms'] / seg['device_ms'], 1)
print(json.dumps(seg))

# ---- 2. masking cost ----------------------------------------------------------------------------------------------------------
layers = workloads.w2l_layers(128)
eng = Wav2LetterEngine(layers, device='cuda:0', conv_mode='fp32')
eng.set_weights(workloads.xavier_params(layers, seed=1))
rng = np.random.default_rng(2)
lengths = [int(rng.integers(200, 1501)) for _ in range(a.utterances)]          # 2-15 s of 10 ms feature frames
buckets = inference.make_buckets(lengths, 64)
batches = []
for idx in buckets:
  t = max(lengths[i] for i in idx)
  xb = np.zeros((len(idx), t, 128), dtype=np.float32)
  for row, i in enumerate(idx):
    xb[row, :lengths[i]] = rng.standard_normal((lengths[i], 128))
  batches.append((torch.as_tensor(xb).to(dev), [lengths[i] for i in idx]))


def forward_all(mask):
  for xb, lens in batches:
    eng.load_batch(xb, lens)
    eng.forward(mask_padding=True) if mask else eng.forward()


def timed(mask, rounds=5):
  forward_all(mask)
  torch.cuda.synchronize()
  out = []
  for _ in range(rounds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    forward_all(mask)
    e1.record()
    torch.cuda.synchronize()
    out.append(e0.elapsed_time(e1))
  return median(out), [round(t, 2) for t in out]


plain_ms, plain_all = timed(False)
masked_ms, masked_all = timed(True)
mask = dict(utterances=a.utterances, batch=64, buckets=len(buckets), frames=[min(lengths), max(lengths)],
            padding_overhead=round(inference.padding_overhead(lengths, buckets), 4),
            unmasked_ms=round(plain_ms, 2), unmasked_ms_all=plain_all, masked_ms=round(masked_ms, 2), masked_ms_all=masked_all,
            masked_over_unmasked=round(masked_ms / plain_ms, 3))
print(json.dumps(mask))
out = dict(what='device silence segmentation + gather against the numpy specification; masked against unmasked forward passes',
           method='segmentation: wall clock around segment_device with a device synchronisation, median of 5 after a warm-up; '
                  'forward: HIP events around load_batch + forward of every bucket, median of 5 after a warm-up',
           device=torch.cuda.get_device_name(0), segmentation=seg, masking=mask)
os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
with open(a.output, 'w') as f:
  json.dump(out, f, indent=1)
  f.write('\n')
