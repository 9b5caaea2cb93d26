#!/usr/bin/env python3
"""Resampling live streams on the device (StreamingResampler, st_resample_stream_f32; StreamingFeatures(source_rate=)): what it costs.

By the protocol of scripts/bench_stream_words.py: host clock around 20 calls that end in a device synchronise, the forms alternating
inside every round, every figure with its median / min / max over the rounds.

  (a) resampler  one step of 200 ms of new audio per stream at 1 / 16 / 64 streams, 16 000 -> 22 050 and 48 000 -> 22 050, the samples
                 already on the device (plan + launch), and with their upload (step_device); against st_resample_kaiser_f32 on ONE signal
                 holding the same number of outputs, its arguments resident.  Per output sample, and the ratio streamed / offline.
  (b) front end  a StreamingFeatures step with source_rate=16000 (200 ms) against the same front end fed 22 050 Hz audio of the same
                 duration: one more table and launch.  Absolute microseconds and the ratio.
  (c) existing   with --parent DIR (a built tree of the commit before): StreamingFeatures.step without a source rate,
                 st_resample_kaiser_f32 at the shape of profiles/transcribe.json (64 x 15 s, 16 000 -> 22 050) and bench.py in
                 alternating processes, this tree against that one, each ratio beside the parent's own max / min over its repeats.

Writes profiles/stream_resample.json (--output)."""
import argparse, ctypes, json, os, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'stream_resample.json'))
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--streams', type=int, nargs='+', default=[1, 16, 64])
ap.add_argument('--parent', default=None, help='a built tree of the parent commit: also measure (c)')
ap.add_argument('--repeats', type=int, default=3, help='(c): processes per tree')
ap.add_argument('--bench-steps', type=int, default=20)
ap.add_argument('--existing-child', default=None, metavar='TREE', help='(internal) measure the existing paths of TREE, print one JSON line')
a = ap.parse_args()
TREE = os.path.abspath(a.existing_child) if a.existing_child else ROOT
sys.path.insert(0, TREE)
import torch  # noqa: E402
from speecht_amd import _lib, audio_io  # noqa: E402
from speecht_amd.streaming import StreamingFeatures  # noqa: E402

if not torch.cuda.is_available():
  sys.exit('bench_stream_resample.py needs a GPU')
dev = torch.device('cuda:0')
MS = 200                       # new audio per stream and step


def clock(fn, calls):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(calls):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / calls * 1e3


def spread(v):
  return dict(median=round(sorted(v)[len(v) // 2], 5), min=round(min(v), 5), max=round(max(v), 5))


def offline_call(lengths, rate, new, seed=3):
  """st_resample_kaiser_f32 on signals of ``lengths`` samples with every argument resident -> (a function that enqueues it, outputs)."""
  rng = np.random.RandomState(seed)
  lens = np.asarray(lengths, dtype=np.int64)
  out_offsets, valid = audio_io.plan_resample(lens, [rate] * len(lens), new)
  in_offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
  audio = torch.as_tensor(rng.uniform(-1, 1, int(lens.sum())).astype(np.float32)).to(dev)
  meta = torch.as_tensor(np.concatenate([in_offsets, out_offsets, valid])).to(dev)
  rates = torch.as_tensor(np.full(len(lens), rate, np.int32)).to(dev)
  n, total = len(lens), int(out_offsets[-1])
  out = torch.empty(total, dtype=torch.float32, device=dev)
  win = audio_io._device_filter(dev)
  P = lambda t: ctypes.c_void_p(t.data_ptr())
  base = meta.data_ptr()
  keep = (audio, meta, rates, out, win)

  def run():
    _lib.call('st_resample_kaiser_f32', P(audio), ctypes.c_void_p(base), n, P(rates), new, ctypes.c_void_p(base + 8 * (n + 1)),
              ctypes.c_void_p(base + 16 * (n + 1)), total, P(win), win.numel(), P(out), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    return keep
  return run, total


def feature_step(front, slots, samples):
  at = [0]

  def step():
    if at[0] + samples > 400 * samples:
      at[0] = 0
    front.step({s: AUDIO[s % len(AUDIO)][at[0]:at[0] + samples] for s in slots})
    at[0] += samples
  return step


def existing_child():
  """(c), one process: the existing paths of the tree this process imports."""
  S = 16
  front = StreamingFeatures(16000, 80, S, max_chunk_samples=3200, device=dev)
  step = feature_step(front, [front.open() for _ in range(S)], 3200)
  clock(step, 5)
  res = dict(features_step_ms=min(clock(step, 20) for _ in range(3)))
  run, _ = offline_call([240000] * 64, 16000, 22050)
  clock(run, 2)
  res['resample_kaiser_f32_ms'] = min(clock(run, 10) for _ in range(3))
  print('CHILD ' + json.dumps(res), flush=True)


AUDIO = [np.random.RandomState(100 + s).uniform(-1, 1, 401 * 9600).astype(np.float32) for s in range(4)]
if a.existing_child:
  existing_child()
  sys.exit(0)

from speecht_amd.streaming import StreamingResampler  # noqa: E402
out = dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, new_audio_ms_per_step=MS,
           timing='host clock around 20 steps (or calls) that end in a device synchronise; the forms alternate inside every round')

# ---- (a) the resampler's step alone
res = []
for rate in (16000, 48000):
  for S in a.streams:
    new = rate * MS // 1000
    rs = StreamingResampler(22050, S, max_chunk_samples=new, device=dev)
    slots = [rs.open(rate) for _ in range(S)]
    chunk = np.concatenate([AUDIO[s % len(AUDIO)][:new] for s in slots])
    d_chunk = torch.from_numpy(chunk).to(dev)
    feeds = {s: AUDIO[s % len(AUDIO)][:new] for s in slots}
    counts, planned = [], []

    def plan_ahead(steps):                                         # the host's tables are made outside the clock: (a) times the launch
      for _ in range(steps):
        table, where, after, total = rs.plan({s: new for s in slots})
        rs.commit(after)
        planned.append((table, total))

    def launch():
      table, total = planned.pop(0)
      rs.launch(table, d_chunk, total)
      counts.append(total)

    def step():
      rs.step_device(feeds)

    plan_ahead(5)
    clock(launch, 5)
    per_step = counts[-1]
    offline, total = offline_call([S * new], rate, 22050)
    clock(offline, 5)
    t = dict(launch=[], step_device=[], offline=[])
    for _ in range(a.rounds):
      plan_ahead(20)
      t['launch'].append(clock(launch, 20))
      t['step_device'].append(clock(step, 20))
      t['offline'].append(clock(offline, 20))
    r = dict(source_rate=rate, streams=S, new_samples_per_stream=new, outputs_per_step=per_step, offline_outputs=total,
             stream_launch_ms=spread(t['launch']), stream_step_device_ms=spread(t['step_device']), offline_ms=spread(t['offline']),
             ns_per_output_stream=round(sorted(t['launch'])[a.rounds // 2] * 1e6 / per_step, 3),
             ns_per_output_offline=round(sorted(t['offline'])[a.rounds // 2] * 1e6 / total, 3),
             ratio_per_output_stream_over_offline=spread([(p / per_step) / (q / total) for p, q in zip(t['launch'], t['offline'])]))
    print(json.dumps(r), flush=True)
    res.append(r)
out['resampler_step'] = res

# ---- (b) a front-end step at a source rate against the same front end fed at the model's rate
res = []
for S in a.streams:
  fronts = {'source_16000': (StreamingFeatures(22050, 80, S, max_chunk_samples=6000, device=dev, source_rate=16000), 3200),
            'model_rate': (StreamingFeatures(22050, 80, S, max_chunk_samples=6000, device=dev), 4410)}
  steps = {k: feature_step(f, [f.open() for _ in range(S)], n) for k, (f, n) in fronts.items()}
  for fn in steps.values():
    clock(fn, 10)
  t = {k: [] for k in steps}
  for _ in range(a.rounds):
    for k, fn in steps.items():
      t[k].append(clock(fn, 20))
  r = dict(streams=S, n_mels=80, step_ms_source_16000=spread(t['source_16000']), step_ms_model_rate=spread(t['model_rate']),
           difference_us=round((sorted(t['source_16000'])[a.rounds // 2] - sorted(t['model_rate'])[a.rounds // 2]) * 1e3, 2),
           ratio_source_over_model_rate=spread([p / q for p, q in zip(t['source_16000'], t['model_rate'])]))
  print(json.dumps(r), flush=True)
  res.append(r)
  del fronts, steps
out['front_end_step'] = res

# ---- (c) the existing paths against the parent commit's build
if a.parent:
  trees = {'this': ROOT, 'parent': os.path.abspath(a.parent)}
  runs = {k: [] for k in trees}
  for _ in range(a.repeats):                                       # alternating processes
    for k, tree in trees.items():
      p = subprocess.run([sys.executable, os.path.abspath(__file__), '--existing-child', tree], capture_output=True, text=True, timeout=600)
      line = [l for l in p.stdout.splitlines() if l.startswith('CHILD ')]
      if p.returncode != 0 or not line:
        sys.exit('the child on {} failed:\n{}\n{}'.format(tree, p.stdout[-2000:], p.stderr[-2000:]))
      r = json.loads(line[0][6:])
      b = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(a.bench_steps), '--warmup', '5'], cwd=tree,
                         capture_output=True, text=True, timeout=900)
      last = [l for l in b.stdout.splitlines() if l.startswith('{')]
      if b.returncode != 0 or not last:
        sys.exit('bench.py in {} failed:\n{}\n{}'.format(tree, b.stdout[-2000:], b.stderr[-2000:]))
      r['bench_py'] = json.loads(last[-1])
      runs[k].append(r)
      print(k, json.dumps(r), flush=True)
  cmp_ = {}
  for k in [k for k in runs['this'][0] if k != 'bench_py']:
    mine, theirs = [r[k] for r in runs['this']], [r[k] for r in runs['parent']]
    cmp_[k] = dict(this=spread(mine), parent=spread(theirs), ratio_this_over_parent=round(sorted(mine)[len(mine) // 2] / sorted(theirs)[len(theirs) // 2], 4),
                   parent_max_over_min=round(max(theirs) / min(theirs), 4),
                   inside_parent_range=bool(min(theirs) <= sorted(mine)[len(mine) // 2] <= max(theirs)))
  mine, theirs = [r['bench_py']['value'] for r in runs['this']], [r['bench_py']['value'] for r in runs['parent']]
  cmp_['bench_py_value'] = dict(this=spread(mine), parent=spread(theirs), parent_max_over_min=round(max(theirs) / min(theirs), 4),
                                ratio_this_over_parent=round(sorted(mine)[len(mine) // 2] / sorted(theirs)[len(theirs) // 2], 4),
                                inside_parent_range=bool(min(theirs) <= sorted(mine)[len(mine) // 2] <= max(theirs)))
  out['existing_paths_vs_parent'] = dict(streams=16, repeats=a.repeats, order='this tree first in every pair', paths=cmp_)

os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
with open(a.output, 'w') as f:
  json.dump(out, f, indent=1)
  f.write('\n')
