#!/usr/bin/env python3
"""Streaming recognition against the stateless form, full-size 80-mel model, 20 new input frames (200 ms) per stream and step,
at 1, 16 and 64 streams.

  stream     StreamingRecognizer.step: eleven products with their epilogues, advance, greedy decode; the new ids come back to the
             host every step (one wait at the end of the step).  `enqueue`: the same steps without reading the ids back, one
             wait after the round -- what the device needs when the host keeps ahead.
  stateless  the only thing possible without carried state: engine.load_batch + forward + greedy_decode on the window that
             yields the same ten new output frames, 212 input frames per stream.

Host clock around work that ends in a device synchronise, the two forms alternating inside every round, median and range of the
rounds.  Streams sustained in real time = streams * 0.2 s / step time.  Weight bytes read per step are counted from the shapes:
every 128-row block of a product reads the layer's packed filters once.  One timed launch trace per stream count names the
kernels a step spends its time in.  Writes profiles/stream.json (--output)."""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speecht_amd import _lib
from speecht_amd.engine import Wav2LetterEngine
from speecht_amd.streaming import StreamingRecognizer
from tests.workloads import synthetic_features, w2l_layers

ap = argparse.ArgumentParser()
ap.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'stream.json'))
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--streams', type=int, nargs='+', default=[1, 16, 64])
a = ap.parse_args()
if not torch.cuda.is_available():
  sys.exit('bench_stream.py needs a GPU')
NEW, WINDOW = 20, 212
eng = Wav2LetterEngine(w2l_layers(80), device='cuda:0')
eng.init_xavier(42)
min_weight_bytes = sum(l.k_pad * l.n_pad * 4 for l in eng.layers)


def clock(fn, calls):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(calls):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / calls * 1e3


def spread(v):
  return dict(median=round(sorted(v)[len(v) // 2], 4), min=round(min(v), 4), max=round(max(v), 4))


results = []
for S in a.streams:
  rec = StreamingRecognizer(eng, S, max_chunk_frames=NEW)
  slots = [rec.open() for _ in range(S)]
  x = np.stack([synthetic_features(s, 4000, 80) for s in range(S)]).astype(np.float32)
  at = [0]

  def stream_step(fetch=True):
    if at[0] + NEW > x.shape[1]:
      at[0] = 0                                                  # (the content does not matter to the time: the counters go on)
    rec.step({slots[s]: x[s, at[0]:at[0] + NEW] for s in range(S)}, fetch=fetch)
    at[0] += NEW

  xw = np.ascontiguousarray(x[:, :WINDOW]).astype(np.float64)
  lens = [WINDOW] * S

  def stateless_step():
    eng.load_batch(xw, lens)
    eng.forward()
    eng.greedy_decode()

  for _ in range(8):                                             # past the 0.99 s look-ahead: every layer emits ten rows per step
    stream_step()
  for _ in range(3):
    stateless_step()
  rows = [S * 10] * len(eng.layers)                           # steady state: ten output frames per stream and layer
  t_stream, t_enqueue, t_stateless = [], [], []
  for _ in range(a.rounds):
    t_stream.append(clock(stream_step, a.steps))
    t_stateless.append(clock(stateless_step, max(a.steps // 2, 1)))
    t_enqueue.append(clock(lambda: stream_step(fetch=False), a.steps))
  with _lib.launch_trace(timed=True) as tr:
    stream_step()
  kernels = {}
  for line in tr.lines:
    name = line.split(' ')[0]
    ms = float(line.rsplit('ms=', 1)[1]) if 'ms=' in line else 0.0
    key = name + (' ' + ' '.join(p for p in line.split(' ') if p.startswith(('Np=', 'Kp='))) if name.startswith('stream_conv') else '')
    kernels[key] = round(kernels.get(key, 0.0) + ms, 4)
  read = sum(l.k_pad * l.n_pad * 4 * -(-r // 128) for l, r in zip(eng.layers, rows))
  ratios = [s / b for s, b in zip(t_stream, t_stateless)]
  res = dict(streams=S, new_frames_per_step=NEW, stateless_window_frames=WINDOW, launches_per_step=rec.launches,
             step_ms=spread(t_stream), step_enqueue_only_ms=spread(t_enqueue), stateless_ms=spread(t_stateless),
             ratio_stream_over_stateless=spread(ratios),
             ratio_enqueue_only_over_stateless=spread([s / b for s, b in zip(t_enqueue, t_stateless)]),
             streams_in_real_time=round(S * 0.2 / (sorted(t_stream)[len(t_stream) // 2] * 1e-3), 1),
             weight_bytes_read_per_step=read, weight_bytes_minimum=min_weight_bytes,
             product_kernel_ms_one_step_traced=kernels)
  print(json.dumps(res), flush=True)
  results.append(res)
  for s in slots:
    rec.close(s)
  del rec
  torch.cuda.empty_cache()

out = dict(device=torch.cuda.get_device_name(0), model='w2l_layers(80), xavier seed 42', rounds=a.rounds, steps_per_round=a.steps,
           timing='host clock around steps that end in a device synchronise; stream and stateless alternate inside every round',
           results=results)
os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
with open(a.output, 'w') as f:
  json.dump(out, f, indent=1)
  f.write('\n')
