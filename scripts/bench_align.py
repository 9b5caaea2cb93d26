#!/usr/bin/env python3
"""Forced alignment alone: st_ctc_align_f32 (engine.align without its host copies) for 64 x 501 and 16 x 1 501 output frames with
labels of realistic length (100-150 and 300-450 ids), beside the host form st_ctc_align_host on the same input and the CTC loss +
gradient call on the same shape (the same sequential chain: one wave per utterance walks the frames).  HIP events, median of 5 x 20
calls; the host form: median of 3 calls.  Writes profiles/align.json (--output)."""
import argparse, ctypes, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speecht_amd import _lib
from speecht_amd.engine import Wav2LetterEngine

ap = argparse.ArgumentParser()
ap.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'align.json'))
a = ap.parse_args()
C = 29
lib = _lib.load()
P = lambda t: ctypes.c_void_p(t.data_ptr())
H = lambda x: ctypes.c_void_p(x.ctypes.data)


def median_us(fn, rounds=5, calls=20):
  for _ in range(3):
    fn()
  torch.cuda.synchronize()
  times = []
  for _ in range(rounds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
      fn()
    e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1) / calls * 1e3)
  return sorted(times)[rounds // 2], [round(t, 1) for t in times]


results = []
for B, T, (l_lo, l_hi) in ((64, 501, (100, 150)), (16, 1501, (300, 450))):
  rng = np.random.default_rng(0)
  logits = rng.normal(size=(B, T, C)).astype(np.float32)
  labels = [rng.integers(0, C - 1, size=int(rng.integers(l_lo, l_hi + 1))).tolist() for _ in range(B)]
  eng = Wav2LetterEngine([(1, 1, 16, C, False)], device='cuda:0')
  eng.load_batch(np.zeros((B, T, 16)), [T] * B)
  eng.X[-1].interior().copy_(torch.as_tensor(logits))
  eng.ctc_lens = torch.full((B,), T, dtype=torch.int32, device='cuda:0')
  eng.set_labels(labels)
  eng._wait_uploads()
  max_len = eng.max_label_len
  N = sum(len(l) for l in labels)
  need = lib.st_ctc_align_ws(B, T, max_len)
  ws = torch.empty(need // 4 + 4, dtype=torch.int32, device='cuda:0')
  spans = torch.empty(2 * N, dtype=torch.int32, device='cuda:0')
  states = torch.empty(B * T, dtype=torch.int32, device='cuda:0')
  score = torch.empty(B, dtype=torch.float32, device='cuda:0')
  status = torch.empty(B, dtype=torch.int32, device='cuda:0')

  def run_align():
    _lib.call('st_ctc_align_f32', eng.X[-1].ref, P(eng.label_ids), P(eng.label_offs), P(eng.ctc_lens), max_len, P(spans), P(states),
              P(score), P(status), P(ws), need, eng.stream_ptr)

  align_us, align_all = median_us(run_align)
  ctc_us, ctc_all = median_us(lambda: eng.ctc_loss_grad(1.0 / B))
  # the host form on the same input
  ids = np.array([i for l in labels for i in l] + [0], dtype=np.int32)
  offs = np.zeros(B + 1, dtype=np.int32)
  offs[1:] = np.cumsum([len(l) for l in labels])
  lens = np.full(B, T, dtype=np.int32)
  h_spans, h_states = np.zeros((N, 2), dtype=np.int32), np.zeros((B, T), dtype=np.int32)
  h_score, h_status = np.zeros(B, dtype=np.float32), np.zeros(B, dtype=np.int32)
  h_ws = np.zeros(need // 8 + 1, dtype=np.float64)
  host_ms = []
  for _ in range(3):
    t0 = time.perf_counter()
    _lib.call('st_ctc_align_host', H(logits), B, T, C, H(ids), H(offs), H(lens), max_len, H(h_spans), H(h_states), H(h_score),
              H(h_status), H(h_ws), h_ws.nbytes)
    host_ms.append((time.perf_counter() - t0) * 1e3)
  same = bool((states.cpu().numpy().reshape(B, T) == h_states).all() and (spans.cpu().numpy().reshape(N, 2) == h_spans).all() and
              (score.cpu().numpy() == h_score).all() and (status.cpu().numpy() == h_status).all())
  results.append(dict(batch=B, output_frames=T, label_lengths=[l_lo, l_hi], max_label_len=max_len,
                      align_device_us=round(align_us, 1), align_device_us_all=align_all,
                      ctc_loss_grad_us=round(ctc_us, 1), ctc_loss_grad_us_all=ctc_all,
                      align_over_ctc_loss_grad=round(align_us / ctc_us, 2),
                      align_host_ms=round(sorted(host_ms)[1], 2), align_host_threads=1, device_equals_host=same))
  print(json.dumps(results[-1]))
out = dict(what='st_ctc_align_f32 (log-softmax + Viterbi + back-trace, three launches) against st_ctc_align_host (one CPU thread) and '
                'st_ctc_loss_grad_hilo_f32 on the same logits and labels; random logits, 29 classes, every utterance full length',
           method='HIP events around 20 back-to-back calls, median of 5 rounds; host form: wall clock, median of 3',
           device=torch.cuda.get_device_name(0), shapes=results)
os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
with open(a.output, 'w') as f:
  json.dump(out, f, indent=1)
  f.write('\n')
