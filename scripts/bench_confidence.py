#!/usr/bin/env python3
"""Word confidences alone: st_ctc_word_conf_f32 (engine.word_confidence without its host copies) for 64 x 501 and 16 x 1 501 output
frames with labels of realistic length (100-150 and 300-450 ids, a space about every 5 ids), beside the host form
st_ctc_word_conf_host on the same input (one thread) and the CTC loss + gradient call on the same logits and labels.  HIP events,
median of 5 x 20 calls; the host form: median of 3 calls.  Writes profiles/confidence.json (--output)."""
import argparse, ctypes, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speecht_amd import _lib, alignment
from speecht_amd.engine import Wav2LetterEngine

ap = argparse.ArgumentParser()
ap.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'confidence.json'))
a = ap.parse_args()
C, SPACE = 29, 27
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


def words_label(rng, n):
  """n ids: words of 1 to 8 letters (4.5 on average) with one space between them."""
  out = []
  while len(out) < n:
    out += rng.integers(0, 27, size=int(rng.integers(1, 9))).tolist() + [SPACE]
  out = out[:n]
  if out[-1] == SPACE:
    out[-1] = 0
  return out


results = []
for B, T, (l_lo, l_hi) in ((64, 501, (100, 150)), (16, 1501, (300, 450))):
  rng = np.random.default_rng(0)
  logits = rng.normal(size=(B, T, C)).astype(np.float32)
  labels = [words_label(rng, int(rng.integers(l_lo, l_hi + 1))) for _ in range(B)]
  eng = Wav2LetterEngine([(1, 1, 16, C, False)], device='cuda:0')
  eng.load_batch(np.zeros((B, T, 16)), [T] * B)
  eng.X[-1].interior().copy_(torch.as_tensor(logits))
  eng.ctc_lens = torch.full((B,), T, dtype=torch.int32, device='cuda:0')
  eng.set_labels(labels)
  eng._wait_uploads()
  max_len = eng.max_label_len
  spans = np.array([(b, s, e) for b, l in enumerate(labels) for s, e in alignment.word_runs(l)], dtype=np.int32)
  W = len(spans)
  d_spans = torch.as_tensor(spans.reshape(-1)).to('cuda:0')
  need = lib.st_ctc_word_conf_ws(B, T, max_len, B + W)
  ws = torch.empty(need // 4 + 4, dtype=torch.int32, device='cuda:0')
  log_prob = torch.empty(B, dtype=torch.float64, device='cuda:0')
  log_conf = torch.empty(W, dtype=torch.float64, device='cuda:0')
  status = torch.empty(B, dtype=torch.int32, device='cuda:0')

  def run_conf():
    _lib.call('st_ctc_word_conf_f32', eng.X[-1].ref, P(eng.label_ids), P(eng.label_offs), P(eng.ctc_lens), max_len, SPACE, P(d_spans), W,
              P(log_prob), P(log_conf), P(status), P(ws), need, eng.stream_ptr)

  conf_us, conf_all = median_us(run_conf)
  ctc_us, ctc_all = median_us(lambda: eng.ctc_loss_grad(1.0 / B))
  # the host form on the same input
  ids = np.array([i for l in labels for i in l] + [0], dtype=np.int32)
  offs = np.zeros(B + 1, dtype=np.int32)
  offs[1:] = np.cumsum([len(l) for l in labels])
  lens = np.full(B, T, dtype=np.int32)
  h_prob, h_conf, h_status = np.zeros(B), np.zeros(W), np.zeros(B, dtype=np.int32)
  h_ws = np.zeros(need // 8 + 1, dtype=np.float64)
  host_ms = []
  for _ in range(3):
    t0 = time.perf_counter()
    _lib.call('st_ctc_word_conf_host', H(logits), B, T, C, H(ids), H(offs), H(lens), max_len, SPACE, H(spans), W, H(h_prob), H(h_conf),
              H(h_status), H(h_ws), h_ws.nbytes)
    host_ms.append((time.perf_counter() - t0) * 1e3)
  same = bool((log_prob.cpu().numpy().view(np.int64) == h_prob.view(np.int64)).all() and
              (log_conf.cpu().numpy().view(np.int64) == h_conf.view(np.int64)).all() and (status.cpu().numpy() == h_status).all())
  results.append(dict(batch=B, output_frames=T, label_lengths=[l_lo, l_hi], max_label_len=max_len, words=W, jobs=B + W,
                      confidence_device_us=round(conf_us, 1), confidence_device_us_all=conf_all,
                      ctc_loss_grad_us=round(ctc_us, 1), ctc_loss_grad_us_all=ctc_all,
                      confidence_over_ctc_loss_grad=round(conf_us / ctc_us, 2),
                      confidence_host_ms=round(sorted(host_ms)[1], 2), confidence_host_threads=1, device_equals_host=same))
  print(json.dumps(results[-1]), flush=True)
out = dict(what='st_ctc_word_conf_f32 (softmax rows + one wave per job + finish, three launches; jobs = utterances + words) against '
                'st_ctc_word_conf_host (one CPU thread) and st_ctc_loss_grad_hilo_f32 on the same logits and labels; random logits, 29 '
                'classes, a space about every 5 ids, every utterance full length',
           method='HIP events around 20 back-to-back calls, median of 5 rounds; host form: wall clock, median of 3',
           device=torch.cuda.get_device_name(0), shapes=results)
os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
with open(a.output, 'w') as f:
  json.dump(out, f, indent=1)
  f.write('\n')
