#!/usr/bin/env python3
"""Keyword spotting alone: st_ctc_spot_f32 for 64 x 501 output frames x 256 keywords of 3-12 ids (16 384 jobs) and 16 x 1 501
frames x 64 phrases of 20-60 ids, beside the host form st_ctc_spot_host on the same input (one thread) and st_ctc_align_f32 on
the same logits with one label per utterance of the same states-per-lane dispatch.  Reports the time per (lattice, frame) of
both, their ratio, the same ratio with one spot job per utterance (equal numbers of waves in flight) and the share of lanes that
own a live state.  HIP events, median of 5 x 20 calls; the host form: median of 3 calls.  Writes profiles/spot.json (--output)."""
import argparse, ctypes, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speecht_amd import _lib
from speecht_amd._lib import Tensor3
from speecht_amd.engine_decode import spot_lattice_kpl

ap = argparse.ArgumentParser()
ap.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'spot.json'))
a = ap.parse_args()
C, DEV = 29, 'cuda:0'
lib = _lib.load()
P = lambda t: ctypes.c_void_p(t.data_ptr())
H = lambda x: ctypes.c_void_p(x.ctypes.data)
STREAM = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


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


def csr(lists):
  offs = np.zeros(len(lists) + 1, dtype=np.int32)
  offs[1:] = np.cumsum([len(l) for l in lists])
  return np.array([i for l in lists for i in l] + [0], dtype=np.int32), offs


results = []
for B, T, K, (l_lo, l_hi) in ((64, 501, 256, (3, 12)), (16, 1501, 64, (20, 60))):
  rng = np.random.default_rng(0)
  logits = rng.normal(size=(B, T, C)).astype(np.float32)
  keywords = [rng.integers(0, C - 1, size=int(rng.integers(l_lo, l_hi + 1))).tolist() for _ in range(K)]
  max_len = max(len(k) for k in keywords)
  kpl = spot_lattice_kpl(max_len)
  jobs = np.array([(b, k) for b in range(B) for k in range(K)], dtype=np.int32)          # utterance-major
  n = len(jobs)
  ids, offs = csr(keywords)
  lens = np.full(B, T, dtype=np.int32)
  x = torch.zeros((B, T, 32), dtype=torch.float32, device=DEV)
  x[:, :, :C] = torch.as_tensor(logits)
  desc = Tensor3(x.data_ptr(), B, T, C, 0, T, 32)
  to = lambda v: torch.as_tensor(np.ascontiguousarray(v)).to(DEV)
  d_ids, d_offs, d_lens, d_jobs = to(ids), to(offs), to(lens), to(jobs.reshape(-1))
  score = torch.empty(n, dtype=torch.float64, device=DEV)
  span = torch.empty((n, 2), dtype=torch.int32, device=DEV)
  status = torch.empty(n, dtype=torch.int32, device=DEV)
  need = lib.st_ctc_spot_ws(B, T, max_len, n)
  ws = torch.empty(need // 4 + 4, dtype=torch.int32, device=DEV)

  def run_spot(count=n, table=d_jobs):
    _lib.call('st_ctc_spot_f32', ctypes.byref(desc), P(d_lens), P(d_ids), P(d_offs), K, max_len, P(table), count, P(score), P(span), None,
              None, P(status), P(ws), need, STREAM)

  spot_us, spot_all = median_us(run_spot)
  # one job per utterance (the longest keyword): as many waves in flight as the alignment has
  longest = int(np.argmax([len(k) for k in keywords]))
  d_few = to(np.array([(b, longest) for b in range(B)], dtype=np.int32).reshape(-1))
  few_us, few_all = median_us(lambda: run_spot(B, d_few))
  run_spot()
  torch.cuda.synchronize()
  got = score.cpu().numpy(), span.cpu().numpy(), status.cpu().numpy()

  # the alignment of one label per utterance of the same dispatch on the same logits
  labels = [keywords[(longest + b) % K] for b in range(B)]
  a_ids, a_offs = csr(labels)
  N = int(a_offs[-1])
  d_aids, d_aoffs = to(a_ids), to(a_offs)
  a_spans = torch.empty((N + 1, 2), dtype=torch.int32, device=DEV)
  a_score = torch.empty(B, dtype=torch.float32, device=DEV)
  a_status = torch.empty(B, dtype=torch.int32, device=DEV)
  a_need = lib.st_ctc_align_ws(B, T, max_len)
  a_ws = torch.empty(a_need // 4 + 4, dtype=torch.int32, device=DEV)
  align_us, align_all = median_us(lambda: _lib.call('st_ctc_align_f32', ctypes.byref(desc), P(d_aids), P(d_aoffs), P(d_lens), max_len,
                                                    P(a_spans), None, P(a_score), P(a_status), P(a_ws), a_need, STREAM))

  # the host form on the same input
  h_score, h_span, h_status = np.zeros(n), np.zeros((n, 2), dtype=np.int32), np.zeros(n, dtype=np.int32)
  h_ws = np.zeros(need // 8 + 1, dtype=np.float64)
  host_ms = []
  for _ in range(3):
    t0 = time.perf_counter()
    _lib.call('st_ctc_spot_host', H(logits), B, T, C, H(lens), H(ids), H(offs), K, max_len, H(jobs), n, H(h_score), H(h_span), None, None,
              H(h_status), H(h_ws), h_ws.nbytes)
    host_ms.append((time.perf_counter() - t0) * 1e3)
  same = bool((got[0].view(np.int64) == h_score.view(np.int64)).all() and (got[1] == h_span).all() and (got[2] == h_status).all())
  spot_ns, few_ns, align_ns = (us * 1e3 / (count * T) for us, count in ((spot_us, n), (few_us, B), (align_us, B)))
  live = float(np.mean([(2 * len(keywords[k]) - 1) / (64.0 * kpl) for _, k in jobs]))
  results.append(dict(batch=B, output_frames=T, keywords=K, keyword_lengths=[l_lo, l_hi], max_keyword_len=max_len, states_per_lane=kpl,
                      jobs=n, spot_device_us=round(spot_us, 1), spot_device_us_all=spot_all,
                      spot_one_job_per_utterance_us=round(few_us, 1), spot_one_job_per_utterance_us_all=few_all,
                      align_us=round(align_us, 1), align_us_all=align_all, align_lattices=B,
                      spot_ns_per_lattice_frame=round(spot_ns, 4), align_ns_per_lattice_frame=round(align_ns, 4),
                      spot_over_align_per_lattice_frame=round(spot_ns / align_ns, 4),
                      spot_one_job_per_utterance_ns_per_lattice_frame=round(few_ns, 4),
                      spot_one_job_per_utterance_over_align=round(few_ns / align_ns, 4),
                      share_of_lanes_with_a_live_state=round(live, 4),
                      spot_host_ms=round(sorted(host_ms)[1], 2), spot_host_threads=1, device_equals_host=same))
  print(json.dumps(results[-1]), flush=True)
out = dict(what='st_ctc_spot_f32 (rows of d + one wave per job, two launches; jobs = every (utterance, keyword) pair, utterance-major) '
                'against st_ctc_spot_host (one CPU thread) and st_ctc_align_f32 (log-softmax rows + Viterbi + back-trace, three '
                'launches) on the same logits with one label per utterance of the same states-per-lane dispatch; random logits, 29 '
                'classes, every utterance full length.  spot_over_align_per_lattice_frame compares time / (lattices x frames): the spot '
                'call keeps every compute unit busy with its jobs while the alignment runs one wave per utterance, so that ratio mostly '
                'measures occupancy; spot_one_job_per_utterance_over_align runs both with one wave per utterance and compares the '
                'frame chains themselves',
           method='HIP events around 20 back-to-back calls, median of 5 rounds; host form: wall clock, median of 3',
           device=torch.cuda.get_device_name(0), shapes=results)
os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
with open(a.output, 'w') as f:
  json.dump(out, f, indent=1)
  f.write('\n')
