#!/usr/bin/env python3
"""Tiled forced alignment alone: st_ctc_align_long_f32 on planted logits (tests/align_oracle.planted_logits, 29 classes) for
  ten minutes: 41 400 output frames, 9 000 labels (beside the host form st_ctc_align_long_host, one call),
  one hour:    248 000 output frames, 54 000 labels (six plants of ten minutes joined; the workspace size is printed),
  and 1 501 output frames with 450 labels, where st_ctc_align_f32 (B = 1) runs on the same input in the same run.
HIP events around back-to-back calls, median of the rounds.  Reports long / st_ctc_align_f32 at the shared shape and the time per
frame-block launch at the hour shape.  Writes profiles/align_long.json (--output)."""
import argparse, ctypes, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speecht_amd import _lib
from speecht_amd._lib import Tensor3
from speecht_amd.engine_decode import ALIGN_LONG_FRAME_BLOCK, ALIGN_LONG_STATE_BLOCK
from tests import align_oracle as AO

ap = argparse.ArgumentParser()
ap.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'align_long.json'))
a = ap.parse_args()
C, PITCH = 29, 32
DEV = 'cuda:0'
lib = _lib.load()
P = lambda t: ctypes.c_void_p(t.data_ptr())
H = lambda x: ctypes.c_void_p(x.ctypes.data)


def median_us(fn, rounds, calls):
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


def planted(rng, T, L, parts=1):
  """Planted logits of ``parts`` equal plants joined in time (labels joined; the ids at a join differ, so the joined path is an
  alignment of the joined label)."""
  xs, lab = [], []
  for k in range(parts):
    part = AO.random_labels(rng, L // parts + (L % parts if k == parts - 1 else 0), C, repeat_prob=0.1)
    while lab and part[0] == lab[-1]:
      part[0] = int(rng.integers(C - 1))
    while len(part) > 1 and part[0] == part[1]:
      part[1] = int(rng.integers(C - 1))
    xs.append(AO.planted_logits(rng, part, T // parts + (T % parts if k == parts - 1 else 0), C)[0])
    lab += part
  return np.concatenate(xs), lab


def long_call(x, lab):
  T, L = x.shape[0], len(lab)
  d_x = torch.zeros((T, PITCH), dtype=torch.float32, device=DEV)
  d_x[:, :C] = torch.as_tensor(x)
  d_ids = torch.as_tensor(np.array(lab + [0], dtype=np.int32)).to(DEV)
  spans = torch.empty((L, 2), dtype=torch.int32, device=DEV)
  score = torch.empty(1, dtype=torch.float64, device=DEV)
  status = torch.empty(1, dtype=torch.int32, device=DEV)
  need = lib.st_ctc_align_long_ws(T, L)
  ws = torch.empty(need // 4 + 4, dtype=torch.int32, device=DEV)
  stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
  run = lambda: _lib.call('st_ctc_align_long_f32', P(d_x), T, C, PITCH, P(d_ids), L, P(spans), P(score), P(status), P(ws), need, stream)
  return run, (d_x, d_ids, spans, score, status), need


def shape_entry(name, x, lab, rounds, calls):
  T, L = x.shape[0], len(lab)
  run, (d_x, d_ids, spans, score, status), need = long_call(x, lab)
  us, us_all = median_us(run, rounds, calls)
  frame_blocks = -(-T // ALIGN_LONG_FRAME_BLOCK)
  state_blocks = -(-(2 * L + 1) // ALIGN_LONG_STATE_BLOCK)
  entry = dict(shape=name, output_frames=T, labels=L, workspace_bytes=int(need), state_blocks=state_blocks, frame_block_launches=frame_blocks,
               launches=frame_blocks + 3, align_long_us=round(us, 1), align_long_us_all=us_all,
               us_per_frame_block_launch=round(us / frame_blocks, 2), status=int(status.cpu()[0]), score=float(score.cpu()[0]))
  return entry, (spans, score, status, d_x, d_ids)


rng = np.random.default_rng(0)
results = []

# ten minutes, beside the host form
x, lab = planted(rng, 41400, 9000)
entry, (spans, score, status, _, _) = shape_entry('ten minutes', x, lab, rounds=5, calls=3)
h_spans, h_score, h_status = np.zeros((len(lab), 2), dtype=np.int32), np.zeros(1), np.zeros(1, dtype=np.int32)
h_ws = np.zeros(entry['workspace_bytes'] // 8 + 1, dtype=np.float64)
h_ids = np.array(lab + [0], dtype=np.int32)
t0 = time.perf_counter()
_lib.call('st_ctc_align_long_host', H(x), x.shape[0], C, C, H(h_ids), len(lab), H(h_spans), H(h_score),
          H(h_status), H(h_ws), h_ws.nbytes)
entry.update(align_long_host_ms=round((time.perf_counter() - t0) * 1e3, 1), align_long_host_threads=1,
             device_equals_host=bool((spans.cpu().numpy() == h_spans).all() and score.cpu().numpy().view(np.int64)[0] == h_score.view(np.int64)[0]
                                     and int(status.cpu()[0]) == int(h_status[0])))
del h_ws
results.append(entry)
print(json.dumps(entry), flush=True)

# one hour
x, lab = planted(rng, 248000, 54000, parts=6)
entry, _ = shape_entry('one hour', x, lab, rounds=3, calls=2)
print('one hour: workspace {} bytes ({:.2f} GiB)'.format(entry['workspace_bytes'], entry['workspace_bytes'] / 2.0 ** 30), flush=True)
results.append(entry)
print(json.dumps(entry), flush=True)
del _
torch.cuda.empty_cache()

# the shape both kernels take: B = 1, the same input, the same run
x, lab = planted(rng, 1501, 450)
T, L = x.shape[0], len(lab)
entry, (spans, score, status, d_x, d_ids) = shape_entry('shared with st_ctc_align_f32', x, lab, rounds=5, calls=20)
d_offs = torch.as_tensor(np.array([0, L], dtype=np.int32)).to(DEV)
d_lens = torch.as_tensor(np.array([T], dtype=np.int32)).to(DEV)
s_spans = torch.empty((L, 2), dtype=torch.int32, device=DEV)
s_states = torch.empty(T, dtype=torch.int32, device=DEV)
s_score = torch.empty(1, dtype=torch.float32, device=DEV)
s_status = torch.empty(1, dtype=torch.int32, device=DEV)
s_need = lib.st_ctc_align_ws(1, T, L)
s_ws = torch.empty(s_need // 4 + 4, dtype=torch.int32, device=DEV)
desc = Tensor3(d_x.data_ptr(), 1, T, C, 0, T, PITCH)
stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
short_us, short_all = median_us(lambda: _lib.call('st_ctc_align_f32', ctypes.byref(desc), P(d_ids), P(d_offs), P(d_lens), L, P(s_spans),
                                                  P(s_states), P(s_score), P(s_status), P(s_ws), s_need, stream), rounds=5, calls=20)
entry.update(align_us=round(short_us, 1), align_us_all=short_all, align_launches=3,
             long_over_align=round(entry['align_long_us'] / short_us, 2),
             same_spans_and_score=bool((spans.cpu().numpy() == s_spans.cpu().numpy()).all() and
                                       np.float32(score.cpu().numpy()[0]) == s_score.cpu().numpy()[0]))
results.append(entry)
print(json.dumps(entry), flush=True)

out = dict(what='st_ctc_align_long_f32 (log-softmax rows, init, one launch of ceil((2 L + 1) / 896) one-wave workgroups per 64-frame block, '
                'one back-trace wave) on planted logits, 29 classes; beside st_ctc_align_long_host (one CPU thread) at the ten-minute '
                'shape and st_ctc_align_f32 (three launches, B = 1) at the shape both take',
           method='HIP events around back-to-back calls, median of the rounds (ten minutes 5 x 3, one hour 3 x 2, shared shape 5 x 20); '
                  'host form: wall clock of one call',
           device=torch.cuda.get_device_name(0), shapes=results)
os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
with open(a.output, 'w') as f:
  json.dump(out, f, indent=1)
  f.write('\n')
