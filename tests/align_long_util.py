"""Callers of st_ctc_align_long_host / st_ctc_align_long_f32 shared by tests/test_align_long_cpu.py and
tests/test_gpu_align_long.py, and the label makers that put repeats on the edges of the state blocks."""
import ctypes

import numpy as np


def _p(a):
  return ctypes.c_void_p(a.ctypes.data)


def state_blocks(L, state_block=896):
  return (2 * L + 1 + state_block - 1) // state_block


def workspace_bytes(T, L):
  """The documented formula of st_ctc_align_long_ws (include/speecht_hip.h)."""
  nb = state_blocks(L)
  return T * (32 * 8 + 56 * 4 * nb) + 2 * (896 * nb + 128) * 8 + 512


def host_align_long(logits, labels, classes=None, fill=None):
  """st_ctc_align_long_host on dense [T, pitch] logits -> (spans [L, 2], score float64, status).  ``fill``: the byte the
  workspace holds before the call."""
  from speecht_amd import _lib
  lib = _lib.load()
  logits = np.ascontiguousarray(logits, dtype=np.float32)
  T, pitch = logits.shape
  C = pitch if classes is None else classes
  L = len(labels)
  ids = np.array(list(labels) + [0], dtype=np.int32)
  spans = np.full((L + 1, 2), -7, dtype=np.int32)
  score = np.full(1, 7.0)
  status = np.full(1, -7, dtype=np.int32)
  need = lib.st_ctc_align_long_ws(T, L)
  assert need == workspace_bytes(T, L)
  ws = np.zeros(need // 8 + 1, dtype=np.float64)
  if fill is not None:
    ws.view(np.uint8)[:] = fill
  _lib.call('st_ctc_align_long_host', _p(logits), T, C, pitch, _p(ids), L, _p(spans), _p(score), _p(status), _p(ws), need)
  assert (spans[-1] == -7).all()                       # nothing written past the last label
  return spans[:L], score[0], int(status[0])


def states_from_spans(spans, T):
  """Per-frame label indices (-1 = blank) of an alignment given by its spans."""
  states = np.full(T, -1, dtype=np.int64)
  for k, (a, b) in enumerate(np.asarray(spans)):
    states[a:b] = k
  return states


def edge_labels(rng, L, C, edges=(896, 1792), repeat_prob=0.2):
  """L random ids in [0, C-1) with adjacent repeats, and a repeat forced on every pair of ids whose states straddle one of the
  state-block ``edges``: state 2k+1 is id k, so the ids around state e are e // 2 - 1, e // 2 and e // 2 + 1."""
  lab = []
  for k in range(L):
    lab.append(lab[-1] if k and rng.random() < repeat_prob else int(rng.integers(C - 1)))
  for e in edges:
    k = e // 2
    if 1 <= k and k + 1 < L:
      lab[k - 1] = lab[k] = lab[k + 1]
  return lab


def device_align_long(dev, logits, labels, classes=None, workspace=None):
  """st_ctc_align_long_f32 on dense [T, C] logits laid out with a row pitch of 32 (the pitch columns 1e30: never read)
  -> (spans [L, 2], score float64, status).  ``workspace``: an int32 device tensor to run in (at least the bytes needed)."""
  import torch
  from speecht_amd import _lib
  lib = _lib.load()
  logits = np.asarray(logits, dtype=np.float32)
  T, C = logits.shape
  C = C if classes is None else classes
  L = len(labels)
  x = torch.full((T, 32), 1e30, dtype=torch.float32, device=dev)
  x[:, :C] = torch.as_tensor(logits[:, :C])
  d_ids = torch.as_tensor(np.array(list(labels) + [0], dtype=np.int32)).to(dev)
  spans = torch.full((L + 1, 2), -7, dtype=torch.int32, device=dev)
  score = torch.full((1,), 7.0, dtype=torch.float64, device=dev)
  status = torch.full((1,), -7, dtype=torch.int32, device=dev)
  need = lib.st_ctc_align_long_ws(T, L)
  assert need == workspace_bytes(T, L)
  ws = torch.empty(need // 4 + 4, dtype=torch.int32, device=dev) if workspace is None else workspace
  assert ws.numel() * 4 >= need
  P = lambda t: ctypes.c_void_p(t.data_ptr())
  _lib.call('st_ctc_align_long_f32', P(x), T, C, 32, P(d_ids), L, P(spans), P(score), P(status), P(ws), need,
            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
  torch.cuda.synchronize()
  spans = spans.cpu().numpy()
  assert (spans[-1] == -7).all()                        # nothing written past the last label
  return spans[:L], float(score.cpu().numpy()[0]), int(status.cpu().numpy()[0])


def same_result(a, b):
  """Spans, the score's bits and the status of two (spans, score, status) results."""
  return (np.array_equal(a[0], b[0]) and np.float64(a[1]).view(np.int64) == np.float64(b[1]).view(np.int64) and a[2] == b[2])
