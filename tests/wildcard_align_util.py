"""Callers of the wildcard entry points (st_ctc_align_wild_* and st_ctc_align_long_wild_*, host and device) shared by
tests/test_wildcard_align_cpu.py and tests/test_gpu_wildcard_align.py, and the checks both apply to a result."""
import ctypes

import numpy as np

from tests import align_oracle as AO
from tests import wildcard_align_oracle as WO

C_PITCH = 32


def _p(a):
  return ctypes.c_void_p(a.ctypes.data)


def _csr(labels):
  lens = [len(l) for l in labels]
  offs = np.zeros(len(labels) + 1, dtype=np.int32)
  offs[1:] = np.cumsum(lens)
  return np.array([i for l in labels for i in l] + [0], dtype=np.int32), offs


def host_align_wild(logits, labels, seq_lens, bias, max_label_len=None, want_fit=True, check=True):
  """st_ctc_align_wild_host on a dense [B, T, C] batch -> (spans list, states [B, T], score [B], status [B], fit list);
  ``check=False``: -> the return code alone."""
  from speecht_amd import _lib
  lib = _lib.load()
  logits = np.ascontiguousarray(logits, dtype=np.float32)
  B, T, C = logits.shape
  ids, offs = _csr(labels)
  N = int(offs[-1])
  max_len = max([len(l) for l in labels] + [0]) if max_label_len is None else max_label_len
  spans = np.full((N + 1, 2), -7, dtype=np.int32)
  states = np.full((B, T), -7, dtype=np.int32)
  score = np.zeros(B, dtype=np.float32)
  status = np.full(B, -7, dtype=np.int32)
  fit = np.full(N + 1, 7.0)
  ws = np.zeros(lib.st_ctc_align_ws(B, T, max(max_len, 0)) // 8 + 1, dtype=np.float64)
  args = (_p(logits), B, T, C, _p(ids), _p(offs), _p(np.asarray(seq_lens, dtype=np.int32)), max_len, float(bias), _p(spans),
          _p(states), _p(score), _p(status), _p(fit) if want_fit else None, _p(ws), ws.nbytes)
  if not check:
    return lib.st_ctc_align_wild_host(*args)
  _lib.call('st_ctc_align_wild_host', *args)
  assert (spans[-1] == -7).all() and fit[-1] == 7.0                # nothing written past the last label
  return ([spans[offs[b]:offs[b + 1]] for b in range(B)], states, score, status, [fit[offs[b]:offs[b + 1]] for b in range(B)])


def host_align_long_wild(logits, labels, bias, classes=None, want_fit=True, check=True):
  """st_ctc_align_long_wild_host on dense [T, pitch] logits -> (spans [L, 2], score float64, status, fit [L])."""
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
  fit = np.full(L + 1, 7.0)
  need = lib.st_ctc_align_long_ws(T, L)
  ws = np.zeros(need // 8 + 1, dtype=np.float64)
  args = (_p(logits), T, C, pitch, _p(ids), L, float(bias), _p(spans), _p(score), _p(status), _p(fit) if want_fit else None, _p(ws),
          need)
  if not check:
    return lib.st_ctc_align_long_wild_host(*args)
  _lib.call('st_ctc_align_long_wild_host', *args)
  assert (spans[-1] == -7).all() and fit[-1] == 7.0
  return spans[:L], score[0], int(status[0]), fit[:L]


def device_align_wild(dev, logits, labels, seq_lens, bias, max_label_len=None, want_states=True, want_fit=True):
  """st_ctc_align_wild_f32 on a dense [B, T, C] batch laid out as padded NWC (halo 0, c_pitch 32, the pitch columns 1e30: never
  read) -> (spans list, states [B, T], score [B], status [B], fit list)."""
  import torch
  from speecht_amd import _lib
  from speecht_amd._lib import Tensor3
  lib = _lib.load()
  logits = np.asarray(logits, dtype=np.float32)
  B, T, C = logits.shape
  ids, offs = _csr(labels)
  N = int(offs[-1])
  max_len = max([len(l) for l in labels] + [0]) if max_label_len is None else max_label_len
  x = torch.full((B, T, C_PITCH), 1e30, dtype=torch.float32, device=dev)
  x[:, :, :C] = torch.as_tensor(logits)
  to = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
  d_ids, d_offs, d_lens = to(ids), to(offs), to(np.asarray(seq_lens, dtype=np.int32))
  spans = torch.full((N + 1, 2), -7, dtype=torch.int32, device=dev)
  states = torch.full((B, T), -7, dtype=torch.int32, device=dev)
  score = torch.zeros(B, dtype=torch.float32, device=dev)
  status = torch.full((B,), -7, dtype=torch.int32, device=dev)
  fit = torch.full((N + 1,), 7.0, dtype=torch.float64, device=dev)
  need = lib.st_ctc_align_ws(B, T, max_len)
  ws = torch.empty(need // 4 + 4, dtype=torch.int32, device=dev)
  P = lambda t: ctypes.c_void_p(t.data_ptr())
  desc = Tensor3(x.data_ptr(), B, T, C, 0, T, C_PITCH)
  _lib.call('st_ctc_align_wild_f32', ctypes.byref(desc), P(d_ids), P(d_offs), P(d_lens), max_len, float(bias), P(spans),
            P(states) if want_states else None, P(score), P(status), P(fit) if want_fit else None, P(ws), need,
            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
  torch.cuda.synchronize()
  spans, fit = spans.cpu().numpy(), fit.cpu().numpy()
  assert (spans[-1] == -7).all() and fit[-1] == 7.0
  return ([spans[offs[b]:offs[b + 1]] for b in range(B)], states.cpu().numpy(), score.cpu().numpy(), status.cpu().numpy(),
          [fit[offs[b]:offs[b + 1]] for b in range(B)])


def device_align_long_wild(dev, logits, labels, bias, want_fit=True):
  """st_ctc_align_long_wild_f32 on dense [T, C] logits at a row pitch of 32 -> (spans [L, 2], score float64, status, fit [L])."""
  import torch
  from speecht_amd import _lib
  lib = _lib.load()
  logits = np.asarray(logits, dtype=np.float32)
  T, C = logits.shape
  L = len(labels)
  x = torch.full((T, C_PITCH), 1e30, dtype=torch.float32, device=dev)
  x[:, :C] = torch.as_tensor(logits)
  d_ids = torch.as_tensor(np.array(list(labels) + [0], dtype=np.int32)).to(dev)
  spans = torch.full((L + 1, 2), -7, dtype=torch.int32, device=dev)
  score = torch.full((1,), 7.0, dtype=torch.float64, device=dev)
  status = torch.full((1,), -7, dtype=torch.int32, device=dev)
  fit = torch.full((L + 1,), 7.0, dtype=torch.float64, device=dev)
  need = lib.st_ctc_align_long_ws(T, L)
  ws = torch.empty(need // 4 + 4, dtype=torch.int32, device=dev)
  P = lambda t: ctypes.c_void_p(t.data_ptr())
  _lib.call('st_ctc_align_long_wild_f32', P(x), T, C, C_PITCH, P(d_ids), L, float(bias), P(spans), P(score), P(status),
            P(fit) if want_fit else None, P(ws), need, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
  torch.cuda.synchronize()
  spans, fit = spans.cpu().numpy(), fit.cpu().numpy()
  assert (spans[-1] == -7).all() and fit[-1] == 7.0
  return spans[:L], float(score.cpu().numpy()[0]), int(status.cpu().numpy()[0]), fit[:L]


def bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_long(a, b):
  """Two (spans, score, status, fit) results of the tiled aligner agree bit for bit (NaN fits by their bits)."""
  return (np.array_equal(a[0], b[0]) and bits([a[1]])[0] == bits([b[1]])[0] and a[2] == b[2] and
          np.array_equal(np.isnan(a[3]), np.isnan(b[3])) and np.array_equal(bits(a[3])[~np.isnan(a[3])], bits(b[3])[~np.isnan(b[3])]))


def check_fit(x, lab, spans, fit, bias):
  """The fit of one aligned utterance against the float64 sum: 1e-9 relative (what tests/test_gpu_align_long.py allows the
  score), wildcards exactly bias * frames, and 0 exactly for labels whose class is the row maximum on all their frames."""
  x = np.asarray(x)
  C = x.shape[1]
  ref = WO.fit64(x, lab, spans, bias)
  assert len(fit) == len(lab)
  for k, (c, (a, b)) in enumerate(zip(lab, spans)):
    if c == WO.wild_id(C):
      assert fit[k] == np.float64(bias) * float(b - a), (k, fit[k])
    else:
      assert abs(fit[k] - ref[k]) <= 1e-9 * abs(ref[k]), (k, fit[k], ref[k])
      assert fit[k] <= 0.0
      if (x[a:b, c] == x[a:b].max(axis=1)).all():                   # the label's logit is the row's largest on all its frames
        assert fit[k] == 0.0, (k, fit[k])


def check_wild_utterance(x, lab, spans, states, score, status, fit, bias, frames=None):
  """One utterance against the oracle, under the accuracy conditions of tests/test_gpu_align.py (align_oracle.accuracy_ratios,
  with the path's score taken over the wildcard's emissions too) -> the two ratios."""
  x = np.asarray(x)
  T = x.shape[0]
  ref = WO.align_wild64(x, lab, bias)
  if states is not None and frames is not None:
    assert (states[T:frames] == -2).all()
  if ref is None:
    assert status != 0 and score == -np.inf and (spans == -1).all() and np.isnan(fit).all()
    if states is not None:
      assert (states[:T] == -2).all()
    return 0.0, 0.0
  assert status == 0
  if states is None:
    states = np.full(T, -1, dtype=np.int64)
    for k, (a, b) in enumerate(spans):
      states[a:b] = k
  st = states[:T]
  assert AO.is_valid_alignment(st, lab)
  assert (spans == AO.spans_from_states(st, len(lab))).all()
  p = WO.path_score_wild64(x, st, lab, bias)
  s_star = ref[2]
  b1 = 2.0 * T * 2.0 ** -24 * abs(s_star)
  b2 = T * 2.0 ** -24 * abs(s_star) + 2.0 ** -23 * abs(s_star)
  ratio = lambda v, b: 0.0 if v <= 0.0 else (v / b if b > 0.0 else np.inf)
  r = ratio(s_star - p, b1), ratio(abs(float(score) - p), b2)
  assert r[0] <= 1.0 and r[1] <= 1.0, r
  check_fit(x, lab, spans, fit, bias)
  return r


def with_wildcards(lab, C, where):
  """``lab`` with wildcards put in: 'first', 'last', 'ends', 'fifth' (every fifth label replaced), 'none'."""
  W = WO.wild_id(C)
  lab = list(lab)
  if where == 'first':
    return [W] + lab
  if where == 'last':
    return lab + [W]
  if where == 'ends':
    return [W] + lab + [W]
  if where == 'fifth':
    return [W if k % 5 == 2 else l for k, l in enumerate(lab)]
  assert where == 'none'
  return lab
