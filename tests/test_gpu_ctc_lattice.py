"""st_ctc_loss_grad_hilo_f32 and st_ctc_greedy_decode called directly (no engine) on hand-built tensors, against the float64
oracle: every states-per-lane dispatch of the lattice kernels, 2 / 3 / 29 / 32 classes, repeats placed on lane boundaries,
exact-fit, chunk-edge and zero-frame lengths, peaked and masked rows (the case table: tests/ctc_cases.py, checked on the CPU by
tests/test_ctc_cases_cpu.py), with poison wherever the kernels must not read and sentinels wherever they must not write.

Bounds (tests/ctc_cases.py): loss 1e-5 relative -- with an absolute floor of 3.42e-6 below a loss of 0.342, 4 x the 8.55e-7
of the float32 model of the recursion there; that model is 2.95e-5 RELATIVE off on the 0.0145 loss of k1-C2's utterance d, so
1e-5 relative alone is out of a float32 lattice's reach on such losses -- the (hi, lo) pair 2e-5 absolute, the gradient 5e-5
of grad_scale."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import w2l_oracle as O
from tests import ctc_cases as CC

pytestmark = pytest.mark.gpu

GRAD_SENTINEL = -777.25
OUT_SENTINEL = -123.0
SCALE = 0.5
# (halo, c_pitch) of the logits and of the gradient tensor: different on purpose, and swapped
LAYOUTS = {'haloed-logits': ((2, 40), (0, 32)), 'haloed-grad': ((0, 32), (2, 40))}


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def _t_pitch(T, halo):
  return T + 2 * halo + 3


def poisoned_logits(rows, T, C, halo, c_pitch, tail):
  """[B, t_pitch, c_pitch]: NaN in the pitch columns, the halo rows and the slack rows; inside the frames, rows from the
  utterance's length on hold +-1e30 (tail='big') or 0."""
  x = np.full((len(rows), _t_pitch(T, halo), c_pitch), np.nan, dtype=np.float32)
  t, c = np.meshgrid(np.arange(T), np.arange(C), indexing='ij')
  big = np.where((t + c) % 2 == 0, np.float32(1e30), np.float32(-1e30))
  for b, u in enumerate(rows):
    Tb = u.shape[0]
    x[b, halo:halo + T, :C] = big if tail == 'big' else 0.0
    x[b, halo:halo + Tb, :C] = u
  return x


def _csr(labels):
  offs = np.zeros(len(labels) + 1, dtype=np.int32)
  offs[1:] = np.cumsum([len(l) for l in labels])
  return np.array([i for l in labels for i in l] + [0], dtype=np.int32), offs


def device_ctc(dev, batch, rows, layout, tail='big', max_label_len=None, label_offsets=None):
  """One st_ctc_loss_grad_hilo_f32 call on utterances ``rows`` of the batch -> dict(loss, lo, status, grad = the WHOLE gradient
  buffer [B, t_pitch, c_pitch], k = states per lane that ran, from the workspace size).  ``label_offsets`` replaces the offsets
  of the rows' concatenated labels."""
  from speecht_amd import _lib
  from speecht_amd._lib import Tensor3
  lib = _lib.load()
  utts = [batch.utterances[r] for r in rows]
  B, T, C = len(utts), batch.frames, batch.C
  (lh, lc), (gh, gc) = LAYOUTS[layout]
  max_len = max(len(u.label) for u in batch.utterances) if max_label_len is None else max_label_len
  to = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
  x = to(poisoned_logits([u.logits for u in utts], T, C, lh, lc, tail))
  ids, offs = _csr([u.label for u in utts])
  if label_offsets is not None:
    offs = np.asarray(label_offsets, dtype=np.int32)
  d_ids, d_offs, d_lens = to(ids), to(offs), to(np.array([u.logits.shape[0] for u in utts], dtype=np.int32))
  grad = torch.full((B, _t_pitch(T, gh), gc), GRAD_SENTINEL, dtype=torch.float32, device=dev)
  loss = torch.full((B,), OUT_SENTINEL, dtype=torch.float32, device=dev)
  lo = torch.full((B,), OUT_SENTINEL, dtype=torch.float32, device=dev)
  status = torch.full((B,), -7, dtype=torch.int32, device=dev)
  need = lib.st_ctc_ws(B, T, max_len)
  k = CC.states_per_lane_from_ws(need, B, T)
  ws = torch.full((need // 4 + 4,), float('nan'), dtype=torch.float32, device=dev)      # a record read before it is written shows
  P = lambda t: ctypes.c_void_p(t.data_ptr())
  x_desc = Tensor3(x.data_ptr(), B, T, C, lh, _t_pitch(T, lh), lc)
  g_desc = Tensor3(grad.data_ptr(), B, T, C, gh, _t_pitch(T, gh), gc)
  _lib.call('st_ctc_loss_grad_hilo_f32', ctypes.byref(x_desc), P(d_ids), P(d_offs), P(d_lens), max_len, SCALE, P(loss), P(lo),
            ctypes.byref(g_desc), P(status), P(ws), need, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
  torch.cuda.synchronize()
  return dict(loss=loss.cpu().numpy(), lo=lo.cpu().numpy(), status=status.cpu().numpy(), grad=grad.cpu().numpy(), k=int(k))


def same_bits(a, b, row_a=slice(None), row_b=slice(None)):
  return all(np.array_equal(np.ascontiguousarray(a[key][row_a]).view(np.int32), np.ascontiguousarray(b[key][row_b]).view(np.int32))
             for key in ('loss', 'lo', 'status', 'grad'))


def check_against_oracle(batch, rows, refs, res, layout):
  """Every assertion on one call's outputs -> worst (loss error / its bound, |hi + lo - ref|, gradient error / grad_scale,
  relative loss error where the bound is the relative one)."""
  T, C = batch.frames, batch.C
  gh, gc = LAYOUTS[layout][1]
  cols = min(gc, 32)
  worst = [0.0, 0.0, 0.0, 0.0]
  for b, r in enumerate(rows):
    u, ref = batch.utterances[r], refs[r]
    Tb = u.logits.shape[0]
    hi, lo, g = res['loss'][b], res['lo'][b], res['grad'][b]
    # what the kernel must leave alone, and the zeros it owes: halo and slack rows, columns from 32 on; rows from Tb on, columns C .. 31
    assert (g[:gh] == GRAD_SENTINEL).all() and (g[gh + T:] == GRAD_SENTINEL).all() and (g[:, cols:] == GRAD_SENTINEL).all()
    inner = g[gh:gh + T, :cols]
    assert (inner[Tb:] == 0).all() and (inner[:, C:] == 0).all()
    if ref is None:
      assert res['status'][b] == 1 and hi == np.inf and lo == 0 and (inner == 0).all()
      continue
    assert res['status'][b] == 0
    ref_loss, ref_grad = ref
    if Tb == 0:
      assert hi == 0 and lo == 0
    pair = float(hi) + float(lo)
    assert abs(float(hi) - ref_loss) <= CC.loss_bound(ref_loss), (u.kind, hi, ref_loss)
    assert abs(pair - ref_loss) <= CC.PAIR_ATOL, (u.kind, pair, ref_loss)
    assert np.float32(pair) == hi                                         # hi is the rounded double, lo the remainder
    assert np.isfinite(inner).all()
    err = float(np.max(np.abs(inner[:Tb, :C] - SCALE * ref_grad), initial=0.0)) / SCALE
    assert err < CC.GRAD_ATOL, (u.kind, err)
    d = abs(float(hi) - ref_loss)
    relative = d / ref_loss if ref_loss > CC.LOSS_FLOOR / CC.LOSS_RTOL else 0.0
    worst = [max(w, v) for w, v in zip(worst, (d / CC.loss_bound(ref_loss), abs(pair - ref_loss), err, relative))]
  return worst


@pytest.mark.parametrize('layout', list(LAYOUTS))
@pytest.mark.parametrize('name', CC.BATCH_NAMES)
def test_lattice_dispatch(dev, name, layout):
  batch = CC.batch_by_name(name)
  refs = CC.oracle_results(name)
  rows = list(range(len(batch.utterances)))
  res = device_ctc(dev, batch, rows, layout)
  assert res['k'] == batch.k                                   # the dispatch this batch is for is the one that ran
  assert res['status'].tolist() == [0] * (len(rows) - 1) + [1]
  worst = check_against_oracle(batch, rows, refs, res, layout)
  # nothing from the utterance's length on is used: the same bits with zeros there; and the same bits run to run
  assert same_bits(res, device_ctc(dev, batch, rows, layout, tail='zero'))
  assert same_bits(res, device_ctc(dev, batch, rows, layout))
  # each utterance alone, under the same dispatch: its row of the batch, bit for bit
  for r in rows[:-1]:
    one = device_ctc(dev, batch, [r], layout)
    assert one['k'] == batch.k and same_bits(one, res, slice(0, 1), slice(r, r + 1)), batch.utterances[r].kind
  # the longest label under the next dispatch: other arithmetic order, same bounds
  i = CC.KPLS.index(batch.k)
  if i + 1 < len(CC.KPLS):
    wider = device_ctc(dev, batch, [0], layout, max_label_len=CC.largest_label(CC.KPLS[i + 1]))
    assert wider['k'] == CC.KPLS[i + 1] and wider['status'].tolist() == [0]
    w2 = check_against_oracle(batch, [0], refs, wider, layout)
    worst = [max(a, b) for a, b in zip(worst, w2)]
  print('{} (k = {}, C = {}, {} frames), {}: worst loss error {:.3g} of its bound, |hi + lo - ref| {:.3g}, gradient {:.3g}, '
        'loss {:.3g} relative'.format(name, batch.k, batch.C, batch.frames, layout, *worst))


@pytest.mark.parametrize('name', ['k1', 'k5'])
def test_negative_label_length_is_refused(dev, name):
  """label_offsets that do not increase give an utterance a negative label length: status 1, loss +inf, a zero gradient, and
  the utterance beside it keeps its bits."""
  batch = CC.batch_by_name(name)
  layout = 'haloed-grad'
  L = len(batch.utterances[0].label)
  kinds = [u.kind for u in batch.utterances]
  rows = [kinds.index('e'), 0]                                  # the empty label, then the longest: the ids are the longest's
  res = device_ctc(dev, batch, rows, layout, label_offsets=[L, 0, L])     # lengths -L and L
  gh, gc = LAYOUTS[layout][1]
  assert res['status'].tolist() == [1, 0]
  assert res['loss'][0] == np.inf and res['lo'][0] == 0
  assert (res['grad'][0][gh:gh + batch.frames, :32] == 0).all()
  assert (res['grad'][0][:gh] == GRAD_SENTINEL).all() and (res['grad'][0][:, 32:] == GRAD_SENTINEL).all()
  alone = device_ctc(dev, batch, [0], layout)
  assert alone['status'].tolist() == [0] and same_bits(res, alone, slice(1, 2), slice(0, 1))


def test_all_ten_dispatches_and_four_class_counts(dev):
  from speecht_amd import _lib
  lib = _lib.load()
  ks = set()
  for batch in CC.all_batches():
    B, T = len(batch.utterances), batch.frames
    ks.add(CC.states_per_lane_from_ws(lib.st_ctc_ws(B, T, max(len(u.label) for u in batch.utterances)), B, T))
  assert sorted(ks) == [1, 2, 3, 4, 5, 6, 8, 10, 12, 16]
  assert {b.C for b in CC.all_batches()} == {2, 3, 29, 32}


# ---- greedy decode ----------------------------------------------------------------------------------------------------------

GREEDY_LENS = [0, 1, 255, 256, 257, 513, 512]
RUN = (250, 261)             # a run of one label over the 256-thread scan's segment boundaries (3 frames per thread at 513 frames)


def greedy_rows(C):
  rng = np.random.default_rng(500 + C)
  rows = [rng.standard_normal((t, C)).astype(np.float32) * 2 for t in GREEDY_LENS]
  rows[2] = np.round(rows[2])                              # exact ties: the lowest index wins
  rows[3][:] = 0.25                                        # all equal: class 0 on every frame
  dead = rng.random(rows[4].shape) < 0.3
  dead[np.arange(rows[4].shape[0]), rng.integers(0, C, rows[4].shape[0])] = False      # (one live class per frame at least)
  rows[4][dead] = -np.inf
  rows[5][:, C - 1] += 1.0
  rows[5][RUN[0]:RUN[1], 0 if C == 2 else 5] += 30.0
  return rows


def device_greedy(dev, rows, C, layout, merge, max_out):
  from speecht_amd import _lib
  from speecht_amd._lib import Tensor3
  halo, c_pitch = layout
  B, T = len(rows), max(GREEDY_LENS)
  to = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
  x = to(poisoned_logits(rows, T, C, halo, c_pitch, 'big'))
  d_lens = to(np.array([r.shape[0] for r in rows], dtype=np.int32))
  ids = torch.full((B * max_out + 64,), -9, dtype=torch.int32, device=dev)
  out_lens = torch.full((B,), -9, dtype=torch.int32, device=dev)
  score = torch.full((B,), OUT_SENTINEL, dtype=torch.float32, device=dev)
  P = lambda t: ctypes.c_void_p(t.data_ptr())
  desc = Tensor3(x.data_ptr(), B, T, C, halo, _t_pitch(T, halo), c_pitch)
  _lib.call('st_ctc_greedy_decode', ctypes.byref(desc), P(d_lens), int(merge), P(ids), max_out, P(out_lens), P(score),
            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
  torch.cuda.synchronize()
  ids = ids.cpu().numpy()
  assert (ids[B * max_out:] == -9).all()                  # nothing past the buffer
  return ids[:B * max_out].reshape(B, max_out), out_lens.cpu().numpy(), score.cpu().numpy()


@pytest.mark.parametrize('C', [2, 29, 32])
def test_greedy_decode_edges(dev, C):
  rows = greedy_rows(C)
  T = max(GREEDY_LENS)
  dense = np.zeros((T, len(rows), C))
  for b, r in enumerate(rows):
    dense[:r.shape[0], b] = r
  for merge in (True, False):
    ref_ids, ref_score = O.ctc_greedy_decode(dense, GREEDY_LENS, merge)
    assert (np.argmax(rows[5][RUN[0]:RUN[1]], axis=1) == (0 if C == 2 else 5)).all()       # the run is there
    assert ref_ids[3] == ([0] if merge else [0] * 256) and ref_ids[0] == []
    longest = max(len(r) for r in ref_ids)
    for layout in ((2, 40), (0, 32)):
      ids, out_lens, score = device_greedy(dev, rows, C, layout, merge, T)
      assert out_lens.tolist() == [len(r) for r in ref_ids]
      for b, r in enumerate(ref_ids):
        assert ids[b, :len(r)].tolist() == r and (ids[b, len(r):] == -9).all(), (C, merge, b)
      np.testing.assert_allclose(score, ref_score[:, 0], rtol=1e-5)
      # max_out smaller than the output: the full count, the first max_out ids, nothing else touched
      small = 7
      assert small < longest
      ids, out_lens, score2 = device_greedy(dev, rows, C, layout, merge, small)
      assert out_lens.tolist() == [len(r) for r in ref_ids] and np.array_equal(score2.view(np.int32), score.view(np.int32))
      for b, r in enumerate(ref_ids):
        n = min(len(r), small)
        assert ids[b, :n].tolist() == r[:n] and (ids[b, n:] == -9).all(), (C, merge, b)
