"""st_ctc_loss_grad_wild_f32 called directly (no engine) on hand-built tensors, against the float64 specification
(tests/wild_ctc_oracle.py): every states-per-lane dispatch, 2 / 3 / 29 / 31 classes, wildcards on lane boundaries, at both ends,
alone, dead on a masked window (the case table: tests/wild_ctc_cases.py, checked on the CPU by tests/test_wild_ctc_cpu.py), with
poison wherever the kernels must not read and sentinels wherever they must not write, in both layouts of
tests/test_gpu_ctc_lattice.py.  Then the engine and one training step of the model.

Bounds: those of tests/ctc_cases.py, unchanged -- loss 1e-5 relative with its absolute floor, the (hi, lo) pair 2e-5, the
gradient GRAD_ATOL = 5e-5 of grad_scale.  The wildcard's share of the gradient, occ_t(wild) * 2^(logy[k] - logS), is a product
of two numbers <= 1, each with the float32 error the plain kernel's y = 2^logy and its occupancies already have, so the plain
bound is kept for it.  Measured on an MI355X over the whole table and both layouts (the figures test_against_the_spec prints): the
gradient is off by at most 3.1e-7 on the utterances with a wildcard (wk3-C2, the longest label) and 3.6e-7 on those without
(wk2), the (hi, lo) pair by at most 1.8e-6 (wk6, the longest label), the loss by at most 0.077 of its bound."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ctc_cases as CC
from tests import test_gpu_ctc_lattice as TL
from tests import wild_ctc_cases as WC
from tests import wild_ctc_oracle as WO

pytestmark = pytest.mark.gpu

SCALE = TL.SCALE
LAYOUTS = TL.LAYOUTS
W = WO.WILDCARD


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return 'cuda:0'


def device_ctc(dev, batch, rows, layout, entry='wild', bias=WC.BIAS, tail='big', max_label_len=None):
  """One call of st_ctc_loss_grad_wild_f32 (``entry='wild'``; the wildcard goes in as the id C) or of st_ctc_loss_grad_hilo_f32
  (``'hilo'``) on utterances ``rows`` of the batch -> dict(loss, lo, status, grad = the WHOLE gradient buffer, k, ret)."""
  from speecht_amd import _lib
  from speecht_amd._lib import Tensor3
  lib = _lib.load()
  utts = [batch.utterances[r] for r in rows]
  B, T, C = len(utts), batch.frames, batch.C
  (lh, lc), (gh, gc) = LAYOUTS[layout]
  max_len = max(len(u.label) for u in batch.utterances) if max_label_len is None else max_label_len
  to = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
  x = to(TL.poisoned_logits([u.logits for u in utts], T, C, lh, lc, tail))
  ids, offs = TL._csr([[C if l == W else l for l in u.label] for u in utts])
  d_ids, d_offs, d_lens = to(ids), to(offs), to(np.array([u.logits.shape[0] for u in utts], dtype=np.int32))
  grad = torch.full((B, TL._t_pitch(T, gh), gc), TL.GRAD_SENTINEL, dtype=torch.float32, device=dev)
  loss = torch.full((B,), TL.OUT_SENTINEL, dtype=torch.float32, device=dev)
  lo = torch.full((B,), TL.OUT_SENTINEL, dtype=torch.float32, device=dev)
  status = torch.full((B,), -7, dtype=torch.int32, device=dev)
  need = lib.st_ctc_ws(B, T, max_len)
  k = CC.states_per_lane_from_ws(need, B, T)
  ws = torch.full((need // 4 + 4,), float('nan'), dtype=torch.float32, device=dev)      # a record read before it is written shows
  P = lambda t: ctypes.c_void_p(t.data_ptr())
  x_desc = Tensor3(x.data_ptr(), B, T, C, lh, TL._t_pitch(T, lh), lc)
  g_desc = Tensor3(grad.data_ptr(), B, T, C, gh, TL._t_pitch(T, gh), gc)
  head = (ctypes.byref(x_desc), P(d_ids), P(d_offs), P(d_lens), max_len, SCALE)
  rest = (P(loss), P(lo), ctypes.byref(g_desc), P(status), P(ws), need, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
  if entry == 'wild':
    ret = lib.st_ctc_loss_grad_wild_f32(*head, float(bias), *rest)
  else:
    ret = lib.st_ctc_loss_grad_hilo_f32(*head, *rest)
  torch.cuda.synchronize()
  return dict(loss=loss.cpu().numpy(), lo=lo.cpu().numpy(), status=status.cpu().numpy(), grad=grad.cpu().numpy(), k=int(k), ret=int(ret))


def figures(batch, rows, refs, res, layout):
  """Layout assertions (exact), then per utterance (kind, loss error / its bound, |hi + lo - ref|, gradient error / grad_scale,
  the same on the label columns of frames where the wildcard holds occupancy)."""
  T, C = batch.frames, batch.C
  gh, gc = LAYOUTS[layout][1]
  cols = min(gc, 32)
  out = []
  for b, r in enumerate(rows):
    u, ref = batch.utterances[r], refs[r]
    Tb = u.logits.shape[0]
    hi, lo, g = res['loss'][b], res['lo'][b], res['grad'][b]
    # what the kernel must leave alone, and the zeros it owes: halo and slack rows, columns from 32 on; rows from Tb on, columns C .. 31
    assert (g[:gh] == TL.GRAD_SENTINEL).all() and (g[gh + T:] == TL.GRAD_SENTINEL).all() and (g[:, cols:] == TL.GRAD_SENTINEL).all()
    inner = g[gh:gh + T, :cols]
    assert (inner[Tb:] == 0).all() and (inner[:, C:] == 0).all(), u.kind
    if ref is None:
      assert res['status'][b] == 1 and hi == np.inf and lo == 0 and (inner == 0).all(), u.kind
      continue
    assert res['status'][b] == 0, u.kind
    ref_loss, ref_grad = ref
    pair = float(hi) + float(lo)
    assert np.float32(pair) == hi and np.isfinite(inner).all(), u.kind
    err = np.abs(inner[:Tb, :C] - SCALE * ref_grad) / SCALE
    out.append((u.kind, abs(float(hi) - ref_loss) / CC.loss_bound(ref_loss), abs(pair - ref_loss), float(err.max(initial=0.0)),
                float(err[:, :C - 1].max(initial=0.0))))
  return out


def test_every_dispatch_is_reached(dev):
  from speecht_amd import _lib
  lib = _lib.load()
  ks = {CC.states_per_lane_from_ws(lib.st_ctc_ws(len(b.utterances), b.frames, max(len(u.label) for u in b.utterances)),
                                   len(b.utterances), b.frames) for b in WC.all_batches()}
  assert sorted(ks) == list(CC.KPLS) and {b.C for b in WC.all_batches()} == {2, 3, 29, 31}


@pytest.mark.parametrize('layout', list(LAYOUTS))
@pytest.mark.parametrize('name', WC.BATCH_NAMES)
def test_against_the_spec(dev, name, layout):
  batch = WC.batch_by_name(name)
  refs = WC.oracle_results(name)
  rows = list(range(len(batch.utterances)))
  res = device_ctc(dev, batch, rows, layout)
  assert res['ret'] == 0 and res['k'] == batch.k                 # the dispatch this batch is for is the one that ran
  assert res['status'].tolist() == [0] * (len(rows) - 1) + [1]
  figs = figures(batch, rows, refs, res, layout)
  for f in figs:
    print('{} {} {:8s} loss error {:.3g} of its bound, |hi + lo - ref| {:.3g}, gradient {:.3g} (label columns {:.3g})'.format(
        name, layout, *f))
  for kind, loss_part, pair_err, grad_err, _ in figs:
    assert loss_part <= 1.0, (kind, loss_part)
    assert pair_err <= CC.PAIR_ATOL, (kind, pair_err)
    assert grad_err < CC.GRAD_ATOL, (kind, grad_err)
  # nothing from the utterance's length on is used: the same bits with zeros there; and the same bits run to run
  assert TL.same_bits(res, device_ctc(dev, batch, rows, layout, tail='zero'))
  assert TL.same_bits(res, device_ctc(dev, batch, rows, layout))
  # the longest label alone: its row of the batch, bit for bit
  one = device_ctc(dev, batch, [0], layout)
  assert one['k'] == batch.k and TL.same_bits(one, res, slice(0, 1), slice(0, 1))


@pytest.mark.parametrize('name', ['wk1', 'wk3', 'wk5', 'wk16', 'wk1-C2', 'wk3-C31'])
def test_another_bias(dev, name):
  """bias 0 and a steep one on the longest label and the masked utterance."""
  batch = WC.batch_by_name(name)
  kinds = [u.kind for u in batch.utterances]
  rows = [kinds.index('long'), kinds.index('masked'), kinds.index('w1')]
  for bias in (0.0, -6.5):
    refs = {r: WO.ctc_loss_and_grad(batch.utterances[r].logits, batch.utterances[r].label, bias) for r in rows}
    res = device_ctc(dev, batch, rows, 'haloed-grad', bias=bias)
    assert res['ret'] == 0
    for kind, loss_part, pair_err, grad_err, _ in figures(batch, rows, refs, res, 'haloed-grad'):
      assert loss_part <= 1.0 and pair_err <= CC.PAIR_ATOL and grad_err < CC.GRAD_ATOL, (bias, kind, loss_part, pair_err, grad_err)


@pytest.mark.parametrize('name', WC.BATCH_NAMES)
def test_without_a_wildcard_the_plain_bits(dev, name):
  """The utterances without a wildcard: from the wildcard entry point the bits of st_ctc_loss_grad_hilo_f32 -- alone, beside
  wildcard utterances, and run to run."""
  batch = WC.batch_by_name(name)
  layout = 'haloed-logits'
  plain = [r for r, u in enumerate(batch.utterances) if not u.wild]
  assert len(plain) == 2
  ref = device_ctc(dev, batch, plain, layout, entry='hilo')
  assert ref['ret'] == 0 and ref['status'].tolist() == [0, 0]
  alone = device_ctc(dev, batch, plain, layout)
  assert alone['ret'] == 0 and TL.same_bits(alone, ref)
  rows = list(range(len(batch.utterances)))
  for _ in range(2):
    beside = device_ctc(dev, batch, rows, layout)
    for b, r in enumerate(plain):
      assert TL.same_bits(beside, ref, slice(r, r + 1), slice(b, b + 1)), batch.utterances[r].kind
  # and whatever the bias
  other = device_ctc(dev, batch, rows, layout, bias=-0.25)
  for b, r in enumerate(plain):
    assert TL.same_bits(other, ref, slice(r, r + 1), slice(b, b + 1))


def test_argument_checks(dev):
  """32 classes leave the wildcard no slot, a positive or NaN bias is no price: an error return and nothing written."""
  from speecht_amd import _lib
  rng = np.random.default_rng(5)
  mk = lambda C: WC.Batch('args', 1, C, 12, [WC.Utterance('x', [0, 1, 0], rng.standard_normal((12, C)).astype(np.float32), True, False)])
  for batch, bias in ((mk(32), -1.0), (mk(29), 0.5), (mk(29), float('nan'))):
    res = device_ctc(dev, batch, [0], 'haloed-grad', bias=bias)
    assert res['ret'] != 0 and _lib.load().st_last_error()
    assert (res['grad'] == TL.GRAD_SENTINEL).all() and res['loss'][0] == TL.OUT_SENTINEL and res['lo'][0] == TL.OUT_SENTINEL
    assert res['status'][0] == -7
  assert device_ctc(dev, mk(31), [0], 'haloed-grad')['ret'] == 0
  assert device_ctc(dev, mk(32), [0], 'haloed-grad', entry='hilo')['ret'] == 0


# ---- the engine and the model ----------------------------------------------------------------------------------------------------

def _recorded_calls(monkeypatch):
  """Every entry point the engine calls from here on, by name."""
  from speecht_amd import engine
  names = []
  real = engine.call

  def recording(name, *args):
    names.append(name)
    return real(name, *args)
  monkeypatch.setattr(engine, 'call', recording)
  return names


def test_engine_loss_and_gradient(dev, monkeypatch):
  from speecht_amd import engine_decode as ED
  from speecht_amd.engine import Wav2LetterEngine
  from tests import workloads as WL
  layers = WL.w2l_layers(16, width=24, fc=40)
  eng = Wav2LetterEngine(layers, device=dev)
  eng.set_weights(WL.xavier_params(layers, seed=7))
  x, seq, labels = WL.make_batch([97, 80, 61], 16, seed=3)
  S = 27
  wild = [[ED.WILDCARD, S] + labels[0][:6] + [S, ED.WILDCARD, S] + labels[0][6:], labels[1], [ED.WILDCARD]]
  names = _recorded_calls(monkeypatch)
  eng.load_batch(x, seq)
  eng.forward()
  # a batch without a wildcard makes the old call, with and without the option
  for kw in (dict(), dict(wildcard=True)):
    del names[:]
    eng.set_labels(labels, **kw)
    eng.ctc_loss_grad(1.0 / 3)
    assert 'st_ctc_loss_grad_hilo_f32' in names and 'st_ctc_loss_grad_wild_f32' not in names
  plain_loss = eng.fetch_losses(precise=True).copy()
  # with one: the wildcard entry point, at the engine's bias, and the specification's numbers on the engine's own logits
  with pytest.raises(ValueError):
    eng.set_labels(wild)                                       # WILDCARD without the option is the error it always was
  for bad in ([[28], [0], [0]], [[0, ED.WILDCARD, ED.WILDCARD], [0], [0]], [[-2], [0], [0]]):
    with pytest.raises(ValueError):
      eng.set_labels(bad, wildcard=True)
  for bias in (None, -0.4):
    if bias is not None:
      eng.wildcard_bias = bias
    assert bias is not None or eng.wildcard_bias == ED.WILDCARD_BIAS == -1.0
    del names[:]
    eng.set_labels(wild, wildcard=True)
    eng.ctc_loss_grad(1.0 / 3)
    assert 'st_ctc_loss_grad_wild_f32' in names and 'st_ctc_loss_grad_hilo_f32' not in names
    loss = eng.fetch_losses(precise=True)
    logits = eng.shape.X[-1].interior().float().cpu().numpy()
    dz = eng.shape.dZ[-1].interior().float().cpu().numpy()
    lens = (np.asarray(seq) // 2).astype(int)                # what the reference feeds CTC (engine.load_batch)
    for b in range(3):
      ref_loss, ref_grad = WO.ctc_loss_and_grad(logits[b, :lens[b]], wild[b], eng.wildcard_bias)
      assert abs(loss[b] - ref_loss) <= CC.loss_bound(ref_loss), (b, loss[b], ref_loss)
      assert np.abs(dz[b, :lens[b]] * 3 - ref_grad).max() < CC.GRAD_ATOL and not dz[b, lens[b]:].any()
    assert loss[1] == plain_loss[1]                             # the utterance without a wildcard: the plain call's loss
  # deferred label errors (data parallelism): the refused utterance gets status 2 and an empty label, nothing raises here
  eng.defer_label_errors = True
  eng.set_labels([[0, ED.WILDCARD, ED.WILDCARD], wild[0], [ED.WILDCARD]], wildcard=True)
  assert eng._rejected_labels == [0] and eng._labels_wild
  eng.ctc_loss_grad(1.0 / 3)
  torch.cuda.synchronize()
  assert eng.shape.ctc_status.cpu().tolist() == [2, 0, 0]


def test_model_step_with_partial_transcripts(dev, tmp_path, monkeypatch):
  from speecht_amd.partial_labels import PartialTranscripts
  from speecht_amd.speech_model import Session, Wav2LetterModel
  from tests.test_gpu_api import make_loader
  loader, coord, _ = make_loader(16, 4, [121, 100, 90, 121], seed=5)
  model = Wav2LetterModel(loader, 16, 29)
  model.add_training_ops(learning_rate=1e-3, partial=PartialTranscripts(ends=True, bias=-0.5))
  model.add_decoding_ops()
  model.finalize(str(tmp_path), 'r', 'train')
  names = _recorded_calls(monkeypatch)
  with Session(dev) as sess:
    model.init_session(sess)
    res = model.step(sess, loss=True, update=True)
    assert np.isfinite(float(res[0])) and model.global_step.eval() == 1
    assert 'st_ctc_loss_grad_wild_f32' in names and model.engine.wildcard_bias == -0.5
    wild_loss = float(res[0])
    del names[:]
    plain = model.step(sess, loss=True, update=False)            # evaluation stays plain
    assert np.isfinite(float(plain[0])) and model.global_step.eval() == 1
    assert 'st_ctc_loss_grad_hilo_f32' in names and 'st_ctc_loss_grad_wild_f32' not in names
    assert wild_loss != float(plain[0])
  coord.request_stop()


def test_cli_train_with_the_wildcard_flags(dev, tmp_path):
  """`speecht-cli train --wildcard --wildcard-ends` on a small cached corpus: two steps, a checkpoint."""
  import os
  import subprocess
  import sys
  from tests.test_cli_data_parallel_cpu import make_corpus
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  make_corpus(str(tmp_path / 'data' / 'preprocessed-power' / 'train'), 8, 16, seed=2)
  args = [sys.executable, os.path.join(root, 'speecht-cli'), 'train', '--data-dir', str(tmp_path / 'data'), '--train-dir',
          str(tmp_path / 'train'), '--log-dir', str(tmp_path / 'log'), '--run-name', 'wild', '--batch-size', '4', '--seed', '11',
          '--steps-per-checkpoint', '2', '--max-steps', '2', '--learning-rate', '1e-3', '--wildcard', '--wildcard-ends',
          '--wildcard-drop', '0.3']
  r = subprocess.run(args, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
  assert r.returncode == 0, r.stdout + r.stderr
  assert "Partial transcripts: PartialTranscripts(token='*', ends=True, bias=-1, drop=0.3, seed=11)" in r.stdout
  assert 'global step 2 learning rate' in r.stdout and r.stdout.count('Model saved') == 1


def test_blank_far_ahead_of_the_labels(dev):
  """Frames on which the blank leads every label class by 720 - 800 nats: exp(label - blank) underflows in double, but the label
  classes are live under the kernels' 2^-30000 rule, and so is the wildcard -- its sum is taken relative to the label classes'
  own maximum.  Loss and (hi, lo) pair within the usual bounds.  The gradient's bound is worked out for these frames: log2 y(k)
  and log2 S + bias are fp32 values of magnitude 1 024 .. 2 048 there (ulp 2^-13), so 2^(logy[k] - (logy[C] - bias)) carries three
  roundings of half an ulp in its exponent, 3 * 2^-14 * ln 2 = 1.27e-4 relative on a share <= 1, on top of GRAD_ATOL.  Measured on an MI355X: 6.0e-5 on the utterance
  whose every frame is such a frame, below 1e-7 on the two others."""
  rng = np.random.default_rng(77)
  C = 29
  bound = CC.GRAD_ATOL + 3 * 2.0 ** -14 * np.log(2.0)

  def logits(frames, far):
    x = (rng.standard_normal((frames, C)) * 2).astype(np.float32)
    for t, gap in far.items():
      x[t, C - 1] = np.float32(x[t, :C - 1].max() + gap)
    return x
  utts = [WC.Utterance('all', [W], logits(3, {0: 760.0, 1: 800.0, 2: 720.0}), True, True),
          WC.Utterance('some', [0, W, 1], logits(9, {3: 800.0, 4: 760.0, 5: 735.0}), True, True),
          WC.Utterance('plain', [0, 1], logits(9, {3: 800.0}), True, False)]
  batch = WC.Batch('far', 1, C, 12, utts)
  rows = [0, 1, 2]
  refs = {r: WO.ctc_loss_and_grad(u.logits, u.label, WC.BIAS) for r, u in enumerate(utts)}
  assert all(np.isfinite(refs[r][0]) for r in rows) and refs[0][0] > 700
  for layout in LAYOUTS:
    res = device_ctc(dev, batch, rows, layout)
    assert res['ret'] == 0 and res['status'].tolist() == [0, 0, 0]
    for kind, loss_part, pair_err, grad_err, _ in figures(batch, rows, refs, res, layout):
      print('far {} {:6s} loss error {:.3g} of its bound, |hi + lo - ref| {:.3g}, gradient {:.3g} (bound {:.3g})'.format(
          layout, kind, loss_part, pair_err, grad_err, bound))
      assert loss_part <= 1.0 and pair_err <= CC.PAIR_ATOL, (kind, loss_part, pair_err)
      assert grad_err < (CC.GRAD_ATOL if kind == 'plain' else bound), (kind, grad_err)
