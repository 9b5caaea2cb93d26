"""Gradient parity checks of one training step, shared by the full-size GPU tests (a helper module, not a conftest).

``run_step`` runs one forward + CTC + backward of a ``case`` (dict of layers, params, x, seq, labels) under the launch
trace; ``compare`` checks an fp32 step against float64 three ways (tests/torch_ref.py); ``stored_operand_checks``
checks a bf16 step kernel by kernel on the device's own stored operands (oracle/w2l_oracle.py)."""
import time

import numpy as np
import torch

from oracle import w2l_oracle as O
from tests import torch_ref as TR

ULP = 2.0 ** -8                       # one bf16 ulp of a tensor's scale


def make_case(layers, params, x, seq, labels, scale=None):
  """``scale``: d loss / d per-utterance loss handed to ctc_loss_grad (default 1 / B, the batch mean)."""
  return dict(layers=layers, params=params, x=x, seq=seq, labels=labels,
              scale=(1.0 / len(seq)) if scale is None else scale)


def run_step(case, mode, fft_conv=False):
  """One forward + CTC + backward on cuda:0 -> (engine, launch trace lines)."""
  from speecht_amd._lib import launch_trace
  from speecht_amd.engine import Wav2LetterEngine
  eng = Wav2LetterEngine(case['layers'], device='cuda:0', conv_mode=mode, fft_conv=fft_conv)
  eng.set_weights(case['params'])
  eng.load_batch(case['x'], case['seq'])
  eng.set_labels(case['labels'])
  with launch_trace() as tr:
    eng.forward()
    eng.ctc_loss_grad(case.get('scale', 1.0 / len(case['seq'])))
    eng.backward()
  torch.cuda.synchronize()
  eng.check_ctc_status()
  return eng, tr.lines


def rel_err(g, r):
  return float(np.max(np.abs(g - r)) / np.max(np.abs(r)))


def scaled_err(a, b):
  """(max, mean) of |a - b| in units of max |b|."""
  s = float(np.max(np.abs(b))) + 1e-30
  d = np.abs(np.asarray(a, np.float64) - b) / s
  return float(d.max()), float(d.mean())


def plane(t3, buf):
  """[B,T,C] float64 copy of the valid region of a bf16 (or fp32) buffer laid out like the padded NWC tensor t3."""
  v = buf.view(t3.batch, t3.t_pitch, t3.c_pitch)[:, t3.halo:t3.halo + t3.frames, :t3.channels]
  return v.float().cpu().numpy().astype(np.float64)


def free_checked_layers(flips):
  """flips[j] = ReLU sign flips (device vs float64) at the output of layer j, j = 0 .. L-2.  Layer i's gradient goes through
  the ReLU masks at the outputs of layers i .. L-2 only: the layers for which all of those agree."""
  return [i for i in range(len(flips) + 1) if sum(flips[i:]) == 0]


def compare(eng, ref, case, grad_tol=2e-4):
  """Three comparisons, from the most independent to the most exact:

  1. logits, per-utterance losses and d avg_loss / d logits against the float64 autograd reference;
  2. the BACKWARD KERNELS at full size: all 22 gradient tensors against float64 back-prop evaluated on the
     device's own stored activations and its own dlogits (tests/torch_ref.backward_from_acts) -- the exact linear
     map the kernels must reproduce, tolerance 2e-4 of each tensor's max;
  3. END TO END, all 22 tensors at the same 2e-4: against a second float64 evaluation of the whole step (its own
     forward activations from the inputs, its own CTC, autograd) whose ReLU pattern is pinned to the one the device
     took (tests/torch_ref.loss_and_grads(relu_masks=...)).  The step has one discontinuity -- a ReLU input within
     fp32 rounding of zero lands on the other side in float64 (1-10 of 4-32 million elements per layer; the flipped
     unit's whole gradient appears or vanishes and the ill-conditioned lower layers amplify it) -- and pinning the
     pattern removes exactly that and nothing else: the pinned pre-activations differ from the free ones by < 1e-6
     at the flipped elements (asserted through the logits), every other number is independent of the device.
     Every layer whose gradient goes through no flipped unit (no flip at the outputs of layers i .. L-2) is also held
     to the same 2e-4 against the free float64 evaluation, where nothing is pinned; the free figures of the other
     layers are printed for the record."""
  logits = eng.logits_time_major().cpu().numpy()
  B = len(case['seq'])
  assert logits.shape == ref['logits'].shape == (-(-int(np.max(case['seq'])) // 2), B, case['layers'][-1][3])
  # frames beyond an utterance's own length are computed too (nothing is masked): compare all
  err = float(np.max(np.abs(logits - ref['logits'])))
  assert err < 1e-4, err
  np.testing.assert_allclose(eng.loss.cpu().numpy(), ref['loss'], rtol=1e-4)
  dl = eng.dZ[-1].interior().cpu().numpy().astype(np.float64)
  dl_err = rel_err(dl, ref['dlogits'])
  assert dl_err < 2e-4, dl_err
  acts = [eng.X[i].interior().cpu().numpy() for i in range(len(eng.layers) + 1)]
  flips = [int(np.sum((acts[i] > 0) != (ref['acts'][i] > 0))) for i in range(1, len(eng.layers))]   # ReLU outputs
  free_checked = free_checked_layers(flips)
  got = eng.get_grads()
  exact, _ = TR.backward_from_acts(acts, case['params'], case['layers'], dl)
  t0 = time.time()
  pinned = TR.loss_and_grads(case['x'], case['seq'], case['labels'], case['params'], case['layers'], dtype=torch.float64,
                             relu_masks=TR.relu_masks_of(acts, case['layers']))
  pin_secs = time.time() - t0
  # the pinned evaluation is the same function as the free one except at the flipped units, whose pre-activations are
  # within rounding of zero: logits and losses agree far below the parity tolerance
  pin_shift = float(np.max(np.abs(pinned['logits'] - ref['logits'])))
  assert pin_shift < 1e-5, pin_shift
  assert float(np.max(np.abs(logits - pinned['logits']))) < 1e-4
  np.testing.assert_allclose(eng.loss.cpu().numpy(), pinned['loss'], rtol=1e-4)
  kernel_report, e2e_report, free_report, failed = [], [], [], []
  for i, ((gF, gb), (xF, xb), (pF, pb), (rF, rb)) in enumerate(zip(got, exact, pinned['grads'], ref['grads'])):
    for name, g, x, p, r in (('filters', gF, xF, pF, rF), ('bias', gb, xb, pb, rb)):
      assert g.shape == x.shape == p.shape == r.shape
      k, e, f = rel_err(g, x), rel_err(g, p), rel_err(g, r)
      kernel_report.append('L%d %s %.1e' % (i, name, k))
      e2e_report.append('L%d %s %.1e' % (i, name, e))
      free_report.append('L%d %s %.1e%s' % (i, name, f, '' if i in free_checked else ' (flips above)'))
      if not k < grad_tol:
        failed.append('kernel L%d %s %.2e' % (i, name, k))
      if not e < grad_tol:
        failed.append('end-to-end (ReLU pattern pinned) L%d %s %.2e' % (i, name, e))
      if i in free_checked and not f < grad_tol:
        failed.append('end-to-end (free, no flipped unit above) L%d %s %.2e' % (i, name, f))
  print('dlogits error %.2e of max; ReLU sign flips vs float64 per layer output: %s' % (dl_err, flips))
  print('backward kernels vs float64 back-prop on the device activations: ' + '; '.join(kernel_report))
  print('end to end vs float64 autograd with the device\'s ReLU pattern (%.1f s, logits moved %.1e by the pinning): '
        % (pin_secs, pin_shift) + '; '.join(e2e_report))
  print('end to end vs the free float64 autograd (asserted for layers %s, no flipped unit above them): ' % free_checked
        + '; '.join(free_report))
  assert not failed, failed
  return err, dl_err


def stored_operand_checks(eng, params, layers, grads, labels, seq, scale, spectral):
  """A bf16 step kernel by kernel on the device's OWN stored operands, where nothing is amplified: every layer's stored output
  against round_bf16(conv(stored input)), every stored activation gradient against round_bf16(mask * back-prop of the stored
  gradient above), every filter / bias gradient against the float64 product of the stored operands; the spectral layers also
  against the direct form.  Here a mismatch can only be a value on a rounding boundary: max <= 1 bf16 ulp of the tensor scale
  (2 in the top binade), mean <= 0.01.  ``params`` float64, ``grads`` the device's, ``scale`` as handed to ctc_loss_grad,
  ``spectral`` the layers run in the frequency domain (eng.fftb).

  (a stored value is the fp32 accumulation rounded to bf16, the expectation the float64 one: where the exact value sits within
  ~1e-7 of a rounding boundary the two may land on neighbouring bf16 values -- one spacing, which in the top binade of the
  tensor is up to 2 ULP of the tensor's maximum; the mean bound says it is a handful of elements)"""
  L = len(layers)
  t0 = time.time()
  Xs = [plane(eng.X[i], eng.Xb[i]) for i in range(L)]                 # stored bf16 inputs of every layer
  dZs = [plane(eng.dZ[i], eng.dZb[i]) for i in range(L)]              # stored bf16 gradients wrt every layer's output
  for i, ((F, b), (W, s, cin, cout, relu)) in enumerate(zip(params, layers)):
    if i in spectral:
      # the frequency-domain layer against ITS storage model on the stored operands: spectra of the stored input, of the stored
      # gradient and of the fp32 master filters rounded to bf16, everything else exact (an element of a spectrum within fp32
      # rounding of a bf16 boundary may land on the other side than in float64: slightly looser means than the W-tap layers')
      y, dx, dF, db = O.block_dft_conv(Xs[i], F, b, relu, dz=dZs[i], store=O.bf16_round)
    else:
      y = O.conv1d_same_fwd(Xs[i], O.bf16_round(F), b, s, relu)
      dx, dF, db = O.conv1d_same_bwd(Xs[i], O.bf16_round(F), None, dZs[i], s, relu=False, need_dx=(i > 0))
    mean_tol = 0.05 if i in spectral else 0.01
    if i in spectral:
      # ... and against the DIRECT form on the same stored operands (the storage model above must not define the
      # accuracy loss of bf16 spectra away).  What bf16 spectra cost relative to the W-tap bf16 kernel, which rounds only its
      # output: the oracle's two forms differ by max 1.5 / mean 0.06 ulp (forward), 1.5 / 0.12 ulp (back-prop) and 2.5e-3 of
      # the maximum (filter gradient, 0.6 ulp) on random data of this layer's shape class; the bounds leave a factor ~3.
      yd = O.conv1d_same_fwd(Xs[i], O.bf16_round(F), b, s, relu)
      dxd, dFd, dbd = O.conv1d_same_bwd(Xs[i], O.bf16_round(F), None, dZs[i], s, relu=False, need_dx=True)
      mx, mean = scaled_err(Xs[i + 1], O.bf16_round(yd))
      print('spectral L%d vs DIRECT form: forward max %.2f ulp mean %.3f ulp' % (i, mx / ULP, mean / ULP))
      assert mx <= 4 * ULP and mean < 0.25 * ULP, ('forward vs direct form', i, mx / ULP, mean / ULP)
      dxm = dxd * (Xs[i] > 0) if layers[i - 1][4] else dxd
      mx, mean = scaled_err(dZs[i - 1], O.bf16_round(dxm))
      print('spectral L%d vs DIRECT form: back-prop max %.2f ulp mean %.3f ulp' % (i, mx / ULP, mean / ULP))
      assert mx <= 4 * ULP and mean < 0.4 * ULP, ('back-prop vs direct form', i, mx / ULP, mean / ULP)
      mxF, _ = scaled_err(grads[i][0], dFd)
      mxb, _ = scaled_err(grads[i][1], dbd)
      print('spectral L%d vs DIRECT form: filter gradient %.1e, bias gradient %.1e of max' % (i, mxF, mxb))
      assert mxF < 8e-3 and mxb < 2e-4, ('filter/bias gradient vs direct form', i, mxF, mxb)
      del yd, dxd, dFd, dxm
    if i + 1 < L:
      mx, mean = scaled_err(Xs[i + 1], O.bf16_round(y))
      assert mx <= 2.01 * ULP and mean < mean_tol * ULP, ('forward', i, mx / ULP, mean / ULP)
    else:
      mx, _ = scaled_err(plane(eng.X[L], eng.X[L].buf), y)            # logits stay fp32
      assert mx < 1e-5, ('logits from stored X10', mx)
    # filter / bias gradient of layer i from its stored operands
    mxF, _ = scaled_err(grads[i][0], dF)
    mxb, _ = scaled_err(grads[i][1], db)
    assert mxF < (1e-3 if i in spectral else 2e-4) and mxb < 2e-4, ('filter/bias gradient', i, mxF, mxb)
    # gradient handed to the layer below: mask of the stored activation, rounded to bf16 when written
    if i > 0:
      if layers[i - 1][4]:
        dx = dx * (Xs[i] > 0)
      mx, mean = scaled_err(dZs[i - 1], O.bf16_round(dx))
      assert mx <= 2.01 * ULP and mean < mean_tol * ULP, ('back-prop to the input', i, mx / ULP, mean / ULP)
    print('kernel-level L%d ok (filters %.1e, bias %.1e of max)' % (i, mxF, mxb))
  # the bf16 copy of d loss / d logits and the fp32 CTC gradient it was rounded from
  mx, _ = scaled_err(dZs[L - 1], O.bf16_round(plane(eng.dZ[L - 1], eng.dZ[L - 1].buf)))
  assert mx == 0.0
  got = eng.logits_time_major().cpu().numpy()
  dl_ref = np.transpose(O.ctc_loss_and_grad(got.astype(np.float64), labels, seq // 2)[1], (1, 0, 2)) * scale
  mx, _ = scaled_err(plane(eng.dZ[L - 1], eng.dZ[L - 1].buf), dl_ref)
  assert mx < 2e-4, mx
  print('kernel-by-kernel checks on the stored operands: %.1f s' % (time.time() - t0))
