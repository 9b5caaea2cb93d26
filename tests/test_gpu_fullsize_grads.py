"""Gradient parity AT BASELINE's headline size (configs[1]: B=32 x 10 s x 80-mel, 250/2000 channels).

The kernels the benchmark runs -- gemm_nn<128,128,2,2,fast> forward and back-prop (incl. the 2-way split-K of
L8's back-prop), gemm_tn<128> with row slabs at M = 16 032 -- are only selected at near-full batch, so this module
runs one full-size step and compares EVERY gradient tensor, the per-utterance losses and the logits with an
independent CPU evaluation of the same step in float64 (tests/torch_ref.py: F.conv1d + F.ctc_loss + autograd,
which agrees with the numpy oracle to 1e-13, tests/test_oracle_conv_ctc.py::test_torch_ref_equals_oracle).
The launch trace of the library is asserted so that the test cannot silently take the small-problem kernels.

Tolerances: logits <= 1e-4 absolute, loss <= 1e-4 relative, d loss / d logits and every
gradient tensor <= 2e-4 of its own max -- kernel by kernel on the device's operands AND end to end against an
independent float64 evaluation with the ReLU pattern pinned to the device's (``compare``, tests/grad_parity.py)."""
import time

import numpy as np
import pytest

from tests import grad_parity as GP
from tests import torch_ref as TR
from tests import workloads as WL

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

FRAMES = [1001] * 30 + [777, 500]                          # ragged tail like a real batch


@pytest.fixture(scope='module')
def case():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  layers = WL.w2l_layers(80)
  params = WL.xavier_params(layers, seed=42, dtype=np.float32)      # non-zero biases
  x, seq, labels = WL.make_batch(FRAMES, 80, seed=3)
  x32 = x.astype(np.float32)
  t0 = time.time()
  ref = TR.loss_and_grads(x32, seq, labels, params, layers, dtype=torch.float64)
  print('float64 CPU reference of the full-size step: %.1f s' % (time.time() - t0))
  return dict(GP.make_case(layers, params, x32, seq, labels), ref=ref)


run_step, compare = GP.run_step, GP.compare


def test_fullsize_fp32_gradients_match_float64_reference(case):
  eng, trace = run_step(case, 'fp32')
  text = '\n'.join(trace)
  # the benchmark's kernels, not the small-problem ones
  fwd_fast = [l for l in trace if l.startswith('gemm_nn<128,128,2,2,fast> epi=0')]
  bwd_fast = [l for l in trace if l.startswith(('gemm_nn<128,128,2,2,fast> epi=1', 'gemm_nn<128,128,2,2,fast-bt> epi=1'))]
  assert len(fwd_fast) == 9, text                                  # L1..L9 forward
  assert len(bwd_fast) == 10, text                                 # back-prop to the input of L10..L1
  assert sum('fast-bt' in l for l in bwd_fast) == 2, text          # the two 1-tap layers read their packed filters transposed
  assert any('splits=2' in l and 'Kp=64512' in l for l in bwd_fast), text        # L8 back-prop: 2 K-halves
  slabbed = [l for l in trace if l.startswith('gemm_tn<') and 'slabs=1 ' not in l]
  assert len(slabbed) >= 9 and all('M=16032' in l for l in trace if l.startswith('gemm_tn<')), text
  compare(eng, case['ref'], case)


def test_fullsize_fp32_frequency_domain_l8_gradients_match_float64_reference(case):
  """The default fp32 step: nine of the eleven layers run in the frequency domain (csrc/conv_fft.hip) -- block DFTs,
  per-bin GEMMs on the fp32 MFMA kernels (batched launches in the trace: 48 bins for the 32-tap layer, 36 for the 7-tap
  layers, 45 for the stride-2 first layer on its polyphase view), fused inverse + epilogue, filter-gradient chains of
  the narrow layers on the side stream.  Same three comparisons and the same tolerances as the W-tap kernels."""
  eng, trace = run_step(case, 'fp32', fft_conv=True)
  text = '\n'.join(trace)
  # L8 (48 bins): forward and back-prop products on the batched convolution kernel, lag products on the batched
  # filter-gradient kernel; the seven 7-tap layers (36 bins) likewise
  # (round 6: the 32-tap layer's complex products in three real products -- gemm_nn_g3 / gemm_tn_g3, conv_fft.hip g3_form)
  assert sum(1 for l in trace if l.startswith('gemm_nn_g3<') and ' batched bins=48 ' in l) == 2, text
  assert sum(1 for l in trace if l.startswith('gemm_tn_g3<') and ' batched bins=48 M=256 ' in l) == 1, text   # the lag products of the 48 bins
  assert sum(1 for l in trace if l.startswith(('gemm_nn<', 'gemm_nn_bins<')) and ' batched bins=36 ' in l) == 14, text
  assert sum(1 for l in trace if l.startswith('gemm_tn<') and ' batched bins=72 M=512 ' in l) == 7, text
  assert not any('Kp=8192' in l or 'Kp=64512' in l or 'Kp=1792' in l for l in trace if 'batched' not in l), text   # no W-tap launch of L1..L8
  # the stride-2 first layer on its polyphase view (25 taps over 2 x 80 channels, 45 bins): forward + filter gradient
  assert sum(1 for l in trace if l.startswith(('gemm_nn<', 'gemm_nn_bins<')) and ' batched bins=45 ' in l) == 1, text
  assert sum(1 for l in trace if l.startswith('gemm_tn<') and ' batched bins=45 ' in l) == 1, text
  assert not any('Kp=3840' in l for l in trace if 'batched' not in l), text
  compare(eng, case['ref'], case)


def test_fullsize_bf16x6_gradients_match_float64_reference(case):
  eng, trace = run_step(case, 'bf16x6')
  assert sum(1 for l in trace if l.startswith('gemm_nn_bf16<256,NP=3>')) >= 4, '\n'.join(trace)
  compare(eng, case['ref'], case)


def test_fullsize_bf16x6_with_frequency_domain_l8(case):
  """bf16x6 mode as it runs by default: the frequency-domain (fp32) L8 between bf16x6 layers -- the planes of its
  neighbours are split from its fp32 outputs."""
  eng, trace = run_step(case, 'bf16x6', fft_conv=True)
  assert sum(1 for l in trace if l.startswith('gemm_nn_g3<') and ' batched bins=48 ' in l) == 2 and \
      sum(1 for l in trace if l.startswith('gemm_tn_g3<') and ' batched bins=48 ' in l) == 1 and \
      any(l.startswith('gemm_nn_bf16<256,NP=3>') for l in trace)
  compare(eng, case['ref'], case)


def test_fullsize_update_matches_reference_adam(case):
  """clip_by_global_norm(5) + TF-Adam at full size: the global norm and the first update of every tensor against
  the oracle's optimizer (speech_model.py:77-82) fed the device's own gradients (whose parity is the tests above)."""
  from oracle import w2l_oracle as O
  eng, _ = run_step(case, 'fp32', fft_conv=True)
  flat = [g.astype(np.float64) for pair in eng.get_grads() for g in pair]
  clipped, gn = O.clip_by_global_norm(flat, 5.0)
  eng.apply_update(lr=1e-4)
  torch.cuda.synchronize()
  assert float(eng.stats[0]) == pytest.approx(gn, rel=1e-5)
  new = eng.get_weights()
  for i, (F, b) in enumerate(case['params']):
    for j, (p0, got) in enumerate(((F, new[i][0]), (b, new[i][1]))):
      g = clipped[2 * i + j]
      want, _, _ = O.adam_tf_step(p0.astype(np.float64), g, np.zeros_like(g), np.zeros_like(g), 1, 1e-4)
      # the first Adam step moves every weight by lr * g/(|g| + eps*sqrt(1-b2)/(1-b1))-ish: compare the DELTA
      d_got, d_want = got.astype(np.float64) - p0, want - p0
      # + one fp32 rounding of the stored weight (the delta can be smaller than an ulp of the weight)
      assert np.max(np.abs(d_got - d_want)) < 1e-4 * np.max(np.abs(d_want)) + 1.2e-7 * np.max(np.abs(p0)) + 1e-12, (i, j)
