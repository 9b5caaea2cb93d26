"""Gradient parity of full-size training steps at the batch shapes real training produces, not just the headline one.

tests/test_gpu_fullsize_grads.py checks one step at 32 x 1001 frames, where every frequency-domain layer has exactly 8 blocks
of 64 output frames and 256 rows per bin: the fused transforms, whole 128-row tiles of the 32-tap layer's per-bin products, no
split reductions in the 1x1 layers.  Real batches are padded to their own longest utterance (speech_input.py:37-45), and the
library switches kernels at these boundaries: more than 8 blocks or rows that are not a multiple of 64 (separate transforms),
a half 128-row tile (a 64-row launch of its own), few workgroups (split reductions), stream-K rounds of the narrow layers'
products, 128-mel input (layer 0's lag products in the split form), few rows (the W-tap kernels with split reductions).

Each case below runs one forward + CTC + backward of the full model (250 / 2000 channels, xavier weights, non-zero biases) with
the default engine settings, asserts from the launch trace that its regime actually ran, and checks the step against float64
(tests/grad_parity.py): fp32 with ``compare`` (logits, losses, dlogits; all 22 gradient tensors kernel by kernel, end to end
with the ReLU pattern pinned, and end to end against the free evaluation for every layer below which no unit flipped, each at
2e-4 of the tensor's max); bf16 activations with the stored-operand checks of the config-3 test and logits / losses end to end
against the bf16-storage oracle, at the config-3 bounds."""
import time

import numpy as np
import pytest

from oracle import w2l_oracle as O
from tests import grad_parity as GP
from tests import torch_ref as TR
from tests import workloads as WL

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

ULP = GP.ULP

# name -> (frames per utterance, ragged tail included; mel bands; batch seed)
CASES = {
    'A': ([1101] * 30 + [901, 640], 80, 21),            # 32 x 11 s: 551 frames after L0, 9 blocks, 288 rows -> 320 per bin
    'B': ([1533] * 6 + [1400, 1100], 80, 22),           # short batch of long utterances: 767 frames, 12 blocks, 96 rows -> 128
    'C': ([1501] * 14 + [1300, 1001], 128, 23),         # the reference's 128-mel features: 751 frames, 12 blocks, 192 rows
    'D': ([201] * 30 + [150, 101], 80, 24),             # 2 s utterances: 101 frames, 2 blocks, 64 rows
    'E': ([601] * 18 + [555, 480], 80, 25),             # odd rows at <= 8 blocks: 301 frames, 5 blocks, 100 rows -> 128
    'F': ([401, 333], 80, 26),                          # few rows: 201 frames, 402 rows (W-tap kernels everywhere)
}


def build_case(name):
  frames, mel, seed = CASES[name]
  layers = WL.w2l_layers(mel)
  params = WL.xavier_params(layers, seed=42, dtype=np.float32)      # non-zero biases
  x, seq, labels = WL.make_batch(frames, mel, seed=seed)
  return GP.make_case(layers, params, x.astype(np.float32), seq, labels)


@pytest.fixture(scope='module')
def cases():
  """name -> case with its free float64 reference (tests/torch_ref.py), each computed once for the module."""
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  memo = {}

  def get(name, ref=True):
    if name not in memo:
      memo[name] = build_case(name)
    case = memo[name]
    if ref and 'ref' not in case:
      t0 = time.time()
      case['ref'] = TR.loss_and_grads(case['x'], case['seq'], case['labels'], case['params'], case['layers'], dtype=torch.float64)
      print('case %s: float64 CPU reference of the step: %.1f s' % (name, time.time() - t0))
    return case
  return get


def count(trace, prefix, *parts):
  return sum(1 for l in trace if l.startswith(prefix) and all(p in l for p in parts))


FUSED = ('idft_dft_rows<', 'idft_ola_dft_rows<')


def assert_separate_transforms(trace):
  text = '\n'.join(trace)
  assert count(trace, FUSED) == 0, text
  assert count(trace, 'dft_rows<') > 0 and count(trace, 'idft_rows<') > 0, text


# ---------------------------------------------------------------- fp32 ----

def test_case_a_32x11s_nine_blocks_half_tiles(cases):
  """Case A: 9 blocks per utterance, 288 rows per bin padded to 320 -- separate transforms; the 32-tap layer's forward as a
  whole-tile launch of 256 rows plus one of 64; its back-prop on 64-row tiles with the reduction split in two."""
  case = cases('A')
  eng, trace = GP.run_step(case, 'fp32', fft_conv=True)
  text = '\n'.join(trace)
  assert_separate_transforms(trace)
  assert count(trace, 'gemm_nn_g3<128> ', ' bins=48 M=256 ', 'ksplit=1 ') == 1, text
  assert count(trace, 'gemm_nn_g3<64> ', ' bins=48 M=64 ', 'ksplit=1 ') == 1, text
  assert count(trace, 'gemm_nn_g3<64,bt> ', ' bins=48 M=320 ', 'ksplit=2 ') == 1, text
  assert count(trace, 'gemm_tn_g3<128> ', ' bins=48 M=320 ') == 1, text
  # the narrow layers' products whole (7 forward, 7 back-prop), not on the stream-K kernel
  assert count(trace, 'gemm_nn<64,128,2,2,', ' batched bins=36 M=320 ') == 14 and count(trace, 'gemm_nn_bins<') == 0, text
  GP.compare(eng, case['ref'], case)


def test_case_b_short_batch_long_utterances_stream_k(cases):
  """Case B: 8 utterances of up to 15 s -- 12 blocks, 96 rows per bin padded to 128: separate transforms; the narrow layers'
  per-bin products on the persistent stream-K kernel; the 32-tap layer's back-prop with the reduction split in two."""
  case = cases('B')
  eng, trace = GP.run_step(case, 'fp32', fft_conv=True)
  text = '\n'.join(trace)
  assert_separate_transforms(trace)
  assert count(trace, 'dft_rows<3> ', 'rows=96 ') == 15, text
  # forward and back-prop of the seven 7-tap layers and the forward of layer 0: persistent stream-K launches
  assert count(trace, 'gemm_nn_bins<64,128,2,2> ', ' batched bins=36 M=128 ', ' streamk ') == 7, text
  assert count(trace, 'gemm_nn_bins<64,128,2,2,bt> ', ' batched bins=36 M=128 ', ' streamk ') == 7, text
  assert count(trace, 'gemm_nn_bins<64,128,2,2> ', ' batched bins=45 M=128 ', ' streamk ') == 1, text
  assert count(trace, 'gemm_nn_g3<128> ', ' bins=48 M=128 ', 'ksplit=1 ') == 1, text
  assert count(trace, 'gemm_nn_g3<64,bt> ', ' bins=48 M=128 ', 'ksplit=2 ') == 1, text
  GP.compare(eng, case['ref'], case)


def test_case_c_128_mel_split_lag_products(cases):
  """Case C: the reference's 128 mel bands -- layer 0's polyphase view is 256 channels wide, so its lag products run as separate
  real and imaginary products; 12 blocks, 192 rows per bin: separate transforms, the 32-tap forward as 128 + 64 rows."""
  case = cases('C')
  eng, trace = GP.run_step(case, 'fp32', fft_conv=True)
  text = '\n'.join(trace)
  assert_separate_transforms(trace)
  assert count(trace, 'gemm_nn_g3<128> ', ' bins=48 M=128 ', 'ksplit=1 ') == 1, text
  assert count(trace, 'gemm_nn_g3<64> ', ' bins=48 M=64 ', 'ksplit=1 ') == 1, text
  assert count(trace, 'gemm_nn_g3<64,bt> ', ' bins=48 M=192 ', 'ksplit=2 ') == 1, text
  # layer 0 (45 bins, 256-channel polyphase view): lag products as 90 real / imaginary products, not 45 complex ones
  assert count(trace, 'gemm_tn<128> ', ' batched bins=90 M=384 ') == 1 and count(trace, 'gemm_tn<', ' batched bins=45 ') == 0, text
  GP.compare(eng, case['ref'], case)


def test_case_d_2s_utterances_fused_transforms_sliced_classifier(cases):
  """Case D: 32 x 2 s -- 2 blocks, 64 rows per bin: the fused transforms; the classification layer's forward reduction sliced."""
  case = cases('D')
  eng, trace = GP.run_step(case, 'fp32', fft_conv=True)
  text = '\n'.join(trace)
  # the layer-to-layer forward transforms (layer 0 -> L1 ... L6 -> L7) and the narrow layers' back-prop fused
  assert count(trace, 'idft_dft_rows<', 'rows=64 ') == 7 and count(trace, 'idft_ola_dft_rows<18,dz-spectra> ', 'rows=64 ') == 7, text
  assert count(trace, 'gemm_nn_g3<64> ', ' bins=48 M=64 ', 'ksplit=1 ') == 1, text
  assert count(trace, 'gemm_nn_g3<64,bt> ', ' bins=48 M=64 ', 'ksplit=2 ') == 1, text
  # L10's forward reduction sliced
  assert count(trace, 'gemm_nn<128,32,4,1,clamped> ', 'epi=0 splits=8 M=3232 Np=32 ') == 1, text
  GP.compare(eng, case['ref'], case)


def test_case_e_odd_rows_few_blocks_separate_transforms(cases):
  """Case E: 5 blocks, but 100 rows per bin padded to 128 -- the separate transforms although the blocks would fit the fused ones."""
  case = cases('E')
  eng, trace = GP.run_step(case, 'fp32', fft_conv=True)
  text = '\n'.join(trace)
  assert_separate_transforms(trace)
  assert count(trace, 'dft_rows<3> ', 'rows=100 ') == 15, text
  assert count(trace, 'gemm_nn_bins<64,128,2,2', ' batched bins=36 M=128 ') == 14, text
  assert count(trace, 'gemm_nn_g3<128> ', ' bins=48 M=128 ', 'ksplit=1 ') == 1, text
  GP.compare(eng, case['ref'], case)


def test_case_f_few_rows_w_tap_split_reductions(cases):
  """Case F: two utterances, 402 rows -- below the frequency path's threshold: W-tap kernels everywhere, split reductions."""
  case = cases('F')
  eng, trace = GP.run_step(case, 'fp32', fft_conv=True)
  text = '\n'.join(trace)
  assert not any(' batched ' in l for l in trace), text
  # L9's forward reduction split in four; L8's forward in four and its back-prop in eight
  assert count(trace, 'gemm_nn<128,128,2,2,fast> ', 'epi=0 splits=4 M=402 Np=2048 Kp=2016 ') == 1, text
  assert count(trace, 'gemm_nn<128,128,2,2,fast> ', 'epi=0 splits=4 M=402 Np=2048 Kp=8192 taps=32 ') == 1, text
  assert count(trace, 'gemm_nn<128,128,2,2,fast> ', 'epi=1 splits=8 M=402 Np=256 Kp=64512 taps=32 ') == 1, text
  # the 7-tap layers' forward split in 14; every filter gradient on the W-tap kernel, one row slab
  assert count(trace, 'gemm_nn<128,128,2,2,fast> ', 'epi=0 splits=14 M=402 Np=256 Kp=1792 taps=7 ') == 7, text
  assert count(trace, 'gemm_tn<', 'slabs=1 ', 'M=402 ') == 11, text
  GP.compare(eng, case['ref'], case)


# ---------------------------------------------------------------- bf16 ----

def run_bf16(cases, name):
  """One bf16 step of a case, its regime common to every shape asserted; -> (case, engine, trace, spectral layers)."""
  case = cases(name, ref=False)
  eng, trace = GP.run_step(case, 'bf16', fft_conv=True)
  text = '\n'.join(trace)
  spectral = set(eng.fftb)
  assert spectral == {8}, (spectral, text)
  # the 32-tap layer's lag products: one launch over the real and imaginary products of its 48 bins
  assert count(trace, 'wgrad_tr_bf16<128,128,32,lag> ', ' bins=96 ') == 1, text
  # the filter gradients of the other stride-1 layers: the transposing-read kernel where tr_eligible takes the geometry
  tr_layers = [i for i in range(1, len(case['layers'])) if i not in spectral and eng._wgrad_tr[i]]
  print('case %s bf16: filter gradients on wgrad_tr_bf16<128,128,32>: layers %s; on the fallback: %s' % (
      name, tr_layers, [i for i in range(1, len(case['layers'])) if i not in spectral and not eng._wgrad_tr[i]]))
  assert count(trace, 'wgrad_tr_bf16<128,128,32> ') == len(tr_layers), text
  return case, eng, trace, spectral


def check_bf16(case, eng, spectral):
  layers, seq, labels = case['layers'], case['seq'], case['labels']
  p64 = [(F.astype(np.float64), b.astype(np.float64)) for F, b in case['params']]
  grads = eng.get_grads()
  t0 = time.time()
  logits = O.wav2letter_forward(case['x'].astype(np.float64), p64, layers, store=O.bf16_round, spectral=spectral)
  loss, _ = O.ctc_loss_and_grad(logits, labels, seq // 2)
  print('bf16-storage oracle forward + CTC: %.1f s' % (time.time() - t0))
  got = eng.logits_time_major().cpu().numpy()
  mx, mean = GP.scaled_err(got, logits)
  print('logits: max %.2f ulp, mean %.3f ulp (bf16 ulp of the tensor scale)' % (mx / ULP, mean / ULP))
  assert mx < 16 * ULP and mean < 0.5 * ULP, (mx, mean)
  np.testing.assert_allclose(eng.loss.cpu().numpy(), loss, rtol=2e-2)
  GP.stored_operand_checks(eng, p64, layers, grads, labels, seq, case['scale'], spectral)


def test_case_a_bf16(cases):
  case, eng, trace, spectral = run_bf16(cases, 'A')
  text = '\n'.join(trace)
  # the 32-tap layer's bin planes padded to a multiple of 128 rows: 288 -> 384
  assert count(trace, 'gemm_nn_bf16<', ' batched bins=48 M=384 ') == 2, text
  assert count(trace, 'wgrad_tr_bf16<128,128,32,lag> ', ' Kp=768 ') == 1, text
  check_bf16(case, eng, spectral)


def test_case_b_bf16(cases):
  case, eng, trace, spectral = run_bf16(cases, 'B')
  text = '\n'.join(trace)
  assert count(trace, 'gemm_nn_bf16<', ' batched bins=48 M=128 ') == 2, text
  check_bf16(case, eng, spectral)


def test_case_d_bf16(cases):
  case, eng, trace, spectral = run_bf16(cases, 'D')
  text = '\n'.join(trace)
  assert count(trace, 'gemm_nn_bf16<', ' batched bins=48 M=128 ') == 2, text
  check_bf16(case, eng, spectral)
