"""The two kernels of a narrow layer's backward pass that were rebuilt to share a CU: the lag products
on 128 x 64 output tiles and the persistent per-bin product kernel without its per-row address registers.  Neither change
may move a bit: every output element keeps its sum order.

The per-bin products are held against the bits of the kernel as it was before the rebuild (236 registers, two workgroups
per CU): tests/golden/streamk_bits_before_footprint.json holds the SHA-256 of its outputs for the inputs below, recorded on
an MI355X from the commit before this one with `python -m tests.test_gpu_coresident_footprints` (the inputs are integer
arithmetic, not a random generator: the same floats everywhere)."""
import ctypes
import hashlib
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'streamk_bits_before_footprint.json')


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('needs a GPU')
  return torch.device('cuda:0')


def lattice(shape, mul, add, scale):
  """Exactly representable float32 in (-1, 1) * scale from the element index: (i * mul + add) mod 2039, centred, / 1024."""
  n = int(np.prod(shape))
  i = np.arange(n, dtype=np.int64)
  return (((i * mul + add) % 2039 - 1019).astype(np.float32) / np.float32(1024.0) * np.float32(scale)).reshape(shape)


P = lambda t: ctypes.c_void_p(t.data_ptr())

# ---------------------------------------------------------------- lag products, 64-wide tile ----

TN_M, TN_K = 64, 128


def tn_operands(dev, products, z_batches, N):
  A = torch.from_numpy(lattice((products, TN_M, TN_K), 7919, 13, 1.0)).to(dev)
  Z = torch.from_numpy(lattice((z_batches, TN_M, N), 104729, 101, 0.5)).to(dev)
  return A, Z


def tn_run(dev, A, Z, N, shift, tile):
  from speecht_amd._lib import call, launch_trace
  products = A.shape[0]
  out = torch.full((products, TN_K, N), float('nan'), dtype=torch.float32, device=dev)
  with launch_trace() as tr:
    call('st_gemm_tn_batched_tile_f32', P(A), TN_K, TN_M * TN_K, P(Z), N, TN_M * N, P(out), TN_K * N, TN_M, TN_K, N, products, shift, tile, None)
  torch.cuda.synchronize()
  assert tr.lines[0].startswith('gemm_tn<%d> batched bins=%d M=%d ' % (tile, products, TN_M)), tr.lines
  return out


@pytest.mark.parametrize('products,shift,N', [(3, 0, 128), (3, 0, 256), (6, 1, 256)])
def test_lag_products_on_the_64_wide_tile(dev, products, shift, N):
  """out[b] = A[b]^T Z[b >> shift] over 64 rows (two stages), 128 x N outputs: one and two column tiles of 128, two and four
  of 64; shift 1 is the shared-Z form (the real and imaginary product of a bin read the same gradient spectra).  Both tiles
  against a float64 product at 2e-6 of the largest output -- the bound the per-bin product tests hold fp32 chains of up to 512
  terms to (64 terms of magnitude < 0.5 here: about sqrt(64) * 2^-24 = 5e-7 expected).  An output element sums its 64 rows in the
  same order on either tile (32 rows per stage, two per MFMA, the tile only decides which wave holds the column): the same bits."""
  A, Z = tn_operands(dev, products, ((products - 1) >> shift) + 1, N)
  ref = np.einsum('bmk,bmn->bkn', A.cpu().numpy().astype(np.float64), Z.cpu().numpy().astype(np.float64)[np.arange(products) >> shift])
  scale = np.abs(ref).max()
  outs = {}
  for tile in (64, 128):
    outs[tile] = tn_run(dev, A, Z, N, shift, tile)
    err = np.abs(outs[tile].cpu().numpy().astype(np.float64) - ref).max() / scale
    print('gemm_tn<%d> products=%d shift=%d N=%d: max err / max |ref| = %.3e' % (tile, products, shift, N, err))
    assert err < 2e-6, (tile, err)
  assert torch.equal(outs[64], outs[128])


def test_lag_product_tile_by_shape(dev):
  """The entry points without a tile argument choose by shape: the 7-tap layers' 72 products of 256 x 256 over 512 rows (288 tiles
  of 128 on 256 CUs) take the 64-wide tile, a handful of products and a launch of several rounds keep 128."""
  from speecht_amd._lib import call, launch_trace
  for products, M, K, N, want in ((72, 64, 256, 256, 64), (3, 64, 128, 256, 128), (90, 64, 256, 256, 128), (72, 576, 256, 256, 128)):
    A = torch.zeros((products, M, K), dtype=torch.float32, device=dev)
    Z = torch.zeros(((products + 1) // 2, M, N), dtype=torch.float32, device=dev)
    out = torch.empty((products, K, N), dtype=torch.float32, device=dev)
    with launch_trace() as tr:
      call('st_gemm_tn_batched_shared_f32', P(A), K, M * K, P(Z), N, M * N, P(out), K * N, M, K, N, products, 1, None)
    torch.cuda.synchronize()
    assert tr.lines[0].startswith('gemm_tn<%d> batched bins=%d M=%d ' % (want, products, M)), tr.lines
    assert float(out.abs().max()) == 0.0


# ---------------------------------------------------------------- per-bin products, persistent kernel ----

# (bins, M, K, N) -> expected "wgs= upw=" of the plan at 64 / 96 workgroups per XCD (csrc/streamk_map.h):
#   5 bins x (128 x 256): 20 tiles, 3 per XCD label, of 3 / 5 k-tiles -- 9 / 15 units per label, one workgroup each whatever the
#   slot count: every tile is cut into single k-tiles (3 or 5 pieces, 2 or 4 hand-offs per tile);
#   37 bins x (192 x 256) over 96: 222 tiles, 28 per label, 84 units -- 64 workgroups of two units (tiles cut 2 + 1 or 1 + 2) or
#   84 of one: the smallest shape at which the two slot counts give different plans.
SK_SHAPES = {(5, 128, 96, 256): {64: 'wgs=72 upw=1', 96: 'wgs=72 upw=1'},
             (5, 128, 160, 256): {64: 'wgs=120 upw=1', 96: 'wgs=120 upw=1'},
             (37, 192, 96, 256): {64: 'wgs=512 upw=2', 96: 'wgs=672 upw=1'}}
SK_CASES = [(shape, slots, bt) for shape in SK_SHAPES for slots in (64, 96) for bt in (False, True)]


def sk_key(shape, slots, bt):
  return 'bins%d_M%d_K%d_N%d_slots%d_%s' % (shape + (slots, 'bt' if bt else 'nn'))


def sk_operands(dev, shape):
  bins, M, K, N = shape
  A = torch.from_numpy(lattice((bins, M, K), 7919, 13, 1.0)).to(dev)
  B = torch.from_numpy(lattice((bins, K, N), 104729, 101, 1.0 / math.sqrt(K))).to(dev)
  return A, B


def sk_launches(dev, A, B, slots, bt, reps):
  """`reps` forced stream-K launches, each over an output full of NaN; returns the outputs and the trace line."""
  from speecht_amd import _lib
  from speecht_amd._lib import call, launch_trace, set_tuning
  lib = _lib.load()
  bins, M, K = A.shape
  N = B.shape[2]
  Bop = B.transpose(1, 2).contiguous() if bt else B
  entry = 'st_gemm_nn_batched_bt_ws_f32' if bt else 'st_gemm_nn_batched_ws_f32'
  ws_bytes = lib.st_gemm_nn_batched_ws_bytes()
  ws = torch.full((ws_bytes // 4,), float('nan'), dtype=torch.float32, device=dev)            # scratch: any content
  outs = []
  set_tuning('streamk', 1)
  set_tuning('streamk_slots', slots)
  try:
    for _ in range(reps):
      C = torch.full((bins, M, N), float('nan'), dtype=torch.float32, device=dev)
      with launch_trace() as tr:
        call(entry, P(A), K, M * K, P(Bop), K * N, P(C), N, M * N, M, K, N, bins, P(ws), ws_bytes, None)
      outs.append(C)
    torch.cuda.synchronize()
  finally:
    set_tuning('streamk', 0)
    set_tuning('streamk_slots', 0)
  return outs, tr.lines[0]


def sk_digest(C):
  return hashlib.sha256(C.cpu().numpy().tobytes()).hexdigest()


def lost_count():
  from speecht_amd._lib import call
  n = ctypes.c_uint32(0)
  call('st_streamk_lost_count', ctypes.byref(n))
  return n.value


@pytest.mark.parametrize('shape,slots,bt', SK_CASES, ids=[sk_key(*c) for c in SK_CASES])
def test_persistent_products_keep_their_bits_in_the_smaller_footprint(dev, shape, slots, bt):
  """Shapes whose tiles are cut between workgroups (SK_SHAPES), forced through the persistent kernel, both operand forms.  Twenty
  launches over dirty outputs: the same bits each time, the bits of the kernel before the rebuild at the same plan (the sum
  order head + next + ... is fixed, so any difference is a bug), within fp32 rounding of a float64 product, no hand-off lost."""
  A, B = sk_operands(dev, shape)
  before = lost_count()
  outs, line = sk_launches(dev, A, B, slots, bt, 20)
  assert line.startswith('gemm_nn_bins<64,128,2,2,bt> batched' if bt else 'gemm_nn_bins<64,128,2,2> batched') and ' streamk ' in line, line
  assert ' %s ' % SK_SHAPES[shape][slots] in line, line
  for o in outs[1:]:
    assert torch.equal(outs[0], o)
  assert lost_count() == before
  ref = torch.matmul(A.double(), B.double())
  err = float((outs[0].double() - ref).abs().max() / ref.abs().max())
  print('gemm_nn_bins %s: max err / max |ref| = %.3e' % (sk_key(shape, slots, bt), err))
  assert err < 2e-6, err
  with open(GOLDEN) as f:
    golden = json.load(f)
  assert sk_digest(outs[0]) == golden[sk_key(shape, slots, bt)]


if __name__ == '__main__':
  # records the golden file's content from whatever library this tree builds (run it on the commit to compare against)
  device = torch.device('cuda:0')
  digests = {}
  for shape_, slots_, bt_ in SK_CASES:
    A_, B_ = sk_operands(device, shape_)
    outs_, _ = sk_launches(device, A_, B_, slots_, bt_, 1)
    digests[sk_key(shape_, slots_, bt_)] = sk_digest(outs_[0])
  print(json.dumps(digests, indent=1, sort_keys=True))
