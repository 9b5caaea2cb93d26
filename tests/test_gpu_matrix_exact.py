"""The time-domain matrix kernels through their C entry points on exact-integer data (tests/exact_cases.py): fp32 results equal the
integer reference BIT FOR BIT, stored bf16 results its round-to-nearest-even, in every tile form, split and dispatch branch.
The tests build the st_tensor3 descriptors themselves (halo, frame pitch, channel pitch and left padding are the test's choice, not
the engine's), put every written buffer between guard regions, keep the guard pattern in the halo rows of the output tensors and
assert the launch-trace line that proves which kernel form ran; where the trace does not name the form (whole-stage or clamped
bf16 kernel, ring depth and workgroup map of the transposing filter gradient) the host expression of the .hip file gives it.
The three-plane (bf16x6) kernels run on planes of independent integers: six kept plane products, output planes equal to split3 of the
result; their layout kernels are compared with the numpy model of split3 on real floats.
The last test asserts that the union of the forms seen is the required list."""
import ctypes
import os

import numpy as np
import pytest

from tests import exact_cases as E

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SEEN = set()          # first word of every trace line of every case
COVERAGE = []         # (test id, trace line) in the order the cases ran: printed by the last test
REQUIRED = {
    'gemm_nn<64,128,2,2,clamped>', 'gemm_nn<128,128,2,2,fast>', 'gemm_nn<128,128,2,2,clamped>', 'gemm_nn<128,64,2,2,clamped>',
    'gemm_nn<128,32,4,1,clamped>', 'gemm_nn<64,128,2,2,fast-bt>', 'gemm_nn<128,128,2,2,fast-bt>',
    'gemm_tn<128>', 'gemm_tn<64>', 'gemm_tn<32>',
    'gemm_nn_bf16<128,NP=1>', 'gemm_nn_bf16<256,NP=1>', 'conv_taps_bf16<128,128,64,panel>', 'wgrad_tr_bf16<128,128,32>',
    'gemm_nn_bf16<128,NP=3>', 'gemm_nn_bf16<256,NP=3>',
}
BF16_FORMS = set()    # (tile, whole stages) of the bf16 general kernel, from the host expressions
TR_FORMS = set()      # (ring, map, bias in tile) of the transposing filter gradient


@pytest.fixture(scope='module')
def dev():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return torch.device('cuda:0')


def P(t, offset=0):
  return ctypes.c_void_p(t.data_ptr() + offset)


def t3(g, ptr):
  from speecht_amd._lib import Tensor3
  return Tensor3(ptr.value, g.batch, g.frames, g.channels, g.halo, g.t_pitch, g.c_pitch)


class Guarded:
  """A device buffer between guard regions, initialised from a host image of bit patterns (tests/exact_cases.py)."""

  def __init__(self, dev, image):
    self.bits16 = image.dtype == np.uint16
    self.buf = torch.from_numpy(image.view(np.int16 if self.bits16 else np.int32)).to(dev)
    self.ptr = P(self.buf, E.GUARD_WORDS * (2 if self.bits16 else 4))

  def read(self):
    return self.buf.cpu().numpy().view(np.uint16 if self.bits16 else np.uint32)


def in_f32(dev, g, data):
  """an input tensor: zero halos and pad channels, SLACK_ROWS zero rows behind it"""
  img = np.concatenate([E.embed(g, data).reshape(-1), np.zeros(E.SLACK_ROWS * g.c_pitch, np.float32)])
  return torch.from_numpy(img).to(dev)


def in_bf16(dev, g, data):
  """the same as a bf16 plane (small integers: exact); the slack rows are the 40 zero rows st_conv1d_nwc_bwd_filter_tr_bf16 demands"""
  return in_f32(dev, g, data).to(torch.bfloat16)


OPERAND_SLACK = 1 << 16     # zero elements behind every read-only operand (filters, bias)


def dev_f32(dev, a):
  a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
  return torch.from_numpy(np.concatenate([a, np.zeros(OPERAND_SLACK, np.float32)])).to(dev)


def dev_bits16(dev, a):
  a = np.ascontiguousarray(a).view(np.int16).reshape(-1)
  return torch.from_numpy(np.concatenate([a, np.zeros(OPERAND_SLACK, np.int16)])).to(dev)


def scratch(dev, nbytes):
  """a workspace of any content (NaN): what a call reads of it, it has written"""
  return torch.full((int(nbytes) // 4 + 64,), float('nan'), device=dev)


def bias_vector(L, d, n_pad):
  b = np.zeros(n_pad, np.float32)
  b[:L.cout] = d['bias']
  return b


def act_geo(L):
  """the mask tensor: the geometry of dx with front and back halo swapped"""
  g = L.x_geo
  return g._replace(halo=g.t_pitch - g.frames - g.halo)


def traced(fn):
  from speecht_amd._lib import launch_trace
  with launch_trace() as tr:
    fn()
  torch.cuda.synchronize()
  case = os.environ.get('PYTEST_CURRENT_TEST', '').split('::')[-1].split(' ')[0]
  for l in tr.lines:
    SEEN.add(l.split(' ')[0])
    COVERAGE.append((case, l.split(' gflop=')[0]))
  return tr.lines


def field(line, name):
  return int(line.split(name + '=')[1].split(' ')[0])


def only(lines, prefix):
  hit = [l for l in lines if l.startswith(prefix)]
  assert len(hit) == 1, (prefix, lines)
  return hit[0]


def ok(err):
  assert err is None, err


# ---- layout kernels: bit-exact against the index formulas of include/speecht_hip.h on arbitrary data ---------------------------
@pytest.mark.parametrize('cin,cout', [(40, 130), (128, 128)])
@pytest.mark.parametrize('W', [1, 7, 48])
def test_filter_layout_kernels(dev, W, cin, cout):
  from speecht_amd._lib import call
  rng = np.random.default_rng(W * 1000 + cin)
  F = rng.standard_normal((W, cin, cout)).astype(np.float32)
  cpi, cpo = E.round_up(cin, 16), E.round_up(cout, 16)
  _, kp, n_pad = E.packed_dims(W, cpi, cout)
  want = E.pack_ref(F, cpi)
  Fd = dev_f32(dev, F)
  packed = Guarded(dev, E.guarded_flat_image(kp * n_pad))
  call('st_pack_filters_f32', P(Fd), W, cin, cout, cpi, packed.ptr, None)
  ok(E.check_guarded_flat(packed.read(), E.f32_bits(want), what='pack', shape=want.shape))
  Pd = dev_f32(dev, want)
  back = Guarded(dev, E.guarded_flat_image(F.size))
  call('st_unpack_filters_f32', P(Pd), W, cin, cout, cpi, back.ptr, None)
  ok(E.check_guarded_flat(back.read(), E.f32_bits(F), what='unpack', shape=F.shape))
  want_t = E.flip_transpose_ref(want, W, cin, cout, cpi, cpo)
  flipped = Guarded(dev, E.guarded_flat_image(want_t.size))
  call('st_filters_flip_transpose_f32', P(Pd), W, cin, cout, cpi, cpo, flipped.ptr, None)
  ok(E.check_guarded_flat(flipped.read(), E.f32_bits(want_t), what='flip_transpose', shape=want_t.shape))
  wt = Guarded(dev, E.guarded_flat_image(kp * n_pad, bits16=True))
  call('st_filters_bf16', P(Pd), kp, n_pad, wt.ptr, None)
  ok(E.check_guarded_flat(wt.read(), E.filters_bf16_ref(want), bits16=True, what='filters_bf16', shape=(n_pad, kp)))
  want_b = E.filters_bwd_bf16_ref(want, W, cin, cout, cpi, cpo)
  image = E.guarded_flat_image(want_b.size, bits16=True)
  image[E.GUARD_WORDS:-E.GUARD_WORDS] = 0                  # zero-initialised by the caller
  wtt = Guarded(dev, image)
  call('st_filters_bwd_bf16', P(Pd), W, cin, cout, cpi, cpo, wtt.ptr, None)
  ok(E.check_guarded_flat(wtt.read(), want_b, bits16=True, what='filters_bwd_bf16', shape=want_b.shape))
  torch.cuda.synchronize()


def test_cast_bf16_rounds_to_nearest_even(dev):
  """against torch's conversion, on the integers to 2^16 (every odd multiple of half a bf16 step among them is a tie), on random normal
  numbers, on ties at random exponents and on their two neighbours"""
  from speecht_amd._lib import call
  rng = np.random.default_rng(5)
  ints = np.arange(1 << 16, dtype=np.float32)
  rnd = (rng.standard_normal(1 << 16) * np.exp(rng.uniform(-20, 20, 1 << 16))).astype(np.float32)
  ties = ((rng.integers(0x0080, 0x7F00, 1 << 12).astype(np.uint32) << 16) | np.uint32(0x8000)).view(np.float32)
  near = np.concatenate([np.nextafter(ties, np.float32(0)), np.nextafter(ties, np.float32(np.inf))])
  src = np.concatenate([ints, -ints, rnd, ties, -ties, near])
  src = src[:src.size // 4 * 4]
  want = torch.from_numpy(src).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
  assert np.array_equal(want, E.bf16_bits(src))
  out = Guarded(dev, E.guarded_flat_image(src.size, bits16=True))
  sd = dev_f32(dev, src)
  call('st_cast_bf16', P(sd), src.size, out.ptr, None)
  torch.cuda.synchronize()
  ok(E.check_guarded_flat(out.read(), want, bits16=True, what='cast_bf16'))


# ---- bf16 activations: the general kernel, the LDS-panel kernel -----------------------------------------------------------------
def run_fwd_bf16(dev, L, out, use_ws=True, relu=True):
  """st_conv1d_nwc_fwd_ws_bf16 into y_f32 (out = 'f32') or y_bf16 ('bf16'); returns the trace lines"""
  from speecht_amd import _lib
  lib = _lib.load()
  d = E.case_data(L)
  E.assert_exact_range(L, 'fwd')
  E.check_geometry(L, 'fwd')
  xg, yg = L.x_geo, L.y_geo
  _, kp, n_pad = E.packed_dims(L.W, xg.c_pitch, L.cout)
  xb = in_bf16(dev, xg, d['x'])
  wt = dev_bits16(dev, E.filters_bf16_ref(E.pack_ref(d['F'].astype(np.float32), xg.c_pitch)))
  bias = dev_f32(dev, bias_vector(L, d, n_pad))
  y = Guarded(dev, E.guarded_tensor_image(yg, bits16=out == 'bf16'))
  X, Y = t3(xg, P(xb)), t3(yg, y.ptr)
  need = lib.st_conv1d_fwd_bf16_ws(ctypes.byref(X), ctypes.byref(Y), L.W)
  ws = scratch(dev, need) if use_ws and need else None
  lines = traced(lambda: _lib.call('st_conv1d_nwc_fwd_ws_bf16', ctypes.byref(X), P(xb), P(wt), P(bias), L.W, L.stride, L.pad_left, int(relu),
                                   ctypes.byref(Y), y.ptr if out == 'bf16' else None, y.ptr if out == 'f32' else None,
                                   P(ws) if ws is not None else None, need if ws is not None else 0, None))
  ref = E.ref_fwd(d['x'], d['F'], d['bias'], L.pad_left, L.stride, relu)
  ok(E.check_guarded_tensor(y.read(), yg, ref, n_pad, bits16=out == 'bf16', what='{} fwd {}'.format(L.name, out)))
  return lines


def run_bwd_data_bf16(dev, L, mask):
  from speecht_amd import _lib
  lib = _lib.load()
  d = E.case_data(L)
  E.assert_exact_range(L, 'bwd_data')
  E.check_geometry(L, 'bwd_data')
  xg, yg, ag = L.x_geo, L.y_geo, act_geo(L)
  n_pad = E.npad_of(L.cin)
  zb = in_bf16(dev, yg, d['dz'])
  ab = in_bf16(dev, ag, d['act'])
  wtt = dev_bits16(dev, E.filters_bwd_bf16_ref(E.pack_ref(d['F'].astype(np.float32), xg.c_pitch), L.W, L.cin, L.cout, xg.c_pitch, yg.c_pitch))
  dx = Guarded(dev, E.guarded_tensor_image(xg, bits16=True))
  Z, A, X = t3(yg, P(zb)), t3(ag, P(ab)), t3(xg, dx.ptr)
  need = lib.st_conv1d_bwd_data_bf16_ws(ctypes.byref(Z), ctypes.byref(X), L.W)
  ws = scratch(dev, need)
  lines = traced(lambda: _lib.call('st_conv1d_nwc_bwd_data_bf16', ctypes.byref(Z), P(zb), P(wtt), L.W, L.pad_left,
                                   ctypes.byref(A) if mask else None, P(ab) if mask else None, ctypes.byref(X), dx.ptr, P(ws), need, None))
  ref = E.ref_bwd_data(d['dz'], d['F'], L.pad_left, L.T, act=d['act'] if mask else None)
  ok(E.check_guarded_tensor(dx.read(), xg, ref, n_pad, bits16=True, what='{} bwd_data mask={}'.format(L.name, mask)))
  return lines


def assert_general_bf16(L, lines, M, n_pad, k_valid, taps, c_pitch, splits):
  """the trace line of gemm_nn_bf16_kernel: tile and splits as the host expressions give them; records (tile, whole stages)"""
  tile = E.bf16_tile(M, n_pad, splits)
  line = only(lines, 'gemm_nn_bf16<')
  assert line.startswith('gemm_nn_bf16<{},NP=1> splits={} M={} Np={} '.format(tile, splits, M, n_pad)), (L.name, line)
  BF16_FORMS.add((tile, E.bf16_whole_stages(tile, taps, c_pitch, k_valid)))
  return tile


GENERAL_FWD_FORMS = {'one-tile': (128, True), 'tile128-whole': (128, True), 'tile128-clamped-taps': (128, False),
                     'tile128-clamped-ktail': (128, False)}


def test_bf16_single_tile_product_is_exact(dev):
  """The supposition everything else rests on, with nothing else in play: one 128 x 128 tile, one tap, K = 64, no bias, no ReLU --
  the bf16 MFMA accumulates integer sums below 2^24 exactly."""
  L = E.BF16_GENERAL[0]
  assert L.B * L.T <= 128 and L.cout == 128 and L.W == 1 and L.x_geo.c_pitch == 64
  run_fwd_bf16(dev, L, 'f32', relu=False)


@pytest.mark.parametrize('out', ['f32', 'bf16'])
@pytest.mark.parametrize('L', E.BF16_GENERAL, ids=lambda L: L.name)
def test_bf16_general_forward(dev, L, out):
  splits = E.bf16_fwd_splits(L)
  lines = run_fwd_bf16(dev, L, out)
  xg = L.x_geo
  tile = assert_general_bf16(L, lines, L.B * L.t_out, E.npad_of(L.cout), L.W * xg.c_pitch, L.W, xg.c_pitch, splits)
  if L.name in GENERAL_FWD_FORMS:
    assert (tile, E.bf16_whole_stages(tile, L.W, xg.c_pitch, L.W * xg.c_pitch)) == GENERAL_FWD_FORMS[L.name]
  if L.name.startswith('fwd-split'):
    assert splits > 1
    lines = run_fwd_bf16(dev, L, out, use_ws=False)                 # the workspace-less call: one unsplit launch, the same bits
    assert ' splits=1 ' in only(lines, 'gemm_nn_bf16<')


@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('L', [L for L in E.BF16_GENERAL if L.stride == 1], ids=lambda L: L.name)
def test_bf16_general_backprop(dev, L, mask):
  splits = E.bf16_bwd_data_splits(L)
  assert (splits > 1) == (L.name == 'bwd-split')
  lines = run_bwd_data_bf16(dev, L, mask)
  yg = L.y_geo
  assert_general_bf16(L, lines, L.B * L.T, E.npad_of(L.cin), L.W * yg.c_pitch, L.W, yg.c_pitch, splits)


@pytest.mark.parametrize('out', ['f32', 'bf16'])
@pytest.mark.parametrize('L', E.BF16_TILE256, ids=lambda L: L.name)
def test_bf16_pingpong_tile(dev, L, out):
  lines = run_fwd_bf16(dev, L, out)
  xg = L.x_geo
  tile = assert_general_bf16(L, lines, L.B * L.t_out, E.npad_of(L.cout), xg.c_pitch, 1, xg.c_pitch, 1)
  assert tile == 256 and E.bf16_whole_stages(256, 1, xg.c_pitch, xg.c_pitch) == (L.name == 'tile256-whole')


@pytest.mark.parametrize('L', E.BF16_PANEL + E.BF16_PANEL_REFUSED, ids=lambda L: L.name)
def test_bf16_panel_kernel(dev, L):
  """conv_taps_bf16 forward (bias + ReLU) and back-prop with mask; ten taps or a tile grid just below the threshold take the
  general kernel and give the same bits"""
  panel = L in E.BF16_PANEL
  assert E.taps_panel_eligible(L.x_geo, L.y_geo, L.W, L.pad_left) == panel
  assert E.taps_panel_eligible(L.y_geo, L.x_geo, L.W, L.W - 1 - L.pad_left, act_geo(L)) == panel
  for lines in (run_fwd_bf16(dev, L, 'bf16'), run_bwd_data_bf16(dev, L, True)):
    if panel:
      Q = (L.B - 1) * L.x_geo.t_pitch + L.T
      assert only(lines, 'conv_taps_bf16<').startswith('conv_taps_bf16<128,128,64,panel> M={} '.format(Q)), lines
      assert ' taps={} '.format(L.W) in lines[0]
    else:
      only(lines, 'gemm_nn_bf16<128,NP=1>')


# ---- bf16 filter gradient ---------------------------------------------------------------------------------------------------------
def run_wgrad_bf16(dev, L, entry):
  """st_conv1d_nwc_bwd_filter_tr_bf16 (entry = 'tr') or st_conv1d_nwc_bwd_filter_bf16 ('copies'); returns the trace lines and the
  raw dpacked / dbias buffers"""
  from speecht_amd import _lib
  lib = _lib.load()
  d = E.case_data(L)
  E.assert_exact_range(L, 'bwd_filter')
  E.check_geometry(L, 'bwd_filter')
  xg, yg = L.x_geo, L.y_geo
  _, kp, n_pad = E.packed_dims(L.W, xg.c_pitch, L.cout)
  assert lib.st_conv1d_bwd_filter_tr_bf16_slack_rows() == E.SLACK_ROWS
  xb, zb = in_bf16(dev, xg, d['x']), in_bf16(dev, yg, d['dz'])
  dpacked = Guarded(dev, E.guarded_flat_image(kp * n_pad))
  dbias = Guarded(dev, E.guarded_flat_image(n_pad))
  X, Z = t3(xg, P(xb)), t3(yg, P(zb))
  name = 'st_conv1d_nwc_bwd_filter_tr_bf16' if entry == 'tr' else 'st_conv1d_nwc_bwd_filter_bf16'
  query = lib.st_conv1d_bwd_filter_tr_bf16_ws if entry == 'tr' else lib.st_conv1d_bwd_filter_bf16_ws
  need = query(ctypes.byref(X), ctypes.byref(Z), L.W, L.stride, L.pad_left)
  assert need > 0, L.name
  ws = scratch(dev, need)
  lines = traced(lambda: _lib.call(name, ctypes.byref(X), P(xb), ctypes.byref(Z), P(zb), L.W, L.stride, L.pad_left, dpacked.ptr, dbias.ptr,
                                   P(ws), need, None))
  dF, db = E.ref_bwd_filter(d['x'], d['dz'], L.W, L.pad_left, L.stride)
  got_p, got_b = dpacked.read(), dbias.read()
  ok(E.check_guarded_flat(got_p, E.dpacked_ref(dF, xg.c_pitch), what='{} {} dpacked'.format(L.name, entry), shape=(kp, n_pad),
                          kept_from=L.W * xg.c_pitch * n_pad, row_pitch=xg.c_pitch))
  ok(E.check_guarded_flat(got_b, E.padded_vector_bits(db, n_pad), what='{} {} dbias'.format(L.name, entry)))
  return lines, got_p[:E.GUARD_WORDS + L.W * xg.c_pitch * n_pad], got_b


TR_EXPECT = {'tr-unsplit-bias-direct': (1, 8, 2, True), 'tr-split2': (2, 8, 2, True), 'tr-split8-map1': (8, 8, 1, True),
             'tr-pitch48': (1, 8, 2, False), 'tr-pitch128-no-pad-channel': (2, 8, 2, False), 'tr-ring4': (1, 4, 2, True)}


@pytest.mark.parametrize('L', E.BF16_WGRAD_TR, ids=lambda L: L.name)
def test_bf16_filter_gradient_transposing_reads(dev, L):
  """wgrad_tr_bf16 in every split map, ring depth and bias path -- and the entry point with transposed copies on the same geometry:
  bit-identical dpacked and dbias"""
  assert E.tr_eligible(L)
  plan = E.tr_plan(L)
  assert (plan.splits, plan.ring, plan.map, plan.in_tile) == TR_EXPECT[L.name], plan
  lines, p_tr, b_tr = run_wgrad_bf16(dev, L, 'tr')
  xg = L.x_geo
  assert only(lines, 'wgrad_tr_bf16<').startswith('wgrad_tr_bf16<128,128,32> M={} Np={} rows={} stages={} splits={} '.format(
      L.W * xg.c_pitch, E.npad_of(L.cout), plan.rows, plan.stages, plan.splits)), lines
  if L.name == 'tr-split8-map1':
    assert plan.rows >= 2048 and plan.stages % plan.splits
  TR_FORMS.add((plan.ring, plan.map, plan.in_tile, plan.splits > 1))
  lines, p_c, b_c = run_wgrad_bf16(dev, L, 'copies')
  only(lines, 'gemm_nn_bf16<')
  assert np.array_equal(p_tr, p_c) and np.array_equal(b_tr, b_c)


@pytest.mark.parametrize('L', E.BF16_WGRAD_COPIES, ids=lambda L: L.name)
def test_bf16_filter_gradient_transposed_copies(dev, L):
  lines, _, _ = run_wgrad_bf16(dev, L, 'copies')
  line = only(lines, 'gemm_nn_bf16<')
  tile = 256 if L.name == 'copies-tile256' else 128
  assert line.startswith('gemm_nn_bf16<{},NP=1> '.format(tile)), line
  assert (field(line, 'splits') > 1) == (L.name == 'copies-stride2-split'), line
  if L.name == 'copies-other-pitch':
    assert L.x_geo.t_pitch != L.y_geo.t_pitch


# ---- fp32: gemm_nn (forward, back-prop to the input) and gemm_tn (filter gradient) ------------------------------------------------
def run_fwd_f32(dev, L, use_ws, relu=True):
  from speecht_amd import _lib
  lib = _lib.load()
  d = E.case_data(L)
  E.assert_exact_range(L, 'fwd')
  E.check_geometry(L, 'fwd')
  xg, yg = L.x_geo, L.y_geo
  _, kp, n_pad = E.packed_dims(L.W, xg.c_pitch, L.cout)
  x = in_f32(dev, xg, d['x'])
  packed = dev_f32(dev, E.pack_ref(d['F'].astype(np.float32), xg.c_pitch))
  bias = dev_f32(dev, bias_vector(L, d, n_pad))
  y = Guarded(dev, E.guarded_tensor_image(yg))
  X, Y = t3(xg, P(x)), t3(yg, y.ptr)
  need = lib.st_conv1d_fwd_ws(ctypes.byref(X), ctypes.byref(Y), L.W)
  ws = scratch(dev, need) if use_ws and need else None
  lines = traced(lambda: _lib.call('st_conv1d_nwc_fwd_ws_f32', ctypes.byref(X), P(packed), P(bias), L.W, L.stride, L.pad_left, int(relu),
                                   ctypes.byref(Y), P(ws) if ws is not None else None, need if ws is not None else 0, None))
  ref = E.ref_fwd(d['x'], d['F'], d['bias'], L.pad_left, L.stride, relu)
  ok(E.check_guarded_tensor(y.read(), yg, ref, n_pad, what='{} fwd f32 ws={}'.format(L.name, use_ws)))
  return lines


def run_bwd_data_f32(dev, L, mask, one_tap=False):
  """st_conv1d_nwc_bwd_data_bias_f32 (or the one-tap entry point on the forward filters) with dx, mask and dbias_dx"""
  from speecht_amd import _lib
  lib = _lib.load()
  d = E.case_data(L)
  E.assert_exact_range(L, 'bwd_data')
  E.check_geometry(L, 'bwd_data')
  xg, yg, ag = L.x_geo, L.y_geo, act_geo(L)
  n_pad = E.npad_of(L.cin)
  z = in_f32(dev, yg, d['dz'])
  a = in_f32(dev, ag, d['act'])
  packed = E.pack_ref(d['F'].astype(np.float32), xg.c_pitch)
  filt = dev_f32(dev, packed if one_tap else E.flip_transpose_ref(packed, L.W, L.cin, L.cout, xg.c_pitch, yg.c_pitch))
  dx = Guarded(dev, E.guarded_tensor_image(xg))
  db = Guarded(dev, E.guarded_flat_image(n_pad))
  Z, A, X = t3(yg, P(z)), t3(ag, P(a)), t3(xg, dx.ptr)
  need = lib.st_conv1d_bwd_data_bias_ws(ctypes.byref(Z), ctypes.byref(X), L.W)
  ws = scratch(dev, need)
  A_ = ctypes.byref(A) if mask else None
  if one_tap:
    fn = lambda: _lib.call('st_conv1d_1tap_bwd_data_bias_f32', ctypes.byref(Z), P(filt), A_, ctypes.byref(X), db.ptr, P(ws), need, None)
  else:
    fn = lambda: _lib.call('st_conv1d_nwc_bwd_data_bias_f32', ctypes.byref(Z), P(filt), L.W, L.pad_left, A_, ctypes.byref(X), db.ptr, P(ws),
                           need, None)
  lines = traced(fn)
  ref = E.ref_bwd_data(d['dz'], d['F'], L.pad_left, L.T, act=d['act'] if mask else None)
  E.assert_column_sums_exact(ref)
  ok(E.check_guarded_tensor(dx.read(), xg, ref, n_pad, what='{} bwd_data f32 mask={}'.format(L.name, mask)))
  ok(E.check_guarded_flat(db.read(), E.padded_vector_bits(ref.reshape(-1, L.cin).sum(axis=0), n_pad), what=L.name + ' dbias_dx'))
  return lines


def nn_form(n_pad, tiles128, splits, whole):
  if n_pad == 32:
    return 'gemm_nn<128,32,4,1,clamped>'
  if n_pad == 64:
    return 'gemm_nn<128,64,2,2,clamped>'
  if tiles128 >= 192 or splits > 1:
    return 'gemm_nn<128,128,2,2,{}>'.format('fast' if whole else 'clamped')
  return 'gemm_nn<64,128,2,2,clamped>'


F32_FWD_EXPECT = {   # case -> (form with a workspace, its splits)
    'f32-small': ('gemm_nn<128,128,2,2,clamped>', 3), 'f32-np64': ('gemm_nn<128,64,2,2,clamped>', 1), 'f32-np32': ('gemm_nn<128,32,4,1,clamped>', 1),
    'f32-fwd-split-fast': ('gemm_nn<128,128,2,2,fast>', 3), 'f32-fwd-split-midtap': ('gemm_nn<128,128,2,2,fast>', 5),
    'f32-fwd-split-clamped': ('gemm_nn<128,128,2,2,clamped>', 3), 'f32-fwd-split-np32': ('gemm_nn<128,32,4,1,clamped>', 8),
    'f32-pad-left-0': ('gemm_nn<128,128,2,2,clamped>', 3), 'f32-pad-left-w-1': ('gemm_nn<128,128,2,2,clamped>', 3),
    'f32-stride2': ('gemm_nn<128,128,2,2,clamped>', 24),
}


@pytest.mark.parametrize('use_ws', [False, True])
@pytest.mark.parametrize('L', E.F32_NN, ids=lambda L: L.name)
def test_f32_forward(dev, L, use_ws):
  """gemm_nn in its tile forms; with a workspace the reduction splits of fwd_splits (both branches: n_pad 32 at M >= 1 024 rows, and
  few tiles -- 'midtap': 21 k-steps in 5 splits of 5, the last one step long, the second starting at step 5 of 7-tap groups)"""
  xg = L.x_geo
  M, n_pad = L.B * L.t_out, E.npad_of(L.cout)
  nk = E.ceil_div(xg.c_pitch, 32) * L.W
  splits = E.f32_fwd_splits(M, n_pad, nk)
  per = E.ceil_div(nk, splits)
  form, used = F32_FWD_EXPECT[L.name]
  assert E.ceil_div(nk, per) == used
  if L.name == 'f32-fwd-split-midtap':
    assert nk - (used - 1) * per < per and per % L.W
  lines = run_fwd_f32(dev, L, use_ws)
  whole = xg.c_pitch % 32 == 0 and (L.W * xg.c_pitch) % 32 == 0
  want = nn_form(n_pad, E.ceil_div(M, 128) * (n_pad // 128) if n_pad % 128 == 0 else 0, used if use_ws else 1, whole)
  assert not use_ws or want == form
  line = only(lines, 'gemm_nn<')
  assert line.startswith('{} epi=0 splits={} M={} Np={} '.format(want, used if use_ws else 1, M, n_pad)), line


@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('L', [L for L in E.F32_NN if L.stride == 1], ids=lambda L: L.name)
def test_f32_backprop_fused_column_sums(dev, L, mask):
  """unsplit launches collect dbias_dx in the epilogue of the kernel that writes dx; M = 100 rows: the last row tile lies partly
  outside M"""
  yg = L.y_geo
  M, n_pad = L.B * L.T, E.npad_of(L.cin)
  assert E.f32_nn_splits(M, n_pad, E.round_up(L.W * yg.c_pitch, 32)) == 1
  lines = run_bwd_data_f32(dev, L, mask)
  want = nn_form(n_pad, E.ceil_div(M, 128) * (n_pad // 128) if n_pad % 128 == 0 else 0, 1, False)
  assert only(lines, 'gemm_nn<').startswith('{} epi=1 splits=1 M={} Np={} '.format(want, M, n_pad)), lines


@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('L', E.F32_BWD_SPLIT, ids=lambda L: L.name)
def test_f32_backprop_reduction_splits(dev, L, mask):
  """nn_splits 8 (few tiles, 512 k-tiles) and 2 (130 tiles): slabs summed by splitk_epilogue_kernel with the mask, the column sums
  read back from dx"""
  yg = L.y_geo
  M, n_pad = L.B * L.T, E.npad_of(L.cin)
  splits = E.f32_nn_splits(M, n_pad, L.W * yg.c_pitch)
  assert splits == (8 if L.name == 'f32-nn-splits8' else 2)
  lines = run_bwd_data_f32(dev, L, mask)
  assert only(lines, 'gemm_nn<').startswith('gemm_nn<128,128,2,2,fast> epi=1 splits={} M={} Np={} '.format(splits, M, n_pad)), lines


@pytest.mark.parametrize('mask', [False, True])
@pytest.mark.parametrize('L', E.F32_1TAP, ids=lambda L: L.name)
def test_f32_one_tap_backprop_on_forward_filters(dev, L, mask):
  """st_conv1d_1tap_bwd_data_bias_f32: the transposed-operand forms in both tile sizes, unsplit and split"""
  yg = L.y_geo
  assert yg.c_pitch % 32 == 0 and E.npad_of(L.cin) % 128 == 0 and E.npad_of(L.cout) >= yg.c_pitch
  M, n_pad = L.B * L.T, E.npad_of(L.cin)
  splits = E.f32_nn_splits(M, n_pad, yg.c_pitch)
  tiles = E.ceil_div(M, 128) * (n_pad // 128)
  lines = run_bwd_data_f32(dev, L, mask, one_tap=True)
  tile = 64 if tiles < 192 and splits <= 1 else 128
  assert tile == (64 if L.name == 'f32-1tap-bt64' else 128) and (splits > 1) == (L.name == 'f32-1tap-bt128-split')
  assert only(lines, 'gemm_nn<').startswith('gemm_nn<{},128,2,2,fast-bt> epi=1 splits={} M={} Np={} '.format(tile, splits, M, n_pad)), lines


TN_EXPECT = {'tn128-straddle': (128, 1), 'tn64-slabs': (64, 2), 'tn32-tiny5': (32, 1), 'tn128-tiny1': (128, 1), 'tn128-supertile': (128, 1),
             'tn128-stride2-slabs': (128, 2)}


@pytest.mark.parametrize('L', E.F32_TN, ids=lambda L: L.name)
def test_f32_filter_gradient(dev, L):
  """gemm_tn<128 | 64 | 32>, one slab and several, and st_bias_grad_f32 on the same gradient"""
  from speecht_amd import _lib
  lib = _lib.load()
  d = E.case_data(L)
  E.assert_exact_range(L, 'bwd_filter')
  E.check_geometry(L, 'bwd_filter')
  xg, yg = L.x_geo, L.y_geo
  _, kp, n_pad = E.packed_dims(L.W, xg.c_pitch, L.cout)
  x, z = in_f32(dev, xg, d['x']), in_f32(dev, yg, d['dz'])
  dpacked = Guarded(dev, E.guarded_flat_image(kp * n_pad))
  dbias = Guarded(dev, E.guarded_flat_image(n_pad))
  dbias2 = Guarded(dev, E.guarded_flat_image(n_pad))
  X, Z = t3(xg, P(x)), t3(yg, P(z))
  need = lib.st_conv1d_bwd_filter_ws(ctypes.byref(X), ctypes.byref(Z), L.W)
  need2 = lib.st_bias_grad_ws(ctypes.byref(Z))
  ws, ws2 = scratch(dev, need), scratch(dev, need2)

  def fn():
    _lib.call('st_conv1d_nwc_bwd_filter_f32', ctypes.byref(X), ctypes.byref(Z), L.W, L.stride, L.pad_left, dpacked.ptr, dbias.ptr, P(ws), need,
              None)
    _lib.call('st_bias_grad_f32', ctypes.byref(Z), dbias2.ptr, P(ws2), need2, None)
  lines = traced(fn)
  dF, db = E.ref_bwd_filter(d['x'], d['dz'], L.W, L.pad_left, L.stride)
  ok(E.check_guarded_flat(dpacked.read(), E.dpacked_ref(dF, xg.c_pitch), what=L.name + ' dpacked', shape=(kp, n_pad),
                          kept_from=L.W * xg.c_pitch * n_pad, row_pitch=xg.c_pitch))
  ok(E.check_guarded_flat(dbias.read(), E.padded_vector_bits(db, n_pad), what=L.name + ' dbias'))
  ok(E.check_guarded_flat(dbias2.read(), E.padded_vector_bits(db, n_pad), what=L.name + ' st_bias_grad_f32'))
  tile, slabs = TN_EXPECT[L.name]
  M = L.B * L.t_out
  line = only(lines, 'gemm_tn<')
  assert line.startswith('gemm_tn<{}> slabs={} '.format(tile, slabs)) and ' M={} '.format(M) in line, line
  if L.name == 'tn128-supertile':
    assert E.ceil_div(kp, 128) % 8 == 0 and (n_pad // 128) % 8 == 0 and M == 64
  if L.name == 'tn128-straddle':
    assert L.T % 32 and L.T > 32 and M % 32                     # a 32-row step straddles an utterance end; M no multiple of 32


# ---- three planes per operand (bf16x6): gemm_nn_bf16_kernel<..., NP = 3>, its epilogues, slab_epilogue_kernel<3>, the layout kernels ----
# Planes of independent integers (E.make_planes): the result is the six kept plane products, bit for bit, and the output planes are
# split3 of it.  Input planes lie at exactly the plane stride the entry point derives, slack only behind the last one.
X6_FORMS = set()      # (tile, whole stages) of the NP = 3 kernel, from the host expressions


def planes_in(dev, g, planes):
  """three bf16 planes of a tensor, batch * t_pitch * c_pitch apart, SLACK_ROWS zero rows behind the last"""
  img = np.concatenate([E.embed(g, p).reshape(-1) for p in planes] + [np.zeros(E.SLACK_ROWS * g.c_pitch, np.float32)])
  return torch.from_numpy(img).to(dev).to(torch.bfloat16)


def assert_x6(L, lines, M, n_pad, k_valid, taps, c_pitch, splits):
  """the trace line of the NP = 3 kernel: tile and splits as the host mirrors give them; records (tile, whole stages)"""
  tile = E.x6_tile(M, n_pad, splits)
  line = only(lines, 'gemm_nn_bf16<')
  assert line.startswith('gemm_nn_bf16<{},NP=3> splits={} M={} Np={} '.format(tile, splits, M, n_pad)), (L.name, line)
  assert field(line, 'splits') == splits and field(line, 'taps') == taps, line
  X6_FORMS.add((tile, E.x6_whole_stages(tile, taps, c_pitch, k_valid)))
  return tile


def run_fwd_x6(dev, L, relu, planes):
  """st_exp_conv1d_fwd_bf16x6 into y (fp32) and, with `planes`, into the three planes of y"""
  from speecht_amd import _lib
  d = E.case_planes(L, 'fwd')
  E.assert_exact_range6(L, 'fwd')
  E.check_geometry(L, 'fwd')
  assert E.x6_preconditions(L, 'fwd')
  xg, yg = L.x_geo, L.y_geo
  _, kp, n_pad = E.packed_dims(L.W, xg.c_pitch, L.cout)
  xp = planes_in(dev, xg, d['x'])
  wp = dev_bits16(dev, E.filter_planes_fwd(d['F'], xg.c_pitch))
  bias = dev_f32(dev, bias_vector(L, d, n_pad))
  y = Guarded(dev, E.guarded_tensor_image(yg))
  yp = Guarded(dev, E.guarded_planes_image(yg)) if planes else None
  X, Y = t3(xg, P(xp)), t3(yg, y.ptr)
  lines = traced(lambda: _lib.call('st_exp_conv1d_fwd_bf16x6', ctypes.byref(X), P(xp), P(wp), P(bias), L.W, L.stride, L.pad_left, int(relu),
                                   ctypes.byref(Y), yp.ptr if planes else None, None))
  ref = E.case_ref6(L, 'fwd')
  ref = np.maximum(ref, 0) if relu else ref
  what = '{} fwd x6 relu={} planes={}'.format(L.name, relu, planes)
  ok(E.check_guarded_tensor(y.read(), yg, ref, n_pad, what=what))
  if planes:
    ok(E.check_guarded_planes(yp.read(), yg, ref, n_pad, what=what))
  return lines


def run_bwd_data_x6(dev, L, mask, planes, use_ws=True):
  """st_exp_conv1d_bwd_data_bf16x6 with the fp32 mask tensor or without, into dx and, with `planes`, into its three planes"""
  from speecht_amd import _lib
  lib = _lib.load()
  d = E.case_planes(L, 'bwd_data')
  E.assert_exact_range6(L, 'bwd_data', E.X6_SCALE[L.name])
  E.check_geometry(L, 'bwd_data')
  assert E.x6_preconditions(L, 'bwd_data')
  xg, yg, ag = L.x_geo, L.y_geo, act_geo(L)
  n_pad = E.npad_of(L.cin)
  zp = planes_in(dev, yg, d['dz'])
  a = in_f32(dev, ag, d['act'])
  wp = dev_bits16(dev, E.filter_planes_bwd(d['F'], xg.c_pitch, yg.c_pitch))
  dx = Guarded(dev, E.guarded_tensor_image(xg))
  dxp = Guarded(dev, E.guarded_planes_image(xg)) if planes else None
  Z, A, X = t3(yg, P(zp)), t3(ag, P(a)), t3(xg, dx.ptr)
  need = lib.st_exp_conv1d_bwd_data_bf16x6_ws(ctypes.byref(Z), ctypes.byref(X), L.W)
  assert (need > 0) == (E.bf16_bwd_data_splits(L) > 1)
  ws = scratch(dev, need) if use_ws and need else None
  lines = traced(lambda: _lib.call('st_exp_conv1d_bwd_data_bf16x6', ctypes.byref(Z), P(zp), P(wp), L.W, L.pad_left,
                                   ctypes.byref(A) if mask else None, ctypes.byref(X), dxp.ptr if planes else None,
                                   P(ws) if ws is not None else None, need if ws is not None else 0, None))
  ref = E.case_ref6(L, 'bwd_data')
  ref = ref * (d['act'] > 0) if mask else ref
  what = '{} bwd_data x6 mask={} planes={} ws={}'.format(L.name, mask, planes, use_ws)
  ok(E.check_guarded_tensor(dx.read(), xg, ref, n_pad, what=what))
  if planes:
    ok(E.check_guarded_planes(dxp.read(), xg, ref, n_pad, what=what))
  return lines


def run_wgrad_x6(dev, L):
  """st_exp_conv1d_bwd_filter_bf16x6 on transposed planes laid out as modes/bf16x6.py produces them"""
  from speecht_amd import _lib
  d = E.case_planes(L, 'bwd_filter')
  E.assert_exact_range6(L, 'bwd_filter')
  E.check_geometry(L, 'bwd_filter')
  assert E.x6_preconditions(L, 'bwd_filter')
  xg, tq = L.x_geo, E.wgrad6_tq(L)
  _, kp, n_pad = E.packed_dims(L.W, xg.c_pitch, L.cout)
  xt, zt = E.wgrad6_operands(L, d['x'], d['dz'])
  xtd, ztd = dev_bits16(dev, xt), dev_bits16(dev, zt)
  dpacked = Guarded(dev, E.guarded_flat_image(kp * n_pad))
  lines = traced(lambda: _lib.call('st_exp_conv1d_bwd_filter_bf16x6', P(xtd), P(ztd), L.B, tq, L.W, xg.c_pitch, xg.halo - L.pad_left, L.cout,
                                   dpacked.ptr, None))
  ok(E.check_guarded_flat(dpacked.read(), E.dpacked_ref(E.case_ref6(L, 'bwd_filter'), xg.c_pitch), what=L.name + ' x6 dpacked', shape=(kp, n_pad),
                          kept_from=L.W * xg.c_pitch * n_pad, row_pitch=xg.c_pitch))
  return lines


X6_FWD_RUNS = [(L, relu, planes) for L in E.X6_FWD for relu in (False, True) for planes in (False, True)]      # case-major: one reference each
X6_BWD_RUNS = [(L, mask, planes) for L in E.X6_BWD_DATA for mask in (False, True) for planes in (False, True)]
run_id = lambda names: lambda r: '{}-{}{}-{}{}'.format(r[0].name, names[0], int(r[1]), names[1], int(r[2]))


@pytest.mark.parametrize('L,relu,planes', X6_FWD_RUNS, ids=list(map(run_id(('relu', 'planes')), X6_FWD_RUNS)))
def test_x6_forward(dev, L, relu, planes):
  """the 128 tile with one, two and three 32-deep stages, clamped stages, both padding extremes, fewer frames than taps, stride 2; the
  256 tile (ring of three, ping-pong) with one to four 16-deep stages at the threshold of 192 tiles"""
  lines = run_fwd_x6(dev, L, relu, planes)
  xg = L.x_geo
  tile = assert_x6(L, lines, L.B * L.t_out, E.npad_of(L.cout), L.W * xg.c_pitch, L.W, xg.c_pitch, 1)
  assert tile == (256 if L.name.startswith('x6-t256') else 128)


@pytest.mark.parametrize('L,mask,planes', X6_BWD_RUNS, ids=list(map(run_id(('mask', 'planes')), X6_BWD_RUNS)))
def test_x6_backprop(dev, L, mask, planes):
  """in-kernel epilogue of both tiles and, in the split case, slab_epilogue_kernel<3>; without a workspace the split case falls back
  to one launch and gives the same bits"""
  splits = E.bf16_bwd_data_splits(L)
  assert splits == (2 if L.name == 'x6-bwd-split' else 1)
  lines = run_bwd_data_x6(dev, L, mask, planes)
  yg = L.y_geo
  tile = assert_x6(L, lines, L.B * L.T, E.npad_of(L.cin), L.W * yg.c_pitch, L.W, yg.c_pitch, splits)
  assert tile == (256 if L.name == 'x6-bwd-t256' else 128)
  if splits > 1:
    lines = run_bwd_data_x6(dev, L, mask, planes, use_ws=False)
    assert_x6(L, lines, L.B * L.T, E.npad_of(L.cin), L.W * yg.c_pitch, L.W, yg.c_pitch, 1)


@pytest.mark.parametrize('L', E.X6_BWD_FILTER, ids=lambda L: L.name)
def test_x6_filter_gradient(dev, L):
  lines = run_wgrad_x6(dev, L)
  xg = L.x_geo
  tile = assert_x6(L, lines, L.W * xg.c_pitch, E.npad_of(L.cout), L.B * E.wgrad6_tq(L), 1, xg.c_pitch, 1)
  assert tile == (256 if L.name == 'x6-wgrad-t256' else 128)


def check_planes_flat(after, want, what, shape):
  """check_guarded_flat for planes that may be non-finite: where the model gives a NaN the kernel must have written one (any NaN but
  the fill pattern); finite values, zeros and infinities compare by bits, so infinities by sign"""
  after = np.array(after, dtype=np.uint16)
  body = after[E.GUARD_WORDS:-E.GUARD_WORDS]
  want = np.asarray(want, dtype=np.uint16).reshape(-1)
  is_nan = lambda b: (b & np.uint16(0x7FFF)) > np.uint16(0x7F80)
  agree = is_nan(want) & is_nan(body) & (body != E.FILL16)
  body[agree] = want[agree]
  return E.check_guarded_flat(after, want, bits16=True, what=what, shape=shape)


SPECIAL_F32 = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0xFF7F7FFF,
                        0xFF7F8000, 0xFF7F8001, 0x7F7FFFFF, 0xFF7FFFFF], dtype=np.uint32).view(np.float32)


@pytest.mark.parametrize('n', [4, 1020, 4 * (4096 * 256) + 4])
def test_split3_planes(dev, n):
  """st_exp_split3_bf16 against E.split3 on floats with full mantissas (exponents -100..100), +-0, +-inf, NaN and both sides of the bit
  pattern 0x7F7F8000 where bf16(x) overflows; the largest n enters the grid-stride loop (4096 blocks of 256 lanes of 4 elements)"""
  from speecht_amd._lib import call
  src = E.random_f32(np.random.default_rng(n), n)
  k = min(SPECIAL_F32.size, n - 2)
  src[1:1 + k] = SPECIAL_F32[:k]
  src[n - 1 - k:n - 1] = SPECIAL_F32[:k]
  want = E.plane_bits(E.split3(src))
  assert np.count_nonzero(want[2] & 0x7FFF) > 0.4 * n
  out = Guarded(dev, E.guarded_flat_image(3 * n, bits16=True))
  sd = dev_f32(dev, src)
  call('st_exp_split3_bf16', P(sd), n, out.ptr, None)
  torch.cuda.synchronize()
  ok(check_planes_flat(out.read(), want, 'split3 n={}'.format(n), (3, n)))


def test_split3_of_nothing_succeeds_and_writes_nothing(dev):
  from speecht_amd import _lib
  lib = _lib.load()
  image = E.guarded_flat_image(48, bits16=True)
  out = Guarded(dev, image)
  sd = dev_f32(dev, np.ones(16, np.float32))
  assert lib.st_exp_split3_bf16(P(sd), 0, out.ptr, None) == 0
  torch.cuda.synchronize()
  assert np.array_equal(out.read(), image)


@pytest.mark.parametrize('k_pad,n_pad', [(32, 32), (96, 128), (2080, 160)])
def test_split3_transpose_planes(dev, k_pad, n_pad):
  """st_exp_split3_transpose_bf16: planes 3 x [n_pad][k_pad] of packed [k_pad][n_pad]"""
  from speecht_amd._lib import call
  packed = E.random_f32(np.random.default_rng(k_pad + n_pad), k_pad * n_pad).reshape(k_pad, n_pad)
  want = E.plane_bits(E.split3(packed.T))
  out = Guarded(dev, E.guarded_flat_image(3 * n_pad * k_pad, bits16=True))
  pd = dev_f32(dev, packed)
  call('st_exp_split3_transpose_bf16', P(pd), k_pad, n_pad, out.ptr, None)
  torch.cuda.synchronize()
  ok(E.check_guarded_flat(out.read(), want, bits16=True, what='split3_transpose', shape=(3, n_pad, k_pad)))


@pytest.mark.parametrize('c_pitch,rows,row0,t_pitch', [(48, 45, 2, 50), (256, 64, 1, 66)])
def test_transpose_split3_planes(dev, c_pitch, rows, row0, t_pitch):
  """st_exp_transpose_split3_bf16: plane[c][b * tq + j] = split3(t[b][row0 + j][c]) for j < rows; the frames from `rows` to tq and the
  slack behind every plane keep the fill pattern"""
  from speecht_amd._lib import call
  batch, tq = 3, 64
  plane_elems = c_pitch * batch * tq + E.XT_SLACK
  g = E.Geo(batch, rows, c_pitch, row0, t_pitch, c_pitch)
  src = E.random_f32(np.random.default_rng(c_pitch), batch * t_pitch * c_pitch).reshape(batch, t_pitch, c_pitch)
  bits = E.plane_bits(E.split3(src))
  want = np.stack([E.transposed_ref(b, row0, rows, tq, c_pitch, E.XT_SLACK, fill=E.FILL16) for b in bits])
  assert want.shape == (3, plane_elems) and (rows == tq or np.count_nonzero(want == E.FILL16) > 3 * E.XT_SLACK)
  out = Guarded(dev, E.guarded_flat_image(3 * plane_elems, bits16=True))
  sd = dev_f32(dev, src)
  T = t3(g, P(sd))
  call('st_exp_transpose_split3_bf16', ctypes.byref(T), row0, rows, tq, plane_elems, out.ptr, None)
  torch.cuda.synchronize()
  ok(E.check_guarded_flat(out.read(), want, bits16=True, what='transpose_split3', shape=(3, plane_elems)))


def test_x6_filter_gradient_chain_as_the_mode_calls_it(dev):
  """st_exp_transpose_split3_bf16 of integer tensors (m = l = 0), then st_exp_conv1d_bwd_filter_bf16x6 on its planes, with the arguments
  of modes/bf16x6.py: the two agree on tq, x_first_row and the slack, and the product is E.ref_bwd_filter"""
  from speecht_amd import _lib
  L = E.X6_BWD_FILTER[3]
  d = E.case_data(L)
  E.assert_exact_range(L, 'bwd_filter')
  xg, yg, tq = L.x_geo, L.y_geo, E.wgrad6_tq(L)
  _, kp, n_pad = E.packed_dims(L.W, xg.c_pitch, L.cout)
  red = L.B * tq
  x, z = in_f32(dev, xg, d['x']), in_f32(dev, yg, d['dz'])
  xt = torch.zeros(3 * (xg.c_pitch * red + E.XT_SLACK) + OPERAND_SLACK, dtype=torch.bfloat16, device=dev)       # zero planes, as the engine's
  zt = torch.zeros(3 * n_pad * red + OPERAND_SLACK, dtype=torch.bfloat16, device=dev)
  dpacked = Guarded(dev, E.guarded_flat_image(kp * n_pad))
  X, Z = t3(xg, P(x)), t3(yg, P(z))

  def fn():
    _lib.call('st_exp_transpose_split3_bf16', ctypes.byref(X), 0, xg.t_pitch, tq, xg.c_pitch * red + E.XT_SLACK, P(xt), None)
    _lib.call('st_exp_transpose_split3_bf16', ctypes.byref(Z), yg.halo, yg.frames, tq, n_pad * red, P(zt), None)
    _lib.call('st_exp_conv1d_bwd_filter_bf16x6', P(xt), P(zt), L.B, tq, L.W, xg.c_pitch, xg.halo - L.pad_left, L.cout, dpacked.ptr, None)
  lines = traced(fn)
  only(lines, 'gemm_nn_bf16<128,NP=3>')
  dF, _ = E.ref_bwd_filter(d['x'], d['dz'], L.W, L.pad_left)
  ok(E.check_guarded_flat(dpacked.read(), E.dpacked_ref(dF, xg.c_pitch), what='x6 filter gradient chain', shape=(kp, n_pad),
                          kept_from=L.W * xg.c_pitch * n_pad, row_pitch=xg.c_pitch))
  planes = xt.cpu().view(torch.int16).numpy().view(np.uint16)[:3 * (xg.c_pitch * red + E.XT_SLACK)].reshape(3, -1)
  assert np.array_equal(planes[0], E.transposed_ref(E.bf16_bits(E.embed(xg, d['x'])), 0, xg.t_pitch, tq, xg.c_pitch, E.XT_SLACK))
  assert not (planes[1:] & 0x7FFF).any()


def test_x6_entry_points_refuse_what_they_cannot_run(dev):
  """n_pad 32 forward, n_pad 64 in back-prop to the input, tq = 48 in the filter gradient, n = 6 in split3: an error status, no launch,
  and every output buffer as it was"""
  from speecht_amd import _lib
  lib = _lib.load()

  def refused(fn, *outs):
    before = [o.read() for o in outs]
    with _lib.launch_trace() as tr:
      rc = fn()
    torch.cuda.synchronize()
    assert rc != 0 and tr.lines == [] and lib.st_last_error()
    for o, b in zip(outs, before):
      assert np.array_equal(o.read(), b)

  L = E.layer('x6-refused-fwd', 2, 50, 40, 29, 7, xcp=48)
  assert E.npad_of(L.cout) == 32 and not E.x6_preconditions(L, 'fwd')
  d = E.make_planes(L)
  xg, yg = L.x_geo, L.y_geo
  xp = planes_in(dev, xg, d['x'])
  wp = dev_bits16(dev, E.filter_planes_fwd(d['F'], xg.c_pitch))
  bias = dev_f32(dev, bias_vector(L, d, 32))
  y, yp = Guarded(dev, E.guarded_tensor_image(yg)), Guarded(dev, E.guarded_planes_image(yg))
  X, Y = t3(xg, P(xp)), t3(yg, y.ptr)
  refused(lambda: lib.st_exp_conv1d_fwd_bf16x6(ctypes.byref(X), P(xp), P(wp), P(bias), L.W, 1, L.pad_left, 1, ctypes.byref(Y), yp.ptr, None), y, yp)

  L = E.layer('x6-refused-bwd', 2, 50, 40, 100, 7, xcp=48)
  assert E.npad_of(L.cin) == 64 and not E.x6_preconditions(L, 'bwd_data')
  d = E.make_planes(L)
  xg, yg = L.x_geo, L.y_geo
  zp = planes_in(dev, yg, d['dz'])
  wp = dev_bits16(dev, E.filter_planes_bwd(d['F'], xg.c_pitch, yg.c_pitch))
  dx, dxp = Guarded(dev, E.guarded_tensor_image(xg)), Guarded(dev, E.guarded_planes_image(xg))
  Z, X = t3(yg, P(zp)), t3(xg, dx.ptr)
  refused(lambda: lib.st_exp_conv1d_bwd_data_bf16x6(ctypes.byref(Z), P(zp), P(wp), L.W, L.pad_left, None, ctypes.byref(X), dxp.ptr, None, 0, None),
          dx, dxp)

  L = E.X6_BWD_FILTER[0]
  d = E.case_planes(L, 'bwd_filter')
  xg = L.x_geo
  _, kp, n_pad = E.packed_dims(L.W, xg.c_pitch, L.cout)
  xt, zt = E.wgrad6_operands(L, d['x'], d['dz'])
  xtd, ztd = dev_bits16(dev, xt), dev_bits16(dev, zt)
  dpacked = Guarded(dev, E.guarded_flat_image(kp * n_pad))
  assert E.wgrad6_tq(L) > 48
  refused(lambda: lib.st_exp_conv1d_bwd_filter_bf16x6(P(xtd), P(ztd), L.B, 48, L.W, xg.c_pitch, xg.halo - L.pad_left, L.cout, dpacked.ptr, None), dpacked)

  out = Guarded(dev, E.guarded_flat_image(24, bits16=True))
  sd = dev_f32(dev, np.ones(8, np.float32))
  refused(lambda: lib.st_exp_split3_bf16(P(sd), 6, out.ptr, None), out)


def test_every_required_form_ran():
  """Runs last: the union of the trace forms of this module's cases is the required list, the bf16 general kernel ran in both tiles
  with whole and with clamped stages, the transposing filter gradient in both ring depths, both maps and both bias paths, the
  three-plane kernel in both tiles with whole stages and in the 128 tile with clamped ones (its 256 tile has no clamped form to reach:
  E.x6_whole_stages)."""
  for case, line in COVERAGE:
    print('{:<75} {}'.format(case, line))
  assert SEEN == REQUIRED, (sorted(SEEN - REQUIRED), sorted(REQUIRED - SEEN))
  assert BF16_FORMS == {(128, True), (128, False), (256, True), (256, False)}, BF16_FORMS
  assert {f[0] for f in TR_FORMS} == {4, 8} and {f[1] for f in TR_FORMS} == {1, 2} and {f[2] for f in TR_FORMS} == {True, False}
  assert {f[3] for f in TR_FORMS} == {True, False}
  assert X6_FORMS == {(128, True), (128, False), (256, True)}, X6_FORMS
