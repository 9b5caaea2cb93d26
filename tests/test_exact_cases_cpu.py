"""tests/exact_cases.py without a GPU: the integer reference against the oracle, bf16 rounding against torch, the data's lack of blind
spots, the exactness and geometry conditions of every GPU case, and the comparison's own ability to see one wrong element; for the
three-plane (bf16x6) cases the numpy model of split3, the six-term references against a direct sum over planes, the kernel forms the
host mirrors name, and the share of nonzero elements in the reference's m and l planes."""
import numpy as np
import pytest

from oracle import w2l_oracle as O
from tests import exact_cases as E

ALL_LAYERS = [L for cases, _ in E.CALLS for L in cases]


@pytest.mark.parametrize('W,stride,T', [(1, 1, 9), (2, 1, 9), (7, 1, 5), (7, 1, 20), (8, 1, 13), (4, 2, 11), (5, 2, 12), (48, 2, 31)])
def test_integer_reference_equals_the_oracle_at_same_padding(W, stride, T):
  L = E.layer('oracle-%d-%d-%d' % (W, stride, T), 3, T, 5, 7, W, stride=stride)
  d = E.make_data(L)
  x, F, bias, dz = (d[k].astype(np.float64) for k in ('x', 'F', 'bias', 'dz'))
  for relu in (False, True):
    assert np.array_equal(E.ref_fwd(d['x'], d['F'], d['bias'], L.pad_left, stride, relu), O.conv1d_same_fwd(x, F, bias, stride, relu))
  dx, dF, db = O.conv1d_same_bwd(x, F, None, dz, stride, relu=False)
  assert np.array_equal(E.ref_bwd_data(d['dz'], d['F'], L.pad_left, T, stride), dx)
  assert np.array_equal(E.ref_bwd_data(d['dz'], d['F'], L.pad_left, T, stride, act=d['act']), dx * (d['act'] > 0))
  got_dF, got_db = E.ref_bwd_filter(d['x'], d['dz'], W, L.pad_left, stride)
  assert np.array_equal(got_dF, dF) and np.array_equal(got_db, db)
  assert (d['act'] <= 0).any() and (d['act'] > 0).any()


def test_bf16_round_equals_torch():
  torch = pytest.importorskip('torch')
  rng = np.random.default_rng(11)
  for v in (np.arange(1 << 16, dtype=np.float32), rng.integers(0, 1 << 24, 1 << 18).astype(np.float32),
            -rng.integers(0, 1 << 24, 1 << 18).astype(np.float32)):
    want = torch.from_numpy(v).to(torch.bfloat16)
    assert np.array_equal(E.bf16_bits(v), want.view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(O.bf16_round(v), want.to(torch.float64).numpy())
  # ties occur constantly above 256: odd multiples of half a step, rounded to the even neighbour
  assert E.bf16_bits(np.float32(257.0)) == E.bf16_bits(np.float32(256.0)) and E.bf16_bits(np.float32(259.0)) == E.bf16_bits(np.float32(260.0))


def small_copy(L):
  """the same generator (name, widths, channels, stride, padding) on few frames: the properties below do not depend on the length"""
  return L._replace(B=min(L.B, 2), T=min(L.T, 2 * L.W + 3))


@pytest.mark.parametrize('L', ALL_LAYERS, ids=lambda L: L.name)
def test_data_has_no_blind_spot(L):
  """Changing any single interior element of x, F or dz by one changes every reference output that depends on it: no operand value
  is zero, and every element meets at least one tap inside the tensor."""
  S = small_copy(L)
  d = E.make_data(S)
  for a in (d['x'], d['dz']):
    assert set(np.unique(a)) <= {-3, -2, -1, 1, 2, 3}
  assert set(np.unique(d['F'])) <= {-2, -1, 1, 2} and abs(d['bias']).max() <= 4 and (d['act'] <= 0).any()
  pl, s = S.pad_left, S.stride
  y0 = E.ref_fwd(d['x'], d['F'], d['bias'], pl, s)
  dx0 = E.ref_bwd_data(d['dz'], d['F'], pl, S.T, s)
  dF0, db0 = E.ref_bwd_filter(d['x'], d['dz'], S.W, pl, s)
  rng = np.random.default_rng(S.seed + 1)
  for _ in range(2):
    for name in ('x', 'F', 'dz'):
      a = d[name].astype(np.int64)
      pos = tuple(int(rng.integers(0, n)) for n in a.shape)
      a[pos] += 1
      p = dict(d, **{name: a})
      y = E.ref_fwd(p['x'], p['F'], p['bias'], pl, s)
      dx = E.ref_bwd_data(p['dz'], p['F'], pl, S.T, s)
      dF, db = E.ref_bwd_filter(p['x'], p['dz'], S.W, pl, s)
      if name == 'x':
        reaches = any((pos[1] + pl - w) % s == 0 and 0 <= (pos[1] + pl - w) // s < S.t_out for w in range(S.W))
        assert reaches or s > 1                          # stride 1: every frame meets a tap
        assert (not np.array_equal(y, y0)) == reaches and (not np.array_equal(dF, dF0)) == reaches and np.array_equal(dx, dx0)
      elif name == 'F':
        reaches = any(0 <= t * s + pos[0] - pl < S.T for t in range(S.t_out))
        assert (not np.array_equal(y, y0)) == reaches and (not np.array_equal(dx, dx0)) == reaches and np.array_equal(dF, dF0)
      else:
        assert not np.array_equal(db, db0) and not np.array_equal(dx, dx0) and not np.array_equal(dF, dF0) and np.array_equal(y, y0)


def test_every_gpu_case_is_exact_and_fits_its_entry_point():
  names = [L.name for L in ALL_LAYERS]
  assert len(set(names)) == len(names)
  for L, what in E.all_calls():
    E.assert_exact_range(L, what)
    E.check_geometry(L, what)
    assert E.geo_ok(L.x_geo) and E.geo_ok(L.y_geo)
  for L in E.BF16_PANEL + E.BF16_PANEL_REFUSED:
    assert L.x_geo.t_pitch == L.y_geo.t_pitch and L.x_geo.c_pitch == 256 and L.y_geo.c_pitch == 256
    panel = L in E.BF16_PANEL
    assert E.taps_panel_eligible(L.x_geo, L.y_geo, L.W, L.pad_left) == panel
    assert E.taps_panel_eligible(L.y_geo, L.x_geo, L.W, L.W - 1 - L.pad_left, L.x_geo) == panel
  q = [(L.B - 1) * L.x_geo.t_pitch + L.T for L in E.BF16_PANEL[:3]]
  assert all(8064 < v < 8064 + 128 for v in q)                                    # just above the threshold of 64 row tiles
  for L in E.BF16_WGRAD_TR:
    assert E.tr_eligible(L) and L.x_geo.halo != L.y_geo.halo
  for L in E.BF16_TILE256:
    assert E.bf16_tile(L.B * L.T, E.npad_of(L.cout), 1) == 256 and (L.B * L.T) % 256
    assert E.bf16_tile(L.B * L.T - 256, E.npad_of(L.cout), 1) == 128                 # the smallest row count that reaches the tile
  for L in E.F32_1TAP:
    assert L.y_geo.c_pitch % 32 == 0 and E.npad_of(L.cin) % 128 == 0 and E.npad_of(L.cout) >= L.y_geo.c_pitch


@pytest.mark.parametrize('L', [L for L in E.F32_NN + E.F32_1TAP + E.F32_BWD_SPLIT[:1] if L.stride == 1], ids=lambda L: L.name)
def test_column_sums_of_dx_are_exact(L):
  """the second-level sums of st_conv1d_nwc_bwd_data_bias_f32 (the largest case asserts this where it computes its reference)"""
  d = E.make_data(L)
  E.assert_column_sums_exact(E.ref_bwd_data(d['dz'], d['F'], L.pad_left, L.T))


def test_layout_formulas_invert_each_other():
  rng = np.random.default_rng(2)
  W, cin, cout, cpi, cpo = 3, 5, 7, 16, 16
  F = rng.standard_normal((W, cin, cout)).astype(np.float32)
  Pk = E.pack_ref(F, cpi)
  assert Pk.shape == (64, 32) and np.count_nonzero(Pk) == F.size and Pk[2 * cpi + 4, 6] == F[2, 4, 6]
  Q = E.flip_transpose_ref(Pk, W, cin, cout, cpi, cpo)
  assert Q.shape == (64, 32) and Q[0 * cpo + 6, 4] == F[2, 4, 6] and np.count_nonzero(Q) == F.size
  B = E.filters_bwd_bf16_ref(Pk, W, cin, cout, cpi, cpo)
  assert B.shape == (32, 64) and B[4, 0 * cpo + 6] == E.bf16_bits(F[2, 4, 6])
  assert np.array_equal(E.filters_bf16_ref(Pk)[:cout, :W * cpi].reshape(cout, W, cpi)[:, :, :cin], E.bf16_bits(F.transpose(2, 0, 1)))


@pytest.mark.parametrize('bits16', [False, True])
def test_comparison_sees_one_wrong_element(bits16):
  g = E.Geo(2, 5, 20, 3, 10, 32)
  ref = np.arange(2 * 5 * 20).reshape(2, 5, 20) * 3 - 250
  bits = E.bf16_bits if bits16 else E.f32_bits
  good = E.guarded_tensor_image(g, bits16)
  body = good[E.GUARD_WORDS:-E.GUARD_WORDS].reshape(2, 10, 32)
  body[:, 3:8, :20] = bits(ref)
  body[:, 3:8, 20:32] = 0
  assert E.check_guarded_tensor(good, g, ref, 128, bits16) is None
  for where in [(E.GUARD_WORDS - 1,), (good.size - E.GUARD_WORDS,), (E.GUARD_WORDS + 2 * 32 + 1,), (E.GUARD_WORDS + 3 * 32 + 25,),
                (E.GUARD_WORDS + (10 + 7) * 32 + 19,)]:
    bad = good.copy()
    bad[where] ^= 1
    assert E.check_guarded_tensor(bad, g, ref, 128, bits16) is not None, where
  # a channel pitch beyond n_pad: those channels keep the fill pattern
  wide = E.guarded_tensor_image(g, bits16)
  wbody = wide[E.GUARD_WORDS:-E.GUARD_WORDS].reshape(2, 10, 32)
  wbody[:, 3:8, :20] = bits(ref)
  assert E.check_guarded_tensor(wide, g, ref, 20, bits16) is None and E.check_guarded_tensor(good, g, ref, 20, bits16) is not None
  flat = E.guarded_flat_image(64, bits16)
  want = np.arange(64).astype(flat.dtype)
  flat[E.GUARD_WORDS:E.GUARD_WORDS + 48] = want[:48]
  assert E.check_guarded_flat(flat, want, bits16, kept_from=48) is None
  flat[E.GUARD_WORDS + 50] = 0
  assert E.check_guarded_flat(flat, want, bits16, kept_from=48) is not None
  flat[E.GUARD_WORDS + 48:E.GUARD_WORDS + 64] = 0
  assert E.check_guarded_flat(flat, want, bits16, kept_from=48) is None
  flat[E.GUARD_WORDS + 7] ^= 1
  assert 'first at' in E.check_guarded_flat(flat, want, bits16, kept_from=48)


# ---- three planes per operand (bf16x6) --------------------------------------------------------------------------------------------
X6_LAYERS = [(L, what) for cases, what in E.X6_CALLS for L in cases]


def test_split3_round_trip_and_domain():
  x = E.random_f32(np.random.default_rng(3), 100000)
  h, m, l = E.split3(x)
  assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), x.astype(np.float64))
  for p in (h, m, l):                                              # every plane is a bf16 value
    assert np.array_equal(O.bf16_round(p), p.astype(np.float64))
  assert np.count_nonzero(m) > 0.98 * x.size and np.count_nonzero(l) > 0.95 * x.size             # real floats fill all three planes
  edge = np.array([0x7F7F7FFF, 0x7F7F8000, 0xFF7F7FFF, 0xFF7F8000, 0x7F800000, 0x00000000, 0x80000000], dtype=np.uint32).view(np.float32)
  h, m, l = E.split3(edge)
  assert np.isfinite([h[0], m[0], l[0], h[2], m[2], l[2]]).all() and float(h[0]) + float(m[0]) + float(l[0]) == float(edge[0])
  assert h[1] == np.inf and m[1] == -np.inf and np.isnan(l[1]) and h[3] == -np.inf and m[3] == np.inf and np.isnan(l[3])
  assert h[4] == np.inf and np.isnan(m[4]) and np.isnan(l[4])
  assert E.plane_bits((h, m, l))[:, 5:].tolist() == [[0, 0x8000], [0, 0], [0, 0]]
  assert E.canonical16(np.array([0xFFC0, 0x7F81, 0x7F80, 0xFF80, 0x1234], np.uint16)).tolist() == [0x7FC0, 0x7FC0, 0x7F80, 0xFF80, 0x1234]


def windows(x, W, pad_left, stride, t_out):
  """x [B,T,c] -> [B,t_out,W,c], zero outside the tensor"""
  B, T, c = x.shape
  xp = np.zeros((B, pad_left + T + W + stride, c), dtype=np.int64)
  xp[:, pad_left:pad_left + T] = x
  return np.stack([xp[:, w:w + (t_out - 1) * stride + 1:stride] for w in range(W)], axis=2)


@pytest.mark.parametrize('W,stride,T,scale,positive', [(1, 1, 9, 1, False), (3, 1, 9, 64, True), (4, 2, 11, 1, False), (7, 1, 5, 8, True)])
def test_six_term_references_equal_a_direct_sum_over_planes(W, stride, T, scale, positive):
  L = E.layer('six-%d-%d-%d' % (W, stride, T), 2, T, 5, 7, W, stride=stride)
  d = E.make_planes(L, scale, positive)
  x, F, dz = (d[k].astype(np.int64) for k in ('x', 'F', 'dz'))
  assert set(np.unique(np.abs(F[0]))) <= {scale, 2 * scale} and set(np.unique(np.abs(F[1:]))) <= {1, 2}
  assert (x[0] > 0).all() == positive and (F[0] > 0).all() == positive and (dz[0] > 0).all() == positive and (x[1] < 0).any()
  assert (np.abs(d['bias']) >= 1 << 20).all() and (np.abs(d['bias']) < 1 << 23).all() and (d['bias'] < 0).any() and (d['bias'] > 0).any()
  xw = np.stack([windows(p, W, L.pad_left, stride, L.t_out) for p in x])                        # [3,B,t,W,c]
  pair = lambda a, b: np.einsum('btwc,wco->bto', xw[a], F[b])
  six = sum(pair(a, b) for a, b in E.PAIRS6)
  assert np.array_equal(E.ref_fwd6(d['x'], d['F'], d['bias'], L.pad_left, stride), six + d['bias'])
  assert np.array_equal(E.ref_fwd6(d['x'], d['F'], d['bias'], L.pad_left, stride, relu=True), np.maximum(six + d['bias'], 0))
  # each kept term matters, each dropped term would show
  for a in range(3):
    for b in range(3):
      assert np.mean(pair(a, b) != 0) > 0.5, (a, b)
  assert sorted(E.PAIRS6) == sorted((a, b) for a in range(3) for b in range(3) if a + b <= 2)
  gw = np.einsum('bto,btwc->wco', dz[0], xw[0])
  assert np.array_equal(E.ref_bwd_filter(d['x'][0], d['dz'][0], W, L.pad_left, stride)[0], gw)
  assert np.array_equal(E.ref_bwd_filter6(d['x'], d['dz'], W, L.pad_left, stride),
                        sum(np.einsum('bto,btwc->wco', dz[b], xw[a]) for a, b in E.PAIRS6))
  if stride == 1:
    zw = np.stack([windows(p, W, W - 1 - L.pad_left, 1, T) for p in dz])                        # dx[u] = sum_w dz[u - w + pad_left] F[w]
    dx = sum(np.einsum('buwo,wco->buc', zw[a], F[b][::-1]) for a, b in E.PAIRS6)
    assert np.array_equal(E.ref_bwd_data6(d['dz'], d['F'], L.pad_left, T), dx)
    assert np.array_equal(E.ref_bwd_data6(d['dz'], d['F'], L.pad_left, T, act=d['act']), dx * (d['act'] > 0))


def test_six_and_nine_terms_differ_almost_everywhere():
  L = E.layer('six-nine', 1, 100, 64, 128, 1)
  d = E.make_planes(L)
  six = E.ref_fwd6(d['x'], d['F'], 0, 0)
  nine = sum(E.ref_fwd(d['x'][a], d['F'][b], 0, 0) for a in range(3) for b in range(3))
  assert np.mean(six != nine) > 0.95
  for drop in E.PAIRS6:                                             # a missing term, or one paired with the wrong plane
    five = sum(E.ref_fwd(d['x'][a], d['F'][b], 0, 0) for a, b in E.PAIRS6 if (a, b) != drop)
    assert np.mean(five != six) > 0.9
    swapped = five + E.ref_fwd(d['x'][drop[0]], d['F'][(drop[1] + 1) % 3], 0, 0)
    assert np.mean(swapped != six) > 0.9


def test_every_three_plane_case_is_exact_and_fits_its_entry_point():
  names = [L.name for L, _ in X6_LAYERS]
  assert len(set(names + [L.name for L in ALL_LAYERS])) == len(names) + len(ALL_LAYERS)
  assert set(E.X6_SCALE) == {L.name for L in E.X6_BWD_DATA}
  for L, what in X6_LAYERS:
    scale, positive = E.x6_params(L, what)
    E.check_geometry(L, what)
    E.assert_exact_range6(L, what, scale)
    assert E.x6_preconditions(L, what), (L.name, what)
    assert E.geo_ok(L.x_geo) and E.geo_ok(L.y_geo)
    if what == 'bwd_data':                                          # the largest power of two the exact range admits, or the K = 60 case
      n, term, _ = E.reductions6(L, what, 2 * scale)
      assert L.stride == 1 and (term * n >= E.LIMIT or L.name == 'x6-bwd-t256')
  # the bound is sharp enough to mean something: it is what the data can reach (all planes at their largest, one sign)
  n, term, extra = E.reductions6(E.X6_BWD_DATA[0], 'bwd_data', 1024)
  assert term == 3 * 3 * (2 * 1024) + 3 * 3 * 2 and n == 700 and extra == 0
  for bad, what in ((E.layer('r', 2, 50, 40, 29, 7, xcp=48), 'fwd'), (E.layer('r', 2, 50, 40, 100, 7, xcp=48), 'bwd_data')):
    assert not E.x6_preconditions(bad, what)


def x6_form(L, what):
  """(tile, whole stages, splits, stages of the tile's depth) as the host mirrors give them"""
  xg, yg = L.x_geo, L.y_geo
  if what == 'fwd':
    M, n_pad, taps, cp, splits = L.B * L.t_out, E.npad_of(L.cout), L.W, xg.c_pitch, 1
  elif what == 'bwd_data':
    M, n_pad, taps, cp, splits = L.B * L.T, E.npad_of(L.cin), L.W, yg.c_pitch, E.bf16_bwd_data_splits(L)
  else:
    M, n_pad, taps, cp, splits = L.W * xg.c_pitch, E.npad_of(L.cout), 1, L.B * E.wgrad6_tq(L), 1
  tile = E.x6_tile(M, n_pad, splits)
  bk = 32 if tile == 128 else 16
  return tile, E.x6_whole_stages(tile, taps, cp, taps * cp), splits, taps * E.ceil_div(cp, bk)


def test_three_plane_cases_name_every_required_form():
  forms = {L.name: x6_form(L, what) for L, what in X6_LAYERS}
  assert {f[:2] for f in forms.values()} == {(128, True), (128, False), (256, True)}
  assert [forms[n][3] for n in ('x6-k32', 'x6-one-tile', 'x6-k96')] == [1, 2, 3] and all(forms[n][:2] == (128, True) for n in ('x6-k32', 'x6-k96'))
  assert [forms['x6-t256-' + n] for n in ('k16', 'k32', 'k48-taps', 'k64')] == [(256, True, 1, k) for k in (1, 2, 3, 4)]
  assert forms['x6-clamped-taps'][:2] == (128, False) and forms['x6-clamped-1tap'][:2] == (128, False) and forms['x6-stride2-whole'][:2] == (128, True)
  assert {n for n, f in forms.items() if f[2] > 1} == {'x6-bwd-split'} and forms['x6-bwd-split'][:3] == (128, True, 2)
  assert forms['x6-bwd-clamped'][:2] == (128, False) and forms['x6-bwd-whole'][:2] == (128, True) and forms['x6-bwd-t256'][:2] == (256, True)
  assert forms['x6-wgrad-t256'][0] == 256 and all(forms[L.name][0] == 128 for L in E.X6_BWD_FILTER[:4])
  for L in E.X6_FWD[-4:]:                                           # exactly at the threshold of 192 tiles
    assert E.ceil_div(L.B * L.T, 256) * (E.npad_of(L.cout) // 256) == 192 and (L.B * L.T) % 256
  L = E.X6_BWD_FILTER[-1]
  assert E.ceil_div(L.W * L.x_geo.c_pitch, 256) * (E.npad_of(L.cout) // 256) == 192
  assert E.x6_tile(6021, 2048 + 128, 1) == 128 and E.bf16_tile(6021, 2048 + 128, 1) == 256       # NP = 3 alone asks for n_pad % 256 == 0
  L = E.X6_BWD_FILTER[0]
  assert (L.W * L.x_geo.c_pitch) % 128 == 16
  assert E.X6_BWD_FILTER[3].x_geo.halo - E.X6_BWD_FILTER[3].pad_left == 5 and L.x_geo.halo - L.pad_left == 1


@pytest.mark.parametrize('name,what,form', [('x6-one-tile', 'fwd', 'the 128 tile\'s epilogue'), ('x6-t256-k16', 'fwd', 'the 256 tile\'s epilogue'),
                                            ('x6-bwd-split', 'bwd_data', 'slab_epilogue_kernel<3>')])
def test_output_planes_are_nonzero_in_every_writing_form(name, what, form):
  """the reference's m plane is nonzero in more than 90 % of its elements and its l plane in more than half, for one case of each
  kernel form that writes output planes: an m / l swap or a dropped plane cannot hide behind zeros"""
  L = next(L for L, w in X6_LAYERS if L.name == name and w == what)
  tile, _, splits, _ = x6_form(L, what)
  assert (tile, splits > 1) == {'x6-one-tile': (128, False), 'x6-t256-k16': (256, False), 'x6-bwd-split': (128, True)}[name]
  ref = E.case_ref6(L, what)
  assert int(np.abs(ref).max()) < E.LIMIT
  h, m, l = E.split3(ref)
  assert np.array_equal(h.astype(np.int64) + m.astype(np.int64) + l.astype(np.int64), ref)
  assert np.mean(m != 0) > 0.9 and np.mean(l != 0) > 0.5, (form, np.mean(m != 0), np.mean(l != 0))


def test_plane_comparison_sees_a_swap_and_a_wrong_plane_stride():
  g = E.Geo(2, 5, 20, 3, 10, 32)
  ref = (np.arange(2 * 5 * 20).reshape(2, 5, 20) * 83777 - 7000001) % (1 << 24) - (1 << 23)
  h, m, l = E.split3(ref)
  assert np.count_nonzero(l) > 100 and np.count_nonzero(m != l) > 100
  good = E.guarded_planes_image(g)
  n = 2 * 10 * 32
  assert good.size == 3 * n + 2 * E.GUARD_WORDS
  body = good[E.GUARD_WORDS:-E.GUARD_WORDS].reshape(3, 2, 10, 32)
  assert (body[:, :, :3] == E.GUARD16).all() and (body[:, :, 3:8] == E.FILL16).all()
  body[:, :, 3:8, :20] = E.plane_bits((h, m, l))
  body[:, :, 3:8, 20:] = 0
  assert E.check_guarded_planes(good, g, ref, 128) is None
  swapped = good.copy()
  sb = swapped[E.GUARD_WORDS:-E.GUARD_WORDS].reshape(3, 2, 10, 32)
  sb[[1, 2]] = sb[[2, 1]]
  assert 'plane m' in E.check_guarded_planes(swapped, g, ref, 128)
  for where in (E.GUARD_WORDS - 1, E.GUARD_WORDS + 2 * n + 3 * 32 + 5, E.GUARD_WORDS + n + 1, good.size - E.GUARD_WORDS):
    bad = good.copy()
    bad[where] ^= 1
    assert E.check_guarded_planes(bad, g, ref, 128) is not None, where


def test_transposed_operands_of_the_filter_gradient():
  """the layout wgrad6_operands builds, read as st_exp_conv1d_bwd_filter_bf16x6 reads it (row c of x at shift w + x_first_row against
  row n of dz over r = b * tq + t), gives the reference -- and nothing lies where a shifted tap could read another utterance's frames"""
  L = E.layer('wgrad-layout', 2, 20, 5, 7, 3, xe=(2, 0))
  d = E.make_planes(L)
  xt, zt = E.wgrad6_operands(L, d['x'], d['dz'])
  tq, xg = E.wgrad6_tq(L), L.x_geo
  red, n_pad, first = L.B * tq, E.npad_of(L.cout), xg.halo - L.pad_left
  assert xt.shape == (3, xg.c_pitch * red + E.XT_SLACK) and zt.shape == (3, n_pad * red) and first == 2
  val = lambda bits: (bits.astype(np.uint32) << 16).view(np.float32).astype(np.int64)
  X, Z = val(xt), val(zt).reshape(3, n_pad, red)
  want = E.ref_bwd_filter6(d['x'], d['dz'], L.W, L.pad_left)
  got = np.zeros((L.W, xg.c_pitch, n_pad), dtype=np.int64)
  for a, b in E.PAIRS6:
    for w in range(L.W):
      for c in range(xg.c_pitch):
        got[w, c] += Z[b] @ X[a][c * red + w + first:c * red + w + first + red]
  assert np.array_equal(got[:, :L.cin, :L.cout], want) and not got[:, L.cin:].any() and not got[:, :, L.cout:].any()
  img = np.arange(2 * 6 * 16, dtype=np.uint16).reshape(2, 6, 16)
  t = E.transposed_ref(img, 1, 4, 8, 16, slack=3, fill=9)
  assert t.size == 16 * 2 * 8 + 3 and t[5 * 16 + 1 * 8 + 2] == img[1, 3, 5] and t[5 * 16 + 1 * 8 + 4] == 9 and (t[-3:] == 9).all()
