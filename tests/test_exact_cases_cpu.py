"""tests/exact_cases.py without a GPU: the integer reference against the oracle, bf16 rounding against torch, the data's lack of blind
spots, the exactness and geometry conditions of every GPU case, and the comparison's own ability to see one wrong element."""
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
