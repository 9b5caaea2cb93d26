"""Exact-integer cases for the time-domain matrix kernels (csrc/conv_gemm.hip, conv_bf16.hip, conv_taps_bf16.hip, wgrad_tr_bf16.hip).

Every kernel of these families multiplies in fp32 (or in bf16 with exact products) and accumulates in fp32.  With small integer
operands and every partial sum below 2^24 the sums are exact IN ANY ORDER, split or not: the fp32 results must equal an integer
reference bit for bit, stored bf16 results its round-to-nearest-even.  This module is host-only (numpy): the data, the geometry of
the padded NWC tensors the tests build themselves, the references, the layout formulas of include/speecht_hip.h, the guard
patterns and the comparison.  tests/test_exact_cases_cpu.py checks it without a GPU, tests/test_gpu_matrix_exact.py runs it.

Data: x and dz from {+-1, +-2, +-3}, filters from {+-1, +-2}, bias from -4..4, the ReLU-mask source from -2..2."""
import collections
import functools

import numpy as np

from oracle import w2l_oracle as O

LIMIT = 1 << 24
X_VALUES = np.array([-3, -2, -1, 1, 2, 3], dtype=np.int8)
F_VALUES = np.array([-2, -1, 1, 2], dtype=np.int8)
X_MAX, F_MAX, BIAS_MAX = 3, 2, 4

# bit patterns (quiet NaNs with a recognisable payload, so that an accidental read shows up too)
GUARD32, FILL32 = np.uint32(0x7FC5A5A5), np.uint32(0x7FD6B6B6)
GUARD16, FILL16 = np.uint16(0x7FC5), np.uint16(0x7FD6)
GUARD_WORDS = 1024            # elements in front of and behind every written buffer (keeps 2 KB / 4 KB alignment)
SLACK_ROWS = 40               # zero rows behind every INPUT plane (st_conv1d_bwd_filter_tr_bf16_slack_rows)


def round_up(a, m):
  return -(-a // m) * m


def ceil_div(a, b):
  return -(-a // b)


def npad_of(cout):
  return 32 if cout <= 32 else (64 if cout <= 64 else round_up(cout, 128))


def packed_dims(width, cin_pitch, cout):
  """st_packed_dims: (k_valid, k_pad, n_pad)"""
  return width * cin_pitch, round_up(width * cin_pitch, 32), npad_of(cout)


Geo = collections.namedtuple('Geo', 'batch frames channels halo t_pitch c_pitch')


def geo_ok(g):
  """st::tensor_ok"""
  return g.batch > 0 and g.frames > 0 and g.channels > 0 and g.halo >= 0 and g.c_pitch % 16 == 0 and g.c_pitch >= g.channels and \
      g.t_pitch >= g.halo + g.frames


def embed(g, data, dtype=np.float32):
  """[batch, frames, channels] -> the padded NWC image [batch, t_pitch, c_pitch]: zeros in the halo rows and pad channels"""
  out = np.zeros((g.batch, g.t_pitch, g.c_pitch), dtype=dtype)
  out[:, g.halo:g.halo + g.frames, :g.channels] = data
  return out


# ---- one layer: shapes, geometry, data ------------------------------------------------------------------------------------------
class Layer(collections.namedtuple('Layer', 'name B T cin cout W stride pad xcp ycp xe ye')):
  """pad: 'c' the centred SAME padding, 'l' pad_left = 0, 'r' pad_left = W - 1.  xcp / ycp: channel pitches (None: rounded up to 16).
  xe / ye: extra zero rows (front, back) of the input-side and output-side tensors beyond what the taps need; with equal sums a
  stride-1 layer's two tensors share one frame pitch (what conv_taps_bf16 and wgrad_tr_bf16 ask for) at different halos."""
  __slots__ = ()

  @property
  def t_out(self):
    return ceil_div(self.T, self.stride)

  @property
  def pad_left(self):
    if self.pad == 'l':
      return 0
    if self.pad == 'r':
      return self.W - 1
    return O.same_padding(self.T, self.W, self.stride)[1]

  @property
  def x_geo(self):
    pl = self.pad_left
    need = max((self.t_out - 1) * self.stride + self.W - pl - self.T, 0)
    if self.stride == 1:
      need = self.W - 1 - pl
    halo = pl + self.xe[0]
    return Geo(self.B, self.T, self.cin, halo, halo + self.T + need + self.xe[1], self.xcp or round_up(self.cin, 16))

  @property
  def y_geo(self):
    lead = self.W - 1 - self.pad_left if self.stride == 1 else 1
    trail = self.pad_left if self.stride == 1 else 0
    halo = lead + self.ye[0]
    return Geo(self.B, self.t_out, self.cout, halo, halo + self.t_out + trail + self.ye[1], self.ycp or round_up(self.cout, 16))

  @property
  def seed(self):
    return sum((i + 1) * ord(c) for i, c in enumerate(self.name)) % (1 << 31)


def layer(name, B, T, cin, cout, W, stride=1, pad='c', xcp=None, ycp=None, xe=(1, 0), ye=(0, 1)):
  return Layer(name, B, T, cin, cout, W, stride, pad, xcp, ycp, xe, ye)


def make_data(L):
  """Seeded integer data of a layer as int8 arrays: x [B,T,cin], F [W,cin,cout], bias [cout], act [B,T,cin] (the ReLU-mask source of
  back-prop to the input: contains values <= 0), dz [B,t_out,cout]."""
  rng = np.random.default_rng(L.seed)
  x = X_VALUES[rng.integers(0, 6, (L.B, L.T, L.cin))]
  F = F_VALUES[rng.integers(0, 4, (L.W, L.cin, L.cout))]
  bias = rng.integers(-BIAS_MAX, BIAS_MAX + 1, L.cout).astype(np.int8)
  act = rng.integers(-2, 3, (L.B, L.T, L.cin)).astype(np.int8)
  dz = X_VALUES[rng.integers(0, 6, (L.B, L.t_out, L.cout))]
  return dict(x=x, F=F, bias=bias, act=act, dz=dz)


# ---- references: tap-by-tap im2col products in float64 (every value an integer far below 2^53: exact), returned as int64 ---------
def _padded(x, pad_left, rows):
  B, T, C = x.shape
  xp = np.zeros((B, rows, C), dtype=np.float64)
  xp[:, pad_left:pad_left + T] = x
  return xp


def _as_int(a):
  r = np.rint(a)
  assert np.array_equal(r, a)
  return r.astype(np.int64)


def ref_fwd(x, F, bias, pad_left, stride=1, relu=False):
  """y[b,t,o] = act(bias[o] + sum_{w,c} x[b, t*stride + w - pad_left, c] * F[w,c,o])"""
  B, T, cin = x.shape
  W, _, cout = F.shape
  t_out = ceil_div(T, stride)
  xp = _padded(x, pad_left, pad_left + T + W + stride)
  y = np.zeros((B * t_out, cout), dtype=np.float64)
  for w in range(W):
    y += xp[:, w:w + (t_out - 1) * stride + 1:stride].reshape(B * t_out, cin) @ F[w].astype(np.float64)
  y = y.reshape(B, t_out, cout) + np.asarray(bias, dtype=np.float64)
  return _as_int(np.maximum(y, 0.0) if relu else y)


def ref_bwd_data(dz, F, pad_left, T, stride=1, act=None):
  """dx[b,u,c] = [act > 0] * sum_{w,o,t : t*stride + w - pad_left = u} dz[b,t,o] * F[w,c,o]"""
  B, t_out, cout = dz.shape
  W, cin, _ = F.shape
  dxp = np.zeros((B, pad_left + T + W + stride, cin), dtype=np.float64)
  z = dz.reshape(B * t_out, cout).astype(np.float64)
  for w in range(W):
    dxp[:, w:w + (t_out - 1) * stride + 1:stride] += (z @ F[w].astype(np.float64).T).reshape(B, t_out, cin)
  dx = dxp[:, pad_left:pad_left + T]
  if act is not None:
    dx = dx * (act > 0)
  return _as_int(dx)


def ref_bwd_filter(x, dz, W, pad_left, stride=1):
  """dF[w,c,o] = sum_{b,t} x[b, t*stride + w - pad_left, c] * dz[b,t,o];  dbias[o] = sum_{b,t} dz[b,t,o]"""
  B, T, cin = x.shape
  _, t_out, cout = dz.shape
  xp = _padded(x, pad_left, pad_left + T + W + stride)
  z = dz.reshape(B * t_out, cout).astype(np.float64)
  dF = np.stack([xp[:, w:w + (t_out - 1) * stride + 1:stride].reshape(B * t_out, cin).T @ z for w in range(W)])
  return _as_int(dF), _as_int(z.sum(axis=0))


def bf16_bits(a):
  """float values -> the uint16 bit patterns of their round-to-nearest-even bfloat16"""
  r = np.ascontiguousarray(O.bf16_round(a), dtype=np.float32)
  return (r.view(np.uint32) >> 16).astype(np.uint16)


def f32_bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- exactness conditions ---------------------------------------------------------------------------------------------------------
def reductions(L, what):
  """(terms, largest |term|, largest |addend outside the product|) of the sums a call forms.  what: 'fwd' | 'bwd_data' | 'bwd_filter'"""
  if what == 'fwd':
    return L.W * L.cin, X_MAX * F_MAX, BIAS_MAX
  if what == 'bwd_data':
    return L.W * L.cout, X_MAX * F_MAX, 0
  if what == 'bwd_filter':
    return L.B * L.t_out, X_MAX * X_MAX, 0
  raise ValueError(what)


def assert_exact_range(L, what):
  """6 * (reduction length) < 2^24, and the same with the call's true largest term and its bias: every partial sum of every
  subset of the terms is an integer below 2^24, so fp32 accumulation is exact in any order and under any split."""
  n, term, extra = reductions(L, what)
  assert 6 * n < LIMIT, (L.name, what, n)
  assert term * n + extra < LIMIT, (L.name, what, n)


def assert_column_sums_exact(values):
  """Second-level sums (column sums of a result over its rows): exact in any order when the sum of the magnitudes stays below
  2^24 -- a condition on the data, checked on the data."""
  assert int(np.abs(values).reshape(-1, values.shape[-1]).sum(axis=0).max()) < LIMIT


# ---- layout formulas of include/speecht_hip.h ---------------------------------------------------------------------------------
def pack_ref(F, cin_pitch):
  """packed[k_pad][n_pad], k = w * cin_pitch + c, zero in all padding"""
  W, cin, cout = F.shape
  _, kp, npad = packed_dims(W, cin_pitch, cout)
  P = np.zeros((kp, npad), dtype=F.dtype)
  P[:W * cin_pitch].reshape(W, cin_pitch, npad)[:, :cin, :cout] = F
  return P


def flip_transpose_ref(P, W, cin, cout, cin_pitch, cout_pitch):
  """packedT[(w' * cout_pitch + o)][c] = packed[((W-1-w') * cin_pitch + c)][o], [k_pad(W * cout_pitch)][n_pad(cin)]"""
  _, kpt, npt = packed_dims(W, cout_pitch, cin)
  Q = np.zeros((kpt, npt), dtype=P.dtype)
  for w in range(W):
    Q[w * cout_pitch:w * cout_pitch + cout, :cin] = P[(W - 1 - w) * cin_pitch:(W - 1 - w) * cin_pitch + cin, :cout].T
  return Q


def filters_bf16_ref(P):
  """wt[n_pad][k_pad] = bf16(packed[k][n]) as uint16 bits"""
  return bf16_bits(P.T)


def filters_bwd_bf16_ref(P, W, cin, cout, cin_pitch, cout_pitch):
  """out[c][(W-1-w) * cout_pitch + o] = bf16(packed[w * cin_pitch + c][o]), [n_pad(cin)][round_up(W * cout_pitch, 32)], zero elsewhere"""
  out = np.zeros((npad_of(cin), round_up(W * cout_pitch, 32)), dtype=np.uint16)
  for w in range(W):
    out[:cin, (W - 1 - w) * cout_pitch:(W - 1 - w) * cout_pitch + cout] = bf16_bits(P[w * cin_pitch:w * cin_pitch + cin, :cout])
  return out


# ---- guarded buffers: images before the call and comparison after ---------------------------------------------------------------
def _patterns(bits16):
  return (GUARD16, FILL16, np.uint16) if bits16 else (GUARD32, FILL32, np.uint32)


def guarded_tensor_image(g, bits16=False):
  """[guard | batch x t_pitch x c_pitch | guard] as a flat array of bit patterns: the guards AND the halo rows hold the guard
  pattern, the interior rows (all c_pitch columns) the fill pattern."""
  guard, fill, dt = _patterns(bits16)
  body = np.full((g.batch, g.t_pitch, g.c_pitch), guard, dtype=dt)
  body[:, g.halo:g.halo + g.frames] = fill
  return np.concatenate([np.full(GUARD_WORDS, guard, dt), body.reshape(-1), np.full(GUARD_WORDS, guard, dt)])


def guarded_flat_image(n, bits16=False):
  guard, fill, dt = _patterns(bits16)
  return np.concatenate([np.full(GUARD_WORDS, guard, dt), np.full(n, fill, dt), np.full(GUARD_WORDS, guard, dt)])


def first_difference(got, want, shape):
  bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
  if bad.size == 0:
    return None
  return tuple(int(i) for i in np.unravel_index(bad[0], shape)), int(bad.size)


def check_guarded_tensor(after, g, ref, n_pad, bits16=False, what=''):
  """`after`: the buffer of guarded_tensor_image after the call.  Interior channels < channels equal `ref` ([B, frames, channels],
  integers; bf16 planes: their RNE) bit for bit, channels in [channels, min(c_pitch, n_pad)) are zero, channels from n_pad on keep
  the fill pattern, halo rows and guards the guard pattern.  Returns an error text naming the first difference, or None."""
  guard, fill, dt = _patterns(bits16)
  after = np.asarray(after).view(dt)
  if not (np.all(after[:GUARD_WORDS] == guard) and np.all(after[-GUARD_WORDS:] == guard)):
    return '{}: a guard region was written'.format(what)
  body = after[GUARD_WORDS:-GUARD_WORDS].reshape(g.batch, g.t_pitch, g.c_pitch)
  halo = np.ones(g.t_pitch, dtype=bool)
  halo[g.halo:g.halo + g.frames] = False
  if not np.all(body[:, halo] == guard):
    d = first_difference(body[:, halo], np.full_like(body[:, halo], guard), body[:, halo].shape)
    return '{}: halo rows written, first at (b, halo row, c) = {} ({} elements)'.format(what, d[0], d[1])
  inner = body[:, g.halo:g.halo + g.frames]
  want = bf16_bits(ref) if bits16 else f32_bits(ref)
  d = first_difference(inner[:, :, :g.channels], want, want.shape)
  if d:
    b, t, c = d[0]
    gv = inner[b, t, c]
    m = b * g.frames + t
    return ('{}: {} elements differ, first at (b, t, c) = {}: got bits {:#x}, want {:#x} (reference value {}); flat row {} = row {} of '
            '128-row tile {} (row {} of 256-row tile {}), column {} of 128-column tile {}').format(
                what, d[1], d[0], int(gv), int(want[b, t, c]), int(ref[b, t, c]), m, m % 128, m // 128, m % 256, m // 256, c % 128, c // 128)
  stored = min(g.c_pitch, n_pad)
  sign = dt(0x7FFF if bits16 else 0x7FFFFFFF)
  if np.any(inner[:, :, g.channels:stored] & sign):
    return '{}: pad channels [{}, {}) are not zero'.format(what, g.channels, stored)
  if np.any(inner[:, :, stored:] != fill):
    return '{}: channels from n_pad = {} on were written'.format(what, n_pad)
  return None


def check_guarded_flat(after, want_bits, bits16=False, what='', shape=None, kept_from=None, row_pitch=0):
  """A flat guarded buffer against the expected bit patterns; elements from `kept_from` on (rows the call leaves to the caller)
  must be all untouched or all zero.  row_pitch: the channel pitch of a packed filter gradient [k = tap * pitch + channel][n], for the
  message."""
  guard, fill, dt = _patterns(bits16)
  after = np.asarray(after).view(dt)
  if not (np.all(after[:GUARD_WORDS] == guard) and np.all(after[-GUARD_WORDS:] == guard)):
    return '{}: a guard region was written'.format(what)
  body = after[GUARD_WORDS:-GUARD_WORDS]
  want = np.asarray(want_bits).reshape(-1)
  n = want.size if kept_from is None else kept_from
  d = first_difference(body[:n], want[:n], (n,))
  if d:
    i = d[0]
    flat = int(np.flatnonzero(body[:n] != want[:n])[0])
    if shape is not None:
      i = tuple(int(v) for v in np.unravel_index(flat, shape))
    where = ''
    if shape is not None and len(shape) == 2 and row_pitch:
      where = ' (tap {}, channel {} = chunk {} of 32, column tile {})'.format(i[0] // row_pitch, i[0] % row_pitch, i[0] % row_pitch // 32, i[1] // 128)
    return '{}: {} elements differ, first at {}{}: got bits {:#x}, want {:#x}'.format(what, d[1], i, where, int(body[flat]), int(want[flat]))
  if kept_from is not None:
    tail = body[kept_from:]
    if not (np.all(tail == fill) or np.all(tail == 0)):
      return '{}: the rows behind width * c_pitch are neither untouched nor zero'.format(what)
  return None


def dpacked_ref(dF, cin_pitch):
  """the filter gradient in packed layout as fp32 bit patterns [k_pad][n_pad]"""
  return f32_bits(pack_ref(dF, cin_pitch).astype(np.float32))


def padded_vector_bits(v, n_pad):
  out = np.zeros(n_pad, dtype=np.float32)
  out[:v.size] = v
  return out.view(np.uint32)


# ---- host mirrors of the dispatch expressions the trace does not print ---------------------------------------------------------
def bf16_fwd_splits(L):
  """conv_bf16.hip fwd_splits"""
  tiles = ceil_div(L.B * L.t_out, 128) * ceil_div(npad_of(L.cout), 128)
  if tiles >= 128 or npad_of(L.cout) % 128:
    return 1
  chunks = ceil_div(L.x_geo.c_pitch, 64)
  return max(1, min(256 // tiles, chunks if L.W > 1 else chunks // 4))


def bf16_bwd_data_splits(L):
  """conv_bf16.hip bwd_data_splits"""
  tiles = ceil_div(L.B * L.T, 128) * ceil_div(npad_of(L.cin), 128)
  chunks = ceil_div(L.y_geo.c_pitch, 64)
  if tiles >= 384 or chunks * L.W < 128:
    return 1
  return max(1, min(ceil_div(768, tiles), chunks // 4))


def bf16_tile(M, n_pad, splits):
  """conv_bf16.hip launch_gemm<1>: the 256 x 256 ping-pong tile or the 128 x 128 one"""
  return 256 if n_pad >= 256 and ceil_div(M, 256) * ceil_div(n_pad, 256) * max(1, splits) >= 192 else 128


def bf16_whole_stages(tile, taps, c_pitch, k_valid):
  """conv_bf16.hip launch_gemm: FAST (whole stages: 64 deep for the 128 tile, 32 deep for the 256 tile) or clamped"""
  bk = 64 if tile == 128 else 32
  return (c_pitch if taps > 1 else k_valid) % bk == 0


def taps_panel_eligible(a, y, width, lead, act=None):
  """conv_taps_bf16.hip conv_taps_bf16_eligible (a: operand tensor, y: result tensor)"""
  n_pad = npad_of(y.channels)
  if a.c_pitch != 256 or width < 2 or width > 9 or n_pad % 128 or y.c_pitch % 16:
    return False
  if a.t_pitch != y.t_pitch or a.batch != y.batch or a.frames != y.frames or a.halo < lead:
    return False
  if act is not None and (act.t_pitch != y.t_pitch or act.batch != y.batch or act.c_pitch < min(y.c_pitch, n_pad)):
    return False
  Q = (y.batch - 1) * y.t_pitch + y.frames
  return ceil_div(Q, 128) * (n_pad // 128) >= 128


TrPlan = collections.namedtuple('TrPlan', 'rows stages splits tiles ring map in_tile')


def tr_plan(L):
  """wgrad_tr_bf16.hip tr_plan and the launch's ring / map choice"""
  x, dz = L.x_geo, L.y_geo
  n_pad = npad_of(dz.channels)
  rows = (dz.batch - 1) * dz.t_pitch + dz.frames
  stages = ceil_div(rows, 32)
  tiles = L.W * ceil_div(x.c_pitch, 128) * ceil_div(n_pad, 128)
  splits = max(1, min(256 // max(1, tiles), stages // 8))
  if splits == 1 and 128 <= tiles <= 320 and stages >= 64:
    splits = 2
  while splits & (splits - 1):
    splits &= splits - 1
  splits = max(1, min(splits, stages))
  per = ceil_div(stages, splits)
  splits = ceil_div(stages, per)
  grid = splits * tiles
  return TrPlan(rows, stages, splits, tiles, 8 if grid <= 320 else 4, 1 if splits % 8 == 0 else (2 if 8 % splits == 0 else 0),
                x.c_pitch > x.channels and x.c_pitch % 128 == 0)


def tr_eligible(L):
  """wgrad_tr_bf16.hip tr_eligible: shared frame pitch, stride 1, and no read beyond the 40 slack rows"""
  x, dz, pl = L.x_geo, L.y_geo, L.pad_left
  if not (L.stride == 1 and x.t_pitch == dz.t_pitch and x.frames == dz.frames and x.halo >= pl and x.halo - pl + L.W - 1 <= x.t_pitch):
    return False
  plane_rows = x.batch * x.t_pitch
  rows = (dz.batch - 1) * dz.t_pitch + dz.frames
  staged = round_up(rows, 32)
  n_pad = npad_of(dz.channels)
  x_over, z_over = round_up(x.c_pitch, 128) - x.c_pitch, round_up(n_pad, 128) - dz.c_pitch
  x_spill = ceil_div(x_over, x.c_pitch) if x_over > 0 else 0
  z_spill = ceil_div(z_over, dz.c_pitch) if z_over > 0 else 0
  return x.halo - pl + L.W - 1 + staged - 1 + x_spill < plane_rows + SLACK_ROWS and dz.halo + staged - 1 + z_spill < plane_rows + SLACK_ROWS


def f32_nn_splits(M, n_pad, k_pad):
  """conv_gemm.hip nn_splits"""
  if n_pad % 128:
    return 1
  tiles = ceil_div(M, 128) * (n_pad // 128)
  nk = k_pad // 32
  splits = min(8, 256 // tiles) if tiles < 64 and nk >= 256 else (2 if 128 < tiles <= 320 and nk >= 512 else 1)
  while splits > 1 and nk // splits < 64:
    splits -= 1
  return splits


def f32_fwd_splits(M, n_pad, nk):
  """conv_gemm.hip fwd_splits"""
  if n_pad == 32:
    if M < 1024 or nk < 32:
      return 1
    tiles_m = ceil_div(M, 128)
    return max(1, min(8, nk // 4, (512 + tiles_m // 2) // tiles_m))
  if n_pad % 128:
    return 1
  tiles = ceil_div(M, 128) * (n_pad // 128)
  return 1 if tiles >= 128 else max(1, min(256 // tiles, nk // 4))


def check_geometry(L, what):
  """The preconditions of the entry points (include/speecht_hip.h) on the tensors a case builds."""
  x, y, pl = L.x_geo, L.y_geo, L.pad_left
  assert geo_ok(x) and geo_ok(y), L.name
  assert 0 <= pl < L.W or L.W == 1, L.name
  if what in ('fwd', 'bwd_filter'):
    assert x.halo >= pl and (y.frames - 1) * L.stride + L.W - pl <= x.t_pitch - x.halo, L.name
    assert y.frames == ceil_div(x.frames, L.stride), L.name
  if what == 'bwd_data':
    lead = L.W - 1 - pl
    assert L.stride == 1 and lead >= 0 and y.halo >= lead and y.frames + pl <= y.t_pitch - y.halo, L.name
    assert y.t_pitch >= y.halo - lead + y.frames + L.W - 1, L.name


# ---- the cases (test_gpu_matrix_exact.py names the kernel form each one must reach) ----------------------------------------------
# bf16 general kernel, forward (y_f32 and y_bf16) and, at stride 1, back-prop to the input
BF16_GENERAL = [
    layer('one-tile', 1, 100, 64, 128, 1),                                    # the first case: one 128 x 128 tile, one tap, K = 64
    layer('tile128-whole', 2, 70, 64, 100, 1),
    layer('tile128-clamped-taps', 2, 70, 40, 100, 7, xcp=48),
    layer('tile128-clamped-ktail', 2, 70, 90, 100, 1, xcp=96),
    layer('pad-left-0', 2, 70, 40, 100, 7, pad='l', xcp=48),
    layer('pad-left-w-1', 2, 70, 40, 100, 7, pad='r', xcp=48),
    layer('frames-below-taps', 3, 3, 40, 100, 7, xcp=48),
    layer('one-frame', 1, 1, 40, 100, 7, xcp=48),
    layer('stride2-w48', 2, 75, 40, 100, 48, stride=2),
    layer('fwd-split-taps', 1, 100, 250, 250, 7),
    layer('fwd-split-1tap', 1, 100, 2000, 250, 1),
    layer('bwd-split', 2, 50, 100, 512, 16),
]
BF16_TILE256 = [
    layer('tile256-whole', 3, 2007, 60, 2000, 1, xcp=64),
    layer('tile256-clamped', 3, 2007, 40, 2000, 1, xcp=48),
    layer('tile256-half-column-tile', 3, 8107, 40, 300, 1, xcp=48),
]
# the LDS-panel kernel: operand pitch 256, shared frame pitch, ceil(Q / 128) * (n_pad / 128) >= 128
BF16_PANEL = [
    layer('panel-w2', 4, 2020, 250, 250, 2),
    layer('panel-w7', 4, 2020, 250, 250, 7),
    layer('panel-w9', 4, 2020, 250, 250, 9),
    layer('panel-cout128', 8, 2030, 128, 128, 7, xcp=256, ycp=256),
]
BF16_PANEL_REFUSED = [
    layer('general-w10', 4, 2020, 250, 250, 10),
    layer('general-below-threshold', 4, 2005, 250, 250, 7),
]
# bf16 filter gradient: transposing reads (stride 1, shared pitch) and the entry point with transposed copies
BF16_WGRAD_TR = [
    layer('tr-unsplit-bias-direct', 2, 100, 250, 100, 3),
    layer('tr-split2', 2, 300, 250, 100, 3),
    layer('tr-split8-map1', 2, 1030, 250, 250, 7),
    layer('tr-pitch48', 2, 100, 40, 100, 3, xcp=48),
    layer('tr-pitch128-no-pad-channel', 2, 300, 128, 100, 3),
    layer('tr-ring4', 1, 40, 500, 1200, 9),
]
BF16_WGRAD_COPIES = [
    layer('copies-stride2', 2, 75, 40, 100, 6, stride=2),
    layer('copies-stride2-split', 2, 1201, 40, 100, 6, stride=2),
    layer('copies-other-pitch', 2, 100, 40, 100, 3, xcp=48, ye=(2, 4)),
    layer('copies-tile256', 1, 40, 500, 1500, 16),
]
# fp32 forward / back-prop to the input (gemm_nn) and filter gradient (gemm_tn)
F32_NN = [
    layer('f32-small', 2, 50, 40, 100, 7, xcp=48),
    layer('f32-np64', 2, 50, 40, 50, 7, xcp=48),
    layer('f32-np32', 2, 50, 40, 29, 7, xcp=48),
    layer('f32-fwd-split-fast', 1, 100, 64, 100, 7),
    layer('f32-fwd-split-midtap', 1, 100, 90, 100, 7, xcp=96),
    layer('f32-fwd-split-clamped', 1, 100, 40, 100, 7, xcp=48),
    layer('f32-fwd-split-np32', 2, 515, 128, 29, 8),
    layer('f32-pad-left-0', 2, 50, 40, 100, 7, pad='l', xcp=48),
    layer('f32-pad-left-w-1', 2, 50, 40, 100, 7, pad='r', xcp=48),
    layer('f32-stride2', 2, 75, 40, 100, 48, stride=2),
]
F32_BWD_SPLIT = [
    layer('f32-nn-splits8', 2, 50, 100, 1024, 16),
    layer('f32-nn-splits2', 4, 4130, 100, 1024, 16),
]
F32_1TAP = [
    layer('f32-1tap-bt64', 2, 50, 100, 64, 1),
    layer('f32-1tap-bt128', 2, 770, 2000, 32, 1),
    layer('f32-1tap-bt128-split', 2, 50, 100, 8192, 1),
]
F32_TN = [
    layer('tn128-straddle', 3, 50, 40, 130, 3),
    layer('tn64-slabs', 2, 300, 20, 50, 9),
    layer('tn32-tiny5', 4, 5, 40, 29, 3),
    layer('tn128-tiny1', 7, 1, 40, 130, 3),
    layer('tn128-supertile', 2, 32, 1024, 1024, 1),
    layer('tn128-stride2-slabs', 2, 601, 40, 130, 4, stride=2),
]

CALLS = [(BF16_GENERAL, ('fwd', 'bwd_data')), (BF16_TILE256, ('fwd',)), (BF16_PANEL, ('fwd', 'bwd_data')),
         (BF16_PANEL_REFUSED, ('fwd', 'bwd_data')), (BF16_WGRAD_TR, ('bwd_filter',)), (BF16_WGRAD_COPIES, ('bwd_filter',)),
         (F32_NN, ('fwd', 'bwd_data')), (F32_BWD_SPLIT, ('bwd_data',)), (F32_1TAP, ('bwd_data',)), (F32_TN, ('bwd_filter',))]


def all_calls():
  """(layer, call) for every GPU case; stride-2 layers have no back-prop to the input"""
  return [(L, what) for cases, calls in CALLS for L in cases for what in calls if not (what == 'bwd_data' and L.stride != 1)]


@functools.lru_cache(maxsize=4)
def case_data(L):
  """The data of a case, made once and shared (read-only) among the tests that run it."""
  d = make_data(L)
  for a in d.values():
    a.setflags(write=False)
  return d
