"""Exact-integer cases for the time-domain matrix kernels (csrc/conv_gemm.hip, conv_bf16.hip, conv_taps_bf16.hip, wgrad_tr_bf16.hip).

Every kernel of these families multiplies in fp32 (or in bf16 with exact products) and accumulates in fp32.  With small integer
operands and every partial sum below 2^24 the sums are exact IN ANY ORDER, split or not: the fp32 results must equal an integer
reference bit for bit, stored bf16 results its round-to-nearest-even.  This module is host-only (numpy): the data, the geometry of
the padded NWC tensors the tests build themselves, the references, the layout formulas of include/speecht_hip.h, the guard
patterns and the comparison.  tests/test_exact_cases_cpu.py checks it without a GPU, tests/test_gpu_matrix_exact.py runs it.

Data: x and dz from {+-1, +-2, +-3}, filters from {+-1, +-2}, bias from -4..4, the ReLU-mask source from -2..2.

The three-plane (bf16x6, NP = 3) kernels take their h | m | l planes from the caller, so the cases of the last section fill the three
planes of every operand with INDEPENDENT small integers (no valid split of anything): the kernel must return the six kept plane
products and nothing of the three dropped ones, bit for bit, and the three planes of its output must be split3 of that integer."""
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


# ---- three planes per operand (bf16x6: conv_bf16.hip, NP = 3) --------------------------------------------------------------------
# The kernels multiply plane pairs, not numbers: with INDEPENDENT integer planes a_h, a_m, a_l and b_h, b_m, b_l they must return
#   sum_k (a_h b_h + a_h b_m + a_m b_h + a_h b_l + a_l b_h + a_m b_m)
# and nothing of a_m b_l, a_l b_m, a_l b_l.  (On a real split of small integers m = l = 0 and five of the six terms vanish.)
PAIRS6 = ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1))      # (plane of the first operand, plane of the second), 0 1 2 = h m l
BIAS6_MIN, BIAS6_MAX = 1 << 20, (1 << 23) - 1                   # |bias| of the forward cases: wide enough for a nonzero l plane


def split3(x):
  """numpy model of split3 in conv_bf16.hip: h = bf16(x), m = bf16(x - h), l = (x - h) - m, all in fp32 -> three float32 arrays.
  h + m + l == x exactly for 2^-110 <= |x| < bit pattern 0x7F7F8000 (there bf16(x) overflows: h = +-inf, m = -+inf, l = NaN)."""
  x = np.ascontiguousarray(x, dtype=np.float32)
  with np.errstate(invalid='ignore', over='ignore'):
    h = O.bf16_round(x).astype(np.float32)
    r1 = x - h
    m = O.bf16_round(r1).astype(np.float32)
    l = r1 - m
  return h, m, l


def random_f32(rng, n, lo=-100, hi=100):
  """n floats with full 23-bit mantissas, exponents lo..hi and both signs: all three planes of their split are nonzero"""
  bits = (rng.integers(0, 2, n).astype(np.uint32) << 31) | ((rng.integers(lo, hi + 1, n) + 127).astype(np.uint32) << 23) | \
      rng.integers(0, 1 << 23, n).astype(np.uint32)
  return bits.view(np.float32)


def make_planes(L, scale=1, positive_h=False):
  """Three independent integer planes per operand, seeded from L.seed: x [3,B,T,cin] and dz [3,B,t_out,cout] from X_VALUES (int8),
  F [3,W,cin,cout] from F_VALUES (int32), bias [cout] with |bias| in [2^20, 2^23) and random sign, act as make_data.  `scale` (a power
  of two) multiplies the filters' h plane only, positive_h takes |.| of the h planes of x, dz and F: together they make back-prop's
  sums wide enough to need all three output planes (the forward cases get there with the bias)."""
  assert scale >= 1 and scale & (scale - 1) == 0 and scale * F_MAX <= 1 << 15
  rng = np.random.default_rng([L.seed, 3])
  x = X_VALUES[rng.integers(0, 6, (3, L.B, L.T, L.cin), dtype=np.uint8)]
  F = F_VALUES[rng.integers(0, 4, (3, L.W, L.cin, L.cout), dtype=np.uint8)].astype(np.int32)
  dz = X_VALUES[rng.integers(0, 6, (3, L.B, L.t_out, L.cout), dtype=np.uint8)]
  bias = rng.integers(BIAS6_MIN, BIAS6_MAX + 1, L.cout) * rng.choice([-1, 1], L.cout)
  act = rng.integers(-2, 3, (L.B, L.T, L.cin)).astype(np.int8)
  if positive_h:
    x[0], F[0], dz[0] = np.abs(x[0]), np.abs(F[0]), np.abs(dz[0])
  F[0] *= scale
  return dict(x=x, F=F, bias=bias.astype(np.int64), act=act, dz=dz)


def ref_fwd6(xp, Fp, bias, pad_left, stride=1, relu=False):
  """the six kept plane products of the forward pass (int64), bias and ReLU applied once"""
  y = sum(ref_fwd(xp[a], Fp[b], 0, pad_left, stride) for a, b in PAIRS6) + np.asarray(bias, dtype=np.int64)
  return np.maximum(y, 0) if relu else y


def ref_bwd_data6(dzp, Fp, pad_left, T, stride=1, act=None):
  """back-prop to the input: first operand dz, second the filters; the mask applied once"""
  dx = sum(ref_bwd_data(dzp[a], Fp[b], pad_left, T, stride) for a, b in PAIRS6)
  return dx * (act > 0) if act is not None else dx


def ref_bwd_filter6(xp, dzp, W, pad_left, stride=1):
  """filter gradient: first operand x (the rows of the product), second dz"""
  return sum(ref_bwd_filter(xp[a], dzp[b], W, pad_left, stride)[0] for a, b in PAIRS6)


def reductions6(L, what, scale=1):
  """(terms, bound of the six plane products of one term, largest |addend outside the product|).  Forward and back-prop to the input:
  the second operand is the filter, |b_h| <= scale * F_MAX, every other plane value is at most X_MAX or F_MAX -- three products with
  b_h (a_h b_h, a_m b_h, a_l b_h) and three without (a_h b_m, a_h b_l, a_m b_m): 3 X_MAX F_MAX (scale + 1) = 18 (scale + 1).
  Filter gradient: both operands from X_VALUES, 6 X_MAX^2 = 54."""
  n = reductions(L, what)[0]
  if what == 'bwd_filter':
    assert scale == 1
    return n, 6 * X_MAX * X_MAX, 0
  return n, 3 * X_MAX * F_MAX * scale + 3 * X_MAX * F_MAX, BIAS6_MAX if what == 'fwd' else 0


def assert_exact_range6(L, what, scale=1):
  """n * 18 * (scale + 1) (filter gradient: n * 54), plus the forward bias below 2^23, stays below 2^24: every partial sum of every
  subset of the plane products, in any order and under any split, is an integer below 2^24 and fp32 accumulation is exact -- and so is
  the result with its bias, whose split3 planes then add up to it.  A bound on absolute values: it holds with positive_h too."""
  n, term, extra = reductions6(L, what, scale)
  assert term * n + extra < LIMIT, (L.name, what, n, scale)


def plane_bits(planes):
  """three float planes (bf16-representable values, as split3 returns them inside its domain) -> uint16 bit patterns [3, ...]"""
  return np.stack([bf16_bits(p) for p in planes])


def canonical16(bits):
  """bf16 bit patterns with every NaN replaced by one pattern: non-finite planes compare by class (and infinities by sign)"""
  bits = np.array(bits, dtype=np.uint16)
  bits[(bits & np.uint16(0x7FFF)) > np.uint16(0x7F80)] = 0x7FC0
  return bits


def filter_planes_fwd(Fp, cin_pitch):
  """the forward filter operand: 3 x [n_pad][k_pad] uint16, plane stride n_pad * k_pad"""
  return np.stack([filters_bf16_ref(pack_ref(F.astype(np.float32), cin_pitch)) for F in Fp])


def filter_planes_bwd(Fp, cin_pitch, cout_pitch):
  """back-prop's filter operand (st_exp_split3_transpose_bf16 of the flipped, transposed filters): 3 x [n_pad(cin)][k_pad(W * cout_pitch)]"""
  W, cin, cout = Fp[0].shape
  return np.stack([filters_bwd_bf16_ref(pack_ref(F.astype(np.float32), cin_pitch), W, cin, cout, cin_pitch, cout_pitch) for F in Fp])


def transposed_ref(image, row0, rows, tq, c_rows, slack=0, fill=0):
  """transpose_split_kernel on one plane: out[c][b * tq + j] = image[b][row0 + j][c] for j < rows, c < c_pitch, flat with `slack`
  elements behind; every other element is `fill` (the kernel leaves it alone)"""
  B, _, cp = image.shape
  body = np.full((c_rows, B, tq), fill, dtype=image.dtype)
  body[:cp, :, :rows] = image[:, row0:row0 + rows].transpose(2, 0, 1)
  return np.concatenate([body.reshape(-1), np.full(slack, fill, dtype=image.dtype)])


XT_SLACK = 4096               # elements behind every transposed x plane (st_exp_conv1d_bwd_filter_bf16x6: shifted taps read into them)


def wgrad6_tq(L):
  """speecht_amd/modes/bf16x6.py: the transposed planes hold whole frame pitches of x, rounded up to 32"""
  return round_up(max(L.x_geo.t_pitch, L.y_geo.frames), 32)


def wgrad6_operands(L, xp, dzp):
  """the operands of st_exp_conv1d_bwd_filter_bf16x6 as bf16 bit patterns, laid out as modes/bf16x6.py produces them: x planes
  [3][cin_pitch * batch * tq + 4096] from row 0 of the padded tensor, dz planes [3][n_pad * batch * tq] from its first frame"""
  xg, yg, tq = L.x_geo, L.y_geo, wgrad6_tq(L)
  xt = np.stack([transposed_ref(bf16_bits(embed(xg, p)), 0, xg.t_pitch, tq, xg.c_pitch, XT_SLACK) for p in xp])
  zt = np.stack([transposed_ref(bf16_bits(embed(yg, p)), yg.halo, yg.frames, tq, npad_of(L.cout)) for p in dzp])
  return xt, zt


def guarded_planes_image(g):
  """[guard | h | m | l | guard], every plane a tensor image as in guarded_tensor_image, plane stride batch * t_pitch * c_pitch"""
  one = guarded_tensor_image(g, True)
  return np.concatenate([one[:GUARD_WORDS]] + [one[GUARD_WORDS:-GUARD_WORDS]] * 3 + [one[-GUARD_WORDS:]])


def check_guarded_planes(after, g, ref, n_pad, what=''):
  """the buffer of guarded_planes_image after the call: plane by plane the bit patterns of split3(ref), each held to everything
  check_guarded_tensor asks of a 16-bit tensor (pad channels, fill, halo rows)"""
  after = np.asarray(after).view(np.uint16)
  n = g.batch * g.t_pitch * g.c_pitch
  assert after.size == 3 * n + 2 * GUARD_WORDS
  guard = np.full(GUARD_WORDS, GUARD16, np.uint16)
  if not (np.all(after[:GUARD_WORDS] == GUARD16) and np.all(after[-GUARD_WORDS:] == GUARD16)):
    return '{}: a guard region of the planes was written'.format(what)
  for i, p in enumerate(split3(ref)):
    one = np.concatenate([guard, after[GUARD_WORDS + i * n:GUARD_WORDS + (i + 1) * n], guard])
    err = check_guarded_tensor(one, g, p, n_pad, bits16=True, what='{} plane {}'.format(what, 'hml'[i]))
    if err:
      return err
  return None


# host mirrors of the NP = 3 dispatch (bwd_data_splits is shared with NP = 1: bf16_bwd_data_splits; the forward entry point never splits)
def x6_tile(M, n_pad, splits):
  """conv_bf16.hip launch_gemm<3>: the 256 tile only when n_pad is a multiple of 256 (fits256) and the grid is wide"""
  return 256 if n_pad % 256 == 0 and ceil_div(M, 256) * ceil_div(n_pad, 256) * max(1, splits) >= 192 else 128


def x6_whole_stages(tile, taps, c_pitch, k_valid):
  """conv_bf16.hip launch_gemm: FAST (whole stages: 32 deep for the 128 tile, 16 deep for the 256 tile) or clamped.
  Every channel pitch is a multiple of 16 (st::tensor_ok; the filter gradient's reduction is batch * tq with tq % 32 == 0), so the
  256 tile always has whole stages: gemm_nn_bf16_kernel<256, ..., NP = 3, FAST = false> cannot be reached through these entry
  points.  (It stays instantiated: launch_gemm picks FAST at run time.)"""
  bk = 32 if tile == 128 else 16
  return (c_pitch if taps > 1 else k_valid) % bk == 0


def x6_preconditions(L, what):
  """the ST_REQUIRE lines of the st_exp_ entry points in conv_bf16.hip"""
  x, y, pl = L.x_geo, L.y_geo, L.pad_left
  if what == 'fwd':
    return x.halo >= pl and y.frames == ceil_div(x.frames, L.stride) and x.c_pitch % 16 == 0 and npad_of(L.cout) % 128 == 0
  if what == 'bwd_data':
    lead = L.W - 1 - pl
    return lead >= 0 and y.halo >= lead and y.frames == x.frames and y.batch == x.batch and npad_of(L.cin) % 128 == 0
  if what == 'bwd_filter':
    return wgrad6_tq(L) % 32 == 0 and x.c_pitch % 16 == 0 and npad_of(L.cout) % 128 == 0 and x.batch * wgrad6_tq(L) < 1 << 31
  raise ValueError(what)


X6_FWD = [
    layer('x6-one-tile', 1, 100, 64, 128, 1),                                 # K = 64: two stages of the two-slot pipeline
    layer('x6-k32', 1, 100, 32, 128, 1),                                      # one stage
    layer('x6-k96', 1, 100, 96, 128, 1),                                      # three
    layer('x6-clamped-taps', 2, 70, 40, 100, 7, xcp=48),
    layer('x6-clamped-1tap', 2, 70, 40, 100, 1, xcp=48),
    layer('x6-pad-left-0', 2, 70, 40, 100, 7, pad='l', xcp=48),
    layer('x6-pad-left-w-1', 2, 70, 40, 100, 7, pad='r', xcp=48),
    layer('x6-frames-below-taps', 3, 3, 40, 100, 7, xcp=48),
    layer('x6-one-frame', 1, 1, 40, 100, 7, xcp=48),
    layer('x6-stride2-clamped', 2, 75, 40, 100, 48, stride=2),
    layer('x6-stride2-whole', 2, 75, 64, 100, 6, stride=2),
    layer('x6-t256-k16', 3, 2007, 16, 2000, 1),                               # M = 6021, n_pad = 2048: 24 x 8 = 192 tiles of 256 x 256,
    layer('x6-t256-k32', 3, 2007, 32, 2000, 1),                               # the threshold; one to four 16-deep stages of the ring of 3
    layer('x6-t256-k48-taps', 3, 2007, 16, 2000, 3),
    layer('x6-t256-k64', 3, 2007, 60, 2000, 1, xcp=64),
]
X6_BWD_DATA = [
    layer('x6-bwd-clamped', 2, 70, 100, 100, 7),                              # dz pitch 112
    layer('x6-bwd-whole', 2, 70, 100, 128, 7),
    layer('x6-bwd-pad-left-0', 2, 70, 100, 100, 7, pad='l'),
    layer('x6-bwd-pad-left-w-1', 2, 70, 100, 128, 7, pad='r'),
    layer('x6-bwd-split', 2, 50, 100, 512, 16),                               # chunks * W = 128: two splits, slab_epilogue_kernel<3>
    layer('x6-bwd-t256', 3, 2007, 2000, 60, 1, ycp=64),
]
X6_BWD_FILTER = [
    layer('x6-wgrad-m-tail', 2, 100, 40, 100, 3, xcp=48),                     # M = 144: a row-tile tail
    layer('x6-wgrad-long', 2, 300, 250, 100, 3),
    layer('x6-wgrad-1tap', 3, 50, 128, 130, 1),
    layer('x6-wgrad-x-first-row', 2, 100, 40, 100, 3, xcp=48, xe=(5, 0)),
    layer('x6-wgrad-t256', 1, 40, 500, 1500, 16),                             # M = 8192, n_pad = 1536: 32 x 6 = 192 tiles
]
# the power of two on the filters' h plane in back-prop to the input (h planes positive): chosen on the CPU for the share of nonzero
# elements in the reference's l plane, see test_exact_cases_cpu.py; the forward cases and the filter gradient use 1.  The largest
# power of two that assert_exact_range6 admits at K = 700 .. 896 and at K = 8192 gives about 80 % nonzero l; at K = 60 no scale gives
# any (the h plane holds the whole scaled part, the m plane the rest): that case checks that the l plane is written as zeros.
X6_SCALE = {'x6-bwd-clamped': 1024, 'x6-bwd-whole': 1024, 'x6-bwd-pad-left-0': 1024, 'x6-bwd-pad-left-w-1': 1024, 'x6-bwd-split': 64,
            'x6-bwd-t256': 128}
X6_CALLS = [(X6_FWD, 'fwd'), (X6_BWD_DATA, 'bwd_data'), (X6_BWD_FILTER, 'bwd_filter')]


def x6_params(L, what):
  """(scale, positive_h) of a case"""
  return (X6_SCALE[L.name], True) if what == 'bwd_data' else (1, False)


@functools.lru_cache(maxsize=2)
def case_planes(L, what):
  d = make_planes(L, *x6_params(L, what))
  for a in d.values():
    a.setflags(write=False)
  return d


@functools.lru_cache(maxsize=2)
def case_ref6(L, what):
  """the reference of a case without ReLU and mask (either is one np.maximum / one product on top), made once"""
  d = case_planes(L, what)
  if what == 'fwd':
    r = ref_fwd6(d['x'], d['F'], d['bias'], L.pad_left, L.stride)
  elif what == 'bwd_data':
    r = ref_bwd_data6(d['dz'], d['F'], L.pad_left, L.T)
  else:
    r = ref_bwd_filter6(d['x'], d['dz'], L.W, L.pad_left, L.stride)
  r.setflags(write=False)
  return r
