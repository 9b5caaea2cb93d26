"""The SpecAugment specification (DESIGN.md "SpecAugment") in numpy, written from the text and not from the library's header:
Philox4x32-10 in uint64 arithmetic, the plan of one utterance, and the application in float64.

Policy = (W, F, mF, T, mT, p).  Plan of one utterance: [c, w, (f0, f) x mF, (t0, t) x mT], c = w = 0 when it is not warped."""
import numpy as np

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
  """counter: four 32-bit words, key: two -> four 32-bit words (Salmon et al. 2011, the Random123 definition)."""
  c = [np.uint64(v) for v in counter]
  k = [np.uint64(v) for v in key]
  mask, s32 = np.uint64(M32), np.uint64(32)
  for _ in range(10):
    p0 = np.uint64(PHILOX_M0) * c[0]
    p1 = np.uint64(PHILOX_M1) * c[2]
    c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & mask, (p0 >> s32) ^ c[3] ^ k[1], p0 & mask]
    k = [(k[0] + np.uint64(PHILOX_W0)) & mask, (k[1] + np.uint64(PHILOX_W1)) & mask]
  return [int(v) for v in c]


def block(seed, draw_id, index):
  """Block `index` of the utterance's stream: key = the seed's two words, counter = {draw id low, draw id high, block, 0}."""
  seed, draw_id = int(seed) & (2 ** 64 - 1), int(draw_id) & (2 ** 64 - 1)
  return philox4x32_10([draw_id & M32, draw_id >> 32, index, 0], [seed & M32, seed >> 32])


def uniform(x, n):
  """An integer in [0, n] of one 32-bit word."""
  return (x * (n + 1)) >> 32


def ratio_q16(p):
  return int(round(p * 65536))


def plan(policy, seed, draw_id, L, C):
  W, F, mF, T, mT, p = policy
  out = [0, 0]
  if W > 0 and L >= 2 * W + 2:
    r = block(seed, draw_id, 0)
    out = [W + 1 + uniform(r[0], L - 2 * W - 2), uniform(r[1], 2 * W) - W]
  for k in range(mF):
    r = block(seed, draw_id, 1 + k)
    f = uniform(r[0], min(F, C))
    out += [uniform(r[1], C - f), f]
  for k in range(mT):
    r = block(seed, draw_id, 9 + k)
    t = uniform(r[0], min(T, (ratio_q16(p) * L) >> 16))
    out += [uniform(r[1], L - t), t]
  return out


def source_position(pl, L, t):
  """s(t) as (i, r, den): s = i + r / den, in integers.  An utterance that is not warped: (t, 0, 1).  The last row is pinned,
  s(L - 1) = L - 1: that is what both pieces give unless c' = L - 1, where the text's two statements (s(t) = t c / c' for
  t <= c', and s(L - 1) = L - 1) disagree and the fixed end wins."""
  c, w = pl[0], pl[1]
  if c == 0 or t == L - 1:
    return t, 0, 1
  cw = c + w
  if t <= cw:
    num, den, base = t * c, cw, 0
  else:
    num, den, base = (t - cw) * (L - 1 - c), L - 1 - cw, c
  return base + num // den, num % den, den


def apply(policy, pl, x, L):
  """x [T, C] (any float dtype) -> (float64 [T, C], kind [T, C]): kind 0 = the source's element (exact), 1 = masked (exactly 0),
  2 = interpolated between source rows i and i + 1; the third array [T] holds each row's i (the row itself where nothing moves)."""
  W, F, mF, T_, mT, p = policy
  x = np.asarray(x)
  T, C = x.shape
  out = x.astype(np.float64).copy()
  kind = np.zeros((T, C), dtype=np.int8)
  lower = np.arange(T, dtype=np.int64)
  x64 = x.astype(np.float64)
  for t in range(L):
    i, r, den = source_position(pl, L, t)
    lower[t] = i
    if r == 0:
      out[t] = x64[i]
    else:
      out[t] = x64[i] + (r / den) * (x64[i + 1] - x64[i])
      kind[t] = 2
  for k in range(mF):
    f0, f = pl[2 + 2 * k], pl[3 + 2 * k]
    out[:L, f0:f0 + f] = 0.0
    kind[:L, f0:f0 + f] = 1
  for k in range(mT):
    t0, t = pl[2 + 2 * mF + 2 * k], pl[3 + 2 * mF + 2 * k]
    out[t0:t0 + t] = 0.0
    kind[t0:t0 + t] = 1
  return out, kind, lower
