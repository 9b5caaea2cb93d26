"""The waveform-augmentation specification (DESIGN.md "Waveform augmentation") in numpy and float64, written from the text and not
from the library's header: the phase table of a speed, the resampled signal, the fixed-order sums of squares, the gain, the mix
and the draws (Philox4x32-10 with counter word 3 = 1).

A plan is a dict: speed (index into the policy's speeds, -1 = 1/1), M, noisy, clip, offset, snr_centi, lin."""
import fractions
import math

import numpy as np

from tests.spec_augment_oracle import M32, philox4x32_10, uniform

ZEROS, ROLLOFF, BETA = 16, 0.85, 8.555504641634386      # resampy's kaiser_fast
TILE = 256


def half_width(num, den):
  return math.ceil(fractions.Fraction(ZEROS * max(num, den), den))


def out_len(n, num, den):
  return (n * den + num - 1) // num


def table(num, den):
  """float64 [den][2H]: h_phi[j] = fc sinc(fc tau) I0(beta sqrt(1 - (tau/H)^2)) / I0(beta), tau = j - phi/den, j = -H+1 .. H, each row
  divided by its own sum."""
  H = half_width(num, den)
  fc = ROLLOFF * min(1.0, den / num)
  tau = np.arange(-H + 1, H + 1, dtype=np.float64)[None, :] - np.arange(den, dtype=np.float64)[:, None] / den
  r = tau / H
  window = np.where(np.abs(r) < 1.0, np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - r * r))) / np.i0(BETA), 0.0)
  h = fc * np.sinc(fc * tau) * window
  return h / h.sum(axis=1, keepdims=True)


def windows(x, num, den):
  """(phi [M], windows [M][2H] float64): the 2H source samples of every output, zeros outside the utterance."""
  x = np.asarray(x, dtype=np.float64)
  n, H = len(x), half_width(num, den)
  M = out_len(n, num, den)
  t = np.arange(M, dtype=np.int64) * num
  i, phi = t // den, t % den
  src = i[:, None] + np.arange(-H + 1, H + 1, dtype=np.int64)[None, :]
  padded = np.concatenate([x, [0.0]])
  return phi, padded[np.where((src >= 0) & (src < n), src, n)]


def resample(x, num, den, h=None):
  """The speed-changed signal in float64 (h: the table to use, default the float64 one) and the bound's sum_k |h_phi[k] x_k|."""
  if num == den:
    x = np.asarray(x, dtype=np.float64)
    return x.copy(), np.abs(x)
  h = table(num, den) if h is None else np.asarray(h, dtype=np.float64)
  phi, win = windows(x, num, den)
  rows = h[phi]
  return (rows * win).sum(axis=1), np.abs(rows * win).sum(axis=1)


def sum_squares(values):
  """S(v) in its one order: squares in double, tiles of 256 positions folded by the tree v[p] += v[p + s] (s = 128 .. 1) with +0.0
  past the end, tile sums added in tile order starting from +0.0."""
  sq = np.asarray(values, dtype=np.float64) ** 2
  tiles = -(-len(sq) // TILE)
  v = np.zeros((tiles, TILE), dtype=np.float64)
  v.reshape(-1)[:len(sq)] = sq
  s = TILE // 2
  while s >= 1:
    v = v[:, :s] + v[:, s:2 * s]
    s //= 2
  acc = 0.0
  for t in range(tiles):
    acc = acc + float(v[t, 0])
  return acc


def noise_of(bank, offsets, clip, offset, M):
  c = np.asarray(bank[offsets[clip]:offsets[clip + 1]])
  return c[(offset + np.arange(M, dtype=np.int64)) % len(c)]


def gain(sum_s, sum_n, M, lin):
  ps, pn = sum_s / M, sum_n / M
  if ps == 0.0 or pn == 0.0:
    return 0.0
  return math.sqrt(ps / (pn * lin))


def fmaf32(a, z, y):
  """fmaf(a, z, y) of float32 operands, correctly rounded: the product is exact in double, the sum is rounded to odd in double (its
  error is known exactly from the two-sum), and 53 bits rounded to odd round to 24 as the exact value would."""
  p = np.asarray(a, dtype=np.float32).astype(np.float64) * np.asarray(z, dtype=np.float32).astype(np.float64)
  s = np.asarray(y, dtype=np.float32).astype(np.float64)
  r = p + s
  b = r - p
  e = (p - (r - b)) + (s - b)
  even = (r.view(np.int64) & 1) == 0
  r = np.where((e != 0) & even, np.nextafter(r, np.where(e > 0, np.inf, -np.inf)), r)
  return r.astype(np.float32)


def block(seed, draw_id, index):
  seed, draw_id = int(seed) & (2 ** 64 - 1), int(draw_id) & (2 ** 64 - 1)
  return philox4x32_10([draw_id & M32, draw_id >> 32, index, 1], [seed & M32, seed >> 32])


def plan(speeds, noise_prob_q16, snr_centi, seed, draw_id, n, clip_lens, min_samples):
  r0, r1 = block(seed, draw_id, 0), block(seed, draw_id, 1)
  speed = uniform(r0[0], len(speeds) - 1)
  M = out_len(n, *speeds[speed])
  if M <= min_samples:
    speed, M = -1, n
  out = dict(speed=speed, M=M, noisy=0, clip=0, offset=0, snr_centi=0, lin=1.0)
  if len(clip_lens) and (r0[1] >> 16) < noise_prob_q16:
    clip = uniform(r0[2], len(clip_lens) - 1)
    snr = snr_centi[0] + uniform(r1[1], snr_centi[1] - snr_centi[0])
    out.update(noisy=1, clip=clip, offset=uniform(r1[0], int(clip_lens[clip]) - 1), snr_centi=snr, lin=math.pow(10.0, snr / 1000.0))
  return out
