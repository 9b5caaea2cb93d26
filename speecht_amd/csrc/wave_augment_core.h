// Waveform augmentation for training (speed perturbation, additive noise at a drawn SNR) as this library defines it, shared by the
// gfx950 kernels and the host form of csrc/wave_augment.hip (st_wave_augment_f32 / st_wave_augment_host /
// st_wave_augment_plan_host).  Everything that decides a bit of the output is here: which word feeds which draw, the integer time
// map of a speed, the order of the taps, the order of the power sums and the one expression of the gain (explicit fmaf, contraction
// off), so that the device and the host form the same bits.  In words: DESIGN.md "Waveform augmentation"; in numpy:
// tests/wave_augment_oracle.py.
//
// Speed.  A speed is a reduced fraction num/den, 1 <= num, den <= 32, 1/2 <= num/den <= 2.  An utterance of n samples becomes
//   M = ceil(n den / num) samples.  Output m sits at input time m num / den = i + phi / den, i = (m num) div den, phi = (m num) mod den
//   (64-bit integers).  With H = ceil(16 max(1, num/den)) and the speed's table h [den][2H] (float32, made by the caller: a Kaiser-
//   windowed sinc, every row divided by its own sum -- neither form ever evaluates a sinc or a Bessel function),
//     y[m] = acc after  acc = 0;  for k = 0 .. 2H-1: acc = fmaf(h[phi][k], x[i - H + 1 + k], acc)          (float32, in that order)
//   where a source outside [0, n) reads 0.  The speed 1/1 is the copy, bit for bit (its table is never read).
//
// Noise.  A bank is one float32 array of clips (clip k = noise[clip_offsets[k] .. clip_offsets[k+1]), at least one sample each).  A
//   noisy utterance reads clip k circularly from offset o: z[m] = clip_k[(o + m) mod len_k].  With y the M speed-changed samples,
//     Ps = S(y) / M,  Pn = S(z) / M,  a = sqrt(Ps / (Pn lin)), a = 0 when Ps or Pn is 0      (IEEE double; lin = 10^(snr/10))
//     out[m] = fmaf((float)a, z[m], y[m])
//   S(v), the sum of squares of M values, has ONE order: the squares are formed in double (exact), tiles of 256 consecutive
//   positions are folded each by the tree  for s = 128, 64, .. 1: v[p] += v[p + s] (p < s)  with +0.0 at positions past M, and the
//   tile sums are added one after the other in tile order, starting from +0.0.  Nothing depends on the grid, the batch
//   or the utterance's row.
//
// Randomness: Philox4x32-10 (sa_philox of spec_augment_core.h).  key = seed; counter = {draw id low, draw id high, block, 1} -- word 3
//   is 1 where SpecAugment has 0, so one seed and one draw id give the two augmentations different streams.
//   block 0   word 0 -> speed index = uniform(n_speeds - 1),  word 1 -> noisy iff (word >> 16) < noise_prob_q16,
//             word 2 -> clip = uniform(n_clips - 1)
//   block 1   word 0 -> offset = uniform(len_clip - 1),  word 1 -> SNR in hundredths of a dB = snr_lo + uniform(snr_hi - snr_lo)
//   One rule of feasibility: a drawn speed that would leave M <= min_samples is replaced by 1/1 (speed index -1).
//   The plan is made on the HOST only (the caller sizes its buffers by M, and pow(10, .) stays off the device) and uploaded.
#pragma once

#include <math.h>
#include <stdint.h>

#include "spec_augment_core.h"

namespace st {

constexpr int WA_TILE = 256;                         // positions per tile of the power sums
constexpr int WA_MAX_TERM = 32;                      // largest numerator and denominator of a speed
constexpr int WA_MAX_TAPS = 64;                      // 2 H at the speed 2/1
constexpr int WA_MAX_SPEEDS = 8;                     // speeds of one policy

// one utterance's plan, 40 bytes; the kernel reads it from device memory
struct WavePlan {
  int64_t M;                                         // output samples
  int64_t offset;                                    // first sample of the clip (0 .. len - 1)
  double lin;                                        // 10^(snr / 10)
  int32_t speed;                                     // index into the policy's speeds; -1: 1/1
  int32_t noisy;
  int32_t clip;
  int32_t snr_centi;                                 // the drawn SNR in hundredths of a dB (0 when not noisy)
};

struct WavePolicy {
  int n_speeds;
  int num[WA_MAX_SPEEDS], den[WA_MAX_SPEEDS];
  int noise_prob_q16;                                // 0 .. 65536
  int snr_lo, snr_hi;                                // hundredths of a dB
};

ST_SA_HD int wa_half_width(int num, int den) { return num <= den ? 16 : (16 * num + den - 1) / den; }
ST_SA_HD int64_t wa_out_len(int64_t n, int num, int den) { return (n * den + num - 1) / num; }
ST_SA_HD bool wa_speed_ok(int num, int den) {
  if (num < 1 || den < 1 || num > WA_MAX_TERM || den > WA_MAX_TERM || 2 * num < den || num > 2 * den) return false;
  int a = num, b = den;
  while (b) { const int t = a % b; a = b; b = t; }
  return a == 1;
}
// floats of one speed's table
ST_SA_HD int wa_table_floats(int num, int den) { return den * 2 * wa_half_width(num, den); }

ST_SA_HD void wa_block(uint64_t seed, uint64_t draw_id, uint32_t block, uint32_t out[4]) {
  const uint32_t ctr[4] = {(uint32_t)draw_id, (uint32_t)(draw_id >> 32), block, 1u};
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  sa_philox(ctr, key, out);
}

// The plan of an utterance of n samples (host only: pow).  clip_lens: n_clips lengths, each 1 .. 2^31 - 1; none when n_clips = 0
// (then nothing is noisy).
inline WavePlan wa_plan(const WavePolicy& p, uint64_t seed, uint64_t draw_id, int64_t n, const int64_t* clip_lens, int n_clips,
                        int64_t min_samples) {
  uint32_t r0[4], r1[4];
  wa_block(seed, draw_id, 0u, r0);
  WavePlan plan = {n, 0, 1.0, sa_uniform(r0[0], p.n_speeds - 1), 0, 0, 0};
  plan.M = wa_out_len(n, p.num[plan.speed], p.den[plan.speed]);
  if (plan.M <= min_samples) {
    plan.speed = -1;
    plan.M = n;
  }
  if (n_clips > 0 && (int)(r0[1] >> 16) < p.noise_prob_q16) {
    wa_block(seed, draw_id, 1u, r1);
    plan.noisy = 1;
    plan.clip = sa_uniform(r0[2], n_clips - 1);
    plan.offset = sa_uniform(r1[0], (int)(clip_lens[plan.clip] - 1));
    plan.snr_centi = p.snr_lo + sa_uniform(r1[1], p.snr_hi - p.snr_lo);
    plan.lin = pow(10.0, (double)plan.snr_centi / 1000.0);
  }
  return plan;
}

// output sample of phase row `h` (2H taps) over the window x[0 .. 2H) (x[k] = source i - H + 1 + k, 0 outside the utterance)
template <typename Row, typename Win>
ST_SA_HD float wa_taps(const Row& h, const Win& x, int taps) {
#pragma clang fp contract(off)
  float acc = 0.f;
  for (int k = 0; k < taps; ++k) acc = fmaf(h[k], x[k], acc);
  return acc;
}

ST_SA_HD double wa_square(float v) {
#pragma clang fp contract(off)
  return (double)v * (double)v;
}

// the tree of one tile, in place; v[0] is the tile's sum
ST_SA_HD double wa_tile_tree(double* v) {
#pragma clang fp contract(off)
  for (int s = WA_TILE / 2; s >= 1; s >>= 1)
    for (int p = 0; p < s; ++p) v[p] = v[p] + v[p + s];
  return v[0];
}

// `tiles` more tile sums (`stride` doubles apart) added to acc in tile order
ST_SA_HD double wa_fold_tiles(double acc, const double* sums, int tiles, int stride) {
#pragma clang fp contract(off)
  for (int t = 0; t < tiles; ++t) acc = acc + sums[t * stride];
  return acc;
}

ST_SA_HD double wa_gain(double sum_s, double sum_n, int64_t M, double lin) {
#pragma clang fp contract(off)
  const double ps = sum_s / (double)M, pn = sum_n / (double)M;
  if (ps == 0.0 || pn == 0.0) return 0.0;
  return sqrt(ps / (pn * lin));
}

ST_SA_HD float wa_mix(float a, float z, float y) {
#pragma clang fp contract(off)
  return fmaf(a, z, y);
}

// position r mod len in a clip of `len` samples, for any r (the division is skipped where r is already inside the clip)
ST_SA_HD uint32_t wa_wrap(uint32_t r, uint32_t len) { return r >= len ? r % len : r; }

}  // namespace st
