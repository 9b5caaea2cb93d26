// SpecAugment (Park et al. 2019) as this library draws and applies it, shared by the gfx950 kernel and the host form of
// csrc/spec_augment.hip (st_spec_augment_f32 / st_spec_augment_host / st_spec_augment_plan_host).  Everything that decides a bit
// of the output is here: the generator, which word feeds which draw, the integer warp map and the one float expression of a warped
// row (an IEEE division, an IEEE subtraction and an explicit fmaf; contraction off), so that the device and the host form the same
// bits.  The specification in words: DESIGN.md "SpecAugment"; in numpy: tests/spec_augment_oracle.py.
//
// Per utterance of valid length L (its seq_len) and C channels, policy (W, F, mF, T, mT, p):
//   time warp   only if W > 0 and L >= 2W + 2: centre c in [W+1, L-W-1], displacement w in [-W, W], c' = c + w.  Output row t reads
//               source position s(t) = t c / c' (t <= c'), c + (t - c') (L-1-c) / (L-1-c') (t > c'), evaluated in integers:
//               i = num / den, r = num - i den (64-bit products); the row is x[i] when r == 0, else
//               fmaf((float)r / (float)den, x[i+1] - x[i], x[i]).  s(0) = 0, s(c') = c, s(L-1) = L-1; no row beyond L-1 is read.
//               The ends stay where they are: when the draw gives c' = L-1 (c = L-W-1 and w = W) the second piece has no output
//               row of its own and the first would end on s(L-1) = c, so row L-1 is pinned, s(L-1) = L-1, in every case.
//   freq masks  mF times: width f in [0, min(F, C)], start f0 in [0, C - f]; channels [f0, f0+f) of rows [0, L) become 0.
//   time masks  mT times: width t in [0, min(T, floor(p L))], start t0 in [0, L - t]; rows [t0, t0+t) become 0.
//               p is the 16.16 fixed-point integer p_q16 (0 .. 65536): floor(p L) = (p_q16 * L) >> 16.
//   Masks act on the warped utterance; rows at or past L are the source's rows, untouched.
//
// Randomness: Philox4x32-10.  key = {seed low word, seed high word}; counter = {draw id low word, draw id high word, block, 0}.
//   block 0          word 0 -> c = W + 1 + uniform(L - 2W - 2),  word 1 -> w = uniform(2W) - W        (words 2, 3 unused)
//   block 1 + k      frequency mask k (k < 8):  word 0 -> f,  word 1 -> f0                                 (words 2, 3 unused)
//   block 9 + k      time mask k (k < 8):       word 0 -> t,  word 1 -> t0                                 (words 2, 3 unused)
//   uniform(n), an integer in [0, n], of a 32-bit word x:  (x * (n + 1)) >> 32.
// Mask k's draws do not depend on how many masks the policy has, and nothing depends on the utterance's row in its batch, the
// batch size, the padded length or the other utterances: the draw id alone names the utterance's stream.
//
// Plan record of one utterance, int32 [2 + 2 (mF + mT)]: {c, w, (f0, f) x mF, (t0, t) x mT}; c = w = 0 when it is not warped.
#pragma once

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define ST_SA_HD __host__ __device__ __forceinline__
#else
#define ST_SA_HD inline
#endif

namespace st {

constexpr int SA_MAX_MASKS = 8;                      // per kind
constexpr int SA_FREQ_BLOCK = 1, SA_TIME_BLOCK = 1 + SA_MAX_MASKS;
constexpr int SA_PLAN_MAX = 2 + 4 * SA_MAX_MASKS;    // words of the longest plan record

struct SpecPolicy {
  int W, F, mF, T, mT, p_q16;
};

ST_SA_HD int sa_plan_words(const SpecPolicy& p) { return 2 + 2 * (p.mF + p.mT); }

// Philox4x32-10 (Salmon et al. 2011): ten rounds, the key bumped by the Weyl constants between them
ST_SA_HD void sa_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// block `block` of the utterance's stream
ST_SA_HD void sa_block(uint64_t seed, uint64_t draw_id, uint32_t block, uint32_t out[4]) {
  const uint32_t ctr[4] = {(uint32_t)draw_id, (uint32_t)(draw_id >> 32), block, 0u};
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  sa_philox(ctr, key, out);
}

// an integer in [0, n] (n >= 0) of one 32-bit word
ST_SA_HD int sa_uniform(uint32_t x, int n) { return (int)(((uint64_t)x * (uint64_t)((uint32_t)n + 1u)) >> 32); }

ST_SA_HD bool sa_warps(const SpecPolicy& p, int L) { return p.W > 0 && (int64_t)L >= 2 * (int64_t)p.W + 2; }

// Entry e of the plan, a pair of words: e = 0 is (c, w), 1 .. mF the frequency masks, mF + 1 .. mF + mT the time
// masks; one Philox block each, so one lane per entry on the device.
ST_SA_HD void sa_plan_entry(const SpecPolicy& p, uint64_t seed, uint64_t draw_id, int L, int C, int e, int& first, int& second) {
  uint32_t r[4];
  if (e == 0) {
    first = second = 0;
    if (!sa_warps(p, L)) return;
    sa_block(seed, draw_id, 0u, r);
    first = p.W + 1 + sa_uniform(r[0], L - 2 * p.W - 2);
    second = sa_uniform(r[1], 2 * p.W) - p.W;
  } else if (e <= p.mF) {
    sa_block(seed, draw_id, (uint32_t)(SA_FREQ_BLOCK + e - 1), r);
    const int f = sa_uniform(r[0], p.F < C ? p.F : C);
    first = sa_uniform(r[1], C - f);
    second = f;
  } else {
    sa_block(seed, draw_id, (uint32_t)(SA_TIME_BLOCK + e - 1 - p.mF), r);
    const int cap = (int)(((int64_t)p.p_q16 * (int64_t)L) >> 16);
    const int t = sa_uniform(r[0], p.T < cap ? p.T : cap);
    first = sa_uniform(r[1], L - t);
    second = t;
  }
}

// What output row t of an utterance is made of.
enum { SA_ROW_COPY = 0,      // the source's row t as it is (t >= L)
       SA_ROW_VALID = 1,     // source row(s) i (and i + 1 when frac != 0), then the frequency masks
       SA_ROW_ZERO = 2 };    // inside a time mask: zeros, nothing is read
struct SpecRow {
  int kind, i;
  float frac;                // (float)r / (float)den; 0 exactly when the row is x[i]
};

// `plan`: the utterance's record.  0 <= t; 0 <= L.
ST_SA_HD SpecRow sa_row(const SpecPolicy& p, const int* plan, int L, int t) {
#pragma clang fp contract(off)
  SpecRow row = {SA_ROW_COPY, t, 0.f};
  if (t >= L) return row;
  const int* tm = plan + 2 + 2 * p.mF;
  for (int k = 0; k < p.mT; ++k)
    if (t >= tm[2 * k] && t < tm[2 * k] + tm[2 * k + 1]) {
      row.kind = SA_ROW_ZERO;
      return row;
    }
  row.kind = SA_ROW_VALID;
  const int c = plan[0], w = plan[1];
  if (c == 0 || t == L - 1) return row;              // not warped; the last row stays the last row (c' = L - 1 included)
  const int cw = c + w;
  int64_t num, den;
  int base;
  if (t <= cw) { num = (int64_t)t * c; den = cw; base = 0; }
  else { num = (int64_t)(t - cw) * (L - 1 - c); den = L - 1 - cw; base = c; }
  // (the same integers either way: products below 2^32 -- every padded length up to 65 535 frames -- take the 32-bit division, which
  // costs the device a tenth of the 64-bit one)
  const int64_t q = ((uint64_t)num >> 32) == 0 ? (int64_t)((uint32_t)num / (uint32_t)den) : num / den;
  const int64_t r = num - q * den;
  row.i = base + (int)q;
  row.frac = r == 0 ? 0.f : (float)r / (float)den;
  return row;
}

// one element of a warped row: x0 = x[i], x1 = x[i + 1]
ST_SA_HD float sa_lerp(float frac, float x0, float x1) {
#pragma clang fp contract(off)
  return fmaf(frac, x1 - x0, x0);
}

// The utterance's frequency masks as channel intervals [lo, hi), taken out of the plan once (on the device: into registers, so
// that the test per element is compares only, and none at all for a policy without frequency masks).
struct SpecFreqMasks {
  int n;
  int lo[SA_MAX_MASKS], hi[SA_MAX_MASKS];
};

ST_SA_HD SpecFreqMasks sa_freq_masks(const SpecPolicy& p, const int* plan) {
  SpecFreqMasks m;
  m.n = p.mF;
#pragma unroll
  for (int k = 0; k < SA_MAX_MASKS; ++k) {
    const bool on = k < p.mF;
    m.lo[k] = on ? plan[2 + 2 * k] : 0;
    m.hi[k] = on ? plan[2 + 2 * k] + plan[3 + 2 * k] : 0;
  }
  return m;
}

// is channel ch inside one of them?
ST_SA_HD bool sa_channel_masked(const SpecFreqMasks& m, int ch) {
  bool masked = false;
#pragma unroll
  for (int k = 0; k < SA_MAX_MASKS; ++k) {
    if (k >= m.n) break;                             // (the same for every lane: a scalar branch on the device)
    masked |= ch >= m.lo[k] && ch < m.hi[k];
  }
  return masked;
}

}  // namespace st
