// The arithmetic of the CTC best-path (Viterbi) alignment, shared by the gfx950 kernels and the host form of
// csrc/ctc_align.hip (st_ctc_align_f32 / st_ctc_align_host).  Everything that decides which path wins is here and is written
// with IEEE double +, -, *, / and comparisons only (contraction off, no library exp / log), so that the device and the host
// form the same bits and therefore choose the same path, ties included.
//
// Lattice (semantics: include/speecht_hip.h, tests/align_oracle.py): states u = 0 .. 2L, even = blank, odd = label (u-1)/2.
//   v_0(u) = ly_0(class(u)) for u < 2, -inf otherwise
//   v_t(u) = max(v_{t-1}(u), v_{t-1}(u-1), [label(u) != label(u-2)] v_{t-1}(u-2)) + ly_t(class(u))
// Ties go to the smaller move (stay, advance, skip); the move taken is the back-pointer (0, 1, 2).
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define ST_AL_HD __host__ __device__ __forceinline__
#else
#define ST_AL_HD inline
#endif

namespace st {

constexpr int AL_CP = 32;                            // classes per log-softmax row (C <= 32, the rest is padding)
#define ST_AL_NEG_INF (-__builtin_inf())

ST_AL_HD double al_from_bits(long long b) { return __builtin_bit_cast(double, b); }
ST_AL_HD long long al_bits(double x) { return __builtin_bit_cast(long long, x); }

constexpr double AL_LN2_HI = 6.93147180369123816490e-01;   // 32 significant bits: k * AL_LN2_HI is exact for |k| < 2^20
constexpr double AL_LN2_LO = 1.90821492927058770002e-10;

// e^x for x <= 0 (0 below -700, and for NaN): x = k ln2 + r, |r| <= 0.35, Taylor to r^13 (remainder < 4e-18), times 2^k.
ST_AL_HD double al_exp(double x) {
#pragma clang fp contract(off)
  if (!(x > -700.0)) return 0.0;
  const long long k = (long long)(x * 1.44269504088896338700e+00 - 0.5);
  const double kd = (double)k;
  double r = x - kd * AL_LN2_HI;
  r = r - kd * AL_LN2_LO;
  double p = 1.0 / 6227020800.0;
  p = p * r + 1.0 / 479001600.0;
  p = p * r + 1.0 / 39916800.0;
  p = p * r + 1.0 / 3628800.0;
  p = p * r + 1.0 / 362880.0;
  p = p * r + 1.0 / 40320.0;
  p = p * r + 1.0 / 5040.0;
  p = p * r + 1.0 / 720.0;
  p = p * r + 1.0 / 120.0;
  p = p * r + 1.0 / 24.0;
  p = p * r + 1.0 / 6.0;
  p = p * r + 0.5;
  p = p * r + 1.0;
  p = p * r + 1.0;
  return p * al_from_bits((k + 1023) << 52);          // k >= -1011: a normal number
}

// ln s for a normal s >= 1 (here: a sum of at most 32 terms in [0, 1], one of them 1): s = m 2^e, m in (sqrt(1/2), sqrt(2)],
// ln m = 2 atanh(f), f = (m - 1) / (m + 1), |f| <= 0.172, series to f^23 (remainder < 1e-19).
ST_AL_HD double al_log(double s) {
#pragma clang fp contract(off)
  const long long b = al_bits(s);
  long long e = ((b >> 52) & 0x7ff) - 1023;
  double m = al_from_bits((b & 0x000fffffffffffffLL) | 0x3ff0000000000000LL);
  if (m > 1.41421356237309514547) { m = m * 0.5; e += 1; }
  const double f = (m - 1.0) / (m + 1.0);
  const double f2 = f * f;
  double q = 1.0 / 23.0;
  q = q * f2 + 1.0 / 21.0;
  q = q * f2 + 1.0 / 19.0;
  q = q * f2 + 1.0 / 17.0;
  q = q * f2 + 1.0 / 15.0;
  q = q * f2 + 1.0 / 13.0;
  q = q * f2 + 1.0 / 11.0;
  q = q * f2 + 1.0 / 9.0;
  q = q * f2 + 1.0 / 7.0;
  q = q * f2 + 1.0 / 5.0;
  q = q * f2 + 1.0 / 3.0;
  q = q * f2 + 1.0;
  const double lm = 2.0 * f * q;
  const double ed = (double)e;
  return ed * AL_LN2_HI + (lm + ed * AL_LN2_LO);
}

// One class of a log-softmax row: v the logit, m the row's largest logit, s = sum_c al_exp(v_c - m) added as al_row_sum adds.
ST_AL_HD double al_log_softmax(float v, float m, double s) {
#pragma clang fp contract(off)
  const double lz = (double)m + al_log(s);
  return (double)v - lz;
}

// The row sum in the order of a 32-lane xor butterfly (16, 8, 4, 2, 1), which is how the kernel adds: every lane of the
// butterfly ends with the value this fold leaves in e[0] (a + b == b + a bit for bit).
inline double al_row_sum(double (&e)[AL_CP]) {
#pragma clang fp contract(off)
  for (int o = AL_CP / 2; o > 0; o >>= 1)
    for (int c = 0; c < o; ++c) e[c] = e[c] + e[c + o];
  return e[0];
}

// One lattice cell: the best predecessor (ties: stay, then advance, then skip) plus the emission; bp = the move taken.
ST_AL_HD double al_cell(double stay, double adv, double skip, bool skip_ok, double emission, int& bp) {
  double best = stay;
  bp = 0;
  if (adv > best) { best = adv; bp = 1; }
  if (skip_ok && skip > best) { best = skip; bp = 2; }
  return best + emission;
}

// The end state of a lattice of U = 2L+1 states: the last label state unless the last blank is strictly better.
ST_AL_HD int al_end_state(int U, double last_blank, double last_label) {
  return (U > 1 && last_label >= last_blank) ? U - 2 : U - 1;
}

// what `states` holds for lattice state u: the label index, -1 for a blank
ST_AL_HD int al_state_label(int u) { return (u & 1) ? (u >> 1) : -1; }

// ---- the wildcard entry points (st_ctc_align_wild_f32 / st_ctc_align_long_wild_f32) ----
// The wildcard is the id C, one past the blank: its emission is slot C of the [32] row, the row's largest ln-softmax value plus
// the bias.  al_log_softmax(m, m, s) IS that largest value: the row maximum of the logits gives the maximum of the row.
ST_AL_HD double al_wild_emission(float m, double s, double bias) {
#pragma clang fp contract(off)
  return al_log_softmax(m, m, s) + bias;
}

// The largest of the C ln-softmax values of one row (a selection: the same bits in any order of the comparisons, up to the
// sign of a zero, which the sum below does not see).
ST_AL_HD double al_row_max(const double* row, int C) {
  double m = row[0];
  for (int c = 1; c < C; ++c) m = row[c] > m ? row[c] : m;
  return m;
}

// The fit of one label of class c whose span is frames [a, b) of `rows` ([frames][32], slot C = the row maximum, written by the
// row-maximum pass after the back-trace): sum in frame order of ly_t(c) - max_c ly_t(c), 0 where the greedy reading agrees on
// every frame, negative otherwise.  A wildcard (c == C) has the closed form bias * frames; an id outside 0..C gives NaN.
// a and b are clipped to [0, frames_hi] by the caller's choice of frames_hi, so spans a lattice of score -inf left unspecified
// read no row outside the utterance.
ST_AL_HD double al_label_fit(const double* rows, int c, int C, int a, int b, int frames_hi, double bias) {
#pragma clang fp contract(off)
  a = a < 0 ? 0 : a;
  b = b > frames_hi ? frames_hi : b;
  if ((unsigned)c > (unsigned)C) return __builtin_nan("");
  if (c == C) return bias * (double)(b > a ? b - a : 0);
  double f = 0.0;
  for (int t = a; t < b; ++t) f = f + (rows[(long)t * AL_CP + c] - rows[(long)t * AL_CP + C]);
  return f;
}

}  // namespace st
