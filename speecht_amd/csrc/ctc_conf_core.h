// The arithmetic of the CTC word confidences, shared by the gfx950 kernels and the host form of csrc/ctc_conf.hip
// (st_ctc_word_conf_f32 / st_ctc_word_conf_host).  Everything that decides a bit is here and is written with IEEE double
// +, -, *, / and comparisons, exact bit moves and the al_* functions of ctc_align_core.h only (contraction off, no library
// exp / log), so that the device and the host return the same bits.
//
// Lattice (semantics: include/speecht_hip.h, tests/conf_oracle.py): the sum-product CTC forward recursion in the LINEAR
// domain.  A state's value is m * 2^e: m a double in [1, 2) (0: no path reaches the state), e an int of its own per state,
// so that nothing can underflow whatever the frame count and rescaling is a move of exponent bits -- exact.
//   a_0(u) = p_0(class(u)) for u < 2, 0 otherwise
//   a_t(u) = ((a_{t-1}(u) + a_{t-1}(u-1)) + [label(u) != label(u-2)] a_{t-1}(u-2)) * p_t(class(u))
// The three terms are brought to the largest of their exponents first (a term more than 1000 binades below it counts as 0).
// p_t(c) = al_exp(x_c - max x) / sum, the sum in the order of al_row_sum; the emission of the pseudo-label of a word is the
// al_row_sum of the row's p_t(c) with p_t(space) and the padding set to 0.
#pragma once

#include "ctc_align_core.h"

namespace st {

constexpr int CF_CP = AL_CP;             // doubles per softmax row: classes 0 .. C-1 (C <= 30), the two columns below
constexpr int CF_STAR = 30;              // column (and pseudo id) of a word's pseudo-label: sum of p_t(c), c != space
constexpr int CF_DEAD = 31;              // column that holds 0: the blanks beside the pseudo-label, states beyond the lattice
constexpr int CF_MAX_CLASSES = 30;
#define ST_CF_NAN (__builtin_nan(""))
constexpr int CF_EZ = -(1 << 28);        // exponent of a zero state: below anything a path reaches, differences stay in int range

// m * 2^d for d <= 0, exact; 0 when the term lies more than 1000 binades below the one it is added to
ST_AL_HD double cf_scale(double m, int d) {
#pragma clang fp contract(off)
  return d > -1000 ? m * al_from_bits((long long)(d + 1023) << 52) : 0.0;
}

// v * 2^E as (m in [1, 2), exponent); v <= 0, NaN or below the normal numbers: the zero state
ST_AL_HD void cf_norm(double v, int E, double& m, int& e) {
  if (!(v >= 2.2250738585072014e-308)) { m = 0.0; e = CF_EZ; return; }
  const long long b = al_bits(v);
  m = al_from_bits((b & 0x000fffffffffffffLL) | 0x3ff0000000000000LL);
  e = E + (int)((b >> 52) & 0x7ff) - 1023;
}

// p_t(c) of one class: ex = al_exp(x_c - max x), s the row's sum of them
ST_AL_HD double cf_prob(double ex, double s) {
#pragma clang fp contract(off)
  return ex / s;
}

// One lattice cell: ((stay + advance) + skip) * emission
ST_AL_HD void cf_cell(double m0, int e0, double m1, int e1, double m2, int e2, bool skip_ok, double emission, double& m,
                      int& e) {
#pragma clang fp contract(off)
  if (!skip_ok) { m2 = 0.0; e2 = CF_EZ; }
  int E = e0 > e1 ? e0 : e1;
  E = E > e2 ? E : e2;
  const double s = (cf_scale(m0, e0 - E) + cf_scale(m1, e1 - E)) + cf_scale(m2, e2 - E);
  cf_norm(s * emission, E, m, e);
}

// ln(m * 2^e) for m in [1, 4)
ST_AL_HD double cf_ln(double m, int e) {
#pragma clang fp contract(off)
  const double lm = al_log(m);
  const double ed = (double)e;
  return ed * AL_LN2_HI + (lm + ed * AL_LN2_LO);
}

// ln of the lattice's probability: last blank + last label (0, CF_EZ for a lattice of one state); -inf when no path ends
ST_AL_HD double cf_total(double mb, int eb, double ml, int el) {
#pragma clang fp contract(off)
  const int E = eb > el ? eb : el;
  const double s = cf_scale(mb, eb - E) + cf_scale(ml, el - E);
  if (!(s > 0.0)) return ST_AL_NEG_INF;
  return cf_ln(s, E);
}

// log_conf of a word: min(0, ln P(l) - ln P(l with the word replaced)); -inf when P(l) = 0; a job that was not run (NaN)
// gives the one NaN of ST_CF_NAN, not what a subtraction makes of it
ST_AL_HD double cf_log_conf(double ln_p, double ln_p_star) {
#pragma clang fp contract(off)
  if (!(ln_p == ln_p) || !(ln_p_star == ln_p_star)) return ST_CF_NAN;
  if (ln_p == ST_AL_NEG_INF) return ST_AL_NEG_INF;
  const double d = ln_p - ln_p_star;
  return d > 0.0 ? 0.0 : d;
}

// The label array of a job: `first` .. `last`-1 of lab replaced by one CF_STAR (first < 0: lab itself).  Ids outside
// 0 .. blank-1 read the dead column: such a label is the caller's error and must not index outside a row.
ST_AL_HD int cf_job_label(const int* lab, int i, int first, int last, int blank) {
  if (first >= 0 && i == first) return CF_STAR;
  const int id = lab[first >= 0 && i > first ? i + (last - first - 1) : i];
  return (unsigned)id < (unsigned)blank ? id : CF_DEAD;
}

// column of state u of a job's lattice (lab2: what cf_job_label made, L2 ids): a blank beside the pseudo-label is dead
ST_AL_HD int cf_state_column(int u, const int* lab2, int L2, int blank) {
  if (u & 1) return lab2[(u - 1) >> 1];
  const int k = u >> 1;                                   // the blank between labels k-1 and k
  const bool dead = (k > 0 && lab2[k - 1] == CF_STAR) || (k < L2 && lab2[k] == CF_STAR);
  return dead ? CF_DEAD : blank;
}

}  // namespace st
