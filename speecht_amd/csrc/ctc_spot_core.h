// The arithmetic of keyword spotting, shared by the gfx950 kernels and the host form of csrc/ctc_spot.hip (st_ctc_spot_f32 /
// st_ctc_spot_host).  Everything that decides a bit of the outputs is here and is written with IEEE double +, - and comparisons
// only (contraction off; there is no exp or log in this feature), so that the device and the host form the same bits, ties
// included.
//
// Lattice (semantics: include/speecht_hip.h, tests/spot_oracle.py): the 2L+1 CTC states of the keyword, even = blank, odd =
// label (u-1)/2; states 0 and 2L are dead -- an occurrence begins on the first label and ends on the last.  Each live state
// carries a value and the frame its path began on:
//   d_t(c)  = (double)x_t(c) - (double)max_c x_t(c)                       (<= 0; the softmax normaliser cancels)
//   v_t(u)  = best + d_t(class(u)),  best over stay, advance, skip ([label(u) != label(u-2)]) and, for u = 1, enter = 0.0 with
//             start t -- in this order, replaced only by a strictly larger value; the start is -1 where best is -inf
//   end_t   = v_t(2L-1); the result is the largest finite end_t, the LATEST t among equals.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define ST_SP_HD __host__ __device__ __forceinline__
#else
#define ST_SP_HD inline
#endif

namespace st {

constexpr int SP_CP = 32;                            // classes per row of d (C <= 32, the rest is -inf)
#define ST_SP_NEG_INF (-__builtin_inf())

// d of one class: x the logit, m the row's largest logit
ST_SP_HD double sp_ratio(float x, float m) {
#pragma clang fp contract(off)
  return (double)x - (double)m;
}

// the row of d a state reads: its class, kept inside the row whatever the id says (ids outside 0 .. C-2 are the caller's error)
ST_SP_HD int sp_column(int cls) { return cls & (SP_CP - 1); }

// One lattice cell of frame t.  `live`: u in 1 .. 2L-1; `enter`: u == 1.
ST_SP_HD void sp_cell(double stay, int stay_start, double adv, int adv_start, double skip, int skip_start, bool skip_ok, bool enter,
                      bool live, int t, double d, double& v, int& start) {
#pragma clang fp contract(off)
  double best = stay;
  int s = stay_start;
  if (adv > best) { best = adv; s = adv_start; }
  if (skip_ok && skip > best) { best = skip; s = skip_start; }
  if (enter && 0.0 > best) { best = 0.0; s = t; }
  if (best == ST_SP_NEG_INF) s = -1;
  v = live ? best + d : ST_SP_NEG_INF;
  start = live ? s : -1;
}

// The running best over the end frames: a finite end_t replaces an equal one (the latest frame among equals wins).
ST_SP_HD void sp_running_best(double end, int end_start, int t, double& best, int& best_start, int& best_end) {
  if (end > ST_SP_NEG_INF && end >= best) { best = end; best_start = end_start; best_end = t + 1; }
}

// what a job is: (utterance, keyword) of the job table, refused when either lies outside its table, the keyword is empty or
// does not fit the UP states the lattice was dispatched for, or the utterance's length lies outside 0 .. T
struct SpotJob {
  int b, L, Tb;
  long first;          // of the keyword's ids in kw_ids
  bool ok;
};
ST_SP_HD SpotJob sp_job(const int* jobs, int job, int B, int T, int n_keywords, const int* kw_off, const int* seq_lens, int UP) {
  SpotJob j{jobs[2 * (long)job], 0, 0, 0, false};
  const int k = jobs[2 * (long)job + 1];
  if (j.b < 0 || j.b >= B || k < 0 || k >= n_keywords) return j;
  j.first = kw_off[k];
  j.L = (int)((unsigned)kw_off[k + 1] - (unsigned)kw_off[k]);
  j.Tb = seq_lens[j.b];
  j.ok = j.L >= 1 && j.L <= 511 && 2 * j.L + 1 <= UP && j.Tb >= 0 && j.Tb <= T && j.first >= 0 &&
         j.first + j.L <= (long)kw_off[n_keywords];          // (offsets that are not monotone refuse their keywords)
  return j;
}

}  // namespace st
