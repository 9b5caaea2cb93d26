// The log-softmax rows of the alignment lattices, shared by csrc/ctc_align.hip (st_ctc_align_f32) and csrc/ctc_align_long.hip
// (st_ctc_align_long_f32): one lane per (row, class), ln softmax in double into [B*T][32].  The arithmetic is
// ctc_align_core.h's; each file that includes this header gets its own copy of the kernel.
//
// The wildcard entry points (st_ctc_align_wild_f32, st_ctc_align_long_wild_f32) run the WILD form, whose lane c == C also writes
// slot C of the row -- the emission of the wildcard id C -- and, after the back-trace, the two kernels of the fit stage below.
#pragma once

#include "ctc_align_core.h"
#include "ctc_lattice.h"

namespace st {

// ln softmax of every (b, t) row, two rows per wavefront; sums by a 32-lane xor butterfly (the order of st::al_row_sum).  `map` names
// the row: a RowMap for a padded NWC tensor, a RingMap (stream_ring.h) for utterances kept in a stream's ring.
// WILD (C <= 31): lane C writes al_wild_emission = the row's largest value + bias where the plain form writes -inf.
template <typename Map, bool WILD = false>
__device__ __forceinline__ void align_logsoftmax_rows(const float* __restrict__ logits, const Map& map, int B, int T, int C,
                                                      double* __restrict__ ly, double bias = 0.0) {
  const int lane = threadIdx.x & 63, c = lane & 31;
  const long i = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + (lane >> 5);
  const bool row_ok = i < (long)B * T;
  const long ii = row_ok ? i : (long)B * T - 1;
  const int b = (int)(ii / T), t = (int)(ii - (long)b * T);
  const float v = c < C ? logits[map.off(b, t) + c] : -__builtin_inff();
  float m = v;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  double s = c < C ? al_exp((double)v - (double)m) : 0.0;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
  if constexpr (WILD) {
    if (row_ok) ly[i * AL_CP + c] = c == C ? al_wild_emission(m, s, bias) : al_log_softmax(v, m, s);
  } else {
    if (row_ok) ly[i * AL_CP + c] = al_log_softmax(v, m, s);
  }
}

static __global__ __launch_bounds__(256) void align_logsoftmax_kernel(const float* __restrict__ logits, RowMap map, int B, int T,
                                                                      int C, double* __restrict__ ly) {
  align_logsoftmax_rows(logits, map, B, T, C, ly);
}

static __global__ __launch_bounds__(256) void align_logsoftmax_wild_kernel(const float* __restrict__ logits, RowMap map, int B, int T,
                                                                           int C, double bias, double* __restrict__ ly) {
  align_logsoftmax_rows<RowMap, true>(logits, map, B, T, C, ly, bias);
}

// The fit stage, first kernel: after the back-trace nothing reads the wildcard's emission any more, and slot C of every row
// becomes the row's largest ln-softmax value (same geometry as above: two rows per wavefront, a 32-lane butterfly of selections).
static __global__ __launch_bounds__(256) void align_rowmax_kernel(double* __restrict__ ly, long rows, int C) {
  const int lane = threadIdx.x & 63, c = lane & 31;
  const long i = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + (lane >> 5);
  const bool row_ok = i < rows;
  double m = row_ok && c < C ? ly[i * AL_CP + c] : ST_AL_NEG_INF;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) {
    const double other = __shfl_xor(m, o, 64);
    m = other > m ? other : m;
  }
  if (row_ok && c == C) ly[i * AL_CP + C] = m;
}

}  // namespace st
