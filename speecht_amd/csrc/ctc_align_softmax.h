// The log-softmax rows of the alignment lattices, shared by csrc/ctc_align.hip (st_ctc_align_f32) and csrc/ctc_align_long.hip
// (st_ctc_align_long_f32): one lane per (row, class), ln softmax in double into [B*T][32].  The arithmetic is
// ctc_align_core.h's; each file that includes this header gets its own copy of the kernel.
#pragma once

#include "ctc_align_core.h"
#include "ctc_lattice.h"

namespace st {

// ln softmax of every (b, t) row, two rows per wavefront; sums by a 32-lane xor butterfly (the order of st::al_row_sum).  `map` names
// the row: a RowMap for a padded NWC tensor, a RingMap (stream_ring.h) for utterances kept in a stream's ring.
template <typename Map>
__device__ __forceinline__ void align_logsoftmax_rows(const float* __restrict__ logits, const Map& map, int B, int T, int C,
                                                      double* __restrict__ ly) {
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
  if (row_ok) ly[i * AL_CP + c] = al_log_softmax(v, m, s);
}

static __global__ __launch_bounds__(256) void align_logsoftmax_kernel(const float* __restrict__ logits, RowMap map, int B, int T,
                                                                      int C, double* __restrict__ ly) {
  align_logsoftmax_rows(logits, map, B, T, C, ly);
}

}  // namespace st
