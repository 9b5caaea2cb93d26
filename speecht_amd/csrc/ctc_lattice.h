// The one-wave-per-utterance CTC lattice scaffolding shared by ctc.hip (alpha / beta), ctc_align.hip (Viterbi, back-trace and the
// host form) and, for the row map, ctc_beam.hip: the row map, the states-per-lane dispatch list, what a state is (class, skips),
// which labels refuse an utterance, the DPP move between neighbouring lanes and the stage that brings 64-frame chunks of rows to
// LDS.  What a recursion computes stays with its kernel, and so does the gather of a lane's neighbour states, written out in
// each frame loop.  The first half compiles with a plain C++ compiler (tests/host_cpp/ctc_lattice_check.cpp).
#pragma once

#include <stdint.h>

#include <type_traits>

#include "speecht_hip.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define ST_LAT_HD __host__ __device__ __forceinline__
#else
#define ST_LAT_HD inline
#endif

namespace st {

// (b, t) -> float offset of a row of a padded NWC tensor
struct RowMap {
  long batch_stride;
  long row0;
  int row_stride;
  ST_LAT_HD long off(int b, int t) const { return (long)b * batch_stride + row0 + (long)t * row_stride; }
};
inline RowMap row_map(const st_tensor3& t) {
  return RowMap{(long)t.t_pitch * t.c_pitch, (long)t.halo * t.c_pitch, t.c_pitch};
}

// States per lane (KPL) the lattice kernels are instantiated for: 64 * KPL states hold labels of up to 32 * KPL - 1 ids.
#define ST_LATTICE_KPLS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(8) X(10) X(12) X(16)

// the smallest listed KPL whose lattice holds 2L+1 states; -1 for a label length outside 0..511
inline int lattice_kpl(int max_label_len) {
  if (max_label_len < 0) return -1;
#define ST_LATTICE_FITS(K) if (K * 64 >= 2 * max_label_len + 1) return K;
  ST_LATTICE_KPLS(ST_LATTICE_FITS)
#undef ST_LATTICE_FITS
  return -1;
}

// f(std::integral_constant<int, KPL>{}) for a kpl of the list (what lattice_kpl returned); nothing for any other value
template <typename F>
inline void dispatch_kpl(int kpl, F&& f) {
  switch (kpl) {
#define ST_LATTICE_CASE(K) case K: f(std::integral_constant<int, K>{}); break;
    ST_LATTICE_KPLS(ST_LATTICE_CASE)
#undef ST_LATTICE_CASE
  }
}

// State u of the 2L+1: even = blank, odd = label (u-1)/2.  (Callers ask only for u < 2L+1.)
ST_LAT_HD int lattice_class(int u, const int* lab, int blank) { return (u & 1) ? lab[(u - 1) >> 1] : blank; }
// u may be entered from u-2: a label state whose label differs from the previous one (alpha, Viterbi)
ST_LAT_HD bool lattice_skip_from_below(int u, const int* lab) {
  return (u & 1) && u >= 3 && lab[(u - 1) >> 1] != lab[((u - 1) >> 1) - 1];
}
// u may be left for u+2: the mirrored rule (beta)
ST_LAT_HD bool lattice_skip_to_above(int u, int U, const int* lab) {
  return (u & 1) && u + 2 < U && lab[((u - 1) >> 1) + 1] != lab[(u - 1) >> 1];
}

// "Not enough time for target transition sequence": L labels and a blank between adjacent equal ones must fit in the Tb frames,
// Tb in the T the tensor has, the 2L+1 states in the UP the kernel was instantiated for.  L < 0: label_offsets not monotone.
ST_LAT_HD bool lattice_refused(int L, int repeats, int Tb, int T, int UP) {
  return Tb < 0 || Tb > T || L + repeats > Tb || (unsigned)(2 * L + 1) > (unsigned)UP;   // (a negative L wraps above UP)
}

#ifdef __HIPCC__

constexpr int LATTICE_TC = 64;                              // frames per LDS chunk
constexpr int DPP_WAVE_SHR1 = 0x138, DPP_WAVE_SHL1 = 0x130;   // wave_shr:1 (value of the lane below), wave_shl:1 (of the lane above)

// cross-lane move on the VALU (DPP), no LDS round trip; lanes without a source keep `fill`.  8-byte values as two 32-bit moves.
template <int CTRL, typename V>
__device__ __forceinline__ V dpp_shift(V v, V fill) {
  static_assert(std::is_trivially_copyable<V>::value && (sizeof(V) == 4 || sizeof(V) == 8), "dpp_shift: 4 or 8 bytes");
  if constexpr (sizeof(V) == 4) {
    return __builtin_bit_cast(V, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, fill), __builtin_bit_cast(int, v), CTRL,
                                                             0xF, 0xF, false));
  } else {
    const long long vb = __builtin_bit_cast(long long, v), fb = __builtin_bit_cast(long long, fill);
    const int lo = __builtin_amdgcn_update_dpp((int)fb, (int)vb, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(fb >> 32), (int)(vb >> 32), CTRL, 0xF, 0xF, false);
    return __builtin_bit_cast(V, ((long long)hi << 32) | (unsigned int)lo);
  }
}

// adjacent repeats of the label, counted by the whole wave (every lane gets the count); feeds lattice_refused
__device__ __forceinline__ int lattice_repeats(const int* lab, int L, int lane) {
  int rep = 0;
  for (int i = 1 + lane; i < L; i += 64) rep += lab[i] == lab[i - 1];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) rep += __shfl_xor(rep, o, 64);
  return rep;
}

// Stages 64-frame chunks of rows (ROW_ELEMS elements each, 16 bytes per lane and move) through registers into LDS: load() one
// chunk ahead of the frames being walked, store() when the buffer it goes to is free.  Rows past T read row T-1.  No barrier
// in here: a single wave's LDS operations are ordered, and a kernel that wants one has it at the call site.
template <typename Elem, int ROW_ELEMS>
struct ChunkStage {
  static constexpr int VE = 16 / sizeof(Elem), ROW_VECS = ROW_ELEMS / VE, N = LATTICE_TC * ROW_VECS / 64;
  typedef Elem Vec16 __attribute__((ext_vector_type(VE)));
  Vec16 stage[N];
  __device__ __forceinline__ void load(const Elem* rows, int chunk, int T, int lane) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int f = lane + 64 * i;             // 16-byte index inside the chunk
      const int t = min(chunk * LATTICE_TC + f / ROW_VECS, T - 1);
      stage[i] = *reinterpret_cast<const Vec16*>(rows + (long)t * ROW_ELEMS + (f % ROW_VECS) * VE);
    }
  }
  __device__ __forceinline__ void store(Elem* lds_buf, int lane) const {
#pragma unroll
    for (int i = 0; i < N; ++i) *reinterpret_cast<Vec16*>(lds_buf + (lane + 64 * i) * VE) = stage[i];
  }
};

#endif  // __HIPCC__

}  // namespace st
