// Forced alignment: the best-path (Viterbi) CTC alignment of a label sequence on gfx950, and its host form.
//
// The lattice is ctc.hip's (2L+1 states, blank = C-1) with max in place of sum, in log space and in DOUBLE: a max-plus
// recursion rounds one add per frame, and with doubles both the path and its score stay far inside what a float64
// specification can tell apart (tests/align_oracle.py).  All deciding arithmetic lives in ctc_align_core.h, which the host
// form shares: device and host choose the same path bit for bit.
//
// Structure:
//  1. align_logsoftmax: one lane per (row, class), ln softmax in double into the workspace [B*T][32].
//  2. align_viterbi<KPL>: one WAVE per utterance, states dealt KPL-contiguous per lane as in ctc_alpha_beta_kernel: a frame is
//     register arithmetic plus two cross-lane shifts (DPP); emission rows come through LDS in 64-frame chunks, prefetched one
//     chunk ahead.  Every frame leaves one back-pointer row: 2 bits per state, KPL*2 bits = one uint32 per lane, 256 B coalesced.
//  3. align_backtrace<KPL>: one wave per utterance walks the back-pointers from the end state; the rows come through LDS in
//     64-frame chunks (prefetched), so the walk is a chain of LDS reads, not of global loads.  The path of a chunk is kept in
//     LDS and `states` / `spans` are then written by all lanes with plain vector stores.
#include <algorithm>

#include "ctc_align_core.h"
#include "st_common.h"

namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int CP = st::AL_CP;  // class pitch of the log-softmax rows
constexpr int TC = 64;         // frames per LDS chunk
constexpr int BPW = 64;        // back-pointer words per frame (one per lane)
#define NEG_INF_F (-__builtin_inff())

struct RowMap2 {   // (b, t) -> float offset
  long batch_stride;
  long row0;
  int row_stride;
  __device__ __forceinline__ long off(int b, int t) const {
    return (long)b * batch_stride + row0 + (long)t * row_stride;
  }
};

constexpr int SHR1 = 0x138;   // wave_shr:1: the value of the lane below; lane 0 keeps `fill`
__device__ __forceinline__ double dpp_shr1(double v, double fill) {
  const long long vb = st::al_bits(v), fb = st::al_bits(fill);
  const int lo = __builtin_amdgcn_update_dpp((int)fb, (int)vb, SHR1, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(fb >> 32), (int)(vb >> 32), SHR1, 0xF, 0xF, false);
  return st::al_from_bits(((long long)hi << 32) | (unsigned int)lo);
}

// ln softmax of every (b, t) row, two rows per wavefront; sums by a 32-lane xor butterfly (the order of st::al_row_sum)
__global__ __launch_bounds__(256) void align_logsoftmax_kernel(const float* __restrict__ logits, RowMap2 map, int B, int T,
                                                               int C, double* __restrict__ ly) {
  const int lane = threadIdx.x & 63, c = lane & 31;
  const long i = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + (lane >> 5);
  const bool row_ok = i < (long)B * T;
  const long ii = row_ok ? i : (long)B * T - 1;
  const int b = (int)(ii / T), t = (int)(ii - (long)b * T);
  const float v = c < C ? logits[map.off(b, t) + c] : NEG_INF_F;
  float m = v;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  double s = c < C ? st::al_exp((double)v - (double)m) : 0.0;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
  if (row_ok) ly[i * CP + c] = st::al_log_softmax(v, m, s);
}

template <int KPL>
__global__ __launch_bounds__(64) void align_viterbi_kernel(const double* __restrict__ ly, int T, int C,
                                                           const int* __restrict__ label_ids,
                                                           const int* __restrict__ label_off,
                                                           const int* __restrict__ seq_lens,
                                                           unsigned int* __restrict__ bp, int* __restrict__ end_state,
                                                           float* __restrict__ score, int* __restrict__ status) {
  constexpr int UP = KPL * 64;
  __shared__ __attribute__((aligned(16))) double E[2][TC * CP];
  __shared__ double fin[UP];
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  const int blank = C - 1;
  const int* lab = label_ids + label_off[b];
  const int L = label_off[b + 1] - label_off[b];
  const int U = 2 * L + 1;
  const int Tb = seq_lens[b];

  // "Not enough time for target transition sequence": L + #adjacent repeats must fit in Tb (as ctc_alpha_beta_kernel)
  const bool fits = L >= 0 && U <= UP;
  int rep = 0;
  if (fits) for (int i = 1 + lane; i < L; i += 64) rep += lab[i] == lab[i - 1];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) rep += __shfl_xor(rep, o, 64);
  const bool bad = !fits || Tb < 0 || Tb > T || L + rep > Tb;
  if (bad || Tb == 0) {      // no frames and (checked above) an empty label: the empty path, ln p = 0
    if (lane == 0) {
      status[b] = bad ? 1 : 0;
      score[b] = bad ? NEG_INF_F : 0.f;
      end_state[b] = bad ? -1 : 0;
    }
    return;
  }

  int cls[KPL];          // class of each state
  bool skip[KPL];        // may arrive from u-2
#pragma unroll
  for (int j = 0; j < KPL; ++j) {
    const int u = lane * KPL + j;
    const bool odd = (u & 1) && u < U;
    const int li = (u - 1) >> 1;
    cls[j] = odd ? lab[li] : blank;
    skip[j] = odd && u >= 3 && lab[li] != lab[li - 1];
  }

  // stage one 64-frame chunk of log-softmax rows [chunk*TC, +TC) into E[buf]; rows past T read row T-1
  const double* rows = ly + (long)b * T * CP;
  constexpr int STG = TC * CP / 2 / 64;
  f64x2 stage[STG];
  auto chunk_load = [&](int chunk) {
#pragma unroll
    for (int i = 0; i < STG; ++i) {
      const int f = lane + 64 * i;             // 16-byte index inside the chunk
      const int t = min(chunk * TC + f / (CP / 2), T - 1);
      stage[i] = *reinterpret_cast<const f64x2*>(rows + (long)t * CP + (f % (CP / 2)) * 2);
    }
  };
  auto chunk_store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < STG; ++i) *reinterpret_cast<f64x2*>(&E[buf][(lane + 64 * i) * 2]) = stage[i];
  };

  double a[KPL];
  chunk_load(0);
  chunk_store(0);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < KPL; ++j) {
    const int u = lane * KPL + j;
    a[j] = u < 2 && u < U ? E[0][cls[j]] : ST_AL_NEG_INF;
  }
  unsigned int* bprow = bp + (long)b * T * BPW + lane;
  const int nchunks = (Tb + TC - 1) / TC;
  for (int ch = 0; ch < nchunks; ++ch) {
    const int buf = ch & 1;
    if (ch + 1 < nchunks) chunk_load(ch + 1);
    const int t_lo = max(1, ch * TC), t_hi = min(Tb, (ch + 1) * TC);
    for (int t = t_lo; t < t_hi; ++t) {
      const double* e = &E[buf][(t - ch * TC) * CP];
      double em[KPL];
#pragma unroll
      for (int j = 0; j < KPL; ++j) em[j] = e[cls[j]];
      const double up1 = dpp_shr1(a[KPL - 1], ST_AL_NEG_INF);
      const double up2 = KPL >= 2 ? dpp_shr1(a[KPL >= 2 ? KPL - 2 : 0], ST_AL_NEG_INF) : dpp_shr1(up1, ST_AL_NEG_INF);
      double n[KPL];
      unsigned int word = 0;
#pragma unroll
      for (int j = 0; j < KPL; ++j) {
        const double adv = j >= 1 ? a[j >= 1 ? j - 1 : 0] : up1;
        const double skp = j >= 2 ? a[j >= 2 ? j - 2 : 0] : (j == 1 ? up1 : up2);
        int move;
        n[j] = st::al_cell(a[j], adv, skp, skip[j], em[j], move);
        word |= (unsigned int)move << (2 * j);
      }
#pragma unroll
      for (int j = 0; j < KPL; ++j) a[j] = n[j];
      bprow[(long)t * BPW] = word;
    }
    if (ch + 1 < nchunks) {
      chunk_store(buf ^ 1);
      __syncthreads();
    }
  }
#pragma unroll
  for (int j = 0; j < KPL; ++j) fin[lane * KPL + j] = a[j];
  __syncthreads();
  if (lane == 0) {
    const double last_blank = fin[U - 1], last_label = U > 1 ? fin[U - 2] : ST_AL_NEG_INF;
    const int end = st::al_end_state(U, last_blank, last_label);
    status[b] = 0;
    end_state[b] = end;
    score[b] = (float)fin[end];
  }
}

template <int KPL>
__global__ __launch_bounds__(64) void align_backtrace_kernel(const unsigned int* __restrict__ bp, int T,
                                                             const int* __restrict__ label_off,
                                                             const int* __restrict__ seq_lens,
                                                             const int* __restrict__ end_state,
                                                             const int* __restrict__ status, int* __restrict__ spans,
                                                             int* __restrict__ states) {
  __shared__ __attribute__((aligned(16))) unsigned int W[2][TC * BPW];
  __shared__ int path[TC + 1];              // label index (-1: blank) of the chunk's frames; [TC]: the frame after the chunk
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  const int L = label_off[b + 1] - label_off[b];
  int* sp = spans + 2 * (long)label_off[b];
  int* st_out = states ? states + (long)b * T : nullptr;
  if (status[b] != 0) {
    for (int i = lane; i < 2 * L; i += 64) sp[i] = -1;
    if (st_out) for (int t = lane; t < T; t += 64) st_out[t] = -2;
    return;
  }
  const int Tb = seq_lens[b];
  if (st_out) for (int t = Tb + lane; t < T; t += 64) st_out[t] = -2;
  if (Tb == 0) return;

  const unsigned int* rows = bp + (long)b * T * BPW;
  constexpr int STG = TC * BPW / 4 / 64;
  u32x4 stage[STG];
  auto chunk_load = [&](int chunk) {
#pragma unroll
    for (int i = 0; i < STG; ++i) {
      const int f = lane + 64 * i;             // 16-byte index inside the chunk
      const int t = min(chunk * TC + f / (BPW / 4), T - 1);
      stage[i] = *reinterpret_cast<const u32x4*>(rows + (long)t * BPW + (f % (BPW / 4)) * 4);
    }
  };
  auto chunk_store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < STG; ++i) *reinterpret_cast<u32x4*>(&W[buf][(lane + 64 * i) * 4]) = stage[i];
  };

  int u = end_state[b];
  const int last = (Tb - 1) / TC;
  chunk_load(last);
  chunk_store(last & 1);
  __syncthreads();
  for (int ch = last; ch >= 0; --ch) {
    const int buf = ch & 1;
    if (ch > 0) chunk_load(ch - 1);
    const int t_lo = ch * TC, t_hi = min(Tb - 1, t_lo + TC - 1);
    // the walk: the same for every lane (LDS broadcast reads); frame 0 has no back-pointer row
    for (int t = t_hi; t >= t_lo; --t) {
      if (lane == 0) path[t - t_lo] = st::al_state_label(u);
      if (t > 0) {
        const unsigned int word = W[buf][(t - t_lo) * BPW + u / KPL];
        u = max(u - (int)((word >> (2 * (u % KPL))) & 3u), 0);
      }
    }
    __syncthreads();
    {
      const int t = t_lo + lane;
      if (t <= t_hi) {
        const int s = path[lane];
        if (st_out) st_out[t] = s;
        if (t == 0 && s >= 0) sp[2 * s] = 0;
        if (t == Tb - 1) {
          if (s >= 0) sp[2 * s + 1] = Tb;
        } else {
          const int nx = path[lane + 1];       // (lane 63: the first frame of the chunk walked before this one)
          if (nx != s) {
            if (s >= 0) sp[2 * s + 1] = t + 1;
            if (nx >= 0) sp[2 * nx] = t + 1;
          }
        }
      }
    }
    __syncthreads();
    if (lane == 0) path[TC] = path[0];
    if (ch > 0) chunk_store(buf ^ 1);
    __syncthreads();
  }
}

int pick_kpl(int max_label_len) {
  static const int opts[] = {1, 2, 3, 4, 5, 6, 8, 10, 12, 16};
  if (max_label_len < 0) return -1;
  const int U = 2 * max_label_len + 1;
  for (int k : opts) if (k * 64 >= U) return k;
  return -1;
}

RowMap2 make_map2(const st_tensor3& t) {
  RowMap2 m;
  m.batch_stride = (long)t.t_pitch * t.c_pitch;
  m.row0 = (long)t.halo * t.c_pitch;
  m.row_stride = t.c_pitch;
  return m;
}

// the host form of one utterance; ly: [T][32] doubles, bp: [T][UP / 16] words, 2 bits per state
void align_host_one(const float* logits, int T, int C, const int* lab, int L, int Tb, int UP, int* sp, int* st_out,
                    float* score, int* status, double* ly, uint32_t* bp) {
  const int U = 2 * L + 1, blank = C - 1, words = UP / 16;
  bool bad = L < 0 || U > UP || Tb < 0 || Tb > T;
  if (!bad) {
    int rep = 0;
    for (int i = 1; i < L; ++i) rep += lab[i] == lab[i - 1];
    bad = L + rep > Tb;
  }
  *status = bad ? 1 : 0;
  if (bad) {
    *score = NEG_INF_F;
    for (int i = 0; i < 2 * L; ++i) sp[i] = -1;
    if (st_out) for (int t = 0; t < T; ++t) st_out[t] = -2;
    return;
  }
  if (st_out) for (int t = Tb; t < T; ++t) st_out[t] = -2;
  if (Tb == 0) { *score = 0.f; return; }
  for (int t = 0; t < Tb; ++t) {
    const float* row = logits + (long)t * C;
    float m = NEG_INF_F;
    for (int c = 0; c < C; ++c) m = fmaxf(m, row[c]);
    double e[CP];
    for (int c = 0; c < CP; ++c) e[c] = c < C ? st::al_exp((double)row[c] - (double)m) : 0.0;
    const double s = st::al_row_sum(e);
    for (int c = 0; c < C; ++c) ly[(long)t * CP + c] = st::al_log_softmax(row[c], m, s);
  }
  auto cls = [&](int u) { return (u & 1) ? lab[u >> 1] : blank; };
  double col[2][1024];                    // the lattice columns of frames t-1 and t (U <= 1023)
  for (int u = 0; u < U; ++u) col[0][u] = u < 2 ? ly[cls(u)] : ST_AL_NEG_INF;
  for (int t = 1; t < Tb; ++t) {
    const double* a = col[(t - 1) & 1];
    double* n = col[t & 1];
    uint32_t* w = bp + (long)t * words;
    for (int i = 0; i < words; ++i) w[i] = 0;
    for (int u = 0; u < U; ++u) {
      const bool skip_ok = (u & 1) && u >= 3 && lab[u >> 1] != lab[(u >> 1) - 1];
      int move;
      n[u] = st::al_cell(a[u], u >= 1 ? a[u - 1] : ST_AL_NEG_INF, u >= 2 ? a[u - 2] : ST_AL_NEG_INF, skip_ok,
                         ly[(long)t * CP + cls(u)], move);
      w[u >> 4] |= (uint32_t)move << (2 * (u & 15));
    }
  }
  const double* a = col[(Tb - 1) & 1];
  int u = st::al_end_state(U, a[U - 1], U > 1 ? a[U - 2] : ST_AL_NEG_INF);
  *score = (float)a[u];
  int next = -3;                          // label index of frame t + 1 (none after the last frame)
  for (int t = Tb - 1; t >= 0; --t) {
    const int s = st::al_state_label(u);
    if (st_out) st_out[t] = s;
    if (t == Tb - 1) {
      if (s >= 0) sp[2 * s + 1] = Tb;
    } else if (next != s) {
      if (s >= 0) sp[2 * s + 1] = t + 1;
      if (next >= 0) sp[2 * next] = t + 1;
    }
    if (t == 0 && s >= 0) sp[2 * s] = 0;
    next = s;
    if (t > 0) u = std::max(u - (int)((bp[(long)t * words + (u >> 4)] >> (2 * (u & 15))) & 3u), 0);
  }
}

}  // namespace

extern "C" {

size_t st_ctc_align_ws(int batch, int frames, int max_label_len) {
  if (pick_kpl(max_label_len) < 0 || batch <= 0 || frames <= 0) return 0;
  const size_t rows = (size_t)batch * frames;
  // ln-softmax rows [rows][32] double | back-pointer rows [rows][64] uint32 | end state [batch] int32
  return rows * (CP * sizeof(double) + BPW * sizeof(uint32_t)) + (size_t)batch * sizeof(int32_t) + 512;
}

int st_ctc_align_f32(const st_tensor3* logits, const int32_t* label_ids, const int32_t* label_offsets,
                     const int32_t* seq_lens, int max_label_len, int32_t* spans, int32_t* states, float* score,
                     int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  ST_REQUIRE(logits && logits->base && label_ids && label_offsets && seq_lens && spans && score && status && workspace,
             "ctc_align: null argument");
  ST_REQUIRE(logits->batch > 0 && logits->frames > 0 && logits->halo >= 0 && logits->t_pitch >= logits->halo + logits->frames,
             "ctc_align: bad logits shape");
  ST_REQUIRE(logits->channels >= 2 && logits->channels <= CP && logits->c_pitch >= logits->channels,
             "ctc_align: num_classes must be 2..32");
  const int kpl = pick_kpl(max_label_len);
  ST_REQUIRE(kpl > 0, "ctc_align: label length %d outside 0..511", max_label_len);
  ST_REQUIRE(workspace_bytes >= st_ctc_align_ws(logits->batch, logits->frames, max_label_len),
             "ctc_align: workspace too small");
  ST_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "ctc_align: workspace must be 16-byte aligned");
  hipStream_t s = st::as_stream(stream);
  const int B = logits->batch, T = logits->frames, C = logits->channels;
  const size_t rows = (size_t)B * T;
  double* ly = reinterpret_cast<double*>(workspace);
  unsigned int* bp = reinterpret_cast<unsigned int*>(ly + rows * CP);
  int* end_state = reinterpret_cast<int*>(bp + rows * BPW);
  hipLaunchKernelGGL(align_logsoftmax_kernel, dim3((unsigned)((rows + 7) / 8)), dim3(256), 0, s, logits->base,
                     make_map2(*logits), B, T, C, ly);
  switch (kpl) {
#define ST_AL(K)                                                                                                              \
  case K:                                                                                                                     \
    hipLaunchKernelGGL(align_viterbi_kernel<K>, dim3(B), dim3(64), 0, s, ly, T, C, label_ids, label_offsets, seq_lens, bp,     \
                       end_state, score, status);                                                                             \
    hipLaunchKernelGGL(align_backtrace_kernel<K>, dim3(B), dim3(64), 0, s, bp, T, label_offsets, seq_lens, end_state, status, \
                       spans, states);                                                                                        \
    break;
    ST_AL(1) ST_AL(2) ST_AL(3) ST_AL(4) ST_AL(5) ST_AL(6) ST_AL(8) ST_AL(10) ST_AL(12) ST_AL(16)
#undef ST_AL
  }
  return st::check_launch("ctc_align");
}

int st_ctc_align_host(const float* logits, int batch, int frames, int classes, const int32_t* label_ids,
                      const int32_t* label_offsets, const int32_t* seq_lens, int max_label_len, int32_t* spans,
                      int32_t* states, float* score, int32_t* status, void* workspace, size_t workspace_bytes) {
  ST_REQUIRE(logits && label_ids && label_offsets && seq_lens && spans && score && status && workspace,
             "ctc_align: null argument");
  ST_REQUIRE(batch > 0 && frames > 0, "ctc_align: bad logits shape");
  ST_REQUIRE(classes >= 2 && classes <= CP, "ctc_align: num_classes must be 2..32");
  const int kpl = pick_kpl(max_label_len);
  ST_REQUIRE(kpl > 0, "ctc_align: label length %d outside 0..511", max_label_len);
  ST_REQUIRE(workspace_bytes >= st_ctc_align_ws(batch, frames, max_label_len), "ctc_align: workspace too small");
  ST_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "ctc_align: workspace must be 16-byte aligned");
  // one utterance at a time in the first utterance's share of the workspace
  double* ly = reinterpret_cast<double*>(workspace);
  uint32_t* bp = reinterpret_cast<uint32_t*>(ly + (size_t)frames * CP);
  for (int b = 0; b < batch; ++b) {
    const int L = label_offsets[b + 1] - label_offsets[b];
    align_host_one(logits + (size_t)b * frames * classes, frames, classes, label_ids + label_offsets[b], L, seq_lens[b],
                   kpl * 64, spans + 2 * (size_t)label_offsets[b], states ? states + (size_t)b * frames : nullptr, score + b,
                   status + b, ly, bp);
  }
  return ST_OK;
}

}  // extern "C"
