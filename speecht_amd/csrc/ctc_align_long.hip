// Forced alignment of ONE long sequence: the Viterbi lattice of ctc_align.hip cut into (frame block x state block) tiles, so
// that a transcript of tens of thousands of labels aligns against the concatenated frames of a long recording -- and its host
// form.  Semantics, tie rules and the deciding arithmetic are those of st_ctc_align_f32 (ctc_align_core.h): on labels that
// kernel takes, both choose the same path.
//
// Structure:
//  1. align_logsoftmax (ctc_align_softmax.h): the ln-softmax rows [T][32] in double.
//  2. align_long_init: both column buffers = -inf, the fit rule (T >= L + adjacent repeats) -> status.
//  3. align_long_tile, ONE LAUNCH PER FRAME BLOCK of TB = 64 frames, one wave per state block.  Lane l of block j holds the 16
//     states 896 j - 128 + 16 l ...: lanes 8-63 are the 896 states the block owns, lanes 0-7 a halo of 2 TB = 128 states below
//     them.  The tile starts from the column the previous launch left (exact for every state), runs ctc_align.hip's frame loop
//     and knows nothing of the states below its window: what it computes for window state i after k frames is exact from
//     i >= 2 k on, because a state looks at most 2 states down per frame.  After <= 64 frames the owned states (i >= 128) are
//     exact; only they are written: 16 doubles per lane to the other column buffer, one back-pointer word per lane and frame.
//     Nothing here waits on another workgroup: the launch boundary orders the frame blocks.
//  4. align_long_backtrace: one wave.  Inside a 64-frame chunk the path descends at most 126 states below the state it enters
//     the chunk's last frame in, so the 16 back-pointer words per row that end at that state's word hold the whole walk of the
//     chunk: they are brought to LDS, walked there, and the spans are written by all lanes with plain vector stores.
// st_ctc_align_long_wild_f32 (transcripts that leave audio out): the WILD form of 1 writes the emission of the wildcard id C into
// slot C of every row, 2-4 run as they are, and the fit stage follows: align_rowmax (slot C := the row's largest value), then
// align_long_fit, one LANE per label walking its span through the rows (a wildcard: bias * frames, no walk).
#include <algorithm>
#include <cmath>

#include "ctc_align_core.h"
#include "ctc_align_softmax.h"
#include "ctc_lattice.h"
#include "st_common.h"

namespace {

constexpr int SHR1 = st::DPP_WAVE_SHR1;
constexpr int CP = st::AL_CP;          // class pitch of the log-softmax rows
constexpr int TB = st::LATTICE_TC;     // frames per frame block (= per LDS chunk)
constexpr int KPL = 16;                // states per lane
constexpr int HALO = 2 * TB;           // states below the owned ones that a tile recomputes
constexpr int SB = 64 * KPL - HALO;    // states a state block owns: 896
constexpr int OWN0 = HALO / KPL;       // first owning lane: 8
constexpr int BPW = SB / 16;           // back-pointer words per state block and frame: 56
constexpr int WIN = 16;                // back-pointer words per row the back-trace keeps of a chunk
constexpr int MAX_LABELS = 1048575;
static_assert(HALO % KPL == 0 && KPL == 16 && (TB - 1) * 2 + 15 < WIN * 16 - 15, "tile geometry");

inline int state_blocks(int L) { return (2 * L + 1 + SB - 1) / SB; }
inline size_t col_elems(int NB) { return (size_t)SB * NB + HALO; }   // state u of a column is element HALO + u

// both columns = -inf (the HALO elements below state 0 stay so); the fit rule; a refused label has its score here
__global__ __launch_bounds__(256) void align_long_init_kernel(const int* __restrict__ lab, int L, int T, double* __restrict__ col,
                                                              long n, int* __restrict__ status, double* __restrict__ score) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) col[i] = ST_AL_NEG_INF;
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    const int rep = st::lattice_repeats(lab, L, threadIdx.x);
    if (threadIdx.x == 0) {
      const bool bad = L + rep > T;
      *status = bad ? 1 : 0;
      if (bad) *score = ST_AL_NEG_INF;
    }
  }
}

// frame block fb of state block blockIdx.x: column `colin` (after frame 64 fb - 1) -> column `colout` (after the block's last frame)
__global__ __launch_bounds__(64) void align_long_tile_kernel(const double* __restrict__ ly, int T, int C,
                                                             const int* __restrict__ lab, int L, int fb, int NB,
                                                             const double* __restrict__ colin, double* __restrict__ colout,
                                                             unsigned int* __restrict__ bp, const int* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) double E[TB * CP];
  if (*status != 0) return;
  const int lane = threadIdx.x;
  const int blank = C - 1;
  const int U = 2 * L + 1;
  const int u0 = (int)blockIdx.x * SB - HALO + lane * KPL;   // the lane's first state; below 0 in block 0's halo

  int cls[KPL];          // class of each state
  bool skip[KPL];        // may arrive from u-2
#pragma unroll
  for (int j = 0; j < KPL; ++j) {
    const int u = u0 + j;
    const bool real = (unsigned)u < (unsigned)U;
    cls[j] = real ? st::lattice_class(u, lab, blank) : blank;
    skip[j] = real && st::lattice_skip_from_below(u, lab);
  }

  st::ChunkStage<double, CP> stage;
  stage.load(ly, fb, T, lane);
  stage.store(E, lane);
  __syncthreads();
  double a[KPL];
  if (fb == 0) {
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
      const int u = u0 + j;
      a[j] = (unsigned)u < 2u && u < U ? E[cls[j]] : ST_AL_NEG_INF;
    }
  } else {
    const double2* src = reinterpret_cast<const double2*>(colin + HALO + u0);
#pragma unroll
    for (int j = 0; j < KPL; j += 2) {
      const double2 v = src[j / 2];
      a[j] = v.x;
      a[j + 1] = v.y;
    }
  }
  const bool own = lane >= OWN0;
  const long pitch = (long)BPW * NB;
  unsigned int* bprow = bp + (long)blockIdx.x * BPW + (lane - OWN0);
  const int t_lo = max(1, fb * TB), t_hi = min(T, (fb + 1) * TB);
  for (int t = t_lo; t < t_hi; ++t) {
    const double* e = &E[(t - fb * TB) * CP];
    double em[KPL];
#pragma unroll
    for (int j = 0; j < KPL; ++j) em[j] = e[cls[j]];
    const double up1 = st::dpp_shift<SHR1>(a[KPL - 1], ST_AL_NEG_INF);
    const double up2 = st::dpp_shift<SHR1>(a[KPL - 2], ST_AL_NEG_INF);
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
    if (own) bprow[(long)t * pitch] = word;
  }
  if (own) {
    double2* dst = reinterpret_cast<double2*>(colout + HALO + u0);
#pragma unroll
    for (int j = 0; j < KPL; j += 2) dst[j / 2] = make_double2(a[j], a[j + 1]);
  }
}

__global__ __launch_bounds__(64) void align_long_backtrace_kernel(const unsigned int* __restrict__ bp, int T, int L, int NB,
                                                                  const double* __restrict__ col, const int* __restrict__ status,
                                                                  int* __restrict__ spans, double* __restrict__ score) {
  __shared__ unsigned int W[TB * WIN];
  __shared__ int path[TB + 1];              // label index (-1: blank) of the chunk's frames; [TB]: the frame after the chunk
  const int lane = threadIdx.x;
  if (*status != 0) {
    for (long i = lane; i < 2 * (long)L; i += 64) spans[i] = -1;
    return;
  }
  const int U = 2 * L + 1;
  const long pitch = (long)BPW * NB;
  int u = st::al_end_state(U, col[HALO + U - 1], U > 1 ? col[HALO + U - 2] : ST_AL_NEG_INF);
  if (lane == 0) *score = col[HALO + u];
  for (int ch = (T - 1) / TB; ch >= 0; --ch) {
    const int t_lo = ch * TB, t_hi = min(T - 1, t_lo + TB - 1);
    const int w_lo = (u >> 4) - (WIN - 1);   // the window's first word (below 0: those words do not exist and are not visited)
#pragma unroll
    for (int i = 0; i < TB * WIN / 64; ++i) {
      const int f = lane + 64 * i;
      const int t = t_lo + f / WIN, w = w_lo + f % WIN;
      W[f] = (t > 0 && t <= t_hi && w >= 0) ? bp[(long)t * pitch + w] : 0u;   // (frame 0 has no back-pointer row)
    }
    __syncthreads();
    // the walk: the same for every lane (LDS broadcast reads)
    for (int t = t_hi; t >= t_lo; --t) {
      if (lane == 0) path[t - t_lo] = st::al_state_label(u);
      if (t > 0) {
        const unsigned int word = W[(t - t_lo) * WIN + (u >> 4) - w_lo];
        u = max(u - (int)((word >> (2 * (u & 15))) & 3u), 0);
      }
    }
    __syncthreads();
    {
      const int t = t_lo + lane;
      if (t <= t_hi) {
        const int s = path[lane];
        if (t == 0 && s >= 0) spans[2 * s] = 0;
        if (t == T - 1) {
          if (s >= 0) spans[2 * s + 1] = T;
        } else {
          const int nx = path[lane + 1];       // (lane 63: the first frame of the chunk walked before this one)
          if (nx != s) {
            if (s >= 0) spans[2 * s + 1] = t + 1;
            if (nx >= 0) spans[2 * nx] = t + 1;
          }
        }
      }
    }
    __syncthreads();
    if (lane == 0) path[TB] = path[0];
    __syncthreads();
  }
}

// the fit of every label (st_ctc_align_long_wild_f32), after align_rowmax: one lane per label; NaN where the label is refused
__global__ __launch_bounds__(64) void align_long_fit_kernel(const double* __restrict__ ly, int T, int C, const int* __restrict__ lab,
                                                            int L, const int* __restrict__ status, const int* __restrict__ spans,
                                                            double bias, double* __restrict__ fit) {
  const int k = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (k >= L) return;
  fit[k] = *status != 0 ? __builtin_nan("") : st::al_label_fit(ly, lab[k], C, spans[2 * k], spans[2 * k + 1], T, bias);
}

struct Workspace {
  double* ly;          // [T][32]
  uint32_t* bp;        // [T][56 NB]
  double* col[2];      // [896 NB + 128] each
};

Workspace carve(void* workspace, long T, int NB) {
  Workspace w;
  w.ly = reinterpret_cast<double*>(workspace);
  w.bp = reinterpret_cast<uint32_t*>(w.ly + (size_t)T * CP);
  w.col[0] = reinterpret_cast<double*>(w.bp + (size_t)T * BPW * NB);
  w.col[1] = w.col[0] + col_elems(NB);
  return w;
}

}  // namespace

extern "C" {

size_t st_ctc_align_long_ws(long frames, int label_len) {
  if (frames <= 0 || label_len < 0 || label_len > MAX_LABELS) return 0;
  const int NB = state_blocks(label_len);
  return (size_t)frames * (CP * sizeof(double) + (size_t)BPW * sizeof(uint32_t) * NB) + 2 * col_elems(NB) * sizeof(double) + 512;
}

#define ST_ALIGN_LONG_ARGS(NAME)                                                                                              \
  ST_REQUIRE(logits && (label_ids || label_len == 0) && spans && score && status && workspace, NAME ": null argument");      \
  ST_REQUIRE(frames > 0 && frames <= 0x7fffffffL - TB, NAME ": bad number of frames");                                        \
  ST_REQUIRE(classes >= 2 && classes <= CP && row_pitch >= classes, NAME ": num_classes must be 2..32 and <= row_pitch");    \
  ST_REQUIRE(label_len >= 0 && label_len <= MAX_LABELS, NAME ": label length %d outside 0..%d", label_len, MAX_LABELS);      \
  ST_REQUIRE(workspace_bytes >= st_ctc_align_long_ws(frames, label_len), NAME ": workspace too small");                      \
  ST_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, NAME ": workspace must be 16-byte aligned")

// the launches of both device entry points; `bias` (null: the plain form): the WILD softmax stage, `fit` (with a bias only, may be
// null): the fit stage after the back-trace
static int align_long_launch(const char* name, const float* logits, long frames, int classes, int row_pitch, const int32_t* label_ids,
                             int label_len, int32_t* spans, double* score, int32_t* status, void* workspace, void* stream,
                             const double* bias, double* fit) {
  hipStream_t s = st::as_stream(stream);
  const int T = (int)frames, L = label_len, NB = state_blocks(L);
  const Workspace w = carve(workspace, T, NB);
  const dim3 row_grid((unsigned)(((size_t)T + 7) / 8));
  if (bias) {
    hipLaunchKernelGGL(st::align_logsoftmax_wild_kernel, row_grid, dim3(256), 0, s, logits, st::RowMap{0, 0, row_pitch}, 1, T, classes,
                       *bias, w.ly);
  } else {
    hipLaunchKernelGGL(st::align_logsoftmax_kernel, row_grid, dim3(256), 0, s, logits, st::RowMap{0, 0, row_pitch}, 1, T, classes, w.ly);
  }
  const long n = 2 * (long)col_elems(NB);
  hipLaunchKernelGGL(align_long_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, label_ids, L, T, w.col[0], n,
                     status, score);
  // frame block fb reads column fb & 1 (the first reads none) and leaves the other one
  const int nfb = (T + TB - 1) / TB;
  for (int fb = 0; fb < nfb; ++fb)
    hipLaunchKernelGGL(align_long_tile_kernel, dim3(NB), dim3(64), 0, s, w.ly, T, classes, label_ids, L, fb, NB, w.col[fb & 1],
                       w.col[(fb & 1) ^ 1], w.bp, status);
  hipLaunchKernelGGL(align_long_backtrace_kernel, dim3(1), dim3(64), 0, s, w.bp, T, L, NB, w.col[nfb & 1], status, spans, score);
  if (bias && fit && L > 0) {
    hipLaunchKernelGGL(st::align_rowmax_kernel, row_grid, dim3(256), 0, s, w.ly, (long)T, classes);
    hipLaunchKernelGGL(align_long_fit_kernel, dim3((unsigned)((L + 63) / 64)), dim3(64), 0, s, w.ly, T, classes, label_ids, L, status,
                       spans, *bias, fit);
  }
  return st::check_launch(name);
}

// the loops of both host entry points (bias, fit: as above)
static int align_long_host_run(const float* logits, long frames, int classes, int row_pitch, const int32_t* label_ids, int label_len,
                               int32_t* spans, double* score, int32_t* status, void* workspace, const double* bias, double* fit) {
  const long T = frames;
  const int L = label_len, U = 2 * L + 1, blank = classes - 1, NB = state_blocks(L);
  const size_t pitch = (size_t)BPW * NB;
  const Workspace w = carve(workspace, T, NB);
  const int* lab = label_ids;
  long rep = 0;
  for (int i = 1; i < L; ++i) rep += lab[i] == lab[i - 1];
  *status = L + rep > T ? 1 : 0;
  if (*status) {
    *score = ST_AL_NEG_INF;
    for (long i = 0; i < 2 * (long)L; ++i) spans[i] = -1;
    if (fit) for (int i = 0; i < L; ++i) fit[i] = __builtin_nan("");
    return ST_OK;
  }
  for (long t = 0; t < T; ++t) {
    const float* row = logits + t * row_pitch;
    float m = -__builtin_inff();
    for (int c = 0; c < classes; ++c) m = fmaxf(m, row[c]);
    double e[CP];
    for (int c = 0; c < CP; ++c) e[c] = c < classes ? st::al_exp((double)row[c] - (double)m) : 0.0;
    const double s = st::al_row_sum(e);
    for (int c = 0; c < classes; ++c) w.ly[t * CP + c] = st::al_log_softmax(row[c], m, s);
    if (bias) w.ly[t * CP + classes] = st::al_wild_emission(m, s, *bias);
  }
  auto cls = [&](int u) { return st::lattice_class(u, lab, blank); };
  // plain loops over the whole lattice: the columns of frames t-1 and t, state u at element u
  for (int u = 0; u < U; ++u) w.col[0][u] = u < 2 ? w.ly[cls(u)] : ST_AL_NEG_INF;
  for (long t = 1; t < T; ++t) {
    const double* a = w.col[(t - 1) & 1];
    double* n = w.col[t & 1];
    uint32_t* words = w.bp + t * pitch;
    for (size_t i = 0; i < pitch; ++i) words[i] = 0;
    for (int u = 0; u < U; ++u) {
      int move;
      n[u] = st::al_cell(a[u], u >= 1 ? a[u - 1] : ST_AL_NEG_INF, u >= 2 ? a[u - 2] : ST_AL_NEG_INF,
                         st::lattice_skip_from_below(u, lab), w.ly[t * CP + cls(u)], move);
      words[u >> 4] |= (uint32_t)move << (2 * (u & 15));
    }
  }
  const double* a = w.col[(T - 1) & 1];
  int u = st::al_end_state(U, a[U - 1], U > 1 ? a[U - 2] : ST_AL_NEG_INF);
  *score = a[u];
  int next = -3;                          // label index of frame t + 1 (none after the last frame)
  for (long t = T - 1; t >= 0; --t) {
    const int s = st::al_state_label(u);
    if (t == T - 1) {
      if (s >= 0) spans[2 * s + 1] = (int)T;
    } else if (next != s) {
      if (s >= 0) spans[2 * s + 1] = (int)t + 1;
      if (next >= 0) spans[2 * next] = (int)t + 1;
    }
    if (t == 0 && s >= 0) spans[2 * s] = 0;
    next = s;
    if (t > 0) u = std::max(u - (int)((w.bp[t * pitch + (u >> 4)] >> (2 * (u & 15))) & 3u), 0);
  }
  if (fit) {
    for (long t = 0; t < T; ++t) w.ly[t * CP + classes] = st::al_row_max(w.ly + t * CP, classes);
    for (int k = 0; k < L; ++k) fit[k] = st::al_label_fit(w.ly, lab[k], classes, spans[2 * k], spans[2 * k + 1], (int)T, *bias);
  }
  return ST_OK;
}

int st_ctc_align_long_f32(const float* logits, long frames, int classes, int row_pitch, const int32_t* label_ids, int label_len,
                          int32_t* spans, double* score, int32_t* status, void* workspace, size_t workspace_bytes,
                          void* stream) {
  ST_ALIGN_LONG_ARGS("ctc_align_long");
  return align_long_launch("ctc_align_long", logits, frames, classes, row_pitch, label_ids, label_len, spans, score, status, workspace,
                           stream, nullptr, nullptr);
}

int st_ctc_align_long_host(const float* logits, long frames, int classes, int row_pitch, const int32_t* label_ids, int label_len,
                           int32_t* spans, double* score, int32_t* status, void* workspace, size_t workspace_bytes) {
  ST_ALIGN_LONG_ARGS("ctc_align_long");
  return align_long_host_run(logits, frames, classes, row_pitch, label_ids, label_len, spans, score, status, workspace, nullptr, nullptr);
}

// ---- the wildcard forms: the id `classes` is the wildcard, slot `classes` of the rows its emission (so classes <= 31) ----
#define ST_ALIGN_LONG_WILD_ARGS(NAME)                                                                                          \
  ST_ALIGN_LONG_ARGS(NAME);                                                                                                    \
  ST_REQUIRE(classes <= CP - 1, NAME ": num_classes must be 2..31 (the wildcard takes the row's slot after the blank)");      \
  ST_REQUIRE(std::isfinite(wildcard_bias) && wildcard_bias <= 0.0, NAME ": wildcard_bias must be finite and <= 0")

int st_ctc_align_long_wild_f32(const float* logits, long frames, int classes, int row_pitch, const int32_t* label_ids, int label_len,
                               double wildcard_bias, int32_t* spans, double* score, int32_t* status, double* fit, void* workspace,
                               size_t workspace_bytes, void* stream) {
  ST_ALIGN_LONG_WILD_ARGS("ctc_align_long_wild");
  return align_long_launch("ctc_align_long_wild", logits, frames, classes, row_pitch, label_ids, label_len, spans, score, status,
                           workspace, stream, &wildcard_bias, fit);
}

int st_ctc_align_long_wild_host(const float* logits, long frames, int classes, int row_pitch, const int32_t* label_ids, int label_len,
                                double wildcard_bias, int32_t* spans, double* score, int32_t* status, double* fit, void* workspace,
                                size_t workspace_bytes) {
  ST_ALIGN_LONG_WILD_ARGS("ctc_align_long_wild");
  for (int i = 0; i < label_len; ++i) {
    ST_REQUIRE(label_ids[i] >= 0 && label_ids[i] <= classes, "ctc_align_long_wild: label id %d outside 0..%d", label_ids[i], classes);
    ST_REQUIRE(i == 0 || label_ids[i] != classes || label_ids[i - 1] != classes, "ctc_align_long_wild: two adjacent wildcards at label %d", i);
  }
  return align_long_host_run(logits, frames, classes, row_pitch, label_ids, label_len, spans, score, status, workspace, &wildcard_bias,
                             fit);
}

}  // extern "C"
