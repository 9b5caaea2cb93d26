// Forced alignment: the best-path (Viterbi) CTC alignment of a label sequence on gfx950, and its host form.
//
// The lattice is ctc.hip's (2L+1 states, blank = C-1) with max in place of sum, in log space and in DOUBLE: a max-plus
// recursion rounds one add per frame, and with doubles both the path and its score stay far inside what a float64
// specification can tell apart (tests/align_oracle.py).  All deciding arithmetic lives in ctc_align_core.h, which the host
// form shares: device and host choose the same path bit for bit.
//
// Structure:
//  1. align_logsoftmax (ctc_align_softmax.h): one lane per (row, class), ln softmax in double into the workspace [B*T][32].
//  2. align_viterbi<KPL>: one WAVE per utterance, states dealt KPL-contiguous per lane as in ctc_alpha_beta_kernel: a frame is
//     register arithmetic plus two cross-lane shifts (DPP); emission rows come through LDS in 64-frame chunks, prefetched one
//     chunk ahead.  Every frame leaves one back-pointer row: 2 bits per state, KPL*2 bits = one uint32 per lane, 256 B coalesced.
//  3. align_backtrace<KPL>: one wave per utterance walks the back-pointers from the end state; the rows come through LDS in
//     64-frame chunks (prefetched), so the walk is a chain of LDS reads, not of global loads.  The path of a chunk is kept in
//     LDS and `states` / `spans` are then written by all lanes with plain vector stores.
// st_ctc_align_ring_f32 (the finals of live streams, stream_ring.h) runs 2 and 3 as they are behind a ring-mapped form of 1: the rows of
// its utterances come from a stream's ring through a job table, and the lattices ask that table for an utterance's frames.
// st_ctc_align_wild_f32 (transcripts that leave audio out) runs 2 and 3 as they are too: the WILD form of 1 writes the emission of
// the wildcard id C into slot C of every row, which the lattice indexes like any class, and a fit stage follows the back-trace:
//  4. align_rowmax (ctc_align_softmax.h): slot C of every row := the row's largest value; align_fit: one LANE per label walks
//     its span through those rows and writes one double (a wildcard: bias * frames, no walk).
#include <algorithm>
#include <cmath>

#include "ctc_align_core.h"
#include "ctc_align_softmax.h"
#include "ctc_lattice.h"
#include "st_common.h"
#include "stream_ring.h"

namespace {

using st::RowMap;
constexpr int SHR1 = st::DPP_WAVE_SHR1;
constexpr int CP = st::AL_CP;  // class pitch of the log-softmax rows
constexpr int TC = st::LATTICE_TC;   // frames per LDS chunk
constexpr int BPW = 64;        // back-pointer words per frame (one per lane)
#define NEG_INF_F (-__builtin_inff())

// the first stage of st_ctc_align_ring_f32: row t of job b comes from the stream's ring (the job table and a wrap); same arithmetic
__global__ __launch_bounds__(256) void align_logsoftmax_ring_kernel(const float* __restrict__ ring, st::RingMap map, int B, int T, int C,
                                                                    double* __restrict__ ly) {
  st::align_logsoftmax_rows(ring, map, B, T, C, ly);
}

// (Lens: the frames of each utterance -- st::DenseLens, a seq_lens array, or st::RingLens, the job table of the ring entry point)
template <int KPL, typename Lens>
__global__ __launch_bounds__(64) void align_viterbi_kernel(const double* __restrict__ ly, int T, int C,
                                                           const int* __restrict__ label_ids,
                                                           const int* __restrict__ label_off, Lens seq_lens,
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
  const int Tb = seq_lens(b);

  // "Not enough time for target transition sequence": L + #adjacent repeats must fit in Tb
  const int rep = st::lattice_repeats(lab, L, lane);
  const bool bad = st::lattice_refused(L, rep, Tb, T, UP);
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
    cls[j] = u < U ? st::lattice_class(u, lab, blank) : blank;
    skip[j] = u < U && st::lattice_skip_from_below(u, lab);
  }

  const double* rows = ly + (long)b * T * CP;
  st::ChunkStage<double, CP> stage;   // the log-softmax rows of chunk ch are E[ch & 1]
  // (through lambdas: with the two called directly align_viterbi_kernel<16> takes one VGPR more)
  auto chunk_load = [&](int chunk) { stage.load(rows, chunk, T, lane); };
  auto chunk_store = [&](int buf) { stage.store(E[buf], lane); };
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
      const double up1 = st::dpp_shift<SHR1>(a[KPL - 1], ST_AL_NEG_INF);
      const double up2 = st::dpp_shift<SHR1>(KPL >= 2 ? a[KPL >= 2 ? KPL - 2 : 0] : up1, ST_AL_NEG_INF);
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

template <int KPL, typename Lens>
__global__ __launch_bounds__(64) void align_backtrace_kernel(const unsigned int* __restrict__ bp, int T,
                                                             const int* __restrict__ label_off, Lens seq_lens,
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
  const int Tb = seq_lens(b);
  if (st_out) for (int t = Tb + lane; t < T; t += 64) st_out[t] = -2;
  if (Tb == 0) return;

  const unsigned int* rows = bp + (long)b * T * BPW;
  st::ChunkStage<unsigned int, BPW> stage;   // the back-pointer rows of chunk ch are W[ch & 1]

  int u = end_state[b];
  const int last = (Tb - 1) / TC;
  stage.load(rows, last, T, lane);
  stage.store(W[last & 1], lane);
  __syncthreads();
  for (int ch = last; ch >= 0; --ch) {
    const int buf = ch & 1;
    if (ch > 0) stage.load(rows, ch - 1, T, lane);
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
    if (ch > 0) stage.store(W[buf ^ 1], lane);
    __syncthreads();
  }
}

// the fit of every label (st_ctc_align_wild_f32): lane k of block (x, b) has label 64 x + k of utterance b; NaN where refused
__global__ __launch_bounds__(64) void align_fit_kernel(const double* __restrict__ ly, int T, int C, const int* __restrict__ label_ids,
                                                       const int* __restrict__ label_off, const int* __restrict__ seq_lens,
                                                       const int* __restrict__ status, const int* __restrict__ spans, double bias,
                                                       double* __restrict__ fit) {
  const int b = blockIdx.y;
  const int L = label_off[b + 1] - label_off[b];
  const bool bad = status[b] != 0;
  // (the stride: a refused label may be longer than the max_label_len the grid was sized for)
  for (int k = (int)blockIdx.x * 64 + (int)threadIdx.x; k < L; k += (int)gridDim.x * 64) {
    const long n = (long)label_off[b] + k;
    fit[n] = bad ? __builtin_nan("")
                 : st::al_label_fit(ly + (long)b * T * CP, label_ids[n], C, spans[2 * n], spans[2 * n + 1], seq_lens[b], bias);
  }
}

// the host form of one utterance; ly: [T][32] doubles, bp: [T][UP / 16] words, 2 bits per state.  `bias` (null: the plain form):
// the wildcard id C may appear in lab and slot C of the rows carries its emission; `fit` (may be null): [L], as align_fit_kernel
void align_host_one(const float* logits, int T, int C, const int* lab, int L, int Tb, int UP, int* sp, int* st_out,
                    float* score, int* status, double* ly, uint32_t* bp, const double* bias = nullptr, double* fit = nullptr) {
  const int U = 2 * L + 1, blank = C - 1, words = UP / 16;
  int rep = 0;
  if (U <= UP) for (int i = 1; i < L; ++i) rep += lab[i] == lab[i - 1];
  const bool bad = st::lattice_refused(L, rep, Tb, T, UP);
  *status = bad ? 1 : 0;
  if (bad) {
    *score = NEG_INF_F;
    for (int i = 0; i < 2 * L; ++i) sp[i] = -1;
    if (fit) for (int i = 0; i < L; ++i) fit[i] = __builtin_nan("");
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
    if (bias) ly[(long)t * CP + C] = st::al_wild_emission(m, s, *bias);
  }
  auto cls = [&](int u) { return st::lattice_class(u, lab, blank); };
  double col[2][1024];                    // the lattice columns of frames t-1 and t (U <= 1023)
  for (int u = 0; u < U; ++u) col[0][u] = u < 2 ? ly[cls(u)] : ST_AL_NEG_INF;
  for (int t = 1; t < Tb; ++t) {
    const double* a = col[(t - 1) & 1];
    double* n = col[t & 1];
    uint32_t* w = bp + (long)t * words;
    for (int i = 0; i < words; ++i) w[i] = 0;
    for (int u = 0; u < U; ++u) {
      int move;
      n[u] = st::al_cell(a[u], u >= 1 ? a[u - 1] : ST_AL_NEG_INF, u >= 2 ? a[u - 2] : ST_AL_NEG_INF,
                         st::lattice_skip_from_below(u, lab), ly[(long)t * CP + cls(u)], move);
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
  if (fit) {
    for (int t = 0; t < Tb; ++t) ly[(long)t * CP + C] = st::al_row_max(ly + (long)t * CP, C);
    for (int k = 0; k < L; ++k) fit[k] = st::al_label_fit(ly, lab[k], C, sp[2 * k], sp[2 * k + 1], Tb, *bias);
  }
}

// the three stages on B utterances of T rows each: `map` names a row for the softmax stage (which is also the gather), `lens` the
// frames of an utterance for the lattice and the back-trace, which read the workspace only.  `bias` (null: the plain form, and
// always null for a ring): the WILD softmax stage; `fit` (with a bias only, may be null): the fit stage after the back-trace
template <typename Map, typename Lens>
void launch_align(const float* base, Map map, Lens lens, int B, int T, int C, int kpl, const int* label_ids, const int* label_offsets,
                  int* spans, int* states, float* score, int* status, void* workspace, hipStream_t s, const double* bias = nullptr,
                  double* fit = nullptr, int max_label_len = 0) {
  const size_t rows = (size_t)B * T;
  double* ly = reinterpret_cast<double*>(workspace);
  unsigned int* bp = reinterpret_cast<unsigned int*>(ly + rows * CP);
  int* end_state = reinterpret_cast<int*>(bp + rows * BPW);
  const dim3 grid((unsigned)((rows + 7) / 8));
  if constexpr (std::is_same<Map, RowMap>::value) {
    if (bias) {
      hipLaunchKernelGGL(st::align_logsoftmax_wild_kernel, grid, dim3(256), 0, s, base, map, B, T, C, *bias, ly);
    } else {
      hipLaunchKernelGGL(st::align_logsoftmax_kernel, grid, dim3(256), 0, s, base, map, B, T, C, ly);
    }
  } else {
    hipLaunchKernelGGL(align_logsoftmax_ring_kernel, grid, dim3(256), 0, s, base, map, B, T, C, ly);
  }
  st::dispatch_kpl(kpl, [&](auto k) {
    hipLaunchKernelGGL((align_viterbi_kernel<k(), Lens>), dim3(B), dim3(64), 0, s, ly, T, C, label_ids, label_offsets, lens, bp,
                       end_state, score, status);
    hipLaunchKernelGGL((align_backtrace_kernel<k(), Lens>), dim3(B), dim3(64), 0, s, bp, T, label_offsets, lens, end_state, status,
                       spans, states);
  });
  if constexpr (std::is_same<Lens, st::DenseLens>::value) {
    if (bias && fit) {
      hipLaunchKernelGGL(st::align_rowmax_kernel, grid, dim3(256), 0, s, ly, (long)rows, C);
      hipLaunchKernelGGL(align_fit_kernel, dim3((std::max(max_label_len, 1) + 63) / 64, B), dim3(64), 0, s, ly, T, C, label_ids, label_offsets,
                         lens.lens, status, spans, *bias, fit);
    }
  }
}

}  // namespace

extern "C" {

size_t st_ctc_align_ws(int batch, int frames, int max_label_len) {
  if (st::lattice_kpl(max_label_len) < 0 || batch <= 0 || frames <= 0) return 0;
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
  const int kpl = st::lattice_kpl(max_label_len);
  ST_REQUIRE(kpl > 0, "ctc_align: label length %d outside 0..511", max_label_len);
  ST_REQUIRE(workspace_bytes >= st_ctc_align_ws(logits->batch, logits->frames, max_label_len),
             "ctc_align: workspace too small");
  ST_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "ctc_align: workspace must be 16-byte aligned");
  launch_align(logits->base, st::row_map(*logits), st::DenseLens{seq_lens}, logits->batch, logits->frames, logits->channels, kpl,
               label_ids, label_offsets, spans, states, score, status, workspace, st::as_stream(stream));
  return st::check_launch("ctc_align");
}

int st_ctc_align_ring_f32(const float* ring, int max_streams, int cap, int num_classes, const int32_t* jobs, int n_jobs, int max_rows,
                          const int32_t* label_ids, const int32_t* label_offsets, int max_label_len, int32_t* spans, int32_t* states,
                          float* score, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  ST_REQUIRE(ring && jobs && label_ids && label_offsets && spans && score && status && workspace, "ctc_align_ring: null argument");
  ST_REQUIRE(max_streams >= 1 && cap >= 1 && n_jobs >= 1 && max_rows >= 1, "ctc_align_ring: bad ring or job shape");
  ST_REQUIRE(num_classes >= 2 && num_classes <= CP, "ctc_align_ring: num_classes must be 2..32");
  const int kpl = st::lattice_kpl(max_label_len);
  ST_REQUIRE(kpl > 0, "ctc_align_ring: label length %d outside 0..511", max_label_len);
  ST_REQUIRE(workspace_bytes >= st_ctc_align_ws(n_jobs, max_rows, max_label_len), "ctc_align_ring: workspace too small");
  ST_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "ctc_align_ring: workspace must be 16-byte aligned");
  st::trace("ctc_align_ring<%d> jobs=%d rows=%d cap=%d", kpl, n_jobs, max_rows, cap);
  launch_align(ring, st::RingMap{jobs, max_streams, max_rows, cap}, st::RingLens{jobs, max_streams, max_rows}, n_jobs, max_rows,
               num_classes, kpl, label_ids, label_offsets, spans, states, score, status, workspace, st::as_stream(stream));
  return st::check_launch("ctc_align_ring");
}

int st_ctc_align_host(const float* logits, int batch, int frames, int classes, const int32_t* label_ids,
                      const int32_t* label_offsets, const int32_t* seq_lens, int max_label_len, int32_t* spans,
                      int32_t* states, float* score, int32_t* status, void* workspace, size_t workspace_bytes) {
  ST_REQUIRE(logits && label_ids && label_offsets && seq_lens && spans && score && status && workspace,
             "ctc_align: null argument");
  ST_REQUIRE(batch > 0 && frames > 0, "ctc_align: bad logits shape");
  ST_REQUIRE(classes >= 2 && classes <= CP, "ctc_align: num_classes must be 2..32");
  const int kpl = st::lattice_kpl(max_label_len);
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

// ---- the wildcard forms: the id `classes` is the wildcard, slot `classes` of the rows its emission (so classes <= 31) ----

int st_ctc_align_wild_f32(const st_tensor3* logits, const int32_t* label_ids, const int32_t* label_offsets,
                          const int32_t* seq_lens, int max_label_len, double wildcard_bias, int32_t* spans, int32_t* states,
                          float* score, int32_t* status, double* fit, void* workspace, size_t workspace_bytes, void* stream) {
  ST_REQUIRE(logits && logits->base && label_ids && label_offsets && seq_lens && spans && score && status && workspace,
             "ctc_align_wild: null argument");
  ST_REQUIRE(logits->batch > 0 && logits->batch <= 65535 && logits->frames > 0 && logits->halo >= 0 &&
                 logits->t_pitch >= logits->halo + logits->frames,
             "ctc_align_wild: bad logits shape");
  ST_REQUIRE(logits->channels >= 2 && logits->channels <= CP - 1 && logits->c_pitch >= logits->channels,
             "ctc_align_wild: num_classes must be 2..31 (the wildcard takes the row's slot after the blank)");
  ST_REQUIRE(std::isfinite(wildcard_bias) && wildcard_bias <= 0.0, "ctc_align_wild: wildcard_bias must be finite and <= 0");
  const int kpl = st::lattice_kpl(max_label_len);
  ST_REQUIRE(kpl > 0, "ctc_align_wild: label length %d outside 0..511", max_label_len);
  ST_REQUIRE(workspace_bytes >= st_ctc_align_ws(logits->batch, logits->frames, max_label_len),
             "ctc_align_wild: workspace too small");
  ST_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "ctc_align_wild: workspace must be 16-byte aligned");
  launch_align(logits->base, st::row_map(*logits), st::DenseLens{seq_lens}, logits->batch, logits->frames, logits->channels, kpl,
               label_ids, label_offsets, spans, states, score, status, workspace, st::as_stream(stream), &wildcard_bias, fit,
               max_label_len);
  return st::check_launch("ctc_align_wild");
}

int st_ctc_align_wild_host(const float* logits, int batch, int frames, int classes, const int32_t* label_ids,
                           const int32_t* label_offsets, const int32_t* seq_lens, int max_label_len, double wildcard_bias,
                           int32_t* spans, int32_t* states, float* score, int32_t* status, double* fit, void* workspace,
                           size_t workspace_bytes) {
  ST_REQUIRE(logits && label_ids && label_offsets && seq_lens && spans && score && status && workspace,
             "ctc_align_wild: null argument");
  ST_REQUIRE(batch > 0 && frames > 0, "ctc_align_wild: bad logits shape");
  ST_REQUIRE(classes >= 2 && classes <= CP - 1,
             "ctc_align_wild: num_classes must be 2..31 (the wildcard takes the row's slot after the blank)");
  ST_REQUIRE(std::isfinite(wildcard_bias) && wildcard_bias <= 0.0, "ctc_align_wild: wildcard_bias must be finite and <= 0");
  const int kpl = st::lattice_kpl(max_label_len);
  ST_REQUIRE(kpl > 0, "ctc_align_wild: label length %d outside 0..511", max_label_len);
  ST_REQUIRE(workspace_bytes >= st_ctc_align_ws(batch, frames, max_label_len), "ctc_align_wild: workspace too small");
  ST_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "ctc_align_wild: workspace must be 16-byte aligned");
  for (int b = 0; b < batch; ++b)
    for (int i = label_offsets[b]; i < label_offsets[b + 1]; ++i) {
      ST_REQUIRE(label_ids[i] >= 0 && label_ids[i] <= classes, "ctc_align_wild: label id %d outside 0..%d", label_ids[i], classes);
      ST_REQUIRE(i == label_offsets[b] || label_ids[i] != classes || label_ids[i - 1] != classes,
                 "ctc_align_wild: two adjacent wildcards in utterance %d", b);
    }
  double* ly = reinterpret_cast<double*>(workspace);
  uint32_t* bp = reinterpret_cast<uint32_t*>(ly + (size_t)frames * CP);
  for (int b = 0; b < batch; ++b) {
    const int L = label_offsets[b + 1] - label_offsets[b];
    align_host_one(logits + (size_t)b * frames * classes, frames, classes, label_ids + label_offsets[b], L, seq_lens[b],
                   kpl * 64, spans + 2 * (size_t)label_offsets[b], states ? states + (size_t)b * frames : nullptr, score + b,
                   status + b, ly, bp, &wildcard_bias, fit && L > 0 ? fit + label_offsets[b] : nullptr);
  }
  return ST_OK;
}

}  // extern "C"
