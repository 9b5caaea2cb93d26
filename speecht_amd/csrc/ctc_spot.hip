// Keyword spotting: the best occurrence of given keywords in the frames of given utterances on gfx950, and its host form.
//
// The lattice is ctc_align.hip's (2L+1 states, blank = C-1, max-plus in DOUBLE) run on d_t(c) = x_t(c) - max_c x_t(c) in place
// of the log-softmax (the normaliser cancels in the ratio to the greedy reading: no exp, no log), with the two outer blanks
// dead, an entry into the first label at every frame and the start frame travelling with each state's value (semantics:
// include/speecht_hip.h, tests/spot_oracle.py).  All deciding arithmetic lives in ctc_spot_core.h, which the host form shares:
// device and host return the same bits.
//
// Structure:
//  1. spot_ratio: one lane per (row, class), d in double into the workspace [B*T][32], -inf in columns >= C.  The rows serve
//     all jobs of their utterance.
//  2. spot_lattice<KPL>: one WAVE per job of the job table.  States are dealt KPL-contiguous per lane; a frame is register
//     arithmetic plus four cross-lane shifts (DPP: value and start of the two states below a lane's first); the rows come
//     through LDS in 64-frame chunks, prefetched one chunk ahead.  The lane that owns state 2L-1 keeps the running best and
//     writes the job's outputs: there are no back-pointer rows and no back-trace.  The optional trace (end_t and its start for
//     every frame) is collected in LDS per chunk and written coalesced.
#include <algorithm>

#include "ctc_lattice.h"
#include "ctc_spot_core.h"
#include "st_common.h"

namespace {

using st::RowMap;
constexpr int SHR1 = st::DPP_WAVE_SHR1;
constexpr int CP = st::SP_CP;          // doubles per row of d
constexpr int TC = st::LATTICE_TC;     // frames per LDS chunk
#define NEG_INF_F (-__builtin_inff())

// d of every (b, t) row, two rows per wavefront; the row maximum by a 32-lane xor butterfly
__global__ __launch_bounds__(256) void spot_ratio_kernel(const float* __restrict__ logits, RowMap map, int B, int T, int C,
                                                         double* __restrict__ rows) {
  const int lane = threadIdx.x & 63, c = lane & 31;
  const long i = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + (lane >> 5);
  const bool row_ok = i < (long)B * T;
  const long ii = row_ok ? i : (long)B * T - 1;
  const int b = (int)(ii / T), t = (int)(ii - (long)b * T);
  const float v = c < C ? logits[map.off(b, t) + c] : NEG_INF_F;
  float m = v;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (row_ok) rows[i * CP + c] = c < C ? st::sp_ratio(v, m) : ST_SP_NEG_INF;
}

template <int KPL>
__global__ __launch_bounds__(64) void spot_lattice_kernel(const double* __restrict__ ratio_rows, int B, int T, int C,
                                                          const int* __restrict__ seq_lens, const int* __restrict__ kw_ids,
                                                          const int* __restrict__ kw_off, int n_keywords,
                                                          const int* __restrict__ jobs, double* __restrict__ score,
                                                          int* __restrict__ span, double* __restrict__ trace_score,
                                                          int* __restrict__ trace_start, int* __restrict__ status) {
  constexpr int UP = KPL * 64;
  __shared__ __attribute__((aligned(16))) double E[2][TC * CP];
  __shared__ double tr_v[TC];
  __shared__ int tr_s[TC];
  const int job = blockIdx.x;
  const int lane = threadIdx.x;
  const int blank = C - 1;
  const bool trace = trace_score != nullptr;
  const st::SpotJob jb = st::sp_job(jobs, job, B, T, n_keywords, kw_off, seq_lens, UP);
  const int Tb = jb.ok ? jb.Tb : 0;
  double* trv = trace ? trace_score + (long)job * T : nullptr;
  int* trs = trace ? trace_start + (long)job * T : nullptr;
  if (trace) {
    for (int t = Tb + lane; t < T; t += 64) { trv[t] = ST_SP_NEG_INF; trs[t] = -1; }
  }
  if (!jb.ok || Tb == 0) {
    if (lane == 0) {
      status[job] = jb.ok ? 0 : 1;
      score[job] = ST_SP_NEG_INF;
      span[2 * (long)job] = -1;
      span[2 * (long)job + 1] = -1;
    }
    return;
  }
  const int* lab = kw_ids + jb.first;
  const int L = jb.L;
  const int u_end = 2 * L - 1, lane_end = u_end / KPL, j_end = u_end % KPL;

  int col[KPL];          // column of d each state reads
  bool skip[KPL];        // may arrive from u-2
  bool live[KPL];        // u in 1 .. 2L-1
  bool enter[KPL];       // u == 1: an occurrence may begin here at every frame
#pragma unroll
  for (int j = 0; j < KPL; ++j) {
    const int u = lane * KPL + j;
    live[j] = u >= 1 && u <= u_end;
    enter[j] = u == 1;
    col[j] = st::sp_column(live[j] ? st::lattice_class(u, lab, blank) : blank);
    skip[j] = live[j] && st::lattice_skip_from_below(u, lab);
  }

  const double* rows = ratio_rows + (long)jb.b * T * CP;
  st::ChunkStage<double, CP> stage;   // the rows of chunk ch are E[ch & 1]
  auto chunk_load = [&](int chunk) { stage.load(rows, chunk, T, lane); };
  auto chunk_store = [&](int buf) { stage.store(E[buf], lane); };
  double v[KPL];         // value of each state
  int s[KPL];            // the frame its path began on
#pragma unroll
  for (int j = 0; j < KPL; ++j) { v[j] = ST_SP_NEG_INF; s[j] = -1; }
  double best = ST_SP_NEG_INF;       // the running best of the lane's state j_end: the job's on lane_end
  int best_start = -1, best_end = -1;
  chunk_load(0);
  chunk_store(0);
  __syncthreads();
  const int nchunks = (Tb + TC - 1) / TC;
  for (int ch = 0; ch < nchunks; ++ch) {
    const int buf = ch & 1;
    if (ch + 1 < nchunks) chunk_load(ch + 1);
    const int t_lo = ch * TC, t_hi = min(Tb, (ch + 1) * TC);
    for (int t = t_lo; t < t_hi; ++t) {
      const double* e = &E[buf][(t - t_lo) * CP];
      double em[KPL];
#pragma unroll
      for (int j = 0; j < KPL; ++j) em[j] = e[col[j]];
      const double up1v = st::dpp_shift<SHR1>(v[KPL - 1], ST_SP_NEG_INF);
      const int up1s = st::dpp_shift<SHR1>(s[KPL - 1], -1);
      const double up2v = st::dpp_shift<SHR1>(KPL >= 2 ? v[KPL >= 2 ? KPL - 2 : 0] : up1v, ST_SP_NEG_INF);
      const int up2s = st::dpp_shift<SHR1>(KPL >= 2 ? s[KPL >= 2 ? KPL - 2 : 0] : up1s, -1);
      double nv[KPL];
      int ns[KPL];
#pragma unroll
      for (int j = 0; j < KPL; ++j) {
        const double v1 = j >= 1 ? v[j >= 1 ? j - 1 : 0] : up1v;
        const int s1 = j >= 1 ? s[j >= 1 ? j - 1 : 0] : up1s;
        const double v2 = j >= 2 ? v[j >= 2 ? j - 2 : 0] : (j == 1 ? up1v : up2v);
        const int s2 = j >= 2 ? s[j >= 2 ? j - 2 : 0] : (j == 1 ? up1s : up2s);
        st::sp_cell(v[j], s[j], v1, s1, v2, s2, skip[j], enter[j], live[j], t, em[j], nv[j], ns[j]);
      }
#pragma unroll
      for (int j = 0; j < KPL; ++j) { v[j] = nv[j]; s[j] = ns[j]; }
      double end = v[0];
      int end_start = s[0];
#pragma unroll
      for (int j = 1; j < KPL; ++j) {
        if (j == j_end) { end = v[j]; end_start = s[j]; }
      }
      st::sp_running_best(end, end_start, t, best, best_start, best_end);
      if (trace && lane == lane_end) { tr_v[t - t_lo] = end; tr_s[t - t_lo] = end_start; }
    }
    if (trace) {
      __syncthreads();
      if (t_lo + lane < t_hi) { trv[t_lo + lane] = tr_v[lane]; trs[t_lo + lane] = tr_s[lane]; }
    }
    if (ch + 1 < nchunks) {
      chunk_store(buf ^ 1);
      __syncthreads();
    }
  }
  if (lane == lane_end) {
    status[job] = 0;
    score[job] = best;
    span[2 * (long)job] = best_start;
    span[2 * (long)job + 1] = best_end;
  }
}

// the host form of one job on the rows of d [T][32] of its utterance
void spot_host_job(const double* rows, int C, const int* lab, int L, int Tb, double* score, int* span, double* trv, int* trs) {
  const int blank = C - 1, u_end = 2 * L - 1;
  static_assert(2 * 511 + 1 <= 1024, "the columns hold the largest lattice");
  double v[2][1024];                      // the lattice columns of frames t-1 and t (2L+1 <= 1023)
  int s[2][1024];
  int col[1024];
  bool skip[1024];
  for (int u = 0; u <= 2 * L; ++u) {
    const bool live = u >= 1 && u <= u_end;
    col[u] = st::sp_column(live ? st::lattice_class(u, lab, blank) : blank);
    skip[u] = live && st::lattice_skip_from_below(u, lab);
    v[1][u] = ST_SP_NEG_INF;              // frame -1
    s[1][u] = -1;
  }
  double best = ST_SP_NEG_INF;
  int best_start = -1, best_end = -1;
  for (int t = 0; t < Tb; ++t) {
    const double* a = v[(t + 1) & 1];
    const int* as = s[(t + 1) & 1];
    const double* row = rows + (long)t * CP;
    for (int u = 0; u <= 2 * L; ++u)
      st::sp_cell(a[u], as[u], u >= 1 ? a[u - 1] : ST_SP_NEG_INF, u >= 1 ? as[u - 1] : -1, u >= 2 ? a[u - 2] : ST_SP_NEG_INF,
                  u >= 2 ? as[u - 2] : -1, skip[u], u == 1, u >= 1 && u <= u_end, t, row[col[u]], v[t & 1][u], s[t & 1][u]);
    const double end = v[t & 1][u_end];
    const int end_start = s[t & 1][u_end];
    st::sp_running_best(end, end_start, t, best, best_start, best_end);
    if (trv) { trv[t] = end; trs[t] = end_start; }
  }
  *score = best;
  span[0] = best_start;
  span[1] = best_end;
}

bool spot_args_ok(int batch, int frames, int classes, int max_keyword_len, int n_keywords, int n_jobs) {
  return batch > 0 && frames > 0 && classes >= 2 && classes <= CP && max_keyword_len >= 1 && st::lattice_kpl(max_keyword_len) > 0 &&
         n_keywords >= 0 && n_jobs >= 0;
}
#define SPOT_ARGS_TEXT "ctc_spot: needs 2 <= num_classes <= 32, 1 <= max_keyword_len <= 511, n_keywords >= 0, n_jobs >= 0"

}  // namespace

extern "C" {

size_t st_ctc_spot_ws(int batch, int frames, int max_keyword_len, int n_jobs) {
  if (max_keyword_len < 1 || st::lattice_kpl(max_keyword_len) < 0 || batch <= 0 || frames <= 0 || n_jobs < 0) return 0;
  // rows of d [batch * frames][32] double: nothing grows with the jobs
  return (size_t)batch * frames * CP * sizeof(double) + 512;
}

int st_ctc_spot_f32(const st_tensor3* logits, const int32_t* seq_lens, const int32_t* kw_ids, const int32_t* kw_offsets,
                    int n_keywords, int max_keyword_len, const int32_t* jobs, int n_jobs, double* score, int32_t* span,
                    double* trace_score, int32_t* trace_start, int32_t* status, void* workspace, size_t workspace_bytes,
                    void* stream) {
  ST_REQUIRE(logits && logits->base && seq_lens && kw_ids && kw_offsets && workspace, "ctc_spot: null argument");
  ST_REQUIRE(n_jobs <= 0 || (jobs && score && span && status), "ctc_spot: null argument");
  ST_REQUIRE((trace_score == nullptr) == (trace_start == nullptr), "ctc_spot: trace_score and trace_start go together");
  ST_REQUIRE(logits->batch > 0 && logits->frames > 0 && logits->halo >= 0 && logits->t_pitch >= logits->halo + logits->frames &&
             logits->c_pitch >= logits->channels, "ctc_spot: bad logits shape");
  ST_REQUIRE(spot_args_ok(logits->batch, logits->frames, logits->channels, max_keyword_len, n_keywords, n_jobs), SPOT_ARGS_TEXT);
  const int B = logits->batch, T = logits->frames, C = logits->channels;
  ST_REQUIRE(workspace_bytes >= st_ctc_spot_ws(B, T, max_keyword_len, n_jobs), "ctc_spot: workspace too small");
  ST_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "ctc_spot: workspace must be 16-byte aligned");
  if (n_jobs == 0) return ST_OK;
  hipStream_t s = st::as_stream(stream);
  const size_t nrows = (size_t)B * T;
  double* rows = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(spot_ratio_kernel, dim3((unsigned)((nrows + 7) / 8)), dim3(256), 0, s, logits->base, st::row_map(*logits), B,
                     T, C, rows);
  st::dispatch_kpl(st::lattice_kpl(max_keyword_len), [&](auto k) {
    hipLaunchKernelGGL(spot_lattice_kernel<k()>, dim3(n_jobs), dim3(64), 0, s, rows, B, T, C, seq_lens, kw_ids, kw_offsets,
                       n_keywords, jobs, score, span, trace_score, trace_start, status);
  });
  return st::check_launch("ctc_spot");
}

int st_ctc_spot_host(const float* logits, int batch, int frames, int classes, const int32_t* seq_lens, const int32_t* kw_ids,
                     const int32_t* kw_offsets, int n_keywords, int max_keyword_len, const int32_t* jobs, int n_jobs,
                     double* score, int32_t* span, double* trace_score, int32_t* trace_start, int32_t* status, void* workspace,
                     size_t workspace_bytes) {
  ST_REQUIRE(logits && seq_lens && kw_ids && kw_offsets && workspace, "ctc_spot: null argument");
  ST_REQUIRE(n_jobs <= 0 || (jobs && score && span && status), "ctc_spot: null argument");
  ST_REQUIRE((trace_score == nullptr) == (trace_start == nullptr), "ctc_spot: trace_score and trace_start go together");
  ST_REQUIRE(spot_args_ok(batch, frames, classes, max_keyword_len, n_keywords, n_jobs), SPOT_ARGS_TEXT);
  ST_REQUIRE(workspace_bytes >= st_ctc_spot_ws(batch, frames, max_keyword_len, n_jobs), "ctc_spot: workspace too small");
  ST_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "ctc_spot: workspace must be 16-byte aligned");
  const int B = batch, T = frames, C = classes, UP = st::lattice_kpl(max_keyword_len) * 64;
  double* rows = reinterpret_cast<double*>(workspace);
  // the rows of d of the frames that are used
  for (int b = 0; b < B; ++b) {
    const int Tb = std::min(seq_lens[b], T);
    for (int t = 0; t < Tb; ++t) {
      const float* x = logits + ((size_t)b * T + t) * C;
      double* row = rows + ((size_t)b * T + t) * CP;
      float m = NEG_INF_F;
      for (int c = 0; c < C; ++c) m = fmaxf(m, x[c]);
      for (int c = 0; c < CP; ++c) row[c] = c < C ? st::sp_ratio(x[c], m) : ST_SP_NEG_INF;
    }
  }
  for (int job = 0; job < n_jobs; ++job) {
    const st::SpotJob jb = st::sp_job(jobs, job, B, T, n_keywords, kw_offsets, seq_lens, UP);
    const int Tb = jb.ok ? jb.Tb : 0;
    double* trv = trace_score ? trace_score + (size_t)job * T : nullptr;
    int32_t* trs = trace_start ? trace_start + (size_t)job * T : nullptr;
    if (trv) for (int t = Tb; t < T; ++t) { trv[t] = ST_SP_NEG_INF; trs[t] = -1; }
    status[job] = jb.ok ? 0 : 1;
    if (!jb.ok || Tb == 0) {
      score[job] = ST_SP_NEG_INF;
      span[2 * (size_t)job] = span[2 * (size_t)job + 1] = -1;
      continue;
    }
    spot_host_job(rows + (size_t)jb.b * T * CP, C, kw_ids + jb.first, jb.L, Tb, score + job, span + 2 * (size_t)job, trv, trs);
  }
  return ST_OK;
}

}  // extern "C"
