// Word confidences: exact CTC word posteriors on gfx950, and their host form.
//
// log_conf of word j of a label l = ln P(l) - ln P(l*j): P(l) the CTC probability of the label, P(l*j) that of the label with
// word j's ids replaced by one pseudo-label that emits every class but the space and has dead blanks beside it (semantics:
// include/speecht_hip.h, tests/conf_oracle.py).  Both are forward probabilities over lattices of the shape ctc.hip and
// ctc_align.hip walk, here sum-product in the linear domain and in DOUBLE with an integer exponent per state.  All deciding
// arithmetic lives in ctc_conf_core.h, which the host form shares: device and host return the same bits.
//
// Structure:
//  1. conf_softmax: one lane per (row, class), softmax in double into the workspace [B*T][32]; column 30 holds the
//     pseudo-label's emission, column 31 holds 0.  The rows serve all jobs of their utterance.
//  2. conf_lattice<KPL>: one WAVE per job, B + n_words jobs: the full label of each utterance, then one lattice per word.  The
//     wave forms its label array (the word's run replaced) in LDS; states are dealt KPL-contiguous per lane, a frame is
//     register arithmetic plus four cross-lane shifts (DPP); softmax rows come through LDS in 64-frame chunks, prefetched one
//     chunk ahead.  No transcendental on the frame chain.  Leaves ln P of the job in the workspace.
//  3. conf_finish: one thread per output, forms log_prob and the differences.
// st_ctc_word_conf_ring_f32 (the finals of live streams, stream_ring.h) runs 2 and 3 as they are behind a ring-mapped form of 1: the rows
// of its utterances come from a stream's ring through a job table, and the lattices ask that table for an utterance's frames.
#include <algorithm>

#include "ctc_conf_core.h"
#include "ctc_lattice.h"
#include "st_common.h"
#include "stream_ring.h"

namespace {

using st::RowMap;
constexpr int SHR1 = st::DPP_WAVE_SHR1;
constexpr int CP = st::CF_CP;          // doubles per softmax row
constexpr int TC = st::LATTICE_TC;     // frames per LDS chunk
constexpr int EZ = st::CF_EZ;
constexpr int LMAX = 512;              // label ids a job's LDS array holds (labels of up to 511)
#define NEG_INF_F (-__builtin_inff())
#define CF_NAN ST_CF_NAN

// softmax of every (b, t) row, two rows per wavefront; sums by a 32-lane xor butterfly (the order of st::al_row_sum).  `map` names
// the row: a RowMap for a padded NWC tensor, a RingMap (stream_ring.h) for utterances kept in a stream's ring.
template <typename Map>
__device__ __forceinline__ void conf_softmax_rows(const float* __restrict__ logits, const Map& map, int B, int T, int C, int space_id,
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
  const double ex = c < C ? st::al_exp((double)v - (double)m) : 0.0;
  double s = ex;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
  const double p = c < C ? st::cf_prob(ex, s) : 0.0;
  double star = c != space_id ? p : 0.0;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) star = star + __shfl_xor(star, o, 64);
  if (row_ok) rows[i * CP + c] = c == st::CF_STAR ? star : p;          // (column 31: p = 0)
}

__global__ __launch_bounds__(256) void conf_softmax_kernel(const float* __restrict__ logits, RowMap map, int B, int T, int C,
                                                           int space_id, double* __restrict__ rows) {
  conf_softmax_rows(logits, map, B, T, C, space_id, rows);
}
// the first stage of st_ctc_word_conf_ring_f32: row t of job b comes from the stream's ring (the job table and a wrap); same arithmetic
__global__ __launch_bounds__(256) void conf_softmax_ring_kernel(const float* __restrict__ ring, st::RingMap map, int B, int T, int C,
                                                                int space_id, double* __restrict__ rows) {
  conf_softmax_rows(ring, map, B, T, C, space_id, rows);
}

// what a job is: its utterance and, for a word's job, the run of label ids it replaces (first < 0: the full label)
struct Job {
  int b, first, last;
  bool ok;
};
__host__ __device__ inline Job conf_job(int job, int B, const int* __restrict__ word_spans, const int* __restrict__ label_off) {
  if (job < B) return Job{job, -1, -1, true};
  const int* w = word_spans + 3 * (long)(job - B);
  Job j{w[0], w[1], w[2], false};
  if (j.b < 0 || j.b >= B) return j;
  const int L = label_off[j.b + 1] - label_off[j.b];
  j.ok = j.first >= 0 && j.first < j.last && j.last <= L;
  return j;
}

// (Lens: the frames of each utterance -- st::DenseLens, a seq_lens array, or st::RingLens, the job table of the ring entry point)
template <int KPL, typename Lens>
__global__ __launch_bounds__(64) void conf_lattice_kernel(const double* __restrict__ softmax_rows, int B, int T, int C,
                                                          const int* __restrict__ label_ids,
                                                          const int* __restrict__ label_off, Lens seq_lens,
                                                          const int* __restrict__ word_spans, double* __restrict__ ln_p,
                                                          int* __restrict__ status) {
  constexpr int UP = KPL * 64;
  __shared__ __attribute__((aligned(16))) double E[2][TC * CP];
  __shared__ int lab2[LMAX];
  __shared__ double fin_m[2];
  __shared__ int fin_e[2];
  const int job = blockIdx.x;
  const int lane = threadIdx.x;
  const int blank = C - 1;
  const Job jb = conf_job(job, B, word_spans, label_off);
  if (!jb.ok) {
    if (lane == 0) ln_p[job] = CF_NAN;
    return;
  }
  const int b = jb.b;
  const int* lab = label_ids + label_off[b];
  const int L = label_off[b + 1] - label_off[b];
  const int Tb = seq_lens(b);

  // "Not enough time for target transition sequence", decided on the full label for all of the utterance's jobs
  const int rep = st::lattice_repeats(lab, (unsigned)(2 * L + 1) <= (unsigned)UP ? L : 0, lane);
  const bool bad = st::lattice_refused(L, rep, Tb, T, UP);
  if (lane == 0 && jb.first < 0) status[b] = bad ? 1 : 0;
  if (bad || Tb == 0) {      // no frames and (checked above) an empty label: the empty path, ln p = 0
    if (lane == 0) ln_p[job] = bad ? CF_NAN : 0.0;
    return;
  }

  const int L2 = jb.first < 0 ? L : L - (jb.last - jb.first) + 1;
  const int U = 2 * L2 + 1;
  for (int i = lane; i < L2; i += 64) lab2[i] = st::cf_job_label(lab, i, jb.first, jb.last, blank);
  if (lane < 2) { fin_m[lane] = 0.0; fin_e[lane] = EZ; }
  __syncthreads();

  int cls[KPL];          // softmax column of each state
  bool skip[KPL];        // may arrive from u-2
#pragma unroll
  for (int j = 0; j < KPL; ++j) {
    const int u = lane * KPL + j;
    cls[j] = u < U ? st::cf_state_column(u, lab2, L2, blank) : st::CF_DEAD;
    skip[j] = u < U && st::lattice_skip_from_below(u, lab2);
  }

  const double* rows = softmax_rows + (long)b * T * CP;
  st::ChunkStage<double, CP> stage;   // the softmax rows of chunk ch are E[ch & 1]
  auto chunk_load = [&](int chunk) { stage.load(rows, chunk, T, lane); };
  auto chunk_store = [&](int buf) { stage.store(E[buf], lane); };
  double am[KPL];        // mantissa of alpha_t(u)
  int ae[KPL];           // its exponent
  chunk_load(0);
  chunk_store(0);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < KPL; ++j) {
    const int u = lane * KPL + j;
    st::cf_norm(u < 2 && u < U ? E[0][cls[j]] : 0.0, 0, am[j], ae[j]);
  }
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
      const double up1m = st::dpp_shift<SHR1>(am[KPL - 1], 0.0);
      const int up1e = st::dpp_shift<SHR1>(ae[KPL - 1], EZ);
      const double up2m = st::dpp_shift<SHR1>(KPL >= 2 ? am[KPL >= 2 ? KPL - 2 : 0] : up1m, 0.0);
      const int up2e = st::dpp_shift<SHR1>(KPL >= 2 ? ae[KPL >= 2 ? KPL - 2 : 0] : up1e, EZ);
      double nm[KPL];
      int ne[KPL];
#pragma unroll
      for (int j = 0; j < KPL; ++j) {
        const double m1 = j >= 1 ? am[j >= 1 ? j - 1 : 0] : up1m;
        const int e1 = j >= 1 ? ae[j >= 1 ? j - 1 : 0] : up1e;
        const double m2 = j >= 2 ? am[j >= 2 ? j - 2 : 0] : (j == 1 ? up1m : up2m);
        const int e2 = j >= 2 ? ae[j >= 2 ? j - 2 : 0] : (j == 1 ? up1e : up2e);
        st::cf_cell(am[j], ae[j], m1, e1, m2, e2, skip[j], em[j], nm[j], ne[j]);
      }
#pragma unroll
      for (int j = 0; j < KPL; ++j) { am[j] = nm[j]; ae[j] = ne[j]; }
    }
    if (ch + 1 < nchunks) {
      chunk_store(buf ^ 1);
      __syncthreads();
    }
  }
#pragma unroll
  for (int j = 0; j < KPL; ++j) {
    const int u = lane * KPL + j;
    if (u == U - 1) { fin_m[0] = am[j]; fin_e[0] = ae[j]; }
    if (u == U - 2) { fin_m[1] = am[j]; fin_e[1] = ae[j]; }
  }
  __syncthreads();
  if (lane == 0) ln_p[job] = st::cf_total(fin_m[0], fin_e[0], fin_m[1], fin_e[1]);
}

__global__ __launch_bounds__(256) void conf_finish_kernel(const double* __restrict__ ln_p, int B, int n_words,
                                                          const int* __restrict__ word_spans,
                                                          const int* __restrict__ status, double* __restrict__ log_prob,
                                                          double* __restrict__ log_conf) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < B) {
    log_prob[i] = status[i] != 0 ? ST_AL_NEG_INF : ln_p[i];
  } else if (i < B + n_words) {
    const int b = word_spans[3 * (long)(i - B)];
    const bool ok = b >= 0 && b < B && status[b] == 0;
    log_conf[i - B] = ok ? st::cf_log_conf(ln_p[b], ln_p[i]) : CF_NAN;
  }
}

// the host form of one job on the softmax rows [T][32] of its utterance
double conf_host_job(const double* rows, int C, const int* lab, int L, int Tb, int first, int last) {
  const int blank = C - 1;
  const int L2 = first < 0 ? L : L - (last - first) + 1;
  const int U = 2 * L2 + 1;
  int lab2[LMAX];
  for (int i = 0; i < L2; ++i) lab2[i] = st::cf_job_label(lab, i, first, last, blank);
  int cls[2 * LMAX];
  bool skip[2 * LMAX];
  for (int u = 0; u < U; ++u) {
    cls[u] = st::cf_state_column(u, lab2, L2, blank);
    skip[u] = st::lattice_skip_from_below(u, lab2);
  }
  double m[2][2 * LMAX];                  // the lattice columns of frames t-1 and t (U <= 1023)
  int e[2][2 * LMAX];
  for (int u = 0; u < U; ++u) st::cf_norm(u < 2 ? rows[cls[u]] : 0.0, 0, m[0][u], e[0][u]);
  for (int t = 1; t < Tb; ++t) {
    const double* am = m[(t - 1) & 1];
    const int* ae = e[(t - 1) & 1];
    const double* row = rows + (long)t * CP;
    for (int u = 0; u < U; ++u)
      st::cf_cell(am[u], ae[u], u >= 1 ? am[u - 1] : 0.0, u >= 1 ? ae[u - 1] : EZ, u >= 2 ? am[u - 2] : 0.0,
                  u >= 2 ? ae[u - 2] : EZ, skip[u], row[cls[u]], m[t & 1][u], e[t & 1][u]);
  }
  const double* am = m[(Tb - 1) & 1];
  const int* ae = e[(Tb - 1) & 1];
  return st::cf_total(am[U - 1], ae[U - 1], U > 1 ? am[U - 2] : 0.0, U > 1 ? ae[U - 2] : EZ);
}

bool conf_args_ok(int batch, int frames, int classes, int max_label_len, int space_id, int n_words) {
  return batch > 0 && frames > 0 && classes >= 2 && classes <= st::CF_MAX_CLASSES && space_id >= 0 && space_id < classes - 1 &&
         n_words >= 0 && st::lattice_kpl(max_label_len) > 0;
}

// the three stages on B utterances of T rows each: `map` names a row for the softmax stage (which is also the gather), `lens` the
// frames of an utterance for the lattices, which read the workspace only
template <typename Map, typename Lens>
void launch_conf(const float* base, Map map, Lens lens, int B, int T, int C, int max_label_len, const int* label_ids,
                 const int* label_offsets, int space_id, const int* word_spans, int n_words, double* log_prob, double* log_conf,
                 int* status, void* workspace, hipStream_t s) {
  const size_t nrows = (size_t)B * T;
  const int jobs = B + n_words;
  double* rows = reinterpret_cast<double*>(workspace);
  double* ln_p = rows + nrows * CP;
  const dim3 grid((unsigned)((nrows + 7) / 8));
  if constexpr (std::is_same<Map, RowMap>::value) {
    hipLaunchKernelGGL(conf_softmax_kernel, grid, dim3(256), 0, s, base, map, B, T, C, space_id, rows);
  } else {
    hipLaunchKernelGGL(conf_softmax_ring_kernel, grid, dim3(256), 0, s, base, map, B, T, C, space_id, rows);
  }
  st::dispatch_kpl(st::lattice_kpl(max_label_len), [&](auto k) {
    hipLaunchKernelGGL((conf_lattice_kernel<k(), Lens>), dim3(jobs), dim3(64), 0, s, rows, B, T, C, label_ids, label_offsets, lens,
                       word_spans, ln_p, status);
  });
  hipLaunchKernelGGL(conf_finish_kernel, dim3((jobs + 255) / 256), dim3(256), 0, s, ln_p, B, n_words, word_spans, status, log_prob,
                     log_conf);
}

}  // namespace

extern "C" {

size_t st_ctc_word_conf_ws(int batch, int frames, int max_label_len, int max_jobs) {
  if (st::lattice_kpl(max_label_len) < 0 || batch <= 0 || frames <= 0 || max_jobs < batch) return 0;
  // softmax rows [batch * frames][32] double | ln P of every job [max_jobs] double
  return (size_t)batch * frames * CP * sizeof(double) + (size_t)max_jobs * sizeof(double) + 512;
}

int st_ctc_word_conf_f32(const st_tensor3* logits, const int32_t* label_ids, const int32_t* label_offsets,
                         const int32_t* seq_lens, int max_label_len, int space_id, const int32_t* word_spans, int n_words,
                         double* log_prob, double* log_conf, int32_t* status, void* workspace, size_t workspace_bytes,
                         void* stream) {
  ST_REQUIRE(logits && logits->base && label_ids && label_offsets && seq_lens && log_prob && status && workspace,
             "ctc_word_conf: null argument");
  ST_REQUIRE(n_words == 0 || (word_spans && log_conf), "ctc_word_conf: null argument");
  ST_REQUIRE(logits->batch > 0 && logits->frames > 0 && logits->halo >= 0 && logits->t_pitch >= logits->halo + logits->frames &&
             logits->c_pitch >= logits->channels, "ctc_word_conf: bad logits shape");
  ST_REQUIRE(conf_args_ok(logits->batch, logits->frames, logits->channels, max_label_len, space_id, n_words),
             "ctc_word_conf: needs 2 <= num_classes <= 30, 0 <= space_id < num_classes - 1, 0 <= max_label_len <= 511, n_words >= 0");
  const int B = logits->batch, T = logits->frames, C = logits->channels;
  ST_REQUIRE((long)B + n_words <= 0x7fffffffL, "ctc_word_conf: too many jobs");
  ST_REQUIRE(workspace_bytes >= st_ctc_word_conf_ws(B, T, max_label_len, B + n_words), "ctc_word_conf: workspace too small");
  ST_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "ctc_word_conf: workspace must be 16-byte aligned");
  launch_conf(logits->base, st::row_map(*logits), st::DenseLens{seq_lens}, B, T, C, max_label_len, label_ids, label_offsets, space_id,
              word_spans, n_words, log_prob, log_conf, status, workspace, st::as_stream(stream));
  return st::check_launch("ctc_word_conf");
}

int st_ctc_word_conf_ring_f32(const float* ring, int max_streams, int cap, int num_classes, const int32_t* jobs, int n_jobs,
                              int max_rows, const int32_t* label_ids, const int32_t* label_offsets, int max_label_len, int space_id,
                              const int32_t* word_spans, int n_words, double* log_prob, double* log_conf, int32_t* status,
                              void* workspace, size_t workspace_bytes, void* stream) {
  ST_REQUIRE(ring && jobs && label_ids && label_offsets && log_prob && status && workspace, "ctc_word_conf_ring: null argument");
  ST_REQUIRE(n_words == 0 || (word_spans && log_conf), "ctc_word_conf_ring: null argument");
  ST_REQUIRE(max_streams >= 1 && cap >= 1, "ctc_word_conf_ring: bad ring shape");
  ST_REQUIRE(conf_args_ok(n_jobs, max_rows, num_classes, max_label_len, space_id, n_words),
             "ctc_word_conf_ring: needs n_jobs, max_rows >= 1, 2 <= num_classes <= 30, 0 <= space_id < num_classes - 1, "
             "0 <= max_label_len <= 511, n_words >= 0");
  ST_REQUIRE((long)n_jobs + n_words <= 0x7fffffffL, "ctc_word_conf_ring: too many jobs");
  ST_REQUIRE(workspace_bytes >= st_ctc_word_conf_ws(n_jobs, max_rows, max_label_len, n_jobs + n_words),
             "ctc_word_conf_ring: workspace too small");
  ST_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "ctc_word_conf_ring: workspace must be 16-byte aligned");
  st::trace("ctc_word_conf_ring<%d> jobs=%d words=%d rows=%d cap=%d", st::lattice_kpl(max_label_len), n_jobs, n_words, max_rows, cap);
  launch_conf(ring, st::RingMap{jobs, max_streams, max_rows, cap}, st::RingLens{jobs, max_streams, max_rows}, n_jobs, max_rows,
              num_classes, max_label_len, label_ids, label_offsets, space_id, word_spans, n_words, log_prob, log_conf, status, workspace,
              st::as_stream(stream));
  return st::check_launch("ctc_word_conf_ring");
}

int st_ctc_word_conf_host(const float* logits, int batch, int frames, int classes, const int32_t* label_ids,
                          const int32_t* label_offsets, const int32_t* seq_lens, int max_label_len, int space_id,
                          const int32_t* word_spans, int n_words, double* log_prob, double* log_conf, int32_t* status,
                          void* workspace, size_t workspace_bytes) {
  ST_REQUIRE(logits && label_ids && label_offsets && seq_lens && log_prob && status && workspace, "ctc_word_conf: null argument");
  ST_REQUIRE(n_words == 0 || (word_spans && log_conf), "ctc_word_conf: null argument");
  ST_REQUIRE(conf_args_ok(batch, frames, classes, max_label_len, space_id, n_words),
             "ctc_word_conf: needs 2 <= num_classes <= 30, 0 <= space_id < num_classes - 1, 0 <= max_label_len <= 511, n_words >= 0");
  ST_REQUIRE((long)batch + n_words <= 0x7fffffffL, "ctc_word_conf: too many jobs");
  ST_REQUIRE(workspace_bytes >= st_ctc_word_conf_ws(batch, frames, max_label_len, batch + n_words),
             "ctc_word_conf: workspace too small");
  ST_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "ctc_word_conf: workspace must be 16-byte aligned");
  const int B = batch, T = frames, C = classes, UP = st::lattice_kpl(max_label_len) * 64;
  double* rows = reinterpret_cast<double*>(workspace);
  double* ln_p = rows + (size_t)B * T * CP;
  // the utterances: refusal, and the softmax rows of the frames that are used
  for (int b = 0; b < B; ++b) {
    const int* lab = label_ids + label_offsets[b];
    const int L = label_offsets[b + 1] - label_offsets[b], Tb = seq_lens[b];
    int rep = 0;
    if ((unsigned)(2 * L + 1) <= (unsigned)UP) for (int i = 1; i < L; ++i) rep += lab[i] == lab[i - 1];
    status[b] = st::lattice_refused(L, rep, Tb, T, UP) ? 1 : 0;
    if (status[b]) continue;
    for (int t = 0; t < Tb; ++t) {
      const float* x = logits + ((size_t)b * T + t) * C;
      double* row = rows + ((size_t)b * T + t) * CP;
      float m = NEG_INF_F;
      for (int c = 0; c < C; ++c) m = fmaxf(m, x[c]);
      double ex[CP], q[CP];
      for (int c = 0; c < CP; ++c) ex[c] = q[c] = c < C ? st::al_exp((double)x[c] - (double)m) : 0.0;
      const double s = st::al_row_sum(q);
      for (int c = 0; c < CP; ++c) {
        row[c] = c < C ? st::cf_prob(ex[c], s) : 0.0;
        q[c] = c != space_id ? row[c] : 0.0;
      }
      row[st::CF_STAR] = st::al_row_sum(q);
    }
  }
  for (int job = 0; job < B + n_words; ++job) {
    const Job jb = conf_job(job, B, word_spans, label_offsets);
    if (!jb.ok || status[jb.b]) { ln_p[job] = CF_NAN; continue; }
    const int b = jb.b, L = label_offsets[b + 1] - label_offsets[b], Tb = seq_lens[b];
    ln_p[job] = Tb == 0 ? 0.0 : conf_host_job(rows + (size_t)b * T * CP, C, label_ids + label_offsets[b], L, Tb, jb.first, jb.last);
  }
  for (int b = 0; b < B; ++b) log_prob[b] = status[b] ? ST_AL_NEG_INF : ln_p[b];
  for (int w = 0; w < n_words; ++w) {
    const int b = word_spans[3 * (size_t)w];
    const bool ok = b >= 0 && b < B && status[b] == 0;
    log_conf[w] = ok ? st::cf_log_conf(ln_p[b], ln_p[B + w]) : CF_NAN;
  }
  return ST_OK;
}

}  // extern "C"
