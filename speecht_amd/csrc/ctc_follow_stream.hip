// Following a known script in live streams on gfx950, and its host form (semantics: include/speecht_hip.h; specification:
// tests/follow_oracle.py).
//
// The lattice is st_ctc_align_f32's -- max-plus in double on the ln-softmax rows -- for ONE long label per stream, carried across
// steps in the tiled geometry of ctc_align_long.hip: lane l of state block j holds the 16 states 896 j - 128 + 16 l ..., lanes 8-63
// the 896 states the block owns, lanes 0-7 a halo of 128 states recomputed from the lower neighbour's column of the previous
// launch, exact for 64 frames.  No back-pointers: after every frame the best state, lowest among equals, is read out instead.
//
// A step is cut into runs of at most 64 rows per stream; per run:
//  1. (once per step) align_logsoftmax_kernel (ctc_align_softmax.h): the ln-softmax rows of the step's rows [n_rows][32] in double, read in place.
//  2. follow_tile_kernel, one wave per (state block, stream).  It reads the stream's header and table entry, tells the read-out
//     what the stream does in this run (the run record), and, for a stream that takes rows: the current column (frame 0 by
//     formula), the frames, per frame one {value, lowest state} over its owned real states to the workspace, the new column to the
//     SECOND buffer.  A block no finite value can have reached by the run's last frame only leaves -inf there.
//  3. follow_read_kernel, block 0 of a stream: one wave, lane i on frame i of the run folds the blocks' partial maxima, lower block
//     first; pos, the sliding minimum over the last K frames (the header keeps the last 16 positions), then in frame order g, the
//     events and the record; it alone writes the header.  Blocks 1 .. NB of the same launch publish the new column: they copy it
//     over the stream's column, which no wave reads any more.  So the tile kernel never writes what a neighbour's halo still
//     reads, a stream's column is always the first buffer, and a state's bytes do not depend on how the rows were cut.
#include <algorithm>
#include <cstring>
#include <vector>

#include "ctc_align_softmax.h"
#include "ctc_follow_core.h"
#include "ctc_lattice.h"
#include "st_common.h"

namespace {

namespace fl = st::follow;
constexpr int SHR1 = st::DPP_WAVE_SHR1;
constexpr int CP = st::AL_CP;
constexpr int TB = fl::TB, KPL = fl::KPL, HALO = fl::HALO, SB = fl::SB, OWN0 = fl::OWN0;
constexpr int RB = 8;                  // frames whose partial maxima the tile kernel folds across lanes at once
static_assert(TB == st::LATTICE_TC, "a run is one LDS chunk");

struct Args {
  const int32_t* rows;
  const int32_t* table;
  const int32_t* script_ids;
  const int32_t* script_offsets;
  const int32_t* word_starts;
  const int32_t* word_offsets;
  char* state;
  long stream_bytes;
  int max_labels, C, confirm, max_events, n_rows, n_runs;
};

struct Workspace {
  double* ly;          // [max_rows][32]
  fl::Best* best;      // [max_streams][64][NBmax]
  int32_t* run;        // [max_streams][8]
};

Workspace carve(void* workspace, int max_rows, int max_labels, int max_streams) {
  Workspace w;
  w.ly = reinterpret_cast<double*>(workspace);
  w.best = reinterpret_cast<fl::Best*>(w.ly + (size_t)max_rows * CP);
  w.run = reinterpret_cast<int32_t*>(w.best + (size_t)max_streams * TB * fl::state_blocks(max_labels));
  return w;
}

__global__ __launch_bounds__(64) void follow_tile_kernel(Args a, int run, int NBmax, const double* __restrict__ ly,
                                                         fl::Best* __restrict__ best, int32_t* __restrict__ runrec) {
  __shared__ __attribute__((aligned(16))) double E[TB * CP];
  __shared__ double2 R[RB * 64];                              // the lanes' bests of up to RB frames: {value, state}
  const int lane = threadIdx.x, jb = blockIdx.x, s = blockIdx.y;
  const int first = a.table[4 * s], count = a.table[4 * s + 1], limit = a.table[4 * s + 2];
  const int reset = run == 0 && a.table[4 * s + 3] != 0;
  const int L = a.script_offsets[s + 1] - a.script_offsets[s];
  char* sbase = a.state + (long)s * a.stream_bytes;
  const int32_t* hdr = reinterpret_cast<const int32_t*>(sbase);
  const int f0 = count > 0 ? a.rows[2 * (long)first + 1] : 0;
  const int n_all = fl::rows_taken(count, limit, f0);
  const int n = min(max(n_all - TB * run, 0), TB);
  const int what = L <= 0 ? fl::NO_SCRIPT : (L > a.max_labels ? fl::TOO_LONG : (n == 0 && !reset ? fl::SITS_OUT : fl::ACTIVE));
  const int t0 = reset ? 0 : hdr[fl::H_FRAMES];
  const int row0 = first + TB * run;
  if (jb == 0 && lane == 0) {
    const int lost = run == a.n_runs - 1 && n_all > TB * a.n_runs;
    int4* dst = reinterpret_cast<int4*>(runrec + fl::kRunWords * s);
    dst[0] = make_int4(what, 0, t0, n);
    dst[1] = make_int4(row0, L, reset, lost);
  }
  if (what != fl::ACTIVE) return;
  const int U = 2 * L + 1, NB = fl::state_blocks(L);
  if (jb >= NB) return;
  const double* colin = fl::column(sbase, a.max_labels, 0);     // the stream's column
  double* colout = fl::column(sbase, a.max_labels, 1);          // the run's new column, which the read-out launch publishes
  if (jb == 0 && reset) reinterpret_cast<double2*>(colout)[lane] = make_double2(ST_AL_NEG_INF, ST_AL_NEG_INF);   // below state 0
  const int u0 = jb * SB - HALO + lane * KPL;                 // the lane's first state; below 0 in block 0's halo
  const bool own = lane >= OWN0;
  const long t_last = (long)t0 + n - 1;
  if (n == 0 || (long)jb * SB > 2 * t_last + 1) {             // nothing finite can be here yet
    if (own) {
      double2* dst = reinterpret_cast<double2*>(colout + HALO + u0);
#pragma unroll
      for (int j = 0; j < KPL; j += 2) dst[j / 2] = make_double2(ST_AL_NEG_INF, ST_AL_NEG_INF);
    }
    return;
  }
  const int* lab = a.script_ids + a.script_offsets[s];
  const int blank = a.C - 1;
  int cls[KPL];
  bool skip[KPL], real[KPL];
#pragma unroll
  for (int j = 0; j < KPL; ++j) {
    const int u = u0 + j;
    real[j] = (unsigned)u < (unsigned)U;
    cls[j] = real[j] ? st::lattice_class(u, lab, blank) : blank;
    skip[j] = real[j] && st::lattice_skip_from_below(u, lab);
  }
  st::ChunkStage<double, CP> stage;
  stage.load(ly + (long)row0 * CP, 0, n, lane);
  stage.store(E, lane);
  __syncthreads();
  double v[KPL];
  if (t0 == 0) {
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
      const int u = u0 + j;
      v[j] = (unsigned)u < 2u && u < U ? E[cls[j]] : ST_AL_NEG_INF;
    }
  } else {
    const double2* src = reinterpret_cast<const double2*>(colin + HALO + u0);
#pragma unroll
    for (int j = 0; j < KPL; j += 2) {
      const double2 x = src[j / 2];
      v[j] = x.x;
      v[j + 1] = x.y;
    }
  }
  fl::Best* out = best + ((long)s * TB) * NBmax + jb;
  // The block's best owned real state of frame i, off the dependent chain: the next frame does not wait for it.  Per frame a lane
  // folds its own 16 states and parks the pair in LDS; every RB frames the wave folds the parked pairs of all of them at once, 64 / RB
  // lanes per frame -- each RB pairs in lane order, then a butterfly among them -- so the cross-lane moves are paid once per RB frames.
  auto reduce = [&](int i) {
    fl::Best b{ST_AL_NEG_INF, fl::NO_STATE, 0};
#pragma unroll
    for (int j = 0; j < KPL; ++j)
      if (own && real[j]) fl::fold_above(b, v[j], u0 + j);
    R[(i % RB) * 64 + lane] = make_double2(b.v, __builtin_bit_cast(double, (long long)(unsigned)b.u));
    if (i % RB != RB - 1 && i != n - 1) return;
    __syncthreads();
    const int f0 = i - i % RB, fi = lane / (64 / RB), part = lane % (64 / RB);
    fl::Best w{ST_AL_NEG_INF, fl::NO_STATE, 0};
#pragma unroll
    for (int k = 0; k < RB; ++k) {                            // (lanes in order are states in order: the lower one stays among equals)
      const double2 x = R[fi * 64 + part * RB + k];
      fl::fold_above(w, x.x, (int)__builtin_bit_cast(long long, x.y));
    }
#pragma unroll
    for (int o = 64 / RB / 2; o > 0; o >>= 1) {
      const double ov = __shfl_xor(w.v, o, 64);
      const int ou = __shfl_xor(w.u, o, 64);
      fl::fold_any(w, ov, ou);
    }
    if (part == 0 && f0 + fi <= i)
      *reinterpret_cast<double2*>(out + (long)(f0 + fi) * NBmax) = make_double2(w.v, __builtin_bit_cast(double, (long long)(unsigned)w.u));
    __syncthreads();                                          // the next frames park over these
  };
  int i = 0;
  if (t0 == 0) {
    reduce(0);
    i = 1;
  }
  for (; i < n; ++i) {
    const double* e = &E[i * CP];
    double em[KPL];
#pragma unroll
    for (int j = 0; j < KPL; ++j) em[j] = e[cls[j]];
    const double up1 = st::dpp_shift<SHR1>(v[KPL - 1], ST_AL_NEG_INF);
    const double up2 = st::dpp_shift<SHR1>(v[KPL - 2], ST_AL_NEG_INF);
    double nv[KPL];
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
      const double adv = j >= 1 ? v[j >= 1 ? j - 1 : 0] : up1;
      const double skp = j >= 2 ? v[j >= 2 ? j - 2 : 0] : (j == 1 ? up1 : up2);
      int move;
      nv[j] = st::al_cell(v[j], adv, skp, skip[j], em[j], move);
    }
#pragma unroll
    for (int j = 0; j < KPL; ++j) v[j] = nv[j];
    reduce(i);
  }
  if (own) {
    double2* dst = reinterpret_cast<double2*>(colout + HALO + u0);
#pragma unroll
    for (int j = 0; j < KPL; j += 2)
      dst[j / 2] = make_double2(real[j] ? v[j] : ST_AL_NEG_INF, real[j + 1] ? v[j + 1] : ST_AL_NEG_INF);
  }
}

__device__ __forceinline__ int lo32(double x) { return (int)st::al_bits(x); }
__device__ __forceinline__ int hi32(double x) { return (int)(st::al_bits(x) >> 32); }
__device__ __forceinline__ double from32(int lo, int hi) { return st::al_from_bits(((long long)hi << 32) | (unsigned int)lo); }

__global__ __launch_bounds__(64) void follow_read_kernel(Args a, int run, int NBmax, const double* __restrict__ ly,
                                                         const fl::Best* __restrict__ best, const int32_t* __restrict__ runrec,
                                                         int32_t* __restrict__ events, int32_t* __restrict__ result,
                                                         int32_t* __restrict__ trace) {
  const int lane = threadIdx.x, s = blockIdx.y;
  const int32_t* rr = runrec + fl::kRunWords * s;
  const int what = rr[fl::I_WHAT], t0 = rr[fl::I_T0], n = rr[fl::I_N], row0 = rr[fl::I_ROW0], L = rr[fl::I_L];
  const int reset = rr[fl::I_RESET], lost = rr[fl::I_LOST];
  char* sbase = a.state + (long)s * a.stream_bytes;
  if (blockIdx.x > 0) {
    // publish the run's new column, block by block (block 0's wave also the elements below state 0, -inf since the reset)
    const int jb = blockIdx.x - 1;
    if (what != fl::ACTIVE || jb >= fl::state_blocks(L)) return;
    const double2* src = reinterpret_cast<const double2*>(fl::column(sbase, a.max_labels, 1));
    double2* dst = reinterpret_cast<double2*>(fl::column(sbase, a.max_labels, 0));
    if (jb == 0) dst[lane] = src[lane];
    const long at = (HALO + (long)jb * SB) / 2;
#pragma unroll
    for (int k = 0; k < SB / 2 / 64; ++k) dst[at + k * 64 + lane] = src[at + k * 64 + lane];
    return;
  }
  int32_t* rec = result + fl::kResultWords * s;
  int32_t* hdr = reinterpret_cast<int32_t*>(sbase);
  if (what == fl::NO_SCRIPT || what == fl::TOO_LONG) {
    if (run == 0 && lane < fl::kResultWords)
      rec[lane] = lane == fl::R_C ? -1 : (lane == fl::R_STATUS ? (what == fl::TOO_LONG ? fl::STATUS_TOO_LONG : fl::STATUS_NO_SCRIPT) : 0);
    return;
  }
  if (what == fl::SITS_OUT && run > 0) return;
  int frames = t0, nw = 0, c = -1, histv = 0;
  double g = 0.0, b = ST_AL_NEG_INF, end = ST_AL_NEG_INF;
  if (!reset) {
    nw = hdr[fl::H_WORDS];
    c = hdr[fl::H_C];
    g = from32(hdr[fl::H_G], hdr[fl::H_G + 1]);
    b = from32(hdr[fl::H_B], hdr[fl::H_B + 1]);
    end = from32(hdr[fl::H_END], hdr[fl::H_END + 1]);
    histv = hdr[fl::H_HIST + (lane & 15)];
  }
  int count = run == 0 ? 0 : rec[fl::R_EVENTS];
  if (what == fl::ACTIVE) {
    if (n > 0) {
      const int U = 2 * L + 1, NB = fl::state_blocks(L);
      const bool valid = lane < n;
      const long t = (long)t0 + lane;
      fl::Best bt{ST_AL_NEG_INF, fl::NO_STATE, 0};
      double mx = 0.0;
      if (valid) {
        const int nb = (int)min((long)NB, (2 * t + 1) / SB + 1);         // the blocks a finite value can have reached
        const fl::Best* p = best + ((long)s * TB + lane) * NBmax;
        for (int j = 0; j < nb; ++j) fl::fold_above(bt, p[j].v, p[j].u);
        mx = fl::row_max(ly + ((long)row0 + lane) * CP, a.C);
      }
      const int ct = fl::cursor(bt);
      const int pos = fl::position(ct);
      if (trace && valid) trace[row0 + lane] = ct;
      int m = pos;
      for (int k = 1; k < a.confirm; ++k) {
        const int idx = lane - k;
        const int p_run = __shfl(pos, idx & 63, 64);
        const int p_hist = __shfl(histv, (t0 + idx) & 15, 64);
        const int p = idx >= 0 ? p_run : ((long)t0 + idx >= 0 ? p_hist : 0);
        m = min(m, p);
      }
      const int* wstart = a.word_starts + a.word_offsets[s];
      const int W = a.word_offsets[s + 1] - a.word_offsets[s];
      int32_t* ev = events + (long)s * a.max_events * fl::kEventWords;
      const int nn = __builtin_amdgcn_readfirstlane(n);
      for (int i = 0; i < nn; ++i)                                        // g's adds in frame order (a lane's value by v_readlane)
        g = g + from32(__builtin_amdgcn_readlane(lo32(mx), i), __builtin_amdgcn_readlane(hi32(mx), i));
      // The events, without a chain of loads from frame to frame: the word starts increase, so the words reached after frame i are
      // those that begin below the largest m so far -- a prefix maximum over the lanes, then per lane a search that gallops up from
      // the count the run began with -- and frame i emits the words between its neighbour's count and its own.
      int big = valid ? m : 0;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int below = __shfl_up(big, o, 64);
        if (lane >= o) big = max(big, below);
      }
      int lo = nw, step = 1;                                              // words [0, lo) begin below big; find the first that does not
      while (lo + step <= W && wstart[lo + step - 1] < big) { lo += step; step <<= 1; }
      for (step >>= 1; step > 0; step >>= 1)
        if (lo + step <= W && wstart[lo + step - 1] < big) lo += step;
      const int below = __shfl_up(lo, 1, 64);                             // (every lane takes part: a lane that sat out would read as 0)
      const int prev = lane == 0 ? nw : below;
      if (valid)
        for (int j = prev; j < lo; ++j) {                                 // (nw <= prev <= lo <= W)
          const int at = count + (j - nw);
          if (at >= 0 && at < a.max_events) *reinterpret_cast<int2*>(ev + (long)at * fl::kEventWords) = make_int2(j, t0 + lane);
        }
      const int nw_end = __shfl(lo, nn - 1, 64);
      count += nw_end - nw;
      nw = nw_end;
      b = __shfl(bt.v, n - 1, 64);
      c = __shfl(ct, n - 1, 64);
      const double* col = fl::column(sbase, a.max_labels, 1);
      end = col[HALO + st::al_end_state(U, col[HALO + U - 1], col[HALO + U - 2])];
      const int t_last = t0 + n - 1;
      const int f = fl::hist_frame(t_last, lane & 15);
      const int p_new = __shfl(pos, (f - t0) & 63, 64);
      if (f >= t0) histv = p_new;
      frames = t0 + n;
    }
    if (lane < fl::kHeaderWords) {
      int w = 0;
      switch (lane) {
        case fl::H_FRAMES: w = frames; break;
        case fl::H_WORDS: w = nw; break;
        case fl::H_C: w = c; break;
        case fl::H_G: w = lo32(g); break;
        case fl::H_G + 1: w = hi32(g); break;
        case fl::H_B: w = lo32(b); break;
        case fl::H_B + 1: w = hi32(b); break;
        case fl::H_END: w = lo32(end); break;
        case fl::H_END + 1: w = hi32(end); break;
        default: w = lane >= fl::H_HIST ? histv : 0;
      }
      hdr[lane] = w;
    }
  }
  if (lane < fl::kResultWords) {
    const double fit = b - g;
    int w = 0;
    switch (lane) {
      case fl::R_FRAMES: w = frames; break;
      case fl::R_C: w = c; break;
      case fl::R_STATUS: w = (lost ? fl::STATUS_ROWS_LOST : 0) | (run > 0 ? rec[fl::R_STATUS] : 0); break;
      case fl::R_EVENTS: w = count; break;
      case fl::R_FIT: w = lo32(fit); break;
      case fl::R_FIT + 1: w = hi32(fit); break;
      case fl::R_END: w = lo32(end); break;
      case fl::R_END + 1: w = hi32(end); break;
      case fl::R_WORDS: w = nw; break;
      default: w = 0;
    }
    rec[lane] = w;
  }
}

int check(const char* who, const void* logits, int pitch, int C, const void* rows, const void* table, int n_rows, int max_rows,
          int max_stream_rows, int max_streams, const void* script_ids, const void* script_offsets, const void* word_starts,
          const void* word_offsets, int max_labels, int confirm, const void* state, const void* events, int max_events,
          const void* result, const void* workspace, size_t workspace_bytes) {
  ST_REQUIRE(logits && rows && table && script_ids && script_offsets && word_starts && word_offsets && state && events && result &&
                 workspace, "%s: null argument", who);
  ST_REQUIRE(C >= 2 && C <= CP && pitch >= C, "%s: num_classes must be 2..32 and <= pitch", who);
  ST_REQUIRE(max_labels >= 1 && max_labels <= fl::MAX_LABELS, "%s: max_labels %d outside 1..%d", who, max_labels, fl::MAX_LABELS);
  ST_REQUIRE(max_streams >= 1 && max_streams <= 65535, "%s: max_streams %d outside 1..65535", who, max_streams);
  ST_REQUIRE(n_rows >= 0 && n_rows <= max_rows && max_stream_rows >= 0 && max_stream_rows <= max_rows,
             "%s: needs 0 <= n_rows <= max_rows and 0 <= max_stream_rows <= max_rows", who);
  ST_REQUIRE(confirm >= 1 && confirm <= fl::MAX_CONFIRM, "%s: confirm %d outside 1..%d frames", who, confirm, fl::MAX_CONFIRM);
  ST_REQUIRE(max_events >= 1, "%s: max_events must be at least 1", who);
  ST_REQUIRE(reinterpret_cast<uintptr_t>(state) % 16 == 0 && reinterpret_cast<uintptr_t>(workspace) % 16 == 0 &&
                 reinterpret_cast<uintptr_t>(events) % 8 == 0, "%s: state and workspace must be 16-byte aligned, events 8-byte", who);
  ST_REQUIRE(workspace_bytes >= st_ctc_follow_stream_ws(max_rows, max_labels, max_streams), "%s: workspace too small", who);
  return ST_OK;
}

}  // namespace

extern "C" {

size_t st_ctc_follow_stream_state_bytes(int max_labels) {
  if (max_labels < 1 || max_labels > fl::MAX_LABELS) return 0;
  return (size_t)fl::state_bytes(max_labels);
}

size_t st_ctc_follow_stream_ws(int max_rows, int max_labels, int max_streams) {
  if (max_rows < 1 || max_labels < 1 || max_labels > fl::MAX_LABELS || max_streams < 1 || max_streams > 65535) return 0;
  return (size_t)max_rows * CP * sizeof(double) + (size_t)max_streams * TB * fl::state_blocks(max_labels) * sizeof(fl::Best) +
         (size_t)max_streams * fl::kRunWords * sizeof(int32_t) + 256;
}

int st_ctc_follow_stream_step(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* table, int n_rows,
                              int max_rows, int max_stream_rows, int max_streams, const int32_t* script_ids,
                              const int32_t* script_offsets, const int32_t* word_starts, const int32_t* word_offsets, int max_labels,
                              int confirm, void* state, int32_t* events, int max_events, int32_t* result, int32_t* trace,
                              void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = check("follow stream step", logits, pitch, num_classes, rows, table, n_rows, max_rows, max_stream_rows, max_streams,
                    script_ids, script_offsets, word_starts, word_offsets, max_labels, confirm, state, events, max_events, result,
                    workspace, workspace_bytes))
    return e;
  hipStream_t s = st::as_stream(stream);
  const Workspace w = carve(workspace, max_rows, max_labels, max_streams);
  const int NBmax = fl::state_blocks(max_labels);
  const int n_runs = std::max((max_stream_rows + TB - 1) / TB, 1);      // (a step without rows still serves resets and the record)
  const Args a{rows, table, script_ids, script_offsets, word_starts, word_offsets, reinterpret_cast<char*>(state),
               fl::state_bytes(max_labels), max_labels, num_classes, confirm, max_events, n_rows, n_runs};
  st::trace("ctc_follow_stream streams=%d blocks=%d rows=%d runs=%d", max_streams, NBmax, n_rows, n_runs);
  if (n_rows > 0)
    hipLaunchKernelGGL(st::align_logsoftmax_kernel, dim3((unsigned)((n_rows + 7) / 8)), dim3(256), 0, s, logits, st::RowMap{0, 0, pitch},
                       1, n_rows, num_classes, w.ly);
  for (int run = 0; run < n_runs; ++run) {
    hipLaunchKernelGGL(follow_tile_kernel, dim3(NBmax, max_streams), dim3(64), 0, s, a, run, NBmax, w.ly, w.best, w.run);
    hipLaunchKernelGGL(follow_read_kernel, dim3(NBmax + 1, max_streams), dim3(64), 0, s, a, run, NBmax, w.ly, w.best, w.run, events,
                       result, trace);
  }
  return st::check_launch("ctc_follow_stream");
}

int st_ctc_follow_stream_host(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* table, int n_rows,
                              int max_rows, int max_stream_rows, int max_streams, const int32_t* script_ids,
                              const int32_t* script_offsets, const int32_t* word_starts, const int32_t* word_offsets, int max_labels,
                              int confirm, void* state, int32_t* events, int max_events, int32_t* result, int32_t* trace,
                              void* workspace, size_t workspace_bytes) {
  if (int e = check("follow stream host", logits, pitch, num_classes, rows, table, n_rows, max_rows, max_stream_rows, max_streams,
                    script_ids, script_offsets, word_starts, word_offsets, max_labels, confirm, state, events, max_events, result,
                    workspace, workspace_bytes))
    return e;
  const int C = num_classes, blank = C - 1, K = confirm;
  const int n_runs = std::max((max_stream_rows + TB - 1) / TB, 1);
  const long stream_bytes = fl::state_bytes(max_labels);
  const Workspace w = carve(workspace, max_rows, max_labels, max_streams);
  for (long i = 0; i < n_rows; ++i) {
    const float* row = logits + i * pitch;
    float m = -__builtin_inff();
    for (int c = 0; c < C; ++c) m = fmaxf(m, row[c]);
    double e[CP];
    for (int c = 0; c < CP; ++c) e[c] = c < C ? st::al_exp((double)row[c] - (double)m) : 0.0;
    const double sum = st::al_row_sum(e);
    for (int c = 0; c < CP; ++c) w.ly[i * CP + c] = st::al_log_softmax(c < C ? row[c] : -__builtin_inff(), m, sum);
  }
  std::vector<double> next;
  for (int s = 0; s < max_streams; ++s) {
    int32_t* rec = result + (long)fl::kResultWords * s;
    const int L = script_offsets[s + 1] - script_offsets[s];
    if (L <= 0 || L > max_labels) {
      for (int i = 0; i < fl::kResultWords; ++i) rec[i] = 0;
      rec[fl::R_C] = -1;
      rec[fl::R_STATUS] = L > max_labels ? fl::STATUS_TOO_LONG : fl::STATUS_NO_SCRIPT;
      continue;
    }
    const int first = table[4 * s], count = table[4 * s + 1], limit = table[4 * s + 2], reset = table[4 * s + 3] != 0;
    const int f0 = count > 0 ? rows[2 * (long)first + 1] : 0;
    const int n_all = fl::rows_taken(count, limit, f0);
    char* sbase = reinterpret_cast<char*>(state) + s * stream_bytes;
    int32_t* hdr = reinterpret_cast<int32_t*>(sbase);
    const int* lab = script_ids + script_offsets[s];
    const int* wstart = word_starts + word_offsets[s];
    const int W = word_offsets[s + 1] - word_offsets[s];
    const int U = 2 * L + 1;
    const long own = fl::col_elems(fl::state_blocks(L));                 // the elements of a column the script's blocks cover
    int32_t* ev = events + (long)s * max_events * fl::kEventWords;
    int count_ev = 0, status = 0;
    bool touched = false;
    for (int run = 0; run < n_runs; ++run) {
      const int n = std::min(std::max(n_all - TB * run, 0), TB);
      const bool rst = run == 0 && reset;
      if (n == 0 && !rst) continue;
      touched = true;
      if (rst) {
        for (int i = 0; i < fl::kHeaderWords; ++i) hdr[i] = 0;
        hdr[fl::H_C] = -1;
        const double ninf = ST_AL_NEG_INF;
        std::memcpy(hdr + fl::H_B, &ninf, 8);
        std::memcpy(hdr + fl::H_END, &ninf, 8);
      }
      const int t0 = hdr[fl::H_FRAMES];
      double* a = fl::column(sbase, max_labels, 0) + HALO;              // state u at a[u]
      double* o = fl::column(sbase, max_labels, 1) + HALO;
      if (rst)
        for (int i = -HALO; i < 0; ++i) o[i] = ST_AL_NEG_INF;
      for (long u = 0; u < own - HALO; ++u) o[u] = ST_AL_NEG_INF;
      double g, b;
      std::memcpy(&g, hdr + fl::H_G, 8);
      std::memcpy(&b, hdr + fl::H_B, 8);
      int nw = hdr[fl::H_WORDS], c = hdr[fl::H_C];
      int hist[16];
      for (int i = 0; i < 16; ++i) hist[i] = hdr[fl::H_HIST + i];
      next.assign(U, ST_AL_NEG_INF);
      for (int i = 0; i < n; ++i) {
        const long t = (long)t0 + i;
        const double* lyr = w.ly + ((long)first + TB * run + i) * CP;
        // plain loops over the whole lattice: frame t from the column of frame t - 1 (in o from the run's second frame on)
        const double* prev = i == 0 ? a : o;
        for (int u = 0; u < U; ++u) {
          const int cls = st::lattice_class(u, lab, blank);
          if (t == 0) {
            next[u] = u < 2 ? lyr[cls] : ST_AL_NEG_INF;
          } else {
            int move;
            next[u] = st::al_cell(prev[u], u >= 1 ? prev[u - 1] : ST_AL_NEG_INF, u >= 2 ? prev[u - 2] : ST_AL_NEG_INF,
                                  st::lattice_skip_from_below(u, lab), lyr[cls], move);
          }
        }
        fl::Best bt{ST_AL_NEG_INF, fl::NO_STATE, 0};
        for (int u = 0; u < U; ++u) {
          o[u] = next[u];
          fl::fold_above(bt, next[u], u);
        }
        b = bt.v;
        c = fl::cursor(bt);
        if (trace) trace[first + TB * run + i] = c;
        g = g + fl::row_max(lyr, C);
        hist[t & 15] = fl::position(c);
        int m = hist[t & 15];
        for (int k = 1; k < K; ++k) m = std::min(m, t - k >= 0 ? hist[(t - k) & 15] : 0);
        while (nw < W && m >= wstart[nw] + 1) {
          if (count_ev < max_events) { ev[2 * count_ev] = nw; ev[2 * count_ev + 1] = (int)t; }
          ++count_ev;
          ++nw;
        }
      }
      for (long u = -HALO; u < own - HALO; ++u) a[u] = o[u];           // the new column is the stream's
      hdr[fl::H_FRAMES] = t0 + n;
      hdr[fl::H_WORDS] = nw;
      hdr[fl::H_C] = c;
      std::memcpy(hdr + fl::H_G, &g, 8);
      std::memcpy(hdr + fl::H_B, &b, 8);
      if (n > 0) {
        const double end = o[st::al_end_state(U, o[U - 1], o[U - 2])];
        std::memcpy(hdr + fl::H_END, &end, 8);
      }
      for (int i = 0; i < 16; ++i) hdr[fl::H_HIST + i] = hist[i];
      if (run == n_runs - 1 && n_all > TB * n_runs) status |= fl::STATUS_ROWS_LOST;
    }
    (void)touched;
    double g, b;
    std::memcpy(&g, hdr + fl::H_G, 8);
    std::memcpy(&b, hdr + fl::H_B, 8);
    const double fit = b - g;
    for (int i = 0; i < fl::kResultWords; ++i) rec[i] = 0;
    rec[fl::R_FRAMES] = hdr[fl::H_FRAMES];
    rec[fl::R_C] = hdr[fl::H_C];
    rec[fl::R_STATUS] = status;
    rec[fl::R_EVENTS] = count_ev;
    std::memcpy(rec + fl::R_FIT, &fit, 8);
    std::memcpy(rec + fl::R_END, hdr + fl::H_END, 8);
    rec[fl::R_WORDS] = hdr[fl::H_WORDS];
  }
  return ST_OK;
}

}  // extern "C"
