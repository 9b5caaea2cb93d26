// Keyword spotting in live streams on gfx950, and its host form (semantics: include/speecht_hip.h; specification:
// tests/spot_stream_oracle.py).
//
// The lattice is ctc_spot.hip's -- max-plus in double on d_t(c) = x_t(c) - max_c x_t(c), the start frame travelling with each
// state's value -- carried across steps: a (stream, keyword) pair's whole memory is its 2L+1 values and starts, a pending hit and
// the end of the last hit (ctc_spot_stream_core.h).  A step has some ten frames per stream, so a wave per (stream, keyword) would
// be launch and state traffic and little else: a PLAN, made once on the host, packs the keywords' lattices side by side into
// waves of 64 * KPL states.  Each keyword begins on a lane boundary and its two dead outer states (and the dead padding up to the
// boundary) separate it from its neighbours, so sp_cell runs unmodified across the wave: state 1 of a keyword has no skip and
// advances from a dead state.
//
//  spot_stream_kernel<KPL>: one WAVE per (stream, plan wave).  It loads its record of the stream's state (lane-contiguous arrays),
//  forms d of the stream's new rows in LDS in chunks of LATTICE_TC rows (two rows per pass, the row maximum by a 32-lane butterfly),
//  runs the frames with the DPP shifts of spot_lattice_kernel, lets the lanes that own an end state apply the rule and append
//  events (a vector atomicAdd on the stream's count), and stores the record.  A stream without rows, reset or limit leaves at once.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ctc_lattice.h"
#include "ctc_spot_stream_core.h"
#include "st_common.h"

namespace {

namespace ss = st::spot_stream;
constexpr int SHR1 = st::DPP_WAVE_SHR1;
constexpr int CP = st::SP_CP;
constexpr int TC = st::LATTICE_TC;
#define NEG_INF_F (-__builtin_inff())

template <int KPL>
__global__ __launch_bounds__(64) void spot_stream_kernel(const float* __restrict__ logits, int pitch, int C,
                                                         const int* __restrict__ rows, const int* __restrict__ table,
                                                         const int* __restrict__ plan, int n_waves, double threshold, int hold,
                                                         void* __restrict__ state, long stream_bytes, int* __restrict__ events,
                                                         int max_events, int* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) double E[TC * CP];
  const int s = blockIdx.x / n_waves, w = blockIdx.x - s * n_waves;
  const int lane = threadIdx.x;
  // only a plan st_ctc_spot_stream_plan wrote for these classes and this dispatch is believed
  if (plan[ss::H_MAGIC] != ss::kMagic || plan[ss::H_CLASSES] != C || plan[ss::H_KPL] != KPL || plan[ss::H_WAVES] != n_waves) return;
  const int first = table[4 * s], count = table[4 * s + 1], limit = table[4 * s + 2], reset = table[4 * s + 3];
  if (count <= 0 && limit < 0 && !reset) return;             // the stream sits this step out: its record is not touched
  const int f0 = count > 0 ? rows[2 * (long)first + 1] : 0;
  const int n = ss::rows_taken(count, limit, f0);

  const int* wt = plan + ss::kHeaderWords + (long)w * ss::wave_words(KPL);
  int col[KPL];
  bool skip[KPL], live[KPL], enter[KPL];
  int j_end = 0;
#pragma unroll
  for (int j = 0; j < KPL; ++j) {
    const int d = wt[j * 64 + lane];
    col[j] = d & ss::D_COL;
    skip[j] = (d & ss::D_SKIP) != 0;
    live[j] = (d & ss::D_LIVE) != 0;
    enter[j] = (d & ss::D_ENTER) != 0;
    if (d & ss::D_END) j_end = j;
  }
  const int end_kw = wt[KPL * 64 + lane];

  const ss::StateView rec = ss::state_view(state, stream_bytes, s, w, KPL);
  double v[KPL];
  int st_[KPL];
  ss::Pending pend;
  if (reset) {
#pragma unroll
    for (int j = 0; j < KPL; ++j) { v[j] = ST_SP_NEG_INF; st_[j] = -1; }
    ss::init(pend);
  } else {
#pragma unroll
    for (int j = 0; j < KPL; ++j) { v[j] = rec.v[j * 64 + lane]; st_[j] = rec.s[j * 64 + lane]; }
    pend.score = rec.pscore[lane];
    pend.start = rec.pstart[lane];
    pend.end = rec.pend[lane];
    pend.last_end = rec.last[lane];
  }
  int* ev = events + (long)s * max_events * ss::kEventWords;
  auto emit = [&](const ss::Hit& h, int kind) {
    const int at = atomicAdd(&counts[s], 1);
    ss::write_event(ev, max_events, at, end_kw, h, kind);
  };

  const int c = lane & 31;
  for (int r0 = 0; r0 < n; r0 += TC) {
    const int nr = min(TC, n - r0);
    // d of the chunk's rows: two rows per pass, a row's 32 columns on one half of the wave
    for (int p = 0; 2 * p < nr; ++p) {
      const int i = 2 * p + (lane >> 5);
      const long r = (long)first + r0 + min(i, nr - 1);
      const float x = c < C ? logits[r * pitch + c] : NEG_INF_F;
      float m = x;
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
      if (i < nr) E[i * CP + c] = c < C ? st::sp_ratio(x, m) : ST_SP_NEG_INF;
    }
    __syncthreads();
    for (int i = 0; i < nr; ++i) {
      const int t = f0 + r0 + i;
      const double* e = &E[i * CP];
      double em[KPL];
#pragma unroll
      for (int j = 0; j < KPL; ++j) em[j] = e[col[j]];
      const double up1v = st::dpp_shift<SHR1>(v[KPL - 1], ST_SP_NEG_INF);
      const int up1s = st::dpp_shift<SHR1>(st_[KPL - 1], -1);
      const double up2v = st::dpp_shift<SHR1>(KPL >= 2 ? v[KPL >= 2 ? KPL - 2 : 0] : up1v, ST_SP_NEG_INF);
      const int up2s = st::dpp_shift<SHR1>(KPL >= 2 ? st_[KPL >= 2 ? KPL - 2 : 0] : up1s, -1);
      double nv[KPL];
      int ns[KPL];
#pragma unroll
      for (int j = 0; j < KPL; ++j) {
        const double v1 = j >= 1 ? v[j >= 1 ? j - 1 : 0] : up1v;
        const int s1 = j >= 1 ? st_[j >= 1 ? j - 1 : 0] : up1s;
        const double v2 = j >= 2 ? v[j >= 2 ? j - 2 : 0] : (j == 1 ? up1v : up2v);
        const int s2 = j >= 2 ? st_[j >= 2 ? j - 2 : 0] : (j == 1 ? up1s : up2s);
        st::sp_cell(v[j], st_[j], v1, s1, v2, s2, skip[j], enter[j], live[j], t, em[j], nv[j], ns[j]);
      }
#pragma unroll
      for (int j = 0; j < KPL; ++j) { v[j] = nv[j]; st_[j] = ns[j]; }
      if (end_kw >= 0) {
        double end = v[0];
        int end_start = st_[0];
#pragma unroll
        for (int j = 1; j < KPL; ++j) {
          if (j == j_end) { end = v[j]; end_start = st_[j]; }
        }
        ss::Hit h;
        if (ss::rule(end, end_start, t, threshold, hold, pend, h)) emit(h, 0);
      }
    }
    __syncthreads();                                          // the next chunk's rows replace these
  }
  if (limit >= 0 && end_kw >= 0 && pend.end > 0) {            // the stream has finished: what is pending leaves, flushed
    emit(ss::Hit{pend.score, pend.start, pend.end}, 1);
    pend.last_end = pend.end;
    ss::clear(pend);
  }
#pragma unroll
  for (int j = 0; j < KPL; ++j) { rec.v[j * 64 + lane] = v[j]; rec.s[j * 64 + lane] = st_[j]; }
  rec.pscore[lane] = pend.score;
  rec.pstart[lane] = pend.start;
  rec.pend[lane] = pend.end;
  rec.last[lane] = pend.last_end;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------------

struct Packing {
  int kpl, n_waves;
  std::vector<int> wave, first;          // per keyword: its wave and its first state there
};

int pack_keywords(const int32_t* kw_ids, const int32_t* kw_offsets, int n_keywords, int C, int pack, Packing& out) {
  ST_REQUIRE(kw_ids && kw_offsets, "spot stream plan: null argument");
  ST_REQUIRE(n_keywords >= 1 && C >= 2 && C <= CP && (pack == 0 || pack == 1),
             "spot stream plan: needs n_keywords >= 1, 2 <= num_classes <= 32, pack 0 or 1");
  ST_REQUIRE(kw_offsets[0] >= 0, "spot stream plan: kw_offsets[0] is negative");
  int longest = 0;
  for (int k = 0; k < n_keywords; ++k) {
    ST_REQUIRE(kw_offsets[k + 1] >= kw_offsets[k], "spot stream plan: kw_offsets is not monotone at keyword %d", k);
    const long L = (long)kw_offsets[k + 1] - kw_offsets[k];
    ST_REQUIRE(L >= 1 && L <= 511, "spot stream plan: keyword %d has %ld ids, 1 .. 511 supported", k, L);
    longest = std::max(longest, (int)L);
    for (int i = kw_offsets[k]; i < kw_offsets[k + 1]; ++i)
      ST_REQUIRE(kw_ids[i] >= 0 && kw_ids[i] <= C - 2, "spot stream plan: keyword %d has id %d outside 0 .. %d", k, kw_ids[i], C - 2);
  }
  out.kpl = st::lattice_kpl(longest);
  out.wave.resize(n_keywords);
  out.first.resize(n_keywords);
  int wave = 0, lane = 0;                                     // the next free lane of the wave being filled
  for (int k = 0; k < n_keywords; ++k) {
    const int lanes = (2 * (kw_offsets[k + 1] - kw_offsets[k]) + 1 + out.kpl - 1) / out.kpl;
    if (lane > 0 && (!pack || lane + lanes > 64)) { ++wave; lane = 0; }
    ST_REQUIRE(wave < (1 << 24), "spot stream plan: too many waves");
    out.wave[k] = wave;
    out.first[k] = lane * out.kpl;
    lane += lanes;
  }
  out.n_waves = wave + 1;
  return ST_OK;
}

// the header of a plan this file wrote, for num_classes classes (0: any)
bool plan_ok(const int32_t* p, int C) {
  if (!p || p[ss::H_MAGIC] != ss::kMagic) return false;
  const int kpl = p[ss::H_KPL], nw = p[ss::H_WAVES], nk = p[ss::H_KEYWORDS];
  if (nk < 1 || nw < 1 || nw > nk) return false;
  bool listed = false;
#define ST_SS_LISTED(K) listed = listed || kpl == K;
  ST_LATTICE_KPLS(ST_SS_LISTED)
#undef ST_SS_LISTED
  if (!listed || p[ss::H_CLASSES] < 2 || p[ss::H_CLASSES] > CP || (C && p[ss::H_CLASSES] != C)) return false;
  return p[ss::H_WORDS] == ss::plan_words(kpl, nw, nk) && p[ss::H_KW_AT] == ss::kHeaderWords + (long)nw * ss::wave_words(kpl);
}

int check_step(const char* who, const void* logits, int pitch, int C, const void* rows, const void* table, int n_rows, int max_streams,
               const int32_t* plan, double threshold, int hold, const void* state, const void* events, int max_events,
               const void* counts) {
  ST_REQUIRE(logits && rows && table && plan && state && events && counts, "%s: null argument", who);
  ST_REQUIRE(plan_ok(plan, 0), "%s: the plan is not one st_ctc_spot_stream_plan wrote", who);
  ST_REQUIRE(C == plan[ss::H_CLASSES] && pitch >= C, "%s: %d classes at pitch %d, the plan was made for %d classes", who, C, pitch,
             plan[ss::H_CLASSES]);
  ST_REQUIRE(n_rows >= 0 && max_streams >= 1 && max_events >= 1, "%s: needs n_rows >= 0, max_streams >= 1, max_events >= 1", who);
  ST_REQUIRE((long)max_streams * plan[ss::H_WAVES] < (1L << 31), "%s: %d streams of %d waves are more than one launch holds", who,
             max_streams, plan[ss::H_WAVES]);
  ST_REQUIRE(!std::isnan(threshold) && threshold <= 0.0, "%s: threshold must be <= 0 or -inf", who);
  ST_REQUIRE(hold >= 1, "%s: hold %d must be at least 1 frame", who, hold);
  ST_REQUIRE(reinterpret_cast<uintptr_t>(state) % 8 == 0, "%s: state must be 8-byte aligned", who);
  return ST_OK;
}

}  // namespace

extern "C" {

size_t st_ctc_spot_stream_plan_bytes(const int32_t* kw_ids, const int32_t* kw_offsets, int n_keywords, int num_classes, int pack) {
  Packing p;
  if (pack_keywords(kw_ids, kw_offsets, n_keywords, num_classes, pack, p) != ST_OK) return 0;
  return (size_t)ss::plan_words(p.kpl, p.n_waves, n_keywords) * sizeof(int32_t);
}

int st_ctc_spot_stream_plan(const int32_t* kw_ids, const int32_t* kw_offsets, int n_keywords, int num_classes, int pack, void* plan,
                            int* n_waves) {
  ST_REQUIRE(plan && n_waves, "spot stream plan: null argument");
  Packing p;
  if (int e = pack_keywords(kw_ids, kw_offsets, n_keywords, num_classes, pack, p)) return e;
  const int KPL = p.kpl, blank = num_classes - 1;
  const long words = ss::plan_words(KPL, p.n_waves, n_keywords);
  ST_REQUIRE(words < (1L << 31), "spot stream plan: too large");
  int32_t* w = reinterpret_cast<int32_t*>(plan);
  std::memset(w, 0, (size_t)words * sizeof(int32_t));
  w[ss::H_MAGIC] = ss::kMagic;
  w[ss::H_WORDS] = (int32_t)words;
  w[ss::H_KEYWORDS] = n_keywords;
  w[ss::H_CLASSES] = num_classes;
  w[ss::H_KPL] = KPL;
  w[ss::H_WAVES] = p.n_waves;
  w[ss::H_PACK] = pack;
  w[ss::H_KW_AT] = ss::kHeaderWords + p.n_waves * ss::wave_words(KPL);
  for (int wave = 0; wave < p.n_waves; ++wave) {
    int32_t* wt = w + ss::kHeaderWords + (long)wave * ss::wave_words(KPL);
    for (int i = 0; i < KPL * 64; ++i) wt[i] = st::sp_column(blank);     // dead: reads the blank's column, keeps nothing
    for (int l = 0; l < 64; ++l) wt[KPL * 64 + l] = -1;
  }
  for (int k = 0; k < n_keywords; ++k) {
    const int* lab = kw_ids + kw_offsets[k];
    const int L = kw_offsets[k + 1] - kw_offsets[k];
    int32_t* wt = w + ss::kHeaderWords + (long)p.wave[k] * ss::wave_words(KPL);
    for (int u = 1; u <= 2 * L - 1; ++u) {
      const int g = p.first[k] + u;
      int d = st::sp_column(st::lattice_class(u, lab, blank)) | ss::D_LIVE;
      if (st::lattice_skip_from_below(u, lab)) d |= ss::D_SKIP;
      if (u == 1) d |= ss::D_ENTER;
      if (u == 2 * L - 1) { d |= ss::D_END; wt[KPL * 64 + g / KPL] = k; }
      wt[(g % KPL) * 64 + g / KPL] = d;
    }
    int32_t* entry = w + w[ss::H_KW_AT] + 4L * k;
    entry[0] = p.wave[k]; entry[1] = p.first[k]; entry[2] = L; entry[3] = 0;
  }
  *n_waves = p.n_waves;
  return ST_OK;
}

int st_ctc_spot_stream_plan_bind(void* plan, const void* device_copy) {
  int32_t* w = reinterpret_cast<int32_t*>(plan);
  ST_REQUIRE(plan_ok(w, 0), "spot stream plan bind: the plan is not one st_ctc_spot_stream_plan wrote");
  ST_REQUIRE(device_copy && reinterpret_cast<uintptr_t>(device_copy) % 4 == 0, "spot stream plan bind: bad device address");
  const uint64_t a = reinterpret_cast<uintptr_t>(device_copy);
  w[ss::H_DEV_LO] = (int32_t)(uint32_t)a;
  w[ss::H_DEV_HI] = (int32_t)(uint32_t)(a >> 32);
  return ST_OK;
}

size_t st_ctc_spot_stream_state_bytes(const void* plan) {
  const int32_t* w = reinterpret_cast<const int32_t*>(plan);
  if (!plan_ok(w, 0)) return 0;
  return (size_t)w[ss::H_WAVES] * ss::wave_state_bytes(w[ss::H_KPL]);
}

int st_ctc_spot_stream_step(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* table, int n_rows,
                            int max_streams, const void* plan, double threshold, int hold, void* state, int32_t* events,
                            int max_events, int32_t* counts, void* stream) {
  const int32_t* hp = reinterpret_cast<const int32_t*>(plan);
  if (int e = check_step("spot stream step", logits, pitch, num_classes, rows, table, n_rows, max_streams, hp, threshold, hold, state,
                         events, max_events, counts))
    return e;
  const uint64_t dev = (uint64_t)(uint32_t)hp[ss::H_DEV_LO] | ((uint64_t)(uint32_t)hp[ss::H_DEV_HI] << 32);
  ST_REQUIRE(dev != 0, "spot stream step: the plan has no device copy (st_ctc_spot_stream_plan_bind)");
  const int n_waves = hp[ss::H_WAVES];
  const long stream_bytes = (long)n_waves * ss::wave_state_bytes(hp[ss::H_KPL]);
  hipStream_t s = st::as_stream(stream);
  if (hipMemsetAsync(counts, 0, (size_t)max_streams * sizeof(int32_t), s) != hipSuccess) return st::check_launch("spot stream clear");
  st::trace("ctc_spot_stream<%d> streams=%d waves=%d rows=%d", hp[ss::H_KPL], max_streams, n_waves, n_rows);
  st::dispatch_kpl(hp[ss::H_KPL], [&](auto k) {
    hipLaunchKernelGGL(spot_stream_kernel<k()>, dim3((unsigned)(max_streams * n_waves)), dim3(64), 0, s, logits, pitch, num_classes,
                       rows, table, reinterpret_cast<const int*>(dev), n_waves, threshold, hold, state, stream_bytes, events,
                       max_events, counts);
  });
  return st::check_launch("ctc_spot_stream");
}

int st_ctc_spot_stream_host(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* table, int n_rows,
                            int max_streams, const void* plan, double threshold, int hold, void* state, int32_t* events,
                            int max_events, int32_t* counts) {
  const int32_t* hp = reinterpret_cast<const int32_t*>(plan);
  if (int e = check_step("spot stream host", logits, pitch, num_classes, rows, table, n_rows, max_streams, hp, threshold, hold, state,
                         events, max_events, counts))
    return e;
  const int C = num_classes, KPL = hp[ss::H_KPL], n_waves = hp[ss::H_WAVES], n_keywords = hp[ss::H_KEYWORDS];
  const long stream_bytes = (long)n_waves * ss::wave_state_bytes(KPL);
  std::vector<double> d;
  std::vector<int> lab(511), col(1024);
  std::vector<char> skip(1024);
  for (int s = 0; s < max_streams; ++s) {
    counts[s] = 0;
    const int first = table[4 * s], count = table[4 * s + 1], limit = table[4 * s + 2], reset = table[4 * s + 3];
    if (count <= 0 && limit < 0 && !reset) continue;
    const int f0 = count > 0 ? rows[2 * (long)first + 1] : 0;
    const int n = ss::rows_taken(count, limit, f0);
    if (reset) {
      for (int w = 0; w < n_waves; ++w) {
        const ss::StateView rec = ss::state_view(state, stream_bytes, s, w, KPL);
        for (int i = 0; i < KPL * 64; ++i) { rec.v[i] = ST_SP_NEG_INF; rec.s[i] = -1; }
        for (int l = 0; l < 64; ++l) {
          ss::Pending p;
          ss::init(p);
          rec.pscore[l] = p.score; rec.pstart[l] = p.start; rec.pend[l] = p.end; rec.last[l] = p.last_end;
        }
      }
    }
    d.resize((size_t)n * CP);
    for (int i = 0; i < n; ++i) {
      const float* x = logits + ((long)first + i) * pitch;
      float m = NEG_INF_F;
      for (int c = 0; c < C; ++c) m = fmaxf(m, x[c]);
      for (int c = 0; c < CP; ++c) d[(size_t)i * CP + c] = c < C ? st::sp_ratio(x[c], m) : ST_SP_NEG_INF;
    }
    int32_t* ev = events + (long)s * max_events * ss::kEventWords;
    // keyword by keyword, each on its own 2L+1 states: what lies beside them in the wave is never looked at
    for (int k = 0; k < n_keywords; ++k) {
      const int32_t* entry = hp + hp[ss::H_KW_AT] + 4L * k;
      const int w = entry[0], g0 = entry[1], L = entry[2];
      const int32_t* wt = hp + ss::kHeaderWords + (long)w * ss::wave_words(KPL);
      const ss::StateView rec = ss::state_view(state, stream_bytes, s, w, KPL);
      auto at = [&](int u) { const int g = g0 + u; return (g % KPL) * 64 + g / KPL; };
      for (int i = 0; i < L; ++i) lab[i] = wt[at(2 * i + 1)] & ss::D_COL;
      for (int u = 0; u <= 2 * L; ++u) {
        const bool lv = u >= 1 && u <= 2 * L - 1;
        col[u] = st::sp_column(lv ? st::lattice_class(u, lab.data(), C - 1) : C - 1);
        skip[u] = lv && st::lattice_skip_from_below(u, lab.data());
      }
      const int u_end = 2 * L - 1, lane_end = (g0 + u_end) / KPL;
      ss::Pending p{rec.pscore[lane_end], rec.pstart[lane_end], rec.pend[lane_end], rec.last[lane_end]};
      for (int i = 0; i < n; ++i) {
        const int t = f0 + i;
        const double* row = d.data() + (size_t)i * CP;
        for (int u = 2 * L; u >= 0; --u) {                    // downwards: the states below still hold frame t - 1
          double nv;
          int ns;
          st::sp_cell(rec.v[at(u)], rec.s[at(u)], u >= 1 ? rec.v[at(u - 1)] : ST_SP_NEG_INF, u >= 1 ? rec.s[at(u - 1)] : -1,
                      u >= 2 ? rec.v[at(u - 2)] : ST_SP_NEG_INF, u >= 2 ? rec.s[at(u - 2)] : -1, skip[u] != 0, u == 1,
                      u >= 1 && u <= u_end, t, row[col[u]], nv, ns);
          rec.v[at(u)] = nv;
          rec.s[at(u)] = ns;
        }
        ss::Hit h;
        if (ss::rule(rec.v[at(u_end)], rec.s[at(u_end)], t, threshold, hold, p, h)) ss::write_event(ev, max_events, counts[s]++, k, h, 0);
      }
      if (limit >= 0 && p.end > 0) {
        ss::write_event(ev, max_events, counts[s]++, k, ss::Hit{p.score, p.start, p.end}, 1);
        p.last_end = p.end;
        ss::clear(p);
      }
      rec.pscore[lane_end] = p.score; rec.pstart[lane_end] = p.start; rec.pend[lane_end] = p.end; rec.last[lane_end] = p.last_end;
    }
  }
  return ST_OK;
}

}  // extern "C"
