// Waveform augmentation of a training batch (st_wave_augment_f32, st_wave_augment_host, st_wave_augment_plan_host): every
// utterance resampled by its drawn speed and, when it drew noise, mixed with a clip of the noise bank at its drawn SNR.  What is
// drawn and how it is applied: csrc/wave_augment_core.h, shared with the host form.
//
// Two launches over utterances stored one after the other (offsets in samples).
// (a) wave_speed_kernel: a workgroup owns WA_GROUP tiles of 256 outputs of one utterance.  It puts the phase table of the
//     utterance's speed (rows WA_ROW = 65 floats apart: the 64 lanes' phases then sit on different banks) and the source span of its
//     outputs into LDS, then every lane forms one output per tile: 2H fmaf from LDS.  Lane windows start at most two samples apart,
//     so a window read is conflict-free up to the speed 1/1 and two-way above it.  Of a noisy utterance it also writes each tile's
//     two sums of squares (doubles, the fixed tree).  An utterance at 1/1 without noise is copied, 16 bytes per lane where the two
//     sides' alignment allows.
// (b) wave_mix_kernel, noisy utterances only: a workgroup owns WB_SPAN outputs; it adds the utterance's tile sums in tile order
//     (from LDS, one lane per sum: the same value in every workgroup), forms the gain and mixes in place.
// The plan comes from device memory, so the kernels trust none of it: speed and clip indices, lengths and offsets are clamped to
// what the offsets tables and the caller's totals allow before anything is addressed.
#include "wave_augment_core.h"
#include "st_common.h"

namespace {

using st::WavePlan;

constexpr int WA_THREADS = 256;
constexpr int WA_GROUP = 4;                                    // tiles per workgroup of (a)
constexpr int WA_OUTS = WA_GROUP * st::WA_TILE;
constexpr int WA_SPAN = 2 * WA_OUTS + st::WA_MAX_TAPS + 8;     // source samples of WA_OUTS outputs at the speed 2/1, and slack
constexpr int WA_ROW = st::WA_MAX_TAPS + 1;
constexpr int WB_SPAN = 4096;                                  // outputs per workgroup of (b)
constexpr int WB_CHUNK = 1024;                                 // tile sums folded per pass through LDS
constexpr int64_t WA_MAX_LEN = 0x7fffffff;

struct WaveSpeeds {
  int n;
  int num[st::WA_MAX_SPEEDS], den[st::WA_MAX_SPEEDS], table[st::WA_MAX_SPEEDS];      // table: float offset into `tables`
};

struct WaveBatch {
  const float* in;
  const int64_t* in_offsets;
  int64_t in_total;
  const WavePlan* plan;
  const float* tables;
  const float* noise;
  const int64_t* clip_offsets;
  int n_clips;
  float* out;
  const int64_t* out_offsets;
  int64_t out_total, max_out;
  double* sums;                                                // [n_utts][max_tiles][2]
  int64_t max_tiles;
};

// one utterance as the kernels address it
struct Utt {
  const float* x;
  float* y;
  const float* clip;
  int64_t n, M, offset;
  uint32_t len;
  int num, den, table;
  bool noisy;
  double lin;
};

__host__ __device__ inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ Utt utterance(const WaveBatch& b, const WaveSpeeds& sp, int u) {
  Utt t;
  const int64_t i0 = clamp64(b.in_offsets[u], 0, b.in_total), i1 = clamp64(b.in_offsets[u + 1], i0, b.in_total);
  const int64_t o0 = clamp64(b.out_offsets[u], 0, b.out_total), o1 = clamp64(b.out_offsets[u + 1], o0, b.out_total);
  const WavePlan p = b.plan[u];
  t.x = b.in + i0;
  t.n = i1 - i0;
  t.y = b.out + o0;
  t.M = clamp64(p.M, 0, o1 - o0 < b.max_out ? o1 - o0 : b.max_out);
  const bool listed = p.speed >= 0 && p.speed < sp.n;
  t.num = listed ? sp.num[p.speed] : 1;
  t.den = listed ? sp.den[p.speed] : 1;
  t.table = listed ? sp.table[p.speed] : 0;
  t.noisy = false;
  t.clip = nullptr;
  t.len = 1;
  t.offset = 0;
  t.lin = p.lin;
  if (p.noisy && b.n_clips > 0 && b.sums) {
    const int k = p.clip < 0 ? 0 : (p.clip >= b.n_clips ? b.n_clips - 1 : p.clip);
    const int64_t c0 = b.clip_offsets[k], len = b.clip_offsets[k + 1] - c0;
    if (c0 >= 0 && len >= 1 && len <= WA_MAX_LEN) {
      t.noisy = true;
      t.clip = b.noise + c0;
      t.len = (uint32_t)len;
      t.offset = p.offset >= 0 && p.offset < len ? p.offset : 0;
    }
  }
  return t;
}

__global__ __launch_bounds__(WA_THREADS) void wave_speed_kernel(WaveBatch b, WaveSpeeds sp) {
#pragma clang fp contract(off)
  __shared__ float tab[st::WA_MAX_TERM * WA_ROW];
  __shared__ float xs[WA_SPAN];
  __shared__ double red[2][st::WA_TILE];
  const int u = blockIdx.y, tid = threadIdx.x;
  const Utt t = utterance(b, sp, u);
  const int64_t m0 = (int64_t)blockIdx.x * WA_OUTS;
  if (m0 >= t.M) return;
  const int cnt = (int)(t.M - m0 < WA_OUTS ? t.M - m0 : WA_OUTS);
  float v[WA_GROUP];
  if (t.num == t.den) {
    if (!t.noisy) {                                            // the copy
      const float* x = t.x + m0;
      float* y = t.y + m0;
      const int64_t have = t.n - m0 < 0 ? 0 : t.n - m0;         // (M = n in every plan the host makes; a longer M reads zeros)
      const int full = (int)(have < cnt ? have : cnt);
      if (aligned16(x) && aligned16(y)) {
        for (int q = tid; q < (full >> 2); q += WA_THREADS) reinterpret_cast<float4*>(y)[q] = reinterpret_cast<const float4*>(x)[q];
        for (int r = (full & ~3) + tid; r < cnt; r += WA_THREADS) y[r] = r < full ? x[r] : 0.f;
      } else {
        for (int r = tid; r < cnt; r += WA_THREADS) y[r] = r < full ? x[r] : 0.f;
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < WA_GROUP; ++j) {
      const int64_t m = m0 + j * st::WA_TILE + tid;
      v[j] = m < t.M && m < t.n ? t.x[m] : 0.f;
    }
  } else {
    const int H = st::wa_half_width(t.num, t.den), taps = 2 * H;
    for (int idx = tid; idx < t.den * taps; idx += WA_THREADS) {
      const int row = idx / taps;
      tab[row * WA_ROW + idx - row * taps] = b.tables[t.table + idx];
    }
    // output m0 + r sits at source q0 + (r0 + r num) / den: one 64-bit division per workgroup, 32-bit ones per lane
    const int64_t t0 = m0 * t.num, q0 = t0 / t.den;
    const int r0 = (int)(t0 - q0 * t.den);
    const int span = (r0 + (cnt - 1) * t.num) / t.den + taps;   // <= 2 WA_OUTS + 64
    const int64_t first = q0 - H + 1;
    for (int k = tid; k < span; k += WA_THREADS) {
      const int64_t s = first + k;
      xs[k] = s >= 0 && s < t.n ? t.x[s] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < WA_GROUP; ++j) {
      const int r = j * st::WA_TILE + tid;
      v[j] = 0.f;
      if (r < cnt) {
        const int pos = r0 + r * t.num, i = pos / t.den, phi = pos - i * t.den;
        v[j] = st::wa_taps(tab + phi * WA_ROW, xs + i, taps);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < WA_GROUP; ++j) {
    const int r = j * st::WA_TILE + tid;
    if (r < cnt) t.y[m0 + r] = v[j];
  }
  if (!t.noisy) return;
  const uint32_t base = (uint32_t)((uint64_t)(t.offset + m0) % t.len);
  for (int j = 0; j < WA_GROUP && j * st::WA_TILE < cnt; ++j) {
    const int r = j * st::WA_TILE + tid;
    const int64_t tile = m0 / st::WA_TILE + j;
    red[0][tid] = r < cnt ? st::wa_square(v[j]) : 0.0;
    red[1][tid] = r < cnt ? st::wa_square(t.clip[st::wa_wrap(base + (uint32_t)r, t.len)]) : 0.0;
    __syncthreads();
    if (tid < 64) {                                            // the tree's steps 128 and 64 from LDS, 32 .. 1 across the wave
      double s = (red[0][tid] + red[0][tid + 128]) + (red[0][tid + 64] + red[0][tid + 192]);
      double z = (red[1][tid] + red[1][tid + 128]) + (red[1][tid + 64] + red[1][tid + 192]);
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        s = s + __shfl_xor(s, o, 64);
        z = z + __shfl_xor(z, o, 64);
      }
      if (tid == 0 && tile < b.max_tiles) {
        double* d = b.sums + ((int64_t)u * b.max_tiles + tile) * 2;
        d[0] = s;
        d[1] = z;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(WA_THREADS) void wave_mix_kernel(WaveBatch b, WaveSpeeds sp) {
#pragma clang fp contract(off)
  __shared__ double part[2 * WB_CHUNK];
  __shared__ double total[2];
  __shared__ float gain;
  const int u = blockIdx.y, tid = threadIdx.x;
  const Utt t = utterance(b, sp, u);
  const int64_t m0 = (int64_t)blockIdx.x * WB_SPAN;
  if (!t.noisy || m0 >= t.M) return;
  int64_t tiles = (t.M + st::WA_TILE - 1) / st::WA_TILE;
  if (tiles > b.max_tiles) tiles = b.max_tiles;
  const double* sums = b.sums + (int64_t)u * b.max_tiles * 2;
  double acc = 0.0;                                            // lane 0: S(y); lane 64: S(z)
  for (int64_t c = 0; c < tiles; c += WB_CHUNK) {
    const int here = (int)(tiles - c < WB_CHUNK ? tiles - c : WB_CHUNK);
    __syncthreads();
    for (int i = tid; i < 2 * here; i += WA_THREADS) part[i] = sums[2 * c + i];
    __syncthreads();
    if (tid == 0 || tid == 64) acc = st::wa_fold_tiles(acc, part + (tid == 64), here, 2);
  }
  if (tid == 0) total[0] = acc;
  if (tid == 64) total[1] = acc;
  __syncthreads();
  if (tid == 0) gain = (float)st::wa_gain(total[0], total[1], t.M, t.lin);
  __syncthreads();
  const float a = gain;
  if (a == 0.f) return;                                        // nothing is mixed: the bits of (a) stay
  const int cnt = (int)(t.M - m0 < WB_SPAN ? t.M - m0 : WB_SPAN);
  const uint32_t base = (uint32_t)((uint64_t)(t.offset + m0) % t.len);
  float* y = t.y + m0;
  int done = 0;
  if (aligned16(y)) {
    for (int q = tid; q < (cnt >> 2); q += WA_THREADS) {
      float4 w = reinterpret_cast<float4*>(y)[q];
      const uint32_t r = base + 4u * (uint32_t)q;
      w.x = st::wa_mix(a, t.clip[st::wa_wrap(r, t.len)], w.x);
      w.y = st::wa_mix(a, t.clip[st::wa_wrap(r + 1, t.len)], w.y);
      w.z = st::wa_mix(a, t.clip[st::wa_wrap(r + 2, t.len)], w.z);
      w.w = st::wa_mix(a, t.clip[st::wa_wrap(r + 3, t.len)], w.w);
      reinterpret_cast<float4*>(y)[q] = w;
    }
    done = cnt & ~3;
  }
  for (int r = done + tid; r < cnt; r += WA_THREADS) y[r] = st::wa_mix(a, t.clip[st::wa_wrap(base + (uint32_t)r, t.len)], y[r]);
}

int check_speeds(const char* who, const int32_t* speeds, int n_speeds, WaveSpeeds* out) {
  ST_REQUIRE(speeds && n_speeds >= 1 && n_speeds <= st::WA_MAX_SPEEDS, "%s: %d speeds (1 .. %d), or none given", who, n_speeds,
             st::WA_MAX_SPEEDS);
  out->n = n_speeds;
  int at = 0;
  for (int s = 0; s < n_speeds; ++s) {
    const int num = speeds[2 * s], den = speeds[2 * s + 1];
    ST_REQUIRE(st::wa_speed_ok(num, den), "%s: speed %d/%d is not a reduced fraction of terms 1 .. %d between 1/2 and 2", who, num, den,
               st::WA_MAX_TERM);
    out->num[s] = num;
    out->den[s] = den;
    out->table[s] = at;
    at += st::wa_table_floats(num, den);
  }
  return ST_OK;
}

}  // namespace

extern "C" {

int st_wave_augment_plan_host(const int64_t* lengths, const int64_t* draw_ids, int n_utts, uint64_t seed, const int32_t* speeds,
                              int n_speeds, int noise_prob_q16, int snr_lo_centi, int snr_hi_centi, const int64_t* clip_lens,
                              int n_clips, int64_t min_samples, void* plan_out) {
  ST_REQUIRE(lengths && draw_ids && plan_out && n_utts >= 1, "st_wave_augment_plan_host: null argument or %d utterances", n_utts);
  WaveSpeeds sp;
  int rc = check_speeds("st_wave_augment_plan_host", speeds, n_speeds, &sp);
  if (rc != ST_OK) return rc;
  ST_REQUIRE(noise_prob_q16 >= 0 && noise_prob_q16 <= 65536, "st_wave_augment_plan_host: noise probability %d / 65536 lies outside 0 .. 1",
             noise_prob_q16);
  ST_REQUIRE(snr_lo_centi <= snr_hi_centi && snr_lo_centi >= -10000 && snr_hi_centi <= 10000,
             "st_wave_augment_plan_host: SNR range %d .. %d hundredths of a dB (ordered, within -100 .. 100 dB)", snr_lo_centi, snr_hi_centi);
  ST_REQUIRE(n_clips >= 0 && (n_clips == 0 || clip_lens), "st_wave_augment_plan_host: %d clips, or no lengths", n_clips);
  ST_REQUIRE(n_clips > 0 || noise_prob_q16 == 0, "st_wave_augment_plan_host: a noise probability without a noise bank");
  for (int k = 0; k < n_clips; ++k)
    ST_REQUIRE(clip_lens[k] >= 1 && clip_lens[k] <= WA_MAX_LEN, "st_wave_augment_plan_host: clip %d has %lld samples", k, (long long)clip_lens[k]);
  st::WavePolicy pol;
  pol.n_speeds = n_speeds;
  for (int s = 0; s < n_speeds; ++s) { pol.num[s] = sp.num[s]; pol.den[s] = sp.den[s]; }
  pol.noise_prob_q16 = noise_prob_q16;
  pol.snr_lo = snr_lo_centi;
  pol.snr_hi = snr_hi_centi;
  WavePlan* plans = static_cast<WavePlan*>(plan_out);
  for (int u = 0; u < n_utts; ++u) {
    ST_REQUIRE(lengths[u] >= 0 && lengths[u] <= WA_MAX_LEN / 2, "st_wave_augment_plan_host: utterance %d has %lld samples (0 .. 2^30 - 1)", u,
               (long long)lengths[u]);
    plans[u] = st::wa_plan(pol, seed, (uint64_t)draw_ids[u], lengths[u], clip_lens, n_clips, min_samples);
  }
  return ST_OK;
}

size_t st_wave_augment_ws(int n_utts, int64_t max_out) {
  if (n_utts < 1 || max_out < 1) return 0;
  return (size_t)n_utts * (size_t)((max_out + st::WA_TILE - 1) / st::WA_TILE) * 2 * sizeof(double);
}

int st_wave_augment_f32(const float* in, const int64_t* in_offsets, int n_utts, int64_t in_total, const void* plan,
                        const int32_t* speeds, int n_speeds, const float* tables, const float* noise, const int64_t* clip_offsets,
                        int n_clips, float* out, const int64_t* out_offsets, int64_t out_total, int64_t max_out, void* workspace,
                        size_t workspace_bytes, void* stream) {
  ST_REQUIRE(in && in_offsets && plan && tables && out && out_offsets, "st_wave_augment_f32: null argument");
  ST_REQUIRE(n_utts >= 1 && n_utts <= 65535, "st_wave_augment_f32: %d utterances (1 .. 65535)", n_utts);
  ST_REQUIRE(in_total >= 0 && out_total >= 0 && max_out >= 0 && max_out <= WA_MAX_LEN && max_out <= out_total,
             "st_wave_augment_f32: bad totals (in %lld, out %lld, longest output %lld)", (long long)in_total, (long long)out_total,
             (long long)max_out);
  ST_REQUIRE(((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(tables) |
               reinterpret_cast<uintptr_t>(noise)) & 3) == 0 &&
                 ((reinterpret_cast<uintptr_t>(in_offsets) | reinterpret_cast<uintptr_t>(out_offsets) | reinterpret_cast<uintptr_t>(plan) |
                   reinterpret_cast<uintptr_t>(clip_offsets) | reinterpret_cast<uintptr_t>(workspace)) & 7) == 0,
             "st_wave_augment_f32: unaligned argument");
  WaveSpeeds sp;
  int rc = check_speeds("st_wave_augment_f32", speeds, n_speeds, &sp);
  if (rc != ST_OK) return rc;
  ST_REQUIRE(n_clips >= 0 && (n_clips == 0 || (noise && clip_offsets)), "st_wave_augment_f32: %d clips, or no bank", n_clips);
  ST_REQUIRE(n_clips == 0 || (workspace && workspace_bytes >= st_wave_augment_ws(n_utts, max_out)),
             "st_wave_augment_f32: workspace of %zu bytes, %zu needed", workspace_bytes, st_wave_augment_ws(n_utts, max_out));
  if (max_out == 0) return ST_OK;
  WaveBatch b;
  b.in = in; b.in_offsets = in_offsets; b.in_total = in_total;
  b.plan = static_cast<const WavePlan*>(plan);
  b.tables = tables;
  b.noise = noise; b.clip_offsets = clip_offsets; b.n_clips = n_clips;
  b.out = out; b.out_offsets = out_offsets; b.out_total = out_total; b.max_out = max_out;
  b.sums = n_clips > 0 ? static_cast<double*>(workspace) : nullptr;
  b.max_tiles = (max_out + st::WA_TILE - 1) / st::WA_TILE;
  hipStream_t s = st::as_stream(stream);
  const dim3 grid_a((unsigned)((max_out + WA_OUTS - 1) / WA_OUTS), n_utts), grid_b((unsigned)((max_out + WB_SPAN - 1) / WB_SPAN), n_utts);
  if (st::trace_on()) st::trace("wave_speed utts=%d longest=%lld speeds=%d clips=%d blocks=%u", n_utts, (long long)max_out, n_speeds, n_clips, grid_a.x * grid_a.y);
  {
    st::LaunchTimer timer(s);
    st::launch_timed(timer, wave_speed_kernel, grid_a, dim3(WA_THREADS), s, b, sp);
  }
  rc = st::check_launch("wave_speed_kernel");
  if (rc != ST_OK || n_clips == 0) return rc;
  if (st::trace_on()) st::trace("wave_mix utts=%d longest=%lld blocks=%u", n_utts, (long long)max_out, grid_b.x * grid_b.y);
  st::LaunchTimer timer(s);
  st::launch_timed(timer, wave_mix_kernel, grid_b, dim3(WA_THREADS), s, b, sp);
  return st::check_launch("wave_mix_kernel");
}

int st_wave_augment_host(const float* in, const int64_t* in_offsets, int n_utts, const void* plan, const int32_t* speeds, int n_speeds,
                         const float* tables, const float* noise, const int64_t* clip_offsets, int n_clips, float* out,
                         const int64_t* out_offsets, double* sums_out) {
#pragma clang fp contract(off)
  ST_REQUIRE(in && in_offsets && plan && tables && out && out_offsets && n_utts >= 1, "st_wave_augment_host: null argument or %d utterances",
             n_utts);
  WaveSpeeds sp;
  int rc = check_speeds("st_wave_augment_host", speeds, n_speeds, &sp);
  if (rc != ST_OK) return rc;
  ST_REQUIRE(n_clips >= 0 && (n_clips == 0 || (noise && clip_offsets)), "st_wave_augment_host: %d clips, or no bank", n_clips);
  for (int k = 0; k < n_clips; ++k)
    ST_REQUIRE(clip_offsets[k] >= 0 && clip_offsets[k + 1] > clip_offsets[k] && clip_offsets[k + 1] - clip_offsets[k] <= WA_MAX_LEN,
               "st_wave_augment_host: clip %d spans %lld .. %lld", k, (long long)clip_offsets[k], (long long)clip_offsets[k + 1]);
  const WavePlan* plans = static_cast<const WavePlan*>(plan);
  for (int u = 0; u < n_utts; ++u) {
    const WavePlan& p = plans[u];
    const int64_t n = in_offsets[u + 1] - in_offsets[u], cap = out_offsets[u + 1] - out_offsets[u];
    ST_REQUIRE(in_offsets[u] >= 0 && out_offsets[u] >= 0 && n >= 0 && n <= WA_MAX_LEN / 2 && cap >= 0,
               "st_wave_augment_host: utterance %d has bad offsets", u);
    ST_REQUIRE(p.speed >= -1 && p.speed < n_speeds, "st_wave_augment_host: utterance %d plans speed %d of %d", u, p.speed, n_speeds);
    const int num = p.speed < 0 ? 1 : sp.num[p.speed], den = p.speed < 0 ? 1 : sp.den[p.speed];
    ST_REQUIRE(p.M == st::wa_out_len(n, num, den) && p.M <= cap, "st_wave_augment_host: utterance %d plans %lld outputs of %lld samples at %d/%d, room for %lld",
               u, (long long)p.M, (long long)n, num, den, (long long)cap);
    ST_REQUIRE(!p.noisy || (p.clip >= 0 && p.clip < n_clips && p.offset >= 0 && p.offset < clip_offsets[p.clip + 1] - clip_offsets[p.clip] &&
                            p.lin > 0.0),
               "st_wave_augment_host: utterance %d plans clip %d of %d from sample %lld", u, p.clip, n_clips, (long long)p.offset);
  }
  for (int u = 0; u < n_utts; ++u) {
    const WavePlan& p = plans[u];
    const float* x = in + in_offsets[u];
    float* y = out + out_offsets[u];
    const int64_t n = in_offsets[u + 1] - in_offsets[u], M = p.M;
    const int num = p.speed < 0 ? 1 : sp.num[p.speed], den = p.speed < 0 ? 1 : sp.den[p.speed];
    if (num == den) {
      for (int64_t m = 0; m < M; ++m) y[m] = x[m];
    } else {
      const int H = st::wa_half_width(num, den), taps = 2 * H;
      const float* table = tables + sp.table[p.speed];
      float win[st::WA_MAX_TAPS];
      for (int64_t m = 0; m < M; ++m) {
        const int64_t pos = m * num, i = pos / den;
        const int phi = (int)(pos - i * den);
        for (int k = 0; k < taps; ++k) {
          const int64_t s = i - H + 1 + k;
          win[k] = s >= 0 && s < n ? x[s] : 0.f;
        }
        y[m] = st::wa_taps(table + phi * taps, win, taps);
      }
    }
    if (sums_out) sums_out[2 * u] = sums_out[2 * u + 1] = 0.0;
    if (!p.noisy || M == 0) continue;
    const float* clip = noise + clip_offsets[p.clip];
    const int64_t len = clip_offsets[p.clip + 1] - clip_offsets[p.clip];
    double ss = 0.0, sz = 0.0, vs[st::WA_TILE], vz[st::WA_TILE];
    for (int64_t m0 = 0; m0 < M; m0 += st::WA_TILE) {
      for (int r = 0; r < st::WA_TILE; ++r) {
        const bool in_range = m0 + r < M;
        vs[r] = in_range ? st::wa_square(y[m0 + r]) : 0.0;
        vz[r] = in_range ? st::wa_square(clip[(p.offset + m0 + r) % len]) : 0.0;
      }
      ss = ss + st::wa_tile_tree(vs);
      sz = sz + st::wa_tile_tree(vz);
    }
    if (sums_out) { sums_out[2 * u] = ss; sums_out[2 * u + 1] = sz; }
    const float a = (float)st::wa_gain(ss, sz, M, p.lin);
    if (a == 0.f) continue;
    for (int64_t m = 0; m < M; ++m) y[m] = st::wa_mix(a, clip[(p.offset + m) % len], y[m]);
  }
  return ST_OK;
}

}  // extern "C"
