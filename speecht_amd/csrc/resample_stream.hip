// "kaiser_best" resampling of live streams on gfx950: the samples of st_resample_kaiser_f32 on the whole signal, bit for bit,
// however the audio was cut into steps.  The arithmetic is resample_map.h's (st::rs_output_src: the body the offline kernel
// runs), only where sample n -/+ k is read from differs.
//
// The rule (audio_io.resample_ready restates it): with L = RS_NWIN / index_step, the most taps a wing can have, output i of a
// stream that has received N source samples is final iff int(i / ratio) + 1 + L <= N -- wing 1 then has count == limit whatever
// arrives later, and wing 0 depends only on the past.  Once m outputs are out the first source sample still needed is
// max(int(m / ratio) - L, 0).  At most 2 L + 1 samples are therefore retained between steps, whatever the size of the feeds.
//
// State: per stream TWO windows of cap samples, used in turn (the table row says which one is current).  A step reads the
// retained samples from the current window and the new ones straight from `samples`; it writes what the stream retains after the
// step to the OTHER window.  No workgroup writes what another one of the launch reads, so one launch needs no ordering between
// its workgroups, and nothing is moved in place.
//
// resample_stream_kernel: grid (tiles + 1, max_streams).  Workgroup (x, s) with x < the tiles of stream s computes 256
//   consecutive outputs: it stages the tile's source span -- [int(a / ratio) - L, int((b - 1) / ratio) + L + 1] for the outputs
//   [a, b), at most ceil(256 / ratio) + 2 L + 2 samples -- in LDS once, and one thread per output walks its two wings against
//   LDS.  The float64 window table stays in global memory and is read through the cache as in the offline kernel (neighbouring
//   lanes read neighbouring entries of one 4 KiB band).  The last workgroup of a row (x == gridDim.x - 1) writes the stream's
//   next window and its status.  Every workgroup checks the row first (st::rss_check, the host form runs the same code): a row
//   that breaks a bound gets its status and nothing else, and no read leaves the windows whatever the row says.
#include "st_common.h"
#include "resample_map.h"

namespace st {

constexpr int RSS_ROW = 16;                          // int64 words per table row
enum { RSS_RATE, RSS_BASE0, RSS_BASE1, RSS_N0, RSS_SRC, RSS_NEW, RSS_OUT0, RSS_COUNT, RSS_OUT_OFF, RSS_FIN, RSS_N_ORIG, RSS_VALID,
       RSS_TARGET, RSS_PARITY };
enum { RSS_OK, RSS_BAD_ROW, RSS_WINDOW, RSS_BEFORE_BASE, RSS_NOT_READY, RSS_OUT_FULL, RSS_SPAN };
constexpr int RSS_TILE = 256;
constexpr int64_t RSS_MAX_COUNT = (int64_t)1 << 53;  // (double)i is exact below
constexpr int64_t RSS_LDS_BYTES = 65536;

struct RssRow {
  RsParams p;
  bool equal;                                        // source rate == target rate: a copy
  int64_t taps;                                      // L
  int64_t base0, base1, n0, n1, src, out0, count, out_off, valid;   // valid: outputs >= valid are zeros (finished streams)
  int parity;
};

ST_RS_HD int64_t rss_source_index(const RssRow& r, int64_t i) {
  return r.equal ? i : (int64_t)((double)i / r.p.ratio);
}

ST_RS_HD int64_t rss_need(const RssRow& r, int64_t m) {
  const int64_t a = rss_source_index(r, m) - r.taps;
  return a > 0 ? a : 0;
}

// floats of LDS a tile of this ratio needs; > RSS_LDS_BYTES / 4: the stream cannot be served
ST_RS_HD int64_t rss_span(const RssRow& r) {
  const double per = (double)RSS_TILE / r.p.ratio;
  int64_t c = (int64_t)per;
  if ((double)c < per) ++c;
  return c + 2 * r.taps + 2;
}

// The row of an active stream (rate != 0) -> RssRow, or the status that refuses it.
ST_RS_HD int rss_check(const int64_t* t, int sr_new, int64_t cap, int64_t out_capacity, RssRow* r) {
  const int64_t rate = t[RSS_RATE];
  if (rate <= 0 || rate >= ((int64_t)1 << 31)) return RSS_BAD_ROW;
  for (int f = RSS_BASE0; f <= RSS_OUT_OFF; ++f)
    if (t[f] < 0 || t[f] >= RSS_MAX_COUNT) return RSS_BAD_ROW;
  if ((t[RSS_FIN] | 1) != 1 || (t[RSS_PARITY] | 1) != 1) return RSS_BAD_ROW;
  r->p = rs_params((int)rate, sr_new);
  r->equal = rate == sr_new;
  if (!r->equal && r->p.index_step < 1) return RSS_SPAN;
  r->taps = r->equal ? 0 : RS_NWIN / r->p.index_step;
  if (rss_span(*r) * 4 > RSS_LDS_BYTES) return RSS_SPAN;
  r->base0 = t[RSS_BASE0], r->base1 = t[RSS_BASE1], r->n0 = t[RSS_N0], r->n1 = t[RSS_N0] + t[RSS_NEW], r->src = t[RSS_SRC];
  r->out0 = t[RSS_OUT0], r->count = t[RSS_COUNT], r->out_off = t[RSS_OUT_OFF], r->parity = (int)t[RSS_PARITY];
  if (r->base0 > r->n0 || r->n0 - r->base0 > cap || r->base1 < r->base0 || r->base1 > r->n1 || r->n1 - r->base1 > cap) return RSS_WINDOW;
  if (r->out_off + r->count > out_capacity) return RSS_OUT_FULL;
  const int64_t m1 = r->out0 + r->count;
  if (t[RSS_FIN]) {
    const int64_t valid = t[RSS_VALID], target = t[RSS_TARGET];
    if (t[RSS_N_ORIG] != r->n1 || valid < 0 || valid > target || m1 > target) return RSS_NOT_READY;
    if (valid > 0 && rss_source_index(*r, valid - 1) >= r->n1) return RSS_NOT_READY;
    r->valid = valid;
  } else {
    if (r->count > 0 && rss_source_index(*r, m1 - 1) + 1 + r->taps > r->n1) return RSS_NOT_READY;
    if (r->base1 > rss_need(*r, m1)) return RSS_BEFORE_BASE;   // the next step would need what this one drops
    r->valid = m1;
  }
  if (r->count > 0 && r->out0 < r->valid && rss_need(*r, r->out0) < r->base0) return RSS_BEFORE_BASE;
  return RSS_OK;
}

// sample `a` (absolute) of the stream during the step: the current window, then the new samples; 0 outside [base0, n1)
struct RssSource {
  const float* window;                               // the current window: position 0 is sample base0
  const float* fresh;                                // the step's new samples: position 0 is sample n0
  int64_t base0, n0, n1;
  ST_RS_HD float operator()(int64_t a) const {
    if (a < base0 || a >= n1) return 0.0f;
    return a < n0 ? window[a - base0] : fresh[a - n0];
  }
};

ST_RS_HD RssSource rss_source(const RssRow& r, const float* samples, const float* windows, int s, int64_t cap) {
  return RssSource{windows + ((int64_t)s * 2 + r.parity) * cap, samples + r.src, r.base0, r.n0, r.n1};
}

}  // namespace st

namespace {

struct LdsSpan {                                     // the tile's staged source span: position 0 is sample lo
  const float* at;
  int64_t lo;
  __device__ __forceinline__ float operator()(int64_t a) const { return at[a - lo]; }
};

__global__ __launch_bounds__(st::RSS_TILE) void resample_stream_kernel(const float* __restrict__ samples, const int64_t* __restrict__ table,
                                                                      int sr_new, const double* __restrict__ win,
                                                                      float* __restrict__ windows, int64_t cap, int lds_floats,
                                                                      float* __restrict__ out, int64_t out_capacity,
                                                                      int32_t* __restrict__ status) {
  extern __shared__ float span[];
  const int s = blockIdx.y;
  const int64_t* t = table + (int64_t)s * st::RSS_ROW;
  const bool last = blockIdx.x == gridDim.x - 1;
  if (t[st::RSS_RATE] == 0) {                        // the stream sits this step out
    if (last && threadIdx.x == 0) status[s] = st::RSS_OK;
    return;
  }
  st::RssRow r;
  const int code = st::rss_check(t, sr_new, cap, out_capacity, &r);
  if (code != st::RSS_OK) {
    if (last && threadIdx.x == 0) status[s] = code;
    return;
  }
  const st::RssSource source = st::rss_source(r, samples, windows, s, cap);
  if (last) {                                        // what the stream retains goes to its other window
    float* next = windows + ((int64_t)s * 2 + (r.parity ^ 1)) * cap;
    const int64_t keep = r.n1 - r.base1;             // <= cap (rss_check)
    for (int64_t j = threadIdx.x; j < keep; j += st::RSS_TILE) next[j] = source(r.base1 + j);
    if (threadIdx.x == 0) status[s] = st::RSS_OK;
    return;
  }
  const int64_t a = r.out0 + (int64_t)blockIdx.x * st::RSS_TILE;
  const int64_t m1 = r.out0 + r.count;
  if (a >= m1) return;
  const int64_t b = a + st::RSS_TILE < m1 ? a + st::RSS_TILE : m1;
  const int64_t i = a + threadIdx.x;
  float* o = out + r.out_off + (i - r.out0);
  if (r.equal) {
    if (i < b) *o = i < r.valid ? source(i) : 0.0f;
    return;
  }
  const int64_t bv = b < r.valid ? b : r.valid;      // outputs [a, bv) are interpolated, [bv, b) are zeros
  int64_t lo = 0, len = 0;
  if (a < bv) {
    lo = st::rss_source_index(r, a) - r.taps;
    len = st::rss_source_index(r, bv - 1) + r.taps + 2 - lo;
    if (len > lds_floats) return;                    // (the launch sized the LDS for this ratio: never taken)
    for (int64_t j = threadIdx.x; j < len; j += st::RSS_TILE) span[j] = source(lo + j);
  }
  __syncthreads();
  if (i >= b) return;
  *o = i < bv ? (float)st::rs_output_src(LdsSpan{span, lo}, r.n1, r.p, i, win) : 0.0f;
}

}  // namespace

extern "C" {

// bytes of `state`: the device copy of the step's table, then two windows of cap_samples per stream
size_t st_resample_stream_state_bytes(int max_streams, int cap_samples) {
  if (max_streams < 1 || cap_samples < 1) return 0;
  return (size_t)max_streams * st::RSS_ROW * sizeof(int64_t) + (size_t)max_streams * 2 * (size_t)cap_samples * sizeof(float);
}

int st_resample_stream_f32(const float* samples, const int64_t* table, int max_streams, int sr_new, const double* win, int64_t win_len,
                           void* state, size_t state_bytes, int cap_samples, float* out, int64_t out_capacity, int32_t* status,
                           void* stream) {
  ST_REQUIRE(max_streams > 0 && sr_new > 0 && cap_samples > 0 && out_capacity >= 0,
             "st_resample_stream_f32: bad sizes (max_streams %d, sr_new %d, cap_samples %d)", max_streams, sr_new, cap_samples);
  ST_REQUIRE(samples && table && win && state && out && status, "st_resample_stream_f32: null argument");
  ST_REQUIRE(win_len == st::RS_NWIN, "st_resample_stream_f32: the kaiser_best table has %lld entries, got %lld",
             (long long)st::RS_NWIN, (long long)win_len);
  ST_REQUIRE(state_bytes >= st_resample_stream_state_bytes(max_streams, cap_samples),
             "st_resample_stream_f32: state of %zu bytes, %zu needed", state_bytes, st_resample_stream_state_bytes(max_streams, cap_samples));
  // the table is the host's: the launch is sized from it -- the LDS from the smallest ratio, the grid from the most tiles
  int64_t lds_floats = 1, tiles = 0;
  for (int s = 0; s < max_streams; ++s) {
    const int64_t* t = table + (int64_t)s * st::RSS_ROW;
    const int64_t rate = t[st::RSS_RATE];
    if (rate == 0) continue;
    if (rate < 0 || rate >= ((int64_t)1 << 31) || t[st::RSS_COUNT] < 0 || t[st::RSS_COUNT] > out_capacity) continue;   // refused by its status
    st::RssRow r;
    r.p = st::rs_params((int)rate, sr_new);
    r.equal = rate == sr_new;
    ST_REQUIRE(r.equal || r.p.index_step >= 1, "st_resample_stream_f32: stream %d: %lld -> %d Hz is outside the filter table", s,
               (long long)rate, sr_new);
    r.taps = r.equal ? 0 : st::RS_NWIN / r.p.index_step;
    const int64_t need = st::rss_span(r);
    ST_REQUIRE(need * 4 <= st::RSS_LDS_BYTES, "st_resample_stream_f32: stream %d: a tile of %lld -> %d Hz spans %lld samples, more than the LDS holds",
               s, (long long)rate, sr_new, (long long)need);
    if (need > lds_floats) lds_floats = need;
    const int64_t n = (t[st::RSS_COUNT] + st::RSS_TILE - 1) / st::RSS_TILE;
    if (n > tiles) tiles = n;
  }
  ST_REQUIRE(tiles < 65535, "st_resample_stream_f32: %lld tiles in one step", (long long)tiles);
  hipStream_t q = st::as_stream(stream);
  const size_t table_bytes = (size_t)max_streams * st::RSS_ROW * sizeof(int64_t);
  if (hipMemcpyAsync(state, table, table_bytes, hipMemcpyHostToDevice, q) != hipSuccess) return st::check_launch("st_resample_stream_f32: table copy");
  float* windows = reinterpret_cast<float*>(static_cast<char*>(state) + table_bytes);
  if (st::trace_on()) st::trace("resample_stream streams=%d tiles=%lld lds=%lld", max_streams, (long long)tiles, (long long)lds_floats);
  const dim3 grid((unsigned)tiles + 1, (unsigned)max_streams), block(st::RSS_TILE);
  const unsigned lds_bytes = (unsigned)(lds_floats * sizeof(float));
  st::LaunchTimer timer(q);
  if (timer.active())
    hipExtLaunchKernelGGL(resample_stream_kernel, grid, block, lds_bytes, q, timer.start(), timer.stop(), 0, samples,
                          static_cast<const int64_t*>(state), sr_new, win, windows, (int64_t)cap_samples, (int)lds_floats, out, out_capacity,
                          status);
  else
    hipLaunchKernelGGL(resample_stream_kernel, grid, block, lds_bytes, q, samples, static_cast<const int64_t*>(state), sr_new, win, windows,
                       (int64_t)cap_samples, (int)lds_floats, out, out_capacity, status);
  return st::check_launch("resample_stream_kernel");
}

// The same step on host pointers (state included), with the float64 sums beside the float32 samples: out64 compares with
// st_resample_kaiser_host.  No GPU.
int st_resample_stream_host(const float* samples, const int64_t* table, int max_streams, int sr_new, const double* win, int64_t win_len,
                            void* state, size_t state_bytes, int cap_samples, float* out, double* out64, int64_t out_capacity,
                            int32_t* status) {
  ST_REQUIRE(max_streams > 0 && sr_new > 0 && cap_samples > 0 && out_capacity >= 0,
             "st_resample_stream_host: bad sizes (max_streams %d, sr_new %d, cap_samples %d)", max_streams, sr_new, cap_samples);
  ST_REQUIRE(samples && table && win && state && out && out64 && status, "st_resample_stream_host: null argument");
  ST_REQUIRE(win_len == st::RS_NWIN, "st_resample_stream_host: the kaiser_best table has %lld entries, got %lld",
             (long long)st::RS_NWIN, (long long)win_len);
  ST_REQUIRE(state_bytes >= st_resample_stream_state_bytes(max_streams, cap_samples),
             "st_resample_stream_host: state of %zu bytes, %zu needed", state_bytes, st_resample_stream_state_bytes(max_streams, cap_samples));
  const int64_t cap = cap_samples;
  float* windows = reinterpret_cast<float*>(static_cast<char*>(state) + (size_t)max_streams * st::RSS_ROW * sizeof(int64_t));
  for (int s = 0; s < max_streams; ++s) {
    const int64_t* t = table + (int64_t)s * st::RSS_ROW;
    status[s] = st::RSS_OK;
    if (t[st::RSS_RATE] == 0) continue;
    st::RssRow r;
    status[s] = st::rss_check(t, sr_new, cap, out_capacity, &r);
    if (status[s] != st::RSS_OK) continue;
    const st::RssSource source = st::rss_source(r, samples, windows, s, cap);
    for (int64_t k = 0; k < r.count; ++k) {
      const int64_t i = r.out0 + k;
      double v = 0.0;
      if (i < r.valid) v = r.equal ? (double)source(i) : st::rs_output_src(source, r.n1, r.p, i, win);
      out64[r.out_off + k] = v;
      out[r.out_off + k] = (float)v;
    }
    float* next = windows + ((int64_t)s * 2 + (r.parity ^ 1)) * cap;
    for (int64_t j = 0; j < r.n1 - r.base1; ++j) next[j] = source(r.base1 + j);
  }
  return ST_OK;
}

}  // extern "C"
