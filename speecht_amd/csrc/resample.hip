// Batched "kaiser_best" resampling on gfx950: what librosa.load does between decoding and the feature extractor
// (preprocessing.py:169) -- resampy's band-limited interpolation (audio_io.resample_kaiser_best) followed by fix_length --
// for a batch of utterances of different lengths and source rates in one launch.
//
// resample_kernel: one thread per output sample, grid-stride over the concatenated outputs.  The thread finds its utterance
//   by binary search over out_offsets, then runs the shared tap selection and weighting of resample_map.h (the host form
//   st_resample_kaiser_host runs the same code): two wings of <= 64 taps (up-sampling) or <= 64 / ratio taps (down-sampling),
//   float64 throughout, float32 written.  Outputs past the resampled length up to the fix_length target are zeros; an
//   utterance already at the target rate is copied bit for bit.
// Memory: the float64 window (256 KiB) does not fit the LDS; it is read through the cache.  Neighbouring lanes are neighbouring
//   outputs, so at tap k a wave reads 64 entries of one 512-entry (4 KiB) band of the table and source samples within ~100
//   of one another -- the whole wave walks the table band by band, which keeps its working set inside the 32 KiB L1.
#include "st_common.h"
#include "resample_map.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_MAX_BLOCKS = 8192;                  // 32 per CU; the rest by grid stride

__device__ __forceinline__ int find_utt(const int64_t* out_offsets, int n_utts, int64_t i) {
  int lo = 0, hi = n_utts - 1;                       // largest u with out_offsets[u] <= i
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (out_offsets[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ in, const int64_t* __restrict__ in_offsets,
                                                              int n_utts, const int32_t* __restrict__ rates, int sr_new,
                                                              const int64_t* __restrict__ out_offsets,
                                                              const int64_t* __restrict__ out_valid, int64_t total_out,
                                                              const double* __restrict__ win, float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * RS_THREADS;
  for (int64_t g = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; g < total_out; g += stride) {
    const int u = find_utt(out_offsets, n_utts, g);
    const int64_t i = g - out_offsets[u];
    const int64_t src0 = in_offsets[u], n_orig = in_offsets[u + 1] - src0;
    const int sr = rates[u];
    float v = 0.0f;
    if (sr == sr_new) {
      if (i < n_orig) v = in[src0 + i];
    } else if (i < out_valid[u]) {
      v = (float)st::rs_output(in + src0, n_orig, st::rs_params(sr, sr_new), i, win);
    }
    out[g] = v;
  }
}

}  // namespace

extern "C" {

int st_resample_kaiser_f32(const float* in, const int64_t* in_offsets, int n_utts, const int32_t* rates, int sr_new,
                           const int64_t* out_offsets, const int64_t* out_valid, int64_t total_out, const double* win,
                           int64_t win_len, float* out, void* stream) {
  ST_REQUIRE(n_utts > 0 && sr_new > 0 && total_out >= 0, "st_resample_kaiser_f32: bad sizes (n_utts %d, sr_new %d)", n_utts, sr_new);
  ST_REQUIRE(in && in_offsets && rates && out_offsets && out_valid && win && (out || total_out == 0),
             "st_resample_kaiser_f32: null argument");
  ST_REQUIRE(win_len == st::RS_NWIN, "st_resample_kaiser_f32: the kaiser_best table has %lld entries, got %lld",
             (long long)st::RS_NWIN, (long long)win_len);
  if (total_out == 0) return ST_OK;
  const int64_t blocks64 = (total_out + RS_THREADS - 1) / RS_THREADS;
  const int blocks = (int)(blocks64 < RS_MAX_BLOCKS ? blocks64 : RS_MAX_BLOCKS);
  hipStream_t s = st::as_stream(stream);
  if (st::trace_on()) st::trace("resample_kaiser utts=%d out=%lld blocks=%d", n_utts, (long long)total_out, blocks);
  st::LaunchTimer timer(s);
  st::launch_timed(timer, resample_kernel, dim3(blocks), dim3(RS_THREADS), s, in, in_offsets, n_utts, rates, sr_new, out_offsets,
                   out_valid, total_out, win, out);
  return st::check_launch("resample_kernel");
}

// The same computation on the host, float64 out: host pointers, the code of resample_map.h (tests reach it without a GPU)
int st_resample_kaiser_host(const float* in, const int64_t* in_offsets, int n_utts, const int32_t* rates, int sr_new,
                            const int64_t* out_offsets, const int64_t* out_valid, const double* win, int64_t win_len, double* out) {
  ST_REQUIRE(n_utts > 0 && sr_new > 0, "st_resample_kaiser_host: bad sizes (n_utts %d, sr_new %d)", n_utts, sr_new);
  ST_REQUIRE(in_offsets && rates && out_offsets && out_valid && win, "st_resample_kaiser_host: null argument");
  ST_REQUIRE(win_len == st::RS_NWIN, "st_resample_kaiser_host: the kaiser_best table has %lld entries, got %lld",
             (long long)st::RS_NWIN, (long long)win_len);
  for (int u = 0; u < n_utts; ++u) {
    const int64_t n_orig = in_offsets[u + 1] - in_offsets[u], n_out = out_offsets[u + 1] - out_offsets[u];
    ST_REQUIRE(n_orig >= 0 && n_out >= 0 && out_valid[u] >= 0 && out_valid[u] <= n_out && rates[u] > 0,
               "st_resample_kaiser_host: bad offsets or rate of utterance %d", u);
    const float* y = in + in_offsets[u];
    double* o = out + out_offsets[u];
    const st::RsParams p = st::rs_params(rates[u], sr_new);
    for (int64_t i = 0; i < n_out; ++i) {
      if (rates[u] == sr_new) o[i] = i < n_orig ? (double)y[i] : 0.0;
      else o[i] = i < out_valid[u] ? st::rs_output(y, n_orig, p, i, win) : 0.0;
    }
  }
  return ST_OK;
}

}  // extern "C"
