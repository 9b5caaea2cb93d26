// Silence segmentation of recordings on gfx950: cut a batch of mono signals into utterances by the rules of
// include/speecht_hip.h ("Silence segmentation"; the numpy specification is tests/segment_oracle.py) and gather the
// utterances, peak-normalised and padded, into the layout the resampler and the feature kernels read.  Also the row mask
// of the padded batches (st_mask_rows).
//
// Layout of the chunk tables: signal i owns the groups [group_offsets[i], group_offsets[i + 1]) of 64 chunks each, so chunk k
// of signal i is entry 64 * group_offsets[i] + k of chunk_peak / chunk_first / chunk_last and bit k % 64 of word
// group_offsets[i] + k / 64 of chunk_mask; bits of chunks past the signal's last are zero.
//
// seg_peak_kernel    one wave per group: max |x| of its samples, folded into the signal's peak with an integer max on the bits
//                    of the non-negative float (order-independent, so the result is the same in every run).
// seg_chunk_kernel   one wave per group: the group's samples (one contiguous range) in aligned 16-byte loads, lane after lane;
//                    peak, first and last active sample of each chunk are folded in LDS; lane k then writes chunk k and the
//                    ballot of the active lanes is the group's mask word.
// seg_runs_kernel    one wave per signal: a chunk starts a run when no chunk of the G before it is active, and ends one when
//                    none of the G after it is -- local tests, so lane k of the wave decides them for chunk k of a mask word and
//                    two ballots bring the starts and ends of 64 chunks at once; the wave walks those bits in order.  A run
//                    longer than M chunks is cut at the quietest chunk of the window (argmin across the lanes, smallest index on
//                    ties).  Rows are written by lane 0 in time order; a signal has at most one segment per active chunk.
// seg_gather_kernel  one thread per output sample (grid stride): pad zeros, the segment's samples times 0.5 / peak, pad zeros.
// mask_rows_kernel   16-byte zero stores over the rows t >= valid[b] of batch row b; a workgroup without such a row exits at once.
//
// Every result is written with ordinary vector stores.  No kernel waits for another workgroup.
#include "st_common.h"

#include <limits.h>

namespace {

constexpr int SEG_THREADS = 256;                       // four waves, one group each
constexpr int SEG_WAVES = SEG_THREADS / 64;
constexpr int GATHER_THREADS = 256;
constexpr int GATHER_MAX_BLOCKS = 8192;
constexpr int MASK_THREADS = 256;
constexpr int MASK_BLOCK_BYTES = 32768;                // what one workgroup of mask_rows_kernel zeroes at most (whole rows)

// largest i with table[i] <= v, table ascending with table[0] <= v
__device__ __forceinline__ int find_le(const int64_t* table, int n, int64_t v) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid] <= v) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// what a wave needs to know about its group
struct Group {
  int signal;
  int chunk;                 // samples per chunk
  int chunks;                // chunks of this group (1..64)
  int64_t first;             // absolute index of the group's first sample
  int64_t end;               // ... and one past its last
};

__device__ __forceinline__ Group group_of(const int64_t* offsets, const int32_t* rates, const int64_t* group_offsets, int n_signals,
                                          int64_t g) {
  Group r;
  r.signal = find_le(group_offsets, n_signals, g);
  // (an empty signal owns no group: find_le returns the LAST signal whose first group is <= g, which is the owner)
  const int64_t s0 = offsets[r.signal], n = offsets[r.signal + 1] - s0;
  const int rate50 = rates[r.signal] / 50;
  r.chunk = rate50 > 1 ? rate50 : 1;
  const int64_t total_chunks = (n + r.chunk - 1) / r.chunk;
  const int64_t k0 = (g - group_offsets[r.signal]) * 64;
  const int64_t left = total_chunks - k0;
  r.chunks = (int)(left < 64 ? left : 64);
  r.first = s0 + k0 * r.chunk;
  const int64_t e = r.first + (int64_t)r.chunks * r.chunk;
  r.end = e < s0 + n ? e : s0 + n;
  return r;
}

// the four floats at 4 * v of `audio` (16-byte aligned base); entries at or past `total` read as zero and are never used
__device__ __forceinline__ float4 load4(const float* audio, int64_t v, int64_t total) {
  if (4 * v + 3 < total) return reinterpret_cast<const float4*>(audio)[v];
  float4 r = {0.f, 0.f, 0.f, 0.f};
  if (4 * v < total) r.x = audio[4 * v];
  if (4 * v + 1 < total) r.y = audio[4 * v + 1];
  if (4 * v + 2 < total) r.z = audio[4 * v + 2];
  return r;
}

__global__ __launch_bounds__(SEG_THREADS) void seg_peak_kernel(const float* __restrict__ audio, const int64_t* __restrict__ offsets,
                                                               const int32_t* __restrict__ rates,
                                                               const int64_t* __restrict__ group_offsets, int n_signals,
                                                               int64_t total_groups, unsigned* __restrict__ peak_bits) {
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * SEG_WAVES + (threadIdx.x >> 6);
  if (g >= total_groups) return;
  const Group gr = group_of(offsets, rates, group_offsets, n_signals, g);
  const int64_t total = offsets[n_signals];
  float m = 0.f;
  for (int64_t v = (gr.first >> 2) + lane; 4 * v < gr.end; v += 64) {
    const float4 x = load4(audio, v, total);
    const float e[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t p = 4 * v + j;
      if (p >= gr.first && p < gr.end) m = fmaxf(m, fabsf(e[j]));
    }
  }
  m = st::wave_max(m);
  if (lane == 0 && m > 0.f) atomicMax(peak_bits + gr.signal, __float_as_uint(m));
}

__global__ __launch_bounds__(SEG_THREADS) void seg_chunk_kernel(const float* __restrict__ audio, const int64_t* __restrict__ offsets,
                                                                const int32_t* __restrict__ rates,
                                                                const int64_t* __restrict__ group_offsets, int n_signals,
                                                                int64_t total_groups, float threshold2, const float* __restrict__ peaks,
                                                                float* __restrict__ chunk_peak, int32_t* __restrict__ chunk_first,
                                                                int32_t* __restrict__ chunk_last,
                                                                unsigned long long* __restrict__ chunk_mask) {
  __shared__ unsigned s_peak[SEG_WAVES][64];
  __shared__ int s_first[SEG_WAVES][64];
  __shared__ int s_last[SEG_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t g = (int64_t)blockIdx.x * SEG_WAVES + wave;
  const bool live = g < total_groups;                  // (a wave without a group still meets the barriers)
  s_peak[wave][lane] = 0u;
  s_first[wave][lane] = INT_MAX;
  s_last[wave][lane] = -1;
  __syncthreads();
  Group gr = {};
  if (live) {
    gr = group_of(offsets, rates, group_offsets, n_signals, g);
    const int64_t total = offsets[n_signals];
    const float thr = __fmul_rn(threshold2, peaks[gr.signal]);
    for (int64_t v = (gr.first >> 2) + lane; 4 * v < gr.end; v += 64) {
      const float4 x = load4(audio, v, total);
      const float e[4] = {x.x, x.y, x.z, x.w};
      // chunk and offset inside it of the first of the four samples that belongs to the group; the others count on from there
      const int64_t p0 = 4 * v > gr.first ? 4 * v : gr.first;
      const int rel = (int)(p0 - gr.first);
      int k = rel / gr.chunk, off = rel - k * gr.chunk;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t p = 4 * v + j;
        if (p < p0 || p >= gr.end) continue;
        const float a = fabsf(e[j]);
        atomicMax(&s_peak[wave][k], __float_as_uint(a));
        if (a > thr) {
          atomicMin(&s_first[wave][k], off);
          atomicMax(&s_last[wave][k], off);
        }
        if (++off == gr.chunk) {
          off = 0;
          ++k;
        }
      }
    }
  }
  __syncthreads();
  if (!live) return;
  const bool mine = lane < gr.chunks;
  const bool active = mine && s_last[wave][lane] >= 0;
  if (mine) {
    chunk_peak[g * 64 + lane] = __uint_as_float(s_peak[wave][lane]);
    chunk_first[g * 64 + lane] = active ? s_first[wave][lane] : -1;
    chunk_last[g * 64 + lane] = s_last[wave][lane];
  }
  const unsigned long long word = __ballot(active);
  if (lane == 0) chunk_mask[g] = word;
}

// ---- runs and cuts: one wave per signal; everything below is wave-uniform unless it says "lane" --------------------------------

// any active chunk in [lo, hi] (clamped to the signal's words)?  per lane
__device__ __forceinline__ bool any_active(const unsigned long long* words, int64_t n_chunks, int64_t lo, int64_t hi) {
  if (lo < 0) lo = 0;
  if (hi > n_chunks - 1) hi = n_chunks - 1;
  if (lo > hi) return false;
  for (int64_t w = lo >> 6; w <= (hi >> 6); ++w) {
    unsigned long long m = words[w];
    if (w == (lo >> 6)) m &= ~0ull << (lo & 63);
    if (w == (hi >> 6)) m &= ~0ull >> (63 - (hi & 63));
    if (m) return true;
  }
  return false;
}

// first active chunk >= p (the caller knows there is one)
__device__ __forceinline__ int64_t next_active(const unsigned long long* words, int64_t p) {
  int64_t w = p >> 6;
  unsigned long long m = words[w] & (~0ull << (p & 63));
  while (!m) m = words[++w];
  return w * 64 + (__ffsll((long long)m) - 1);
}

// last active chunk <= p (the caller knows there is one)
__device__ __forceinline__ int64_t prev_active(const unsigned long long* words, int64_t p) {
  int64_t w = p >> 6;
  unsigned long long m = words[w] & (~0ull >> (63 - (p & 63)));
  while (!m) m = words[--w];
  return w * 64 + (63 - __clzll((long long)m));
}

__device__ __forceinline__ float peak_over(const float* peak, int64_t lo, int64_t hi, int lane) {       // max over chunks [lo, hi]
  float m = 0.f;
  for (int64_t k = lo + lane; k <= hi; k += 64) m = fmaxf(m, peak[k]);
  return st::wave_max(m);
}

// the quietest chunk of [lo, hi): smallest peak, smallest index among equals
__device__ __forceinline__ int64_t quietest(const float* peak, int64_t lo, int64_t hi, int lane) {
  float best = INFINITY;
  int64_t at = LLONG_MAX;
  for (int64_t k = lo + lane; k < hi; k += 64) {
    const float v = peak[k];
    if (v < best) {                                    // (a lane's indices ascend: strict keeps its earliest)
      best = v;
      at = k;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int64_t oa = __shfl_xor(at, o, 64);
    if (ov < best || (ov == best && oa < at)) {
      best = ov;
      at = oa;
    }
  }
  return at;
}

__global__ __launch_bounds__(64) void seg_runs_kernel(const int64_t* __restrict__ offsets, const int32_t* __restrict__ rates,
                                                      const int64_t* __restrict__ group_offsets, int gap_chunks, int max_chunks,
                                                      const float* __restrict__ chunk_peak, const int32_t* __restrict__ chunk_first,
                                                      const int32_t* __restrict__ chunk_last,
                                                      const unsigned long long* __restrict__ chunk_mask,
                                                      int64_t* __restrict__ seg_ranges, float* __restrict__ seg_peaks,
                                                      int32_t* __restrict__ seg_counts) {
  const int sig = blockIdx.x, lane = threadIdx.x;
  const int64_t n = offsets[sig + 1] - offsets[sig];
  const int rate50 = rates[sig] / 50;
  const int64_t c = rate50 > 1 ? rate50 : 1;
  const int64_t n_chunks = (n + c - 1) / c;
  const int64_t n_words = group_offsets[sig + 1] - group_offsets[sig];
  const unsigned long long* words = chunk_mask + group_offsets[sig];
  const int64_t base = group_offsets[sig] * 64;
  const float* peak = chunk_peak + base;
  const int32_t* first = chunk_first + base;
  const int32_t* last = chunk_last + base;
  const int64_t G = gap_chunks, M = max_chunks;
  int count = 0;

  auto emit = [&](int64_t a, int64_t b) {                // the piece from active chunk a to active chunk b
    const float pk = peak_over(peak, a, b, lane);
    if (lane == 0) {
      int64_t* row = seg_ranges + 2 * (base + count);
      row[0] = a * c + first[a];
      row[1] = b * c + last[b] + 1;
      seg_peaks[base + count] = pk;
    }
    ++count;
  };

  int64_t run_start = -1;
  for (int64_t w = 0; w < n_words; ++w) {
    const unsigned long long word = words[w];
    if (!word) continue;
    const int64_t p = w * 64 + lane;
    const bool active = (word >> lane) & 1;
    const bool is_start = active && !any_active(words, n_chunks, p - G, p - 1);
    const bool is_end = active && !any_active(words, n_chunks, p + 1, p + G);
    unsigned long long starts = __ballot(is_start), ends = __ballot(is_end);
    while (starts | ends) {
      const int bs = starts ? __ffsll((long long)starts) - 1 : 64;
      const int be = ends ? __ffsll((long long)ends) - 1 : 64;
      if (bs <= be) {                                    // (a run of one chunk starts and ends on the same bit: the start first)
        run_start = w * 64 + bs;
        starts &= starts - 1;
        continue;
      }
      ends &= ends - 1;
      const int64_t run_end = w * 64 + be;
      int64_t a = run_start;
      while (run_end - a + 1 > M) {
        const int64_t j = quietest(peak, a + M / 2, a + M, lane);
        emit(a, prev_active(words, j - 1));
        a = next_active(words, j);
      }
      emit(a, run_end);
    }
  }
  if (lane == 0) seg_counts[sig] = count;
}

__global__ __launch_bounds__(GATHER_THREADS) void seg_gather_kernel(const float* __restrict__ audio, const int64_t* __restrict__ src_start,
                                                                    const float* __restrict__ seg_peaks,
                                                                    const int64_t* __restrict__ out_offsets,
                                                                    const int32_t* __restrict__ pads, int n_segments, int64_t total_out,
                                                                    float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * GATHER_THREADS;
  for (int64_t g = (int64_t)blockIdx.x * GATHER_THREADS + threadIdx.x; g < total_out; g += stride) {
    const int s = find_le(out_offsets, n_segments, g);
    const int64_t pad = pads[s];
    const int64_t i = g - out_offsets[s] - pad;
    const int64_t len = out_offsets[s + 1] - out_offsets[s] - 2 * pad;
    float v = 0.f;
    if (i >= 0 && i < len) v = __fmul_rn(audio[src_start[s] + i], __fdiv_rn(0.5f, seg_peaks[s]));
    out[g] = v;
  }
}

__global__ __launch_bounds__(MASK_THREADS) void mask_rows_kernel(char* __restrict__ base, int frames, int halo, int t_pitch,
                                                                 long row_bytes, int rows_per_block, const int32_t* __restrict__ valid) {
  const int b = blockIdx.y;
  int v = valid[b];
  if (v < 0) v = 0;
  const int r0 = blockIdx.x * rows_per_block;
  const int lo = v > r0 ? v : r0;
  const int hi = r0 + rows_per_block < frames ? r0 + rows_per_block : frames;
  if (lo >= hi) return;                                  // no padding row here
  uint4* p = reinterpret_cast<uint4*>(base + ((long)b * t_pitch + halo + lo) * row_bytes);
  const long units = (long)(hi - lo) * row_bytes / 16;
  const uint4 zero = {0u, 0u, 0u, 0u};
  for (long i = threadIdx.x; i < units; i += MASK_THREADS) p[i] = zero;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int st_segment_chunks_f32(const float* audio, const int64_t* offsets, const int32_t* rates, const int64_t* group_offsets,
                          int n_signals, int64_t total_groups, float threshold2, float* peaks, float* chunk_peak,
                          int32_t* chunk_first, int32_t* chunk_last, uint64_t* chunk_mask, void* stream) {
  ST_REQUIRE(n_signals > 0 && total_groups >= 0 && total_groups < ((int64_t)INT_MAX - SEG_WAVES) * SEG_WAVES,
             "st_segment_chunks_f32: bad sizes (%d signals, %lld groups)", n_signals, (long long)total_groups);
  ST_REQUIRE(offsets && rates && group_offsets && peaks, "st_segment_chunks_f32: null argument");
  ST_REQUIRE(threshold2 >= 0.f, "st_segment_chunks_f32: negative threshold");
  hipStream_t s = st::as_stream(stream);
  hipError_t e = hipMemsetAsync(peaks, 0, sizeof(float) * (size_t)n_signals, s);
  if (e != hipSuccess) {
    st::set_error("st_segment_chunks_f32: %s", hipGetErrorString(e));
    return ST_ELAUNCH;
  }
  if (total_groups == 0) return ST_OK;
  ST_REQUIRE(audio && aligned16(audio) && chunk_peak && chunk_first && chunk_last && chunk_mask,
             "st_segment_chunks_f32: null or unaligned buffer");
  const int blocks = (int)((total_groups + SEG_WAVES - 1) / SEG_WAVES);
  if (st::trace_on()) st::trace("segment_peak signals=%d groups=%lld blocks=%d", n_signals, (long long)total_groups, blocks);
  {
    st::LaunchTimer timer(s);
    st::launch_timed(timer, seg_peak_kernel, dim3(blocks), dim3(SEG_THREADS), s, audio, offsets, rates, group_offsets, n_signals,
                     total_groups, reinterpret_cast<unsigned*>(peaks));
  }
  int rc = st::check_launch("seg_peak_kernel");
  if (rc != ST_OK) return rc;
  if (st::trace_on()) st::trace("segment_chunks signals=%d groups=%lld blocks=%d", n_signals, (long long)total_groups, blocks);
  st::LaunchTimer timer(s);
  st::launch_timed(timer, seg_chunk_kernel, dim3(blocks), dim3(SEG_THREADS), s, audio, offsets, rates, group_offsets, n_signals,
                   total_groups, threshold2, peaks, chunk_peak, chunk_first, chunk_last,
                   reinterpret_cast<unsigned long long*>(chunk_mask));
  return st::check_launch("seg_chunk_kernel");
}

int st_segment_runs(const int64_t* offsets, const int32_t* rates, const int64_t* group_offsets, int n_signals, int gap_chunks,
                    int max_chunks, const float* chunk_peak, const int32_t* chunk_first, const int32_t* chunk_last,
                    const uint64_t* chunk_mask, int64_t* seg_ranges, float* seg_peaks, int32_t* seg_counts, void* stream) {
  ST_REQUIRE(n_signals > 0 && gap_chunks >= 1 && max_chunks >= 2, "st_segment_runs: bad sizes (%d signals, gap %d, max %d chunks)",
             n_signals, gap_chunks, max_chunks);
  ST_REQUIRE(offsets && rates && group_offsets && chunk_peak && chunk_first && chunk_last && chunk_mask && seg_ranges && seg_peaks &&
                 seg_counts && aligned16(seg_ranges), "st_segment_runs: null or unaligned argument");
  hipStream_t s = st::as_stream(stream);
  if (st::trace_on()) st::trace("segment_runs signals=%d gap=%d max=%d", n_signals, gap_chunks, max_chunks);
  st::LaunchTimer timer(s);
  st::launch_timed(timer, seg_runs_kernel, dim3(n_signals), dim3(64), s, offsets, rates, group_offsets, gap_chunks, max_chunks,
                   chunk_peak, chunk_first, chunk_last, reinterpret_cast<const unsigned long long*>(chunk_mask), seg_ranges,
                   seg_peaks, seg_counts);
  return st::check_launch("seg_runs_kernel");
}

int st_segment_gather_f32(const float* audio, const int64_t* src_start, const float* seg_peaks, const int64_t* out_offsets,
                          const int32_t* pads, int n_segments, int64_t total_out, float* out, void* stream) {
  ST_REQUIRE(n_segments > 0 && total_out >= 0, "st_segment_gather_f32: bad sizes (%d segments)", n_segments);
  ST_REQUIRE(audio && src_start && seg_peaks && out_offsets && pads && (out || total_out == 0), "st_segment_gather_f32: null argument");
  if (total_out == 0) return ST_OK;
  const int64_t blocks64 = (total_out + GATHER_THREADS - 1) / GATHER_THREADS;
  const int blocks = (int)(blocks64 < GATHER_MAX_BLOCKS ? blocks64 : GATHER_MAX_BLOCKS);
  hipStream_t s = st::as_stream(stream);
  if (st::trace_on()) st::trace("segment_gather segments=%d out=%lld blocks=%d", n_segments, (long long)total_out, blocks);
  st::LaunchTimer timer(s);
  st::launch_timed(timer, seg_gather_kernel, dim3(blocks), dim3(GATHER_THREADS), s, audio, src_start, seg_peaks, out_offsets, pads,
                   n_segments, total_out, out);
  return st::check_launch("seg_gather_kernel");
}

int st_mask_rows(const st_tensor3* t, const int32_t* valid, int elem_bytes, void* stream) {
  ST_REQUIRE(st::tensor_ok(t), "st_mask_rows: bad tensor descriptor");
  ST_REQUIRE(valid && (elem_bytes == 2 || elem_bytes == 4) && aligned16(t->base), "st_mask_rows: null lengths, element size %d or unaligned base",
             elem_bytes);
  ST_REQUIRE(t->batch <= 65535, "st_mask_rows: batch %d exceeds the grid", t->batch);
  const long row_bytes = (long)t->c_pitch * elem_bytes;              // c_pitch % 16 == 0: whole 16-byte units
  int rows = (int)(MASK_BLOCK_BYTES / row_bytes);
  if (rows < 1) rows = 1;
  const int blocks = st::ceil_div(t->frames, rows);
  hipStream_t s = st::as_stream(stream);
  if (st::trace_on()) st::trace("mask_rows batch=%d frames=%d c_pitch=%d elem=%d blocks=%d", t->batch, t->frames, t->c_pitch, elem_bytes, blocks);
  st::LaunchTimer timer(s);
  st::launch_timed(timer, mask_rows_kernel, dim3(blocks, t->batch), dim3(MASK_THREADS), s, reinterpret_cast<char*>(t->base), t->frames,
                   t->halo, t->t_pitch, row_bytes, rows, valid);
  return st::check_launch("mask_rows_kernel");
}

}  // extern "C"
