// Streaming recognition on gfx950: one step of the Wav2Letter forward pass for many open streams at once, state carried
// between steps (speecht_amd/streaming.py drives it; index arithmetic in stream_map.h).
//
// State layout.  Every layer keeps, per stream, a LINEAR WINDOW of recent input frames, [max_streams][cap][c_pitch] floats
// with the engine's padded channel pitch, so that the packed filters packed[k_pad][n_pad] are read in place (no second copy
// of the weights).  Window position 0 of stream s holds the absolute input frame base_s = retain_from(e_s) of that layer;
// the producing layer's epilogue appends new frames behind the retained ones, and after the step st_stream_advance moves
// the still needed tail to the front (one launch for all layers).  The operand of output frame j is then the contiguous run
// of width * c_pitch floats that starts at window position j * stride - pad_left - base_s, exactly what the batch kernels
// read (conv_gemm.hip); frames outside [0, n_s) -- the SAME padding, never stored -- are predicated to zero.
//
// Who counts.  The per-stream counters (frames received n, frames emitted e, window base) are pure functions of how many
// frames were fed, so the HOST keeps them (streaming.plan) and uploads one small table per step: per layer and stream
// {base, n, base after the step}, and per layer the row table (stream, absolute output frame).  Only the decoder's state
// depends on data; it lives on the device (st_ctc_greedy_stream).
//
// Fixed reduction order.  st_stream_conv_f32 is a skinny product: tens of rows against reductions of up to 8 192 and 2 048
// output columns, bound by reading the weights once per step.  Row tiles of 32 run on v_mfma_f32_32x32x2_f32 (bitwise an
// fmaf chain over k); the reduction is cut into slices of a FIXED number of k-tiles per layer (stream_slices: a function of
// the layer's shape only, never of the rows in the launch), the partial tiles go to workspace slabs, and
// stream_epilogue_kernel sums the slabs in slice order before bias and ReLU.  No hand-off between workgroups, no float
// atomics.  A row's result therefore depends on its own operand alone: a stream's logits are bit-identical however its audio
// was cut into chunks and whatever the other streams were doing.
//
// The tile stage of conv_gemm.hip (LDS-DMA, XOR swizzle) is NOT reused: its DMA cannot predicate single frames, and a row
// here may begin in the left padding.  The stage below loads through registers (float4, predicated per frame) into one LDS
// tile with the next tile's loads in flight under the MFMAs.
#include <algorithm>

#include "st_common.h"
#include "stream_map.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BK = 32;           // reduction depth of one LDS stage
constexpr int BM = 128;          // rows per workgroup: 4 waves x one 32-row MFMA tile
constexpr int AP = BK + 4;       // LDS pitch of the operand rows (16-byte aligned, rows spread over the banks)
constexpr int NTHREADS = 256;

struct ConvParams {
  const float* win; int cap, cp;             // input windows [streams][cap][cp]
  const int* info;                           // [streams][4]: {base, n, base after the step, -}
  const int* rows; int n_rows;               // [n_rows][2]: (stream, absolute output frame)
  int max_streams;
  const float* packed; int Kp, Np;           // packed filters [Kp][Np]
  int width, stride, pad_left;
  int kt_per_slice, slices;
  float* slab;                               // [slices][n_rows][Np]
};

// slab[slice][row][n0 ...] = A[row, k-range of the slice] * packed[k-range, n0 ...].  grid (Np / BN, ceil(rows / 128), slices)
template <int NT>
__global__ __launch_bounds__(NTHREADS) void stream_conv_kernel(ConvParams p) {
  constexpr int BN = 32 * NT, BP = BN + 4;
  constexpr int B_LD = BK * BN / 4 / NTHREADS;         // float4 loads of the filter tile per thread (1 or 2)
  static_assert(B_LD >= 1, "tile config");
  __shared__ __attribute__((aligned(16))) float As[BM * AP];
  __shared__ __attribute__((aligned(16))) float Bs[BK * BP];
  __shared__ long r_off[BM];      // float offset of the row's first tap in the windows (may point before the stream's window)
  __shared__ int r_lo[BM], r_hi[BM];   // taps [r_lo, r_hi) of the row read stored frames; the others are padding

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
  const int kt0 = blockIdx.z * p.kt_per_slice;
  const int kt1 = min(kt0 + p.kt_per_slice, p.Kp / BK);

  if (tid < BM) {
    const int m = m0 + tid;
    long off = 0;
    int lo = 0, hi = 0;
    if (m < p.n_rows) {
      const int s = p.rows[2 * m], j = p.rows[2 * m + 1];
      if (s >= 0 && s < p.max_streams) {
        const int base = p.info[4 * s], n = p.info[4 * s + 1];
        const long first = (long)j * p.stride - p.pad_left;           // absolute frame of tap 0
        // tap w reads absolute frame first + w: stored when 0 <= first + w < n and base <= first + w < base + cap
        const long a = std::max<long>(std::max<long>(0, base) - first, 0);
        const long b = std::min<long>(std::min<long>(n, (long)base + p.cap) - first, p.width);
        lo = (int)std::min<long>(a, p.width);
        hi = (int)std::max<long>(b, lo);
        off = ((long)s * p.cap + (first - base)) * p.cp;
      }
    }
    r_off[tid] = off;
    r_lo[tid] = lo;
    r_hi[tid] = hi;
  }
  __syncthreads();

  // operand loads: float4 `i` of this thread is row (tid + 256 i) / 8, slot (tid + 256 i) % 8 of the k-tile
  const float* a_src[4];
  int a_w[4], a_c[4], a_lo[4], a_hi[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = tid + NTHREADS * i, row = idx >> 3, slot = idx & 7;
    const int k = kt0 * BK + slot * 4;
    a_w[i] = k / p.cp;
    a_c[i] = k - a_w[i] * p.cp;
    a_src[i] = p.win + r_off[row];
    a_lo[i] = r_lo[row];
    a_hi[i] = r_hi[row];
  }
  const float* b_src[B_LD];
#pragma unroll
  for (int i = 0; i < B_LD; ++i) {
    const int idx = tid + NTHREADS * i, row = idx / (BN / 4), c4 = idx % (BN / 4);
    b_src[i] = p.packed + (long)(kt0 * BK + row) * p.Np + n0 + c4 * 4;
  }

  f32x4 a_reg[4], b_reg[B_LD];
  auto load_tile = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (a_w[i] >= a_lo[i] && a_w[i] < a_hi[i]) v = *reinterpret_cast<const f32x4*>(a_src[i] + (long)a_w[i] * p.cp + a_c[i]);
      a_reg[i] = v;
      a_c[i] += BK;                                   // the next k-tile (c_pitch >= 16: at most two frames further)
      if (a_c[i] >= p.cp) { a_c[i] -= p.cp; ++a_w[i]; }
      if (a_c[i] >= p.cp) { a_c[i] -= p.cp; ++a_w[i]; }
    }
#pragma unroll
    for (int i = 0; i < B_LD; ++i) {
      b_reg[i] = *reinterpret_cast<const f32x4*>(b_src[i]);
      b_src[i] += (long)BK * p.Np;
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + NTHREADS * i, row = idx >> 3, slot = idx & 7;
      *reinterpret_cast<f32x4*>(As + row * AP + slot * 4) = a_reg[i];
    }
#pragma unroll
    for (int i = 0; i < B_LD; ++i) {
      const int idx = tid + NTHREADS * i, row = idx / (BN / 4), c4 = idx % (BN / 4);
      *reinterpret_cast<f32x4*>(Bs + row * BP + c4 * 4) = b_reg[i];
    }
  };

  f32x16 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
  const bool wave_has_rows = m0 + wave * 32 < p.n_rows;      // wave-uniform

  if (kt0 < kt1) load_tile();
  for (int kt = kt0; kt < kt1; ++kt) {
    store_tile();
    __syncthreads();
    if (kt + 1 < kt1) load_tile();                           // in flight under the MFMAs below
    if (wave_has_rows) {
      const float* as = As + (wave * 32 + l31) * AP + 4 * h;
      const float* bs = Bs + (4 * h) * BP + l31;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 af = *reinterpret_cast<const f32x4*>(as + 8 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int n = 0; n < NT; ++n)
            acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j], bs[(8 * q + j) * BP + 32 * n], acc[n], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  if (!wave_has_rows) return;
  float* slab = p.slab + (long)blockIdx.z * p.n_rows * p.Np;
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wave * 32 + (r >> 2) * 8 + h * 4 + (r & 3);
      if (m < p.n_rows) slab[(long)m * p.Np + n0 + 32 * n + l31] = acc[n][r];
    }
}

struct EpiParams {
  const float* slab; int slices, n_rows, Np;
  const float* bias; int cout, relu;
  const int* rows; int max_streams;
  float* out; int out_cap, out_pitch;
  const int* out_info;          // next layer's {base, n, ...} per stream; null: row m of the launch goes to out[m][out_pitch]
};

// out row = relu(bias + slab[0] + slab[1] + ... in slice order); channels [cout, out_pitch) are written as zeros
__global__ __launch_bounds__(256) void stream_epilogue_kernel(EpiParams p) {
  const int quads = p.out_pitch / 4;
  const long total = (long)p.n_rows * quads;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int m = (int)(idx / quads), c4 = (int)(idx % quads) * 4;
    long pos;
    if (p.out_info) {
      const int s = p.rows[2 * m], j = p.rows[2 * m + 1];
      if (s < 0 || s >= p.max_streams) continue;
      const int at = j - p.out_info[4 * s];                         // position in the next layer's window
      if (at < 0 || at >= p.out_cap) continue;
      pos = (long)s * p.out_cap + at;
    } else {
      if (m >= p.out_cap) continue;
      pos = m;
    }
    const float* src = p.slab + (long)m * p.Np + c4;
    f32x4 v = *reinterpret_cast<const f32x4*>(src);
    for (int s = 1; s < p.slices; ++s) v += *reinterpret_cast<const f32x4*>(src + (long)s * p.n_rows * p.Np);
    v += *reinterpret_cast<const f32x4*>(p.bias + c4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (p.relu) v[e] = fmaxf(v[e], 0.f);
      if (c4 + e >= p.cout) v[e] = 0.f;
    }
    *reinterpret_cast<f32x4*>(p.out + pos * p.out_pitch + c4) = v;
  }
}

// slices of the reduction and k-tiles per slice: about one workgroup per CU (256) for ONE row block of the wide layers, at
// least four k-tiles per slice.  A function of the layer's shape alone.
void stream_slices(int Kp, int Np, int* kt_per_slice, int* slices) {
  const int nk = Kp / BK;
  const int bn = Np % 64 == 0 ? 64 : 32;
  const int tiles_n = Np / bn;
  int want = std::max(1, std::min(st::ceil_div(256, tiles_n), std::max(1, nk / 4)));
  *kt_per_slice = st::ceil_div(nk, want);
  *slices = st::ceil_div(nk, *kt_per_slice);
}

// ---- feed: rows of new features into the first layer's windows -----------------------------------------------------------
__global__ __launch_bounds__(64) void stream_feed_kernel(const float* __restrict__ feat, int channels, const int* __restrict__ table,
                                                         int max_streams, float* __restrict__ win, int cap, int cp) {
  const int r = blockIdx.x;
  const int s = table[2 * r], at = table[2 * r + 1];
  if (s < 0 || s >= max_streams || at < 0 || at >= cap) return;
  float* dst = win + ((long)s * cap + at) * cp;
  for (int c = threadIdx.x; c < cp; c += 64) dst[c] = c < channels ? feat[(long)r * channels + c] : 0.f;
}

// ---- advance: every layer's retained tail to the front of its window ------------------------------------------------------
struct AdvanceLayer { float* win; int cap, cp; };
// grid (streams, layers).  Frames [new_base, n) move from position new_base - base to position 0.  Source and destination
// may overlap (the destination lies in front): the block copies in ascending chunks of 256 float4, every chunk read whole
// before any of it is written, so a chunk's stores can only land on floats that were read in the same or an earlier chunk.
__global__ __launch_bounds__(256) void stream_advance_kernel(const AdvanceLayer* __restrict__ layers, const int* __restrict__ info,
                                                             int max_streams) {
  const int s = blockIdx.x, l = blockIdx.y;
  const AdvanceLayer L = layers[l];
  const int* in = info + ((long)l * max_streams + s) * 4;
  const int base = in[0], n = in[1], new_base = in[2];
  const int shift = new_base - base, keep = n - new_base;
  if (shift <= 0 || keep <= 0 || shift + keep > L.cap) return;            // uniform per block
  f32x4* w = reinterpret_cast<f32x4*>(L.win + (long)s * L.cap * L.cp);
  const long quads = (long)keep * L.cp / 4, d = (long)shift * L.cp / 4;
  for (long q0 = 0; q0 < quads; q0 += 256) {
    const long q = q0 + threadIdx.x;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (q < quads) v = w[q + d];
    __syncthreads();
    if (q < quads) w[q] = v;
  }
}

// ---- greedy decoding carried across steps --------------------------------------------------------------------------------
// One wave per stream.  table[s] = {first row, rows, decode limit (-1: not known yet), reset}; rows of a stream are adjacent
// in the launch and in frame order.  state[s] = {last argmax id, frames decoded, -, -}; score[s] = running sum of the chosen
// logits (double; reported negated).  First maximum on ties, columns below C only, blank = C - 1, repeats merged.
__global__ __launch_bounds__(64) void ctc_greedy_stream_kernel(const float* __restrict__ logits, int pitch, int C,
                                                               const int* __restrict__ rows, const int* __restrict__ table,
                                                               int* __restrict__ state, double* __restrict__ score,
                                                               int* __restrict__ ids, int max_new, int* __restrict__ new_count,
                                                               float* __restrict__ neg_sum) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const int first = table[4 * s], count = table[4 * s + 1], limit = table[4 * s + 2], reset = table[4 * s + 3];
  int last = reset ? -1 : state[4 * s];
  int decoded = reset ? 0 : state[4 * s + 1];
  double sum = reset ? 0.0 : score[s];
  const int blank = C - 1;
  int out = 0;
  for (int r = first; r < first + count; ++r) {
    const int j = rows[2 * r + 1];
    if (limit >= 0 && j >= limit) break;                       // the last row of an odd-length utterance is not decoded
    float v = lane < C ? logits[(long)r * pitch + lane] : -INFINITY;
    int k = lane < C ? lane : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int ok = __shfl_xor(k, o, 64);
      if (ov > v || (ov == v && ok < k)) { v = ov; k = ok; }
    }
    sum += (double)v;
    if (k != blank && k != last) {
      if (lane == 0 && out < max_new) ids[(long)s * max_new + out] = k;
      ++out;
    }
    last = k;
    ++decoded;
  }
  if (lane == 0) {
    state[4 * s] = last;
    state[4 * s + 1] = decoded;
    score[s] = sum;
    new_count[s] = out;
    neg_sum[s] = (float)-sum;
  }
}

}  // namespace

extern "C" {

int st_stream_conv_slices(int width, int cin_pitch, int cout, int* kt_per_slice, int* slices) {
  ST_REQUIRE(width >= 1 && cin_pitch >= 16 && cin_pitch % 16 == 0 && cout >= 1 && kt_per_slice && slices, "stream conv: bad shape");
  int kv, kp, np;
  if (int e = st_packed_dims(width, cin_pitch, cout, &kv, &kp, &np)) return e;
  stream_slices(kp, np, kt_per_slice, slices);
  return ST_OK;
}

size_t st_stream_conv_ws(int n_rows, int width, int cin_pitch, int cout) {
  int kt, slices;
  if (n_rows <= 0 || st_stream_conv_slices(width, cin_pitch, cout, &kt, &slices) != ST_OK) return 0;
  return (size_t)slices * n_rows * st::npad_of(cout) * sizeof(float);
}

int st_stream_conv_f32(const float* windows, int cap, int cin_pitch, const int32_t* info, const int32_t* rows, int n_rows,
                       int max_streams, const float* packed, const float* bias, int width, int stride, int cout, int relu,
                       float* out, int out_cap, int out_pitch, const int32_t* out_info, void* workspace, size_t workspace_bytes,
                       void* stream) {
  ST_REQUIRE(windows && info && rows && packed && bias && out, "stream conv: null argument");
  ST_REQUIRE(n_rows >= 0 && max_streams >= 1 && cap >= 1 && out_cap >= 1, "stream conv: bad sizes");
  ST_REQUIRE(st::stream_map::pad_left_fixed(width, stride), "stream conv: width %d stride %d has no length-independent left padding",
             width, stride);
  int kt, slices;
  if (int e = st_stream_conv_slices(width, cin_pitch, cout, &kt, &slices)) return e;
  int kv, kp, np;
  st_packed_dims(width, cin_pitch, cout, &kv, &kp, &np);
  ST_REQUIRE(out_pitch % 4 == 0 && out_pitch >= cout && out_pitch <= np, "stream conv: output pitch %d not in [%d, %d]", out_pitch, cout, np);
  if (n_rows == 0) return ST_OK;
  if (!workspace || workspace_bytes < st_stream_conv_ws(n_rows, width, cin_pitch, cout)) {
    st::set_error("stream conv: workspace too small (%zu bytes, %zu needed)", workspace_bytes, st_stream_conv_ws(n_rows, width, cin_pitch, cout));
    return ST_EWORKSPACE;
  }
  hipStream_t s = st::as_stream(stream);
  ConvParams p;
  p.win = windows; p.cap = cap; p.cp = cin_pitch;
  p.info = info; p.rows = rows; p.n_rows = n_rows; p.max_streams = max_streams;
  p.packed = packed; p.Kp = kp; p.Np = np;
  p.width = width; p.stride = stride; p.pad_left = st::stream_map::pad_left(width, stride);
  p.kt_per_slice = kt; p.slices = slices;
  p.slab = reinterpret_cast<float*>(workspace);
  const int bn = np % 64 == 0 ? 64 : 32;
  dim3 grid(np / bn, st::ceil_div(n_rows, BM), slices);
  st::trace("stream_conv<%d> rows=%d Np=%d Kp=%d taps=%d slices=%d kt_per_slice=%d", bn, n_rows, np, kp, width, slices, kt);
  {
    st::LaunchTimer timer(s);
    if (bn == 64) st::launch_timed(timer, stream_conv_kernel<2>, grid, dim3(NTHREADS), s, p);
    else st::launch_timed(timer, stream_conv_kernel<1>, grid, dim3(NTHREADS), s, p);
  }
  if (int e = st::check_launch("stream_conv")) return e;
  EpiParams q;
  q.slab = p.slab; q.slices = slices; q.n_rows = n_rows; q.Np = np;
  q.bias = bias; q.cout = cout; q.relu = relu;
  q.rows = rows; q.max_streams = max_streams;
  q.out = out; q.out_cap = out_cap; q.out_pitch = out_pitch; q.out_info = out_info;
  const long quads = (long)n_rows * (out_pitch / 4);
  hipLaunchKernelGGL(stream_epilogue_kernel, dim3((unsigned)std::min<long>((quads + 255) / 256, 4096)), dim3(256), 0, s, q);
  return st::check_launch("stream_epilogue");
}

int st_stream_feed_f32(const float* features, int channels, const int32_t* table, int n_rows, int max_streams, float* windows,
                       int cap, int cin_pitch, void* stream) {
  ST_REQUIRE(features && table && windows, "stream feed: null argument");
  ST_REQUIRE(channels >= 1 && channels <= cin_pitch && n_rows >= 0 && max_streams >= 1 && cap >= 1, "stream feed: bad sizes");
  if (n_rows == 0) return ST_OK;
  hipLaunchKernelGGL(stream_feed_kernel, dim3(n_rows), dim3(64), 0, st::as_stream(stream), features, channels, table, max_streams,
                     windows, cap, cin_pitch);
  return st::check_launch("stream_feed");
}

int st_stream_advance(const void* layer_table, int n_layers, const int32_t* info, int max_streams, void* stream) {
  ST_REQUIRE(layer_table && info && n_layers >= 1 && max_streams >= 1, "stream advance: bad argument");
  static_assert(sizeof(AdvanceLayer) == 16, "layer table entry: {pointer, int32 cap, int32 c_pitch}");
  hipLaunchKernelGGL(stream_advance_kernel, dim3(max_streams, n_layers), dim3(256), 0, st::as_stream(stream),
                     reinterpret_cast<const AdvanceLayer*>(layer_table), info, max_streams);
  return st::check_launch("stream_advance");
}

int st_ctc_greedy_stream(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* table, int max_streams,
                         int32_t* state, double* score, int32_t* ids, int max_new, int32_t* new_count, float* neg_sum_logits,
                         void* stream) {
  ST_REQUIRE(logits && rows && table && state && score && ids && new_count && neg_sum_logits, "greedy stream: null argument");
  ST_REQUIRE(num_classes >= 2 && num_classes <= 64 && pitch >= num_classes && max_streams >= 1 && max_new >= 1,
             "greedy stream: 2..64 classes, pitch >= classes");
  hipLaunchKernelGGL(ctc_greedy_stream_kernel, dim3(max_streams), dim3(64), 0, st::as_stream(stream), logits, pitch, num_classes, rows,
                     table, state, score, ids, max_new, new_count, neg_sum_logits);
  return st::check_launch("ctc_greedy_stream");
}

}  // extern "C"
