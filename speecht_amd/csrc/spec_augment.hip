// SpecAugment on the way into the network (st_spec_augment_f32, st_spec_augment_host, st_spec_augment_plan_host): the copy of a
// staged feature batch [B][T][C] into the padded input tensor X[0], with each utterance's time warp, frequency masks and time
// masks applied as the rows pass.  What is drawn and how it is applied: csrc/spec_augment_core.h, shared with the host form.
//
// One launch.  A workgroup owns SA_ROWS rows of one utterance: it rebuilds the utterance's plan in LDS from the draw id (one lane
// and one Philox block per plan entry), then one lane per row works out what the row is made of (the integer division of the warp
// map happens once per row, not per element), then all lanes move the rows: 16-byte loads and stores across the channels when
// C % 4 == 0 and both sides are 16-byte aligned, single floats otherwise.  A row inside a time mask is a store of zeros with no
// load; a warped row loads two source rows.  Only interior rows and the C valid channels of the destination are written.
#include "spec_augment_core.h"
#include "st_common.h"

namespace {

using st::SpecPolicy;
using st::SpecRow;

constexpr int SA_THREADS = 256;
constexpr int SA_ROWS = 32;                          // rows of one utterance per workgroup

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__device__ __forceinline__ int clamp_len(int L, int T) { return L < 0 ? 0 : (L > T ? T : L); }

template <bool VEC>
__global__ __launch_bounds__(SA_THREADS) void spec_augment_kernel(const float* __restrict__ src, int T, int C,
                                                                  const int32_t* __restrict__ lens,
                                                                  const int64_t* __restrict__ draw_ids, uint64_t seed, SpecPolicy pol,
                                                                  float* __restrict__ dst, int halo, int t_pitch, int c_pitch,
                                                                  int32_t* __restrict__ plan_out) {
  __shared__ int plan[st::SA_PLAN_MAX];
  __shared__ int row_kind[SA_ROWS], row_i[SA_ROWS];
  __shared__ float row_frac[SA_ROWS];
  const int b = blockIdx.y, t0 = blockIdx.x * SA_ROWS, tid = threadIdx.x;
  const int rows = min(SA_ROWS, T - t0);
  const int L = clamp_len(lens[b], T);               // (the engine refuses a length outside 0 .. T before the launch)
  const int entries = 1 + pol.mF + pol.mT, words = 2 * entries;
  if (tid < entries) {
    int first, second;
    st::sa_plan_entry(pol, seed, (uint64_t)draw_ids[b], L, C, tid, first, second);
    plan[2 * tid] = first;
    plan[2 * tid + 1] = second;
    if (plan_out && blockIdx.x == 0) {
      plan_out[(long)b * words + 2 * tid] = first;
      plan_out[(long)b * words + 2 * tid + 1] = second;
    }
  }
  __syncthreads();
  if (tid < rows) {
    const SpecRow r = st::sa_row(pol, plan, L, t0 + tid);
    row_kind[tid] = r.kind;
    row_i[tid] = r.i;
    row_frac[tid] = r.frac;
  }
  __syncthreads();
  const float* s = src + (long)b * T * C;
  float* d = dst + ((long)b * t_pitch + halo + t0) * (long)c_pitch;
  const st::SpecFreqMasks fm = st::sa_freq_masks(pol, plan);
  if (VEC) {
    const int C4 = C >> 2;
    for (int idx = tid; idx < rows * C4; idx += SA_THREADS) {
      const int r = idx / C4, q = idx - r * C4;
      const int kind = row_kind[r];
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (kind != st::SA_ROW_ZERO) {
        const float4* x = reinterpret_cast<const float4*>(s + (long)row_i[r] * C) + q;
        v = x[0];
        const float frac = row_frac[r];
        if (frac != 0.f) {
          const float4 u = x[C4];
          v.x = st::sa_lerp(frac, v.x, u.x);
          v.y = st::sa_lerp(frac, v.y, u.y);
          v.z = st::sa_lerp(frac, v.z, u.z);
          v.w = st::sa_lerp(frac, v.w, u.w);
        }
        if (kind == st::SA_ROW_VALID) {
          const int ch = 4 * q;
          if (st::sa_channel_masked(fm, ch)) v.x = 0.f;
          if (st::sa_channel_masked(fm, ch + 1)) v.y = 0.f;
          if (st::sa_channel_masked(fm, ch + 2)) v.z = 0.f;
          if (st::sa_channel_masked(fm, ch + 3)) v.w = 0.f;
        }
      }
      reinterpret_cast<float4*>(d + (long)r * c_pitch)[q] = v;
    }
  } else {
    for (int idx = tid; idx < rows * C; idx += SA_THREADS) {
      const int r = idx / C, ch = idx - r * C;
      const int kind = row_kind[r];
      float v = 0.f;
      if (kind != st::SA_ROW_ZERO) {
        const float* x = s + (long)row_i[r] * C + ch;
        v = x[0];
        const float frac = row_frac[r];
        if (frac != 0.f) v = st::sa_lerp(frac, v, x[C]);
        if (kind == st::SA_ROW_VALID && st::sa_channel_masked(fm, ch)) v = 0.f;
      }
      d[(long)r * c_pitch + ch] = v;
    }
  }
}

int check_policy(const char* who, int W, int F, int mF, int Tw, int mT, int p_q16) {
  ST_REQUIRE(W >= 0 && F >= 0 && Tw >= 0, "%s: negative time warp %d, frequency-mask width %d or time-mask width %d", who, W, F, Tw);
  ST_REQUIRE(mF >= 0 && mF <= st::SA_MAX_MASKS && mT >= 0 && mT <= st::SA_MAX_MASKS, "%s: %d frequency and %d time masks (0 .. %d each)", who,
             mF, mT, st::SA_MAX_MASKS);
  ST_REQUIRE(p_q16 >= 0 && p_q16 <= 65536, "%s: time-mask ratio %d / 65536 lies outside 0 .. 1", who, p_q16);
  return ST_OK;
}

int check_lengths(const char* who, const int32_t* lens, int B, int T) {
  for (int b = 0; b < B; ++b)
    ST_REQUIRE(lens[b] >= 0 && (T < 0 || lens[b] <= T), "%s: utterance %d has length %d outside 0 .. %d", who, b, lens[b], T);
  return ST_OK;
}

void plan_of(const SpecPolicy& pol, uint64_t seed, uint64_t id, int L, int C, int* plan) {
  for (int e = 0; e < 1 + pol.mF + pol.mT; ++e) st::sa_plan_entry(pol, seed, id, L, C, e, plan[2 * e], plan[2 * e + 1]);
}

}  // namespace

extern "C" {

int st_spec_augment_f32(const float* src, int batch, int frames, int channels, const int32_t* seq_lens, const int64_t* draw_ids,
                        uint64_t seed, int time_warp, int freq_width, int freq_masks, int time_width, int time_masks,
                        int time_ratio_q16, const st_tensor3* dst, int32_t* plan_out, void* stream) {
  ST_REQUIRE(batch >= 1 && frames >= 1 && channels >= 1, "st_spec_augment_f32: bad sizes (batch %d, frames %d, channels %d)", batch,
             frames, channels);
  int rc = check_policy("st_spec_augment_f32", time_warp, freq_width, freq_masks, time_width, time_masks, time_ratio_q16);
  if (rc != ST_OK) return rc;
  ST_REQUIRE(st::tensor_ok(dst) && dst->batch == batch && dst->frames == frames && dst->channels == channels,
             "st_spec_augment_f32: the destination descriptor does not describe a [%d][%d][%d] tensor", batch, frames, channels);
  ST_REQUIRE(src && seq_lens && draw_ids && (reinterpret_cast<uintptr_t>(draw_ids) & 7) == 0 && (reinterpret_cast<uintptr_t>(src) & 3) == 0,
             "st_spec_augment_f32: null or unaligned source, lengths or draw ids");
  ST_REQUIRE(batch <= 65535, "st_spec_augment_f32: batch %d exceeds the grid", batch);
  const SpecPolicy pol = {time_warp, freq_width, freq_masks, time_width, time_masks, time_ratio_q16};
  const bool vec = channels % 4 == 0 && aligned16(src) && aligned16(dst->base);      // (c_pitch % 16 == 0: every row start follows)
  const dim3 grid(st::ceil_div(frames, SA_ROWS), batch);
  hipStream_t s = st::as_stream(stream);
  if (st::trace_on())
    st::trace("spec_augment<%s> batch=%d frames=%d channels=%d W=%d F=%dx%d T=%dx%d p=%d/65536 blocks=%d", vec ? "vec4" : "scalar", batch,
              frames, channels, time_warp, freq_width, freq_masks, time_width, time_masks, time_ratio_q16, grid.x * grid.y);
  st::LaunchTimer timer(s);
  if (vec)
    st::launch_timed(timer, spec_augment_kernel<true>, grid, dim3(SA_THREADS), s, src, frames, channels, seq_lens, draw_ids, seed, pol,
                     dst->base, dst->halo, dst->t_pitch, dst->c_pitch, plan_out);
  else
    st::launch_timed(timer, spec_augment_kernel<false>, grid, dim3(SA_THREADS), s, src, frames, channels, seq_lens, draw_ids, seed, pol,
                     dst->base, dst->halo, dst->t_pitch, dst->c_pitch, plan_out);
  return st::check_launch("spec_augment_kernel");
}

int st_spec_augment_plan_host(const int32_t* seq_lens, const int64_t* draw_ids, int batch, int channels, uint64_t seed, int time_warp,
                              int freq_width, int freq_masks, int time_width, int time_masks, int time_ratio_q16, int32_t* plan_out) {
  ST_REQUIRE(batch >= 1 && channels >= 1, "st_spec_augment_plan_host: bad sizes (batch %d, channels %d)", batch, channels);
  int rc = check_policy("st_spec_augment_plan_host", time_warp, freq_width, freq_masks, time_width, time_masks, time_ratio_q16);
  if (rc != ST_OK) return rc;
  ST_REQUIRE(seq_lens && draw_ids && plan_out, "st_spec_augment_plan_host: null argument");
  rc = check_lengths("st_spec_augment_plan_host", seq_lens, batch, -1);
  if (rc != ST_OK) return rc;
  const SpecPolicy pol = {time_warp, freq_width, freq_masks, time_width, time_masks, time_ratio_q16};
  const int words = st::sa_plan_words(pol);
  for (int b = 0; b < batch; ++b) plan_of(pol, seed, (uint64_t)draw_ids[b], seq_lens[b], channels, plan_out + (long)b * words);
  return ST_OK;
}

int st_spec_augment_host(const float* src, int batch, int frames, int channels, const int32_t* seq_lens, const int64_t* draw_ids,
                         uint64_t seed, int time_warp, int freq_width, int freq_masks, int time_width, int time_masks,
                         int time_ratio_q16, const st_tensor3* dst, int32_t* plan_out) {
  ST_REQUIRE(batch >= 1 && frames >= 1 && channels >= 1, "st_spec_augment_host: bad sizes (batch %d, frames %d, channels %d)", batch,
             frames, channels);
  int rc = check_policy("st_spec_augment_host", time_warp, freq_width, freq_masks, time_width, time_masks, time_ratio_q16);
  if (rc != ST_OK) return rc;
  ST_REQUIRE(st::tensor_ok(dst) && dst->batch == batch && dst->frames == frames && dst->channels == channels,
             "st_spec_augment_host: the destination descriptor does not describe a [%d][%d][%d] tensor", batch, frames, channels);
  ST_REQUIRE(src && seq_lens && draw_ids, "st_spec_augment_host: null argument");
  rc = check_lengths("st_spec_augment_host", seq_lens, batch, frames);
  if (rc != ST_OK) return rc;
  const SpecPolicy pol = {time_warp, freq_width, freq_masks, time_width, time_masks, time_ratio_q16};
  const int words = st::sa_plan_words(pol);
  int plan[st::SA_PLAN_MAX];
  for (int b = 0; b < batch; ++b) {
    const int L = seq_lens[b];
    plan_of(pol, seed, (uint64_t)draw_ids[b], L, channels, plan);
    if (plan_out)
      for (int i = 0; i < words; ++i) plan_out[(long)b * words + i] = plan[i];
    const float* s = src + (long)b * frames * channels;
    const st::SpecFreqMasks fm = st::sa_freq_masks(pol, plan);
    for (int t = 0; t < frames; ++t) {
      const SpecRow row = st::sa_row(pol, plan, L, t);
      float* d = dst->base + st::row_offset(*dst, b, t);
      const float* x = s + (long)row.i * channels;
      for (int ch = 0; ch < channels; ++ch) {
        float v = 0.f;
        if (row.kind != st::SA_ROW_ZERO) {
          v = x[ch];
          if (row.frac != 0.f) v = st::sa_lerp(row.frac, v, x[channels + ch]);
          if (row.kind == st::SA_ROW_VALID && st::sa_channel_masked(fm, ch)) v = 0.f;
        }
        d[ch] = v;
      }
    }
  }
  return ST_OK;
}

}  // extern "C"
