// Endpointing of live streams on the device (semantics: include/speecht_hip.h, stream_endpoint_core.h; specification:
// tests/endpoint_oracle.py).  st_ctc_greedy_endpoint_stream takes the place of st_ctc_greedy_stream when a recogniser endpoints: one
// wave per stream walks the stream's rows of the step with that kernel's argmax network, decodes greedily per utterance, runs the
// rule and writes the step's events and the PIECES -- tables in the {first row, rows, limit, reset} format the beam-search kernels
// already take from device memory, one per utterance the step touches -- so that the searches follow the endpointer without the
// host in between (st_ctc_beam_stream_step_pieces, ctc_beam.hip).  st_stream_endpoint_host is the same walk on host memory.
#include "st_common.h"
#include "stream_endpoint_core.h"

namespace {

namespace ep = st::endpoint;

// the score state of one stream in the wave: lane l keeps slots 4 l .. 4 l + 3; the tree of neighbours is two adds in the lane and six
// steps across the lanes (lane 0 ends with the total, which every lane then takes)
struct WaveSum {
  float* slots;
  int lane;
  float r[4];
  __device__ void load() {
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = slots[4 * lane + i];
  }
  __device__ void add(int j, float v) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (j == 4 * lane + i) r[i] += v;
  }
  __device__ void clear() { r[0] = r[1] = r[2] = r[3] = 0.f; }
  __device__ float total() const {
    float a = (r[0] + r[1]) + (r[2] + r[3]);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) a += __shfl_down(a, o, 64);
    return __shfl(a, 0, 64);
  }
  __device__ void save() {
#pragma unroll
    for (int i = 0; i < 4; ++i) slots[4 * lane + i] = r[i];
  }
};
static_assert(ep::kSumSlots == 4 * 64, "four score slots per lane");

__global__ __launch_bounds__(64) void ctc_greedy_endpoint_stream_kernel(const float* __restrict__ logits, int pitch, int C,
                                                                        const int* __restrict__ rows, const int* __restrict__ table,
                                                                        int max_streams, ep::Params prm, int* __restrict__ state,
                                                                        float* __restrict__ score, int* __restrict__ ids, int max_new,
                                                                        int* __restrict__ new_count, float* __restrict__ neg_sum,
                                                                        int* __restrict__ events, int* __restrict__ pieces, int P) {
  const int s = blockIdx.x, lane = threadIdx.x;
  // the argmax of ctc_greedy_stream_kernel: lanes are classes, first maximum on ties; the result is wave-uniform
  auto argmax = [&](int r, int& k, float& v) {
    v = lane < C ? logits[(long)r * pitch + lane] : -INFINITY;
    k = lane < C ? lane : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int ok = __shfl_xor(k, o, 64);
      if (ov > v || (ov == v && ok < k)) { v = ov; k = ok; }
    }
  };
  WaveSum sum{score + (long)s * ep::kSumSlots, lane, {0.f, 0.f, 0.f, 0.f}};
  sum.load();
  ep::walk(prm, table + 4 * s, rows, argmax, lane == 0, state + ep::kStateWords * s, sum, ids + (long)s * max_new, max_new,
           new_count + s, neg_sum + s, events + (long)s * P * ep::kEventWords, pieces + ep::kPieceWords * s,
           (long)max_streams * ep::kPieceWords, P);
}

int check_common(const char* who, const float* logits, int pitch, int C, const int32_t* rows, const int32_t* table, int max_streams,
                 int space_id, int R, int L, int M, int max_rows, const void* state, const void* score, const void* ids, int max_new,
                 const void* new_count, const void* neg_sum, const void* events, const void* pieces, int n_pieces) {
  ST_REQUIRE(logits && rows && table && state && score && ids && new_count && neg_sum && events && pieces, "%s: null argument", who);
  ST_REQUIRE(C >= 2 && C <= 64 && pitch >= C && max_streams >= 1 && max_new >= 1, "%s: 2..64 classes, pitch >= classes, positive sizes", who);
  ST_REQUIRE(space_id >= -1 && space_id < C, "%s: space_id %d is neither -1 nor a class below %d", who, space_id, C);
  ST_REQUIRE(R >= 1 && L >= 1, "%s: silence_frames %d and lead_frames %d must be positive", who, R, L);
  ST_REQUIRE(M >= L, "%s: max_frames %d is below lead_frames %d (a stretch without speech could outgrow the pool)", who, M, L);
  ST_REQUIRE(max_rows >= 1, "%s: max_rows %d must be positive", who, max_rows);
  ST_REQUIRE(n_pieces >= ep::pieces_for(max_rows, R, L, M), "%s: %d pieces given, steps of up to %d rows per stream need %d", who, n_pieces,
             max_rows, ep::pieces_for(max_rows, R, L, M));
  ST_REQUIRE(reinterpret_cast<uintptr_t>(score) % 4 == 0, "%s: score must be 4-byte aligned", who);
  return ST_OK;
}

}  // namespace

extern "C" {

size_t st_stream_endpoint_state_bytes(void) { return ep::kStateWords * sizeof(int32_t); }

size_t st_stream_endpoint_score_bytes(void) { return ep::kSumSlots * sizeof(float); }

int st_stream_endpoint_pieces(int max_rows, int silence_frames, int lead_frames, int max_frames) {
  return ep::pieces_for(max_rows, silence_frames, lead_frames, max_frames);
}

int st_ctc_greedy_endpoint_stream(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* table,
                                  int max_streams, int space_id, int silence_frames, int lead_frames, int max_frames, int max_rows,
                                  int32_t* state, float* score, int32_t* ids, int max_new, int32_t* new_count, float* neg_sum_logits,
                                  int32_t* events, int32_t* pieces, int n_pieces, void* stream) {
  if (int e = check_common("greedy endpoint stream", logits, pitch, num_classes, rows, table, max_streams, space_id, silence_frames,
                           lead_frames, max_frames, max_rows, state, score, ids, max_new, new_count, neg_sum_logits, events, pieces, n_pieces))
    return e;
  const ep::Params prm{silence_frames, lead_frames, max_frames, space_id, num_classes - 1};
  st::trace("ctc_greedy_endpoint_stream streams=%d R=%d L=%d M=%d pieces=%d", max_streams, silence_frames, lead_frames, max_frames, n_pieces);
  hipLaunchKernelGGL(ctc_greedy_endpoint_stream_kernel, dim3(max_streams), dim3(64), 0, st::as_stream(stream), logits, pitch, num_classes,
                     rows, table, max_streams, prm, state, score, ids, max_new, new_count, neg_sum_logits, events, pieces, n_pieces);
  return st::check_launch("ctc_greedy_endpoint_stream");
}

int st_stream_endpoint_host(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* table, int max_streams,
                            int space_id, int silence_frames, int lead_frames, int max_frames, int max_rows, int32_t* state,
                            float* score, int32_t* ids, int max_new, int32_t* new_count, float* neg_sum_logits, int32_t* events,
                            int32_t* pieces, int n_pieces) {
  if (int e = check_common("stream endpoint host", logits, pitch, num_classes, rows, table, max_streams, space_id, silence_frames,
                           lead_frames, max_frames, max_rows, state, score, ids, max_new, new_count, neg_sum_logits, events, pieces, n_pieces))
    return e;
  const ep::Params prm{silence_frames, lead_frames, max_frames, space_id, num_classes - 1};
  auto argmax = [&](int r, int& k, float& v) {
    const float* x = logits + (long)r * pitch;
    k = 0;
    v = x[0];
    for (int c = 1; c < num_classes; ++c)
      if (x[c] > v) { v = x[c]; k = c; }
  };
  for (int s = 0; s < max_streams; ++s) {
    ep::ScalarSum sum{score + (long)s * ep::kSumSlots};
    ep::walk(prm, table + 4 * s, rows, argmax, true, state + ep::kStateWords * s, sum, ids + (long)s * max_new, max_new,
             new_count + s, neg_sum_logits + s, events + (long)s * n_pieces * ep::kEventWords, pieces + ep::kPieceWords * s,
             (long)max_streams * ep::kPieceWords, n_pieces);
  }
  return ST_OK;
}

}  // extern "C"
