// Word times and confidences for the finals of live streams (semantics: include/speecht_hip.h).  A stream's logits buffer holds one
// step's rows; st_stream_keep_f32 copies them into a ring per stream, and when the endpointer closes an utterance the alignment and
// confidence lattices read its rows back from there (st_ctc_align_ring_f32 in ctc_align.hip, st_ctc_word_conf_ring_f32 in
// ctc_conf.hip: their softmax stage is the gather).  Here: the ring's size, the keep kernel and the host forms of the two ring entry
// points, which gather a job's rows through the same index function (stream_ring.h) and run the existing host recursions.
#include <algorithm>
#include <vector>

#include "st_common.h"
#include "stream_ring.h"

namespace {

// one lane per float: lane c of row r copies logits[r][c] to its stream's slot; rows of a stream or frame the ring cannot hold are
// skipped.  32 lanes write 128 contiguous bytes.
__global__ __launch_bounds__(256) void stream_keep_kernel(const float* __restrict__ logits, int pitch, int C,
                                                          const int* __restrict__ rows, int n_rows, int max_streams,
                                                          float* __restrict__ ring, int cap) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int r = (int)(i / st::RING_PITCH), c = (int)(i % st::RING_PITCH);
  if (r >= n_rows || c >= C) return;
  const int stream = rows[2 * r], frame = rows[2 * r + 1];
  if (stream < 0 || stream >= max_streams || frame < 0) return;
  ring[st::ring_off(stream, frame, cap) + c] = logits[(long)r * pitch + c];
}

// the rows of all jobs as the dense [n_jobs][max_rows][C] array the host recursions take (rows past a job's end and the rows of a
// job the ring cannot serve: zeros, never used) and their seq_lens
void gather_jobs(const float* ring, int max_streams, int cap, int C, const int32_t* jobs, int n_jobs, int max_rows,
                 std::vector<float>& dense, std::vector<int32_t>& lens) {
  dense.assign((size_t)n_jobs * max_rows * C, 0.f);
  lens.resize(n_jobs);
  for (int j = 0; j < n_jobs; ++j) {
    lens[j] = st::ring_job_rows(jobs, j, max_streams, max_rows);
    for (int t = 0; t < lens[j]; ++t) {
      const float* row = ring + st::ring_job_off(jobs, j, t, max_streams, max_rows, cap);
      std::copy(row, row + C, dense.begin() + ((size_t)j * max_rows + t) * C);
    }
  }
}

}  // namespace

extern "C" {

int st_stream_keep_rows(int max_frames, int max_rows) {
  if (max_frames < 1 || max_rows < 1 || (long)max_frames + max_rows > 0x7fffffffL) return 0;
  return max_frames + max_rows;
}

int st_stream_keep_f32(const float* logits, int pitch, int num_classes, const int32_t* rows, int n_rows, int max_streams, float* ring,
                       int cap, void* stream) {
  ST_REQUIRE(logits && rows && ring, "stream_keep: null argument");
  ST_REQUIRE(num_classes >= 1 && num_classes <= st::RING_PITCH && pitch >= num_classes, "stream_keep: num_classes must be 1..32, pitch >= num_classes");
  ST_REQUIRE(n_rows >= 0 && max_streams >= 1 && cap >= 1, "stream_keep: bad sizes");
  if (n_rows == 0) return ST_OK;
  const long lanes = (long)n_rows * st::RING_PITCH;
  st::trace("stream_keep rows=%d streams=%d cap=%d", n_rows, max_streams, cap);
  hipLaunchKernelGGL(stream_keep_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st::as_stream(stream), logits, pitch,
                     num_classes, rows, n_rows, max_streams, ring, cap);
  return st::check_launch("stream_keep");
}

int st_ctc_align_ring_host(const float* ring, int max_streams, int cap, int num_classes, const int32_t* jobs, int n_jobs, int max_rows,
                           const int32_t* label_ids, const int32_t* label_offsets, int max_label_len, int32_t* spans, int32_t* states,
                           float* score, int32_t* status, void* workspace, size_t workspace_bytes) {
  ST_REQUIRE(ring && jobs, "ctc_align_ring: null argument");
  ST_REQUIRE(max_streams >= 1 && cap >= 1 && n_jobs >= 1 && max_rows >= 1, "ctc_align_ring: bad ring or job shape");
  ST_REQUIRE(num_classes >= 2 && num_classes <= st::RING_PITCH, "ctc_align_ring: num_classes must be 2..32");
  std::vector<float> dense;
  std::vector<int32_t> lens;
  gather_jobs(ring, max_streams, cap, num_classes, jobs, n_jobs, max_rows, dense, lens);
  return st_ctc_align_host(dense.data(), n_jobs, max_rows, num_classes, label_ids, label_offsets, lens.data(), max_label_len, spans,
                           states, score, status, workspace, workspace_bytes);
}

int st_ctc_word_conf_ring_host(const float* ring, int max_streams, int cap, int num_classes, const int32_t* jobs, int n_jobs,
                               int max_rows, const int32_t* label_ids, const int32_t* label_offsets, int max_label_len, int space_id,
                               const int32_t* word_spans, int n_words, double* log_prob, double* log_conf, int32_t* status,
                               void* workspace, size_t workspace_bytes) {
  ST_REQUIRE(ring && jobs, "ctc_word_conf_ring: null argument");
  ST_REQUIRE(max_streams >= 1 && cap >= 1 && n_jobs >= 1 && max_rows >= 1, "ctc_word_conf_ring: bad ring or job shape");
  ST_REQUIRE(num_classes >= 2 && num_classes <= st::RING_PITCH, "ctc_word_conf_ring: num_classes must be 2..30");
  std::vector<float> dense;
  std::vector<int32_t> lens;
  gather_jobs(ring, max_streams, cap, num_classes, jobs, n_jobs, max_rows, dense, lens);
  return st_ctc_word_conf_host(dense.data(), n_jobs, max_rows, num_classes, label_ids, label_offsets, lens.data(), max_label_len,
                               space_id, word_spans, n_words, log_prob, log_conf, status, workspace, workspace_bytes);
}

}  // extern "C"
