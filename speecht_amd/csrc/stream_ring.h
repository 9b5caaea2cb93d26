// The ring of logits rows a recogniser keeps per stream for the word times and confidences of its finals (semantics:
// include/speecht_hip.h): ring[max_streams][cap][32] floats, frame f of stream s at slot f % cap.  One index function serves the keep
// kernel (stream_words.hip), the ring-mapped softmax stages of ctc_align.hip and ctc_conf.hip and the host forms, so that all of them
// name the same row.  Also here: what stands in the lattice kernels for seq_lens -- a plain array for the dense entry points, the job
// table for the ring ones.  Compiles with a plain C++ compiler.
#pragma once

#include "ctc_lattice.h"

namespace st {

constexpr int RING_PITCH = 32;      // floats per ring row

// float offset of frame `frame` (>= 0) of stream `stream` in the ring
ST_LAT_HD long ring_off(int stream, long frame, int cap) { return ((long)stream * cap + frame % cap) * RING_PITCH; }

// jobs int32 [n_jobs][3] = {stream, u0, n_rows}.  The rows of a job the ring can serve; -1 for any other job, which the lattice
// kernels then refuse like every length outside 0..frames (lattice_refused): status != 0.
ST_LAT_HD int ring_job_rows(const int* jobs, int j, int max_streams, int max_rows) {
  const int* job = jobs + 3 * (long)j;
  const bool ok = job[0] >= 0 && job[0] < max_streams && job[1] >= 0 && job[2] >= 0 && job[2] <= max_rows;
  return ok ? job[2] : -1;
}

// float offset of row t (0 <= t < max_rows) of job j; a job the ring cannot serve reads stream 0: defined memory, never used
ST_LAT_HD long ring_job_off(const int* jobs, int j, int t, int max_streams, int max_rows, int cap) {
  const int* job = jobs + 3 * (long)j;
  const bool ok = ring_job_rows(jobs, j, max_streams, max_rows) >= 0;
  return ring_off(ok ? job[0] : 0, ok ? (long)job[1] + t : (long)t, cap);
}

// the frames of utterance b, as the lattice kernels ask for them
struct DenseLens {
  const int* lens;
  ST_LAT_HD int operator()(int b) const { return lens[b]; }
};
struct RingLens {
  const int* jobs;
  int max_streams, max_rows;
  ST_LAT_HD int operator()(int b) const { return ring_job_rows(jobs, b, max_streams, max_rows); }
};
// (job, t) -> float offset of a row in the ring: the RowMap of the ring entry points
struct RingMap {
  const int* jobs;
  int max_streams, max_rows, cap;
  ST_LAT_HD long off(int b, int t) const { return ring_job_off(jobs, b, t, max_streams, max_rows, cap); }
};

}  // namespace st
