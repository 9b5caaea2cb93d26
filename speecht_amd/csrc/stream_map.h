// Index arithmetic of streaming recognition (conv_stream.hip, speecht_amd/streaming.py): which output frames of a SAME-padded
// conv1d layer are final given how many input frames have arrived, and which input frames it still has to keep.  Pure
// functions of (width, stride) and a stream's counters, for host and device; speecht_amd/streaming.py carries the same
// arithmetic in Python (tests/test_stream_cpu.py and tests/host_cpp/stream_map_check.cpp hold both to a brute-force
// enumeration of receptive fields).
//
// SAME padding puts pad_total = (t_out - 1) * stride + width - T zeros around an utterance of T frames, the smaller half
// on the left.  For the strides this model has (1 and 2) the left part does not depend on T: (width - stride) / 2.  Output
// frame j reads the absolute input frames j * stride - pad_left ... + width - 1; frames outside [0, T) read as zero.
#pragma once

#if defined(__HIPCC__)
#define ST_SM_HD __host__ __device__
#else
#define ST_SM_HD
#endif

namespace st {
namespace stream_map {

// left SAME padding; length-independent only when (width - stride) / 2 == (width - 1) / 2 (pad_left_fixed)
ST_SM_HD inline int pad_left(int width, int stride) { return width > stride ? (width - stride) / 2 : 0; }
ST_SM_HD inline bool pad_left_fixed(int width, int stride) {
  return stride >= 1 && width >= stride && (width - stride) / 2 == (width - 1) / 2;
}

// number of output frames that are final after n input frames.  Open stream: output j is ready when its last tap has
// arrived, j * stride - pad_left + width - 1 <= n - 1.  Finished stream: every j < ceil(n / stride).
ST_SM_HD inline long ready_count(long n, int width, int stride, bool finished) {
  if (n <= 0) return 0;
  if (finished) return (n + stride - 1) / stride;
  const long last = n - width + pad_left(width, stride);   // largest j * stride that is ready
  return last < 0 ? 0 : last / stride + 1;
}

// frames to emit now: n frames received, e emitted so far
ST_SM_HD inline long emit_count(long n, long e, int width, int stride, bool finished) {
  const long r = ready_count(n, width, stride, finished);
  return r > e ? r - e : 0;
}

// first absolute input frame the layer still needs once e outputs are out (negative indices are padding, never stored)
ST_SM_HD inline long retain_from(long e, int width, int stride) {
  const long f = e * stride - pad_left(width, stride);
  return f > 0 ? f : 0;
}

// first absolute input frame that output j reads (may be negative: left padding)
ST_SM_HD inline long first_tap(long j, int width, int stride) { return j * stride - pad_left(width, stride); }

// logits rows that greedy decoding takes of an utterance of T input frames (the engine decodes seq_len / 2 rows)
ST_SM_HD inline long decode_limit(long total_input_frames) { return total_input_frames / 2; }

}  // namespace stream_map
}  // namespace st
