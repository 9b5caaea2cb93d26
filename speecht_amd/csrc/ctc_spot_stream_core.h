// Keyword spotting in live streams: what the gfx950 kernel and the host form of csrc/ctc_spot_stream.hip share beside the lattice
// arithmetic of ctc_spot_core.h -- the causal hit rule, the layout of a plan (keywords packed into waves) and of a stream's state
// record.  The rule is IEEE double comparisons and ONE multiply (contraction off), so that device and host form the same bits.
// Compiles with a plain C++ compiler.  Semantics: include/speecht_hip.h; float64 specification: tests/spot_stream_oracle.py.
#pragma once

#include <stdint.h>

#include "ctc_spot_core.h"

namespace st {
namespace spot_stream {

// ---- the rule -------------------------------------------------------------------------------------------------------------------

// what one (stream, keyword) pair keeps beside its lattice column: the pending hit (end == 0: none; then score = -inf and
// start = -1, so that a record's bits do not depend on its history) and the end of the last hit emitted
struct Pending {
  double score;
  int start, end, last_end;
};
ST_SP_HD void clear(Pending& p) { p.score = ST_SP_NEG_INF; p.start = -1; p.end = 0; }
ST_SP_HD void init(Pending& p) { clear(p); p.last_end = 0; }

struct Hit {
  double score;
  int start, end;
};

// whether frame t's end state (value e, start a) is a candidate: finite, begun at or after the last emitted hit's end, and its
// score per frame at or above the threshold -- e >= threshold * frames, one multiply
ST_SP_HD bool candidate(double e, int a, int t, double threshold, int last_end) {
#pragma clang fp contract(off)
  if (!(e > ST_SP_NEG_INF) || a < last_end) return false;
  const double bound = threshold * (double)(t + 1 - a);
  return e >= bound;
}

// Steps 1 .. 4 of the rule after the lattice update of frame t.  At most one hit leaves per frame (a hit made pending on this
// frame ends at t + 1 and hold >= 1): true when `out` is it.
ST_SP_HD bool rule(double e, int a, int t, double threshold, int hold, Pending& p, Hit& out) {
  const bool cand = candidate(e, a, t, threshold, p.last_end);
  bool emitted = false;
  if (p.end > 0 && cand && a >= p.end) {                      // 2. the candidate lies behind the pending hit: that one is final
    out = Hit{p.score, p.start, p.end};
    p.last_end = p.end;
    clear(p);
    emitted = true;
  }
  if (cand && (p.end == 0 || e >= p.score)) {                 // 3. the better of overlapping candidates stays, the later among equals
    p.score = e; p.start = a; p.end = t + 1;
  }
  if (p.end > 0 && t + 1 - p.end >= hold) {                   // 4. nothing better has come for `hold` frames
    out = Hit{p.score, p.start, p.end};
    p.last_end = p.end;
    clear(p);
    emitted = true;
  }
  return emitted;
}

// the rows of a table entry {first row, rows, limit or -1, reset} a spotter consumes, f0 the frame of its first row
ST_SP_HD int rows_taken(int count, int limit, int f0) {
  if (count <= 0) return 0;
  if (limit < 0) return count;
  const long left = (long)limit - f0;
  return left <= 0 ? 0 : (left < count ? (int)left : count);
}

// ---- a plan ---------------------------------------------------------------------------------------------------------------------
// int32 words: a header of kHeaderWords, n_waves wave tables of (KPL + 1) * 64 words, n_keywords keyword entries of 4 words.
//   header      {magic, total words, n_keywords, num_classes, KPL, n_waves, pack, first word of the keyword entries,
//                device address lo, hi (st_ctc_spot_stream_plan_bind; 0 until then), 0 ...}
//   wave table  desc [KPL][64]: state j of lane l is state l * KPL + j of the wave -- bits 0..4 the column of d it reads, bit 5 may
//               arrive from two states below, bit 6 live, bit 7 enter (state 1 of a keyword), bit 8 end (state 2L - 1);
//               then end_kw [64]: the keyword whose end state the lane holds, or -1 (a keyword begins on a lane boundary, so a
//               lane holds at most one)
//   keyword     {wave, first state in the wave (a multiple of KPL), L, 0}
constexpr int kMagic = 0x53505331;          // "SPS1"
constexpr int kHeaderWords = 16;
constexpr int kEventWords = 8;
enum Header { H_MAGIC, H_WORDS, H_KEYWORDS, H_CLASSES, H_KPL, H_WAVES, H_PACK, H_KW_AT, H_DEV_LO, H_DEV_HI };
constexpr int D_COL = 31, D_SKIP = 32, D_LIVE = 64, D_ENTER = 128, D_END = 256;

ST_SP_HD int wave_words(int kpl) { return (kpl + 1) * 64; }
ST_SP_HD long plan_words(int kpl, int n_waves, int n_keywords) {
  return kHeaderWords + (long)n_waves * wave_words(kpl) + 4L * n_keywords;
}

// ---- a stream's state: n_waves records --------------------------------------------------------------------------------------------
//   value double [KPL][64], start int32 [KPL][64], pending score double [64], pending start, pending end, last_end int32 [64] each
// -- every array lane-contiguous, so that a wave loads and stores its record in whole 256- and 512-byte runs.
ST_SP_HD long wave_state_bytes(int kpl) { return 64L * (12 * kpl + 20); }
struct StateView {
  double* v;
  int* s;
  double* pscore;
  int *pstart, *pend, *last;
};
ST_SP_HD StateView state_view(void* state, long stream_bytes, int stream, int wave, int kpl) {
  char* base = reinterpret_cast<char*>(state) + (long)stream * stream_bytes + (long)wave * wave_state_bytes(kpl);
  StateView w;
  w.v = reinterpret_cast<double*>(base);
  w.s = reinterpret_cast<int*>(base + 512L * kpl);
  w.pscore = reinterpret_cast<double*>(base + 768L * kpl);
  w.pstart = reinterpret_cast<int*>(base + 768L * kpl + 512);
  w.pend = w.pstart + 64;
  w.last = w.pstart + 128;
  return w;
}

// one event {keyword, start, end, kind, score bits lo, hi, 0, 0} into slot `at` of a stream's list, if the list holds it
ST_SP_HD void write_event(int* events, int max_events, int at, int keyword, const Hit& h, int kind) {
  if (at >= max_events) return;
  int* e = events + (long)at * kEventWords;
  const long long bits = __builtin_bit_cast(long long, h.score);
  e[0] = keyword; e[1] = h.start; e[2] = h.end; e[3] = kind;
  e[4] = (int)bits; e[5] = (int)(bits >> 32); e[6] = 0; e[7] = 0;
}

}  // namespace spot_stream
}  // namespace st
