// Following a known script in live streams: what the gfx950 kernels and the host form of csrc/ctc_follow_stream.hip share beside the
// lattice arithmetic of ctc_align_core.h -- the tile geometry, the layout of a stream's state, of the result record and of the
// workspace's run record, and the pieces of the causal read-out (cursor, sliding minimum, best-of-two).  Everything that decides is
// IEEE double comparisons, additions and subtractions, so that device and host form the same bits.  Compiles with a plain C++
// compiler.  Semantics: include/speecht_hip.h; float64 specification: tests/follow_oracle.py.
#pragma once

#include <stdint.h>

#include "ctc_align_core.h"

namespace st {
namespace follow {

// ---- geometry: align_long_tile_kernel's ---------------------------------------------------------------------------------------------
constexpr int TB = 64;                 // rows of one run: what the halo keeps exact
constexpr int KPL = 16;                // states per lane
constexpr int HALO = 2 * TB;           // states below the owned ones that a tile recomputes
constexpr int SB = 64 * KPL - HALO;    // states a state block owns: 896
constexpr int OWN0 = HALO / KPL;       // first owning lane: 8
constexpr int MAX_BLOCKS = 64;         // the read-out's wave holds one block per lane
constexpr int MAX_LABELS = (MAX_BLOCKS * SB - 1) / 2;   // 28671
constexpr int MAX_CONFIRM = 16;

ST_AL_HD int state_blocks(int L) { return (2 * L + 1 + SB - 1) / SB; }
ST_AL_HD long col_elems(int NB) { return (long)SB * NB + HALO; }     // state u of a column is element HALO + u

// ---- a stream's state: a header of 32 int32 words, then two columns of col_elems(state_blocks(max_labels)) doubles ----------------------
//   header {0, frames consumed since the reset, words reached, c of the last frame (-1: none),
//           g lo, hi, b lo, hi, end_score lo, hi, 0 x 6, pos of the newest frame f with f % 16 == i for i = 0 .. 15}
// The first column is the stream's; a run leaves its new column in the second and the read-out launch copies it over the first, so
// between steps both hold the same and a stream's state is a function of its rows alone.
enum Header { H_FRAMES = 1, H_WORDS, H_C, H_G, H_B = 6, H_END = 8, H_HIST = 16 };
constexpr int kHeaderWords = 32;
ST_AL_HD long state_bytes(int max_labels) { return kHeaderWords * 4L + 2 * col_elems(state_blocks(max_labels)) * 8L; }
ST_AL_HD double* column(void* stream_state, int max_labels, int which) {
  return reinterpret_cast<double*>(reinterpret_cast<char*>(stream_state) + kHeaderWords * 4L) +
         (which ? col_elems(state_blocks(max_labels)) : 0L);
}

// ---- the result record: 16 int32 words per stream ---------------------------------------------------------------------------------------
//   {frames, c, status, events of this step (the true count), fit lo, hi, end_score lo, hi, words reached so far, 0 ...}
enum Result { R_FRAMES, R_C, R_STATUS, R_EVENTS, R_FIT, R_END = 6, R_WORDS = 8 };
constexpr int kResultWords = 16;
constexpr int kEventWords = 2;         // {word, frame}
constexpr int STATUS_TOO_LONG = 1, STATUS_NO_SCRIPT = 2, STATUS_ROWS_LOST = 4;

// ---- the run record the tile kernel leaves the read-out in the workspace: 8 int32 words per stream ----------------------------------
//   {what the stream does in this run, 0, frames before the run, rows of the run, first row of the run
//    in the launch, script length, reset, rows beyond the step's last run}
enum Run { I_WHAT, I_T0 = 2, I_N, I_ROW0, I_L, I_RESET, I_LOST };
constexpr int kRunWords = 8;
constexpr int SITS_OUT = 0, ACTIVE = 1, TOO_LONG = 2, NO_SCRIPT = 3;

// one partial maximum {value, lowest state attaining it (INT32_MAX: none)}: 16 bytes, written with one vector store
struct Best {
  double v;
  int u, pad;
};
constexpr int NO_STATE = 0x7fffffff;
// fold a state, or a block, that lies ABOVE everything folded so far: only a strictly larger value replaces the lower one
ST_AL_HD void fold_above(Best& b, double v, int u) {
  if (v > b.v) { b.v = v; b.u = u; }
}
// fold in any order (the butterfly of a wave): the larger value, the lower state among equals
ST_AL_HD void fold_any(Best& b, double v, int u) {
  if (v > b.v || (v == b.v && u < b.u)) { b.v = v; b.u = u; }
}
ST_AL_HD int cursor(const Best& b) { return b.v > ST_AL_NEG_INF ? b.u : -1; }     // c_t
ST_AL_HD int position(int c) { return c <= 0 ? 0 : (c + 1) >> 1; }                // pos_t: labels the state c has entered

// the newest frame f <= t_last with f % 16 == slot (what the header's history keeps in `slot`); may be negative: no such frame
ST_AL_HD int hist_frame(int t_last, int slot) { return t_last - ((t_last - slot) & 15); }

// the rows of a table entry {first row, rows, limit or -1, reset} a follower consumes, f0 the frame of its first row
ST_AL_HD int rows_taken(int count, int limit, int f0) {
  if (count <= 0) return 0;
  if (limit < 0) return count;
  const long left = (long)limit - f0;
  return left <= 0 ? 0 : (left < count ? (int)left : count);
}

// the largest ln-softmax value of a row (the greedy reading's term of g)
ST_AL_HD double row_max(const double* row, int C) {
  double m = row[0];
  for (int c = 1; c < C; ++c) m = row[c] > m ? row[c] : m;
  return m;
}

}  // namespace follow
}  // namespace st
