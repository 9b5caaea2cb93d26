// Endpointing of live streams (stream_endpoint.hip; specification: tests/endpoint_oracle.py): the state machine that cuts a
// stream's logits rows into utterances, for host and device.  The rule is a pure function of the stream's rows -- never of how
// they were cut into steps or of the other streams:
//
//   row t is SILENT when its argmax (first maximum on ties, columns below num_classes only) is the blank (C - 1) or space_id
//   (-1: no such class), SPEECH otherwise.  Row t always joins the open utterance [u0, ...).  A speech row sets started and
//   run = 0, a silent row increments run.  Then, with len = t + 1 - u0, the first of these that applies fires:
//     1 (silence)  started && run >= R     the utterance [u0, t + 1) is final
//     2 (length)   started && len >= M     final as well, cut where it stands
//     3 (discard)  !started && len >= L    no utterance: the rows are dropped (long silence fills no pool; L <= M)
//   and after any event u0 = t + 1, started = false, run = 0.  When the stream finishes (limit >= 0; rows at or past the limit are
//   not consumed) a non-empty open stretch ends with event 4 (end of stream) if it has started and with event 3 otherwise.
//
// g = min(L, R + 1, M) rows lie between two events and the first event of a step can fall on its first row, so a step of at most
// n rows per stream holds at most 1 + (n - 1) / g row events and 2 + (n - 1) / g PIECES: runs of the step's rows that belong to
// one utterance, in the {first row, rows, limit, reset} format of the streaming decoders' tables.
//
// The sum of an utterance's chosen logits is added up in the order of the whole-utterance greedy decoder (ctc_greedy_kernel), so that
// a final's score equals that decoder's on the utterance's rows bit for bit: row i of the utterance goes to slot i % 256 (float, in
// row order), and the 256 slots are summed as a binary tree of neighbours.  The slots are the stream's score state.
//
// `walk` is one stream's step -- greedy decoding, the rule, the events and the pieces -- written once: the kernel runs it with all
// 64 lanes in step (the argmax is the wave's, lane 0 writes), the host form with a scalar argmax.
#pragma once

#if defined(__HIPCC__)
#define ST_EP_HD __host__ __device__
#else
#define ST_EP_HD
#endif

namespace st {
namespace endpoint {

enum { EV_NONE = 0, EV_SILENCE = 1, EV_LENGTH = 2, EV_DISCARD = 3, EV_END = 4 };
constexpr int kEventWords = 8;   // {kind, u0, end, first_speech or -1, last_speech, ids_end, -sum (float bits), utterance index}
constexpr int kPieceWords = 4;   // {first row, rows, limit, reset}
constexpr int kStateWords = 8;
constexpr int kSumSlots = 256;   // floats of score state per stream

struct Params {
  int R, L, M;        // silence_frames, lead_frames, max_frames
  int space, blank;   // the silent classes (space -1: only the blank)
};

struct State {        // one stream's record between steps: kStateWords int32
  int u0;             // first frame of the open utterance
  int started;
  int run;            // trailing silent rows
  int first_speech, last_speech;   // -1 while not started
  int index;          // finals so far: the index of the open utterance
  int last;           // greedy decoding: the previous row's argmax (-1 at the start of an utterance)
  int next;           // rows consumed so far: the next row's absolute frame
};

ST_EP_HD inline bool params_ok(int R, int L, int M) { return R >= 1 && L >= 1 && M >= L; }

// pieces (and event slots) per stream for steps of at most max_rows rows per stream; 0: bad arguments
ST_EP_HD inline int pieces_for(int max_rows, int R, int L, int M) {
  if (max_rows < 1 || !params_ok(R, L, M)) return 0;
  int g = L < M ? L : M;
  if (R < g) g = R + 1;            // (R + 1 <= g  <=>  R < g)
  return 2 + (max_rows - 1) / g;
}

ST_EP_HD inline void reset(State& s) {
  s.u0 = 0; s.started = 0; s.run = 0; s.first_speech = -1; s.last_speech = -1; s.index = 0; s.last = -1; s.next = 0;
}

// row t joins the open utterance; returns the event that fires on it (EV_NONE: none)
ST_EP_HD inline int take_row(State& s, const Params& p, int t, bool silent) {
  if (silent) {
    ++s.run;
  } else {
    if (!s.started) { s.started = 1; s.first_speech = t; }
    s.last_speech = t;
    s.run = 0;
  }
  s.next = t + 1;
  const int len = t + 1 - s.u0;
  if (s.started) return s.run >= p.R ? EV_SILENCE : (len >= p.M ? EV_LENGTH : EV_NONE);
  return len >= p.L ? EV_DISCARD : EV_NONE;
}

// after an event: the next utterance opens at `end`
ST_EP_HD inline void close_utterance(State& s, int kind, int end) {
  if (kind != EV_DISCARD) ++s.index;
  s.u0 = end; s.started = 0; s.run = 0; s.first_speech = -1; s.last_speech = -1; s.last = -1;
}

// the score state on plain memory (the host form; the kernel keeps four slots per lane in registers)
struct ScalarSum {
  float* slots;
  ST_EP_HD void add(int j, float v) { slots[j] += v; }
  ST_EP_HD void clear() { for (int i = 0; i < kSumSlots; ++i) slots[i] = 0.f; }
  ST_EP_HD float total() const {
    float f[kSumSlots];
    for (int i = 0; i < kSumSlots; ++i) f[i] = slots[i];
    for (int o = 1; o < kSumSlots; o <<= 1)
      for (int i = 0; i + o < kSumSlots; i += 2 * o) f[i] += f[i + o];
    return f[0];
  }
  ST_EP_HD void save() {}
};

ST_EP_HD inline int float_bits(float v) {
  union { float f; int i; } u;
  u.f = v;
  return u.i;
}

// One stream's step.  tab = the host's {first row, rows, limit, reset}; rows [n][2] (stream, absolute frame); argmax(r, &k, &v):
// class and value of row r of the launch.  st: the stream's record; sum: the open utterance's score state, loaded (add / total /
// clear / save: ScalarSum, or the kernel's register form).
// ids [max_new]: the step's new ids, all utterances concatenated; events [P][8]; pieces: this stream's entry of piece p at
// pieces[p * piece_stride].  Only `writer` stores (the kernel: lane 0; every lane computes the same).  Slots from P on are never
// written: more events than P cannot happen while the stream's rows stay within the cap P was sized for.
template <class Argmax, class Sum>
ST_EP_HD inline void walk(const Params& prm, const int* tab, const int* rows, Argmax argmax, bool writer, int* st_words, Sum& sum,
                          int* ids, int max_new, int* new_count, float* neg_sum, int* events, int* pieces, long piece_stride, int P) {
  const int first = tab[0], count = tab[1], limit = tab[2], host_reset = tab[3];
  State s;
  if (host_reset) {
    reset(s);
    sum.clear();
  } else {
    s.u0 = st_words[0]; s.started = st_words[1]; s.run = st_words[2]; s.first_speech = st_words[3];
    s.last_speech = st_words[4]; s.index = st_words[5]; s.last = st_words[6]; s.next = st_words[7];
  }
  int p = 0, ev = 0, out = 0;
  int piece_first = first, piece_rows = 0, piece_reset = host_reset ? 1 : 0;
  auto put_piece = [&](int limit_of_piece) {
    if (writer && p < P) {
      int* q = pieces + (long)p * piece_stride;
      const bool empty = piece_rows == 0;
      q[0] = empty ? 0 : piece_first;
      q[1] = piece_rows;
      q[2] = limit_of_piece;
      q[3] = piece_reset;
    }
    ++p;
  };
  auto put_event = [&](int kind, int end) {
    const float total = sum.total();
    if (writer && ev < P) {
      int* e = events + ev * kEventWords;
      e[0] = kind; e[1] = s.u0; e[2] = end; e[3] = s.first_speech; e[4] = s.last_speech; e[5] = out;
      e[6] = float_bits(-total); e[7] = s.index;
    }
    ++ev;
  };
  for (int r = first; r < first + count; ++r) {
    const int t = rows[2 * r + 1];
    if (limit >= 0 && t >= limit) break;
    int k;
    float v;
    argmax(r, k, v);
    sum.add((t - s.u0) & (kSumSlots - 1), v);
    if (k != prm.blank && k != s.last) {
      if (writer && out < max_new) ids[out] = k;
      ++out;
    }
    s.last = k;
    ++piece_rows;
    const int kind = take_row(s, prm, t, k == prm.blank || k == prm.space);
    if (kind != EV_NONE) {
      put_event(kind, t + 1);
      put_piece(kind == EV_DISCARD ? -1 : t + 1);
      close_utterance(s, kind, t + 1);
      sum.clear();
      piece_first = r + 1; piece_rows = 0; piece_reset = 1;
    }
  }
  // the piece that stays open -- or, at the end of the stream, closes what is left
  int last_limit = -1, last_kind = EV_NONE;
  if (limit >= 0 && s.next > s.u0) {
    last_kind = s.started ? EV_END : EV_DISCARD;
    put_event(last_kind, s.next);
    if (last_kind == EV_END) last_limit = s.next;
  }
  if (piece_rows > 0 || piece_reset || last_limit >= 0) put_piece(last_limit);
  if (last_kind != EV_NONE) {
    close_utterance(s, last_kind, s.next);
    sum.clear();
  }
  const float open_total = sum.total();
  sum.save();
  if (writer) {
    for (int q = p; q < P; ++q) {
      int* w = pieces + (long)q * piece_stride;
      w[0] = 0; w[1] = 0; w[2] = -1; w[3] = 0;
    }
    if (ev < P) events[ev * kEventWords] = EV_NONE;
    st_words[0] = s.u0; st_words[1] = s.started; st_words[2] = s.run; st_words[3] = s.first_speech;
    st_words[4] = s.last_speech; st_words[5] = s.index; st_words[6] = s.last; st_words[7] = s.next;
    *new_count = out;
    *neg_sum = -open_total;
  }
}

}  // namespace endpoint
}  // namespace st
