// The endpointer's walk (speecht_amd/csrc/stream_endpoint_core.h) on the host: seeded streams of silent and speech rows, every
// parameter triple of the Python sweep, cut into steps in several ways.  Whatever the cut, the events must be those of the rule applied
// to the whole stream in one go (written out again below), the pieces must tile the consumed rows in order with their limit and reset
// flags, the ids and sums must be the greedy decoding of each stretch alone, and nothing may be written behind the outputs.
// Built and run by tests/test_endpoint_host.py under the address and undefined-behaviour sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "stream_endpoint_core.h"

namespace ep = st::endpoint;

struct Event { int kind, u0, end, first, last, index; std::vector<int> ids; float neg_sum; };

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// the rule on a whole stream of `limit` rows (argmax ids k, values v)
static std::vector<Event> whole_stream(const std::vector<int>& k, const std::vector<float>& v, int limit, const ep::Params& p) {
  std::vector<Event> out;
  int u0 = 0, started = 0, run = 0, first = -1, last = -1, index = 0;
  auto close = [&](int kind, int end) {
    Event e{kind, u0, end, first, last, index, {}, 0.f};
    float slots[ep::kSumSlots] = {0.f};     // the whole-utterance greedy decoder's order: slot i % 256, then a tree of neighbours
    int prev = -1;
    for (int t = u0; t < end; ++t) {
      slots[(t - u0) % ep::kSumSlots] += v[t];
      if (k[t] != p.blank && k[t] != prev) e.ids.push_back(k[t]);
      prev = k[t];
    }
    for (int o = 1; o < ep::kSumSlots; o <<= 1)
      for (int i = 0; i + o < ep::kSumSlots; i += 2 * o) slots[i] += slots[i + o];
    e.neg_sum = -slots[0];
    out.push_back(e);
    if (kind != ep::EV_DISCARD) ++index;
    u0 = end; started = 0; run = 0; first = last = -1;
  };
  for (int t = 0; t < limit; ++t) {
    const bool silent = k[t] == p.blank || k[t] == p.space;
    if (silent) ++run;
    else { if (!started) { started = 1; first = t; } last = t; run = 0; }
    const int len = t + 1 - u0;
    if (started && run >= p.R) close(ep::EV_SILENCE, t + 1);
    else if (started && len >= p.M) close(ep::EV_LENGTH, t + 1);
    else if (!started && len >= p.L) close(ep::EV_DISCARD, t + 1);
  }
  if (limit > u0) close(started ? ep::EV_END : ep::EV_DISCARD, limit);
  return out;
}

static int fail(const char* what, int a, int b) { printf("FAILED: %s (%d, %d)\n", what, a, b); return 1; }

static int check_stream(int C, int space, int R, int L, int M, int T, int cut, bool finish_apart, long counts[5]) {
  const ep::Params prm{R, L, M, space, C - 1};
  const int pitch = 32, extra = 3, max_rows = cut + extra, P = ep::pieces_for(max_rows, R, L, M), guard = 5;
  const int limit = T - extra;
  // logits: a chosen class per row above the noise; columns from C on hold a larger value that must not be looked at
  std::vector<float> logits((size_t)T * pitch, 9.f);
  std::vector<int> k(T);
  std::vector<float> v(T);
  bool quiet = rnd() & 1;
  for (int t = 0; t < T;) {
    const int choices[8] = {1, 2, R, R + 1, L, L + 1, M + 2, M / 2 + 1};
    const int span = choices[rnd() % 8];
    for (int j = t; j < t + span && j < T; ++j) {
      for (int c = 0; c < C; ++c) logits[(size_t)j * pitch + c] = (float)(rnd() % 1000) / 500.f - 1.f;
      int c = C - 1;
      if (quiet) { if (space >= 0 && (rnd() & 1)) c = space; }
      else if (C > 2 || space < 0) { do c = rnd() % (C - 1); while (c == space); }
      logits[(size_t)j * pitch + c] = 2.f;
      if (rnd() % 8 == 0) logits[(size_t)j * pitch + C - 1] = 2.f;       // a tie with the blank: the lower index wins
      k[j] = 0; v[j] = logits[(size_t)j * pitch];
      for (int q = 1; q < C; ++q)
        if (logits[(size_t)j * pitch + q] > v[j]) { v[j] = logits[(size_t)j * pitch + q]; k[j] = q; }
    }
    t += span;
    quiet = !quiet;
  }
  const std::vector<Event> want = whole_stream(k, v, limit, prm);
  // the stream in steps
  std::vector<int> state(ep::kStateWords, 0x5A5A5A5A), rows((size_t)max_rows * 2), ids(max_rows + guard), events(P * ep::kEventWords + guard),
      pieces(P * ep::kPieceWords + guard);
  std::vector<float> score_slots(ep::kSumSlots, 1e30f);
  ep::ScalarSum score{score_slots.data()};
  size_t at = 0;                      // next wanted event
  int fed = 0, covered = 0;           // rows consumed; rows the pieces have tiled
  bool pending_reset = false, first_step = true, done = false;
  std::vector<int> open_ids;          // ids of the open stretch so far
  while (!done) {
    int n = limit - fed < cut ? limit - fed : cut;
    const bool last_rows = fed + n >= limit;
    bool finishing = last_rows && !finish_apart;
    if (last_rows && finish_apart && n == 0) finishing = true;
    const int offered = n + (finishing ? (T - fed - n < extra ? T - fed - n : extra) : 0);
    for (int j = 0; j < offered; ++j) { rows[2 * j] = 0; rows[2 * j + 1] = fed + j; }
    const int tab[4] = {0, offered, finishing ? limit : -1, first_step ? 1 : 0};
    std::fill(ids.begin(), ids.end(), -77);
    std::fill(events.begin(), events.end(), -77);
    std::fill(pieces.begin(), pieces.end(), -77);
    int new_count = -77;
    float neg = NAN;
    const float* base = logits.data() + (size_t)fed * pitch;
    auto argmax = [&](int r, int& kk, float& vv) {
      const float* x = base + (size_t)r * pitch;
      kk = 0; vv = x[0];
      for (int c = 1; c < C; ++c)
        if (x[c] > vv) { vv = x[c]; kk = c; }
    };
    ep::walk(prm, tab, rows.data(), argmax, true, state.data(), score, ids.data(), max_rows, &new_count, &neg, events.data(), pieces.data(),
             ep::kPieceWords, P);
    for (int g = 0; g < guard; ++g)
      if (ids[max_rows + g] != -77 || events[P * ep::kEventWords + g] != -77 || pieces[P * ep::kPieceWords + g] != -77)
        return fail("a write behind the outputs", fed, g);
    // events: the next ones of the whole-stream list; ids and sums per stretch
    int id_at = 0, n_events = 0;
    for (int e = 0; e < P && events[e * 8] != 0; ++e, ++n_events) {
      const int* ev = &events[e * 8];
      if (at >= want.size()) return fail("an event too many", fed, e);
      const Event& w = want[at++];
      if (ev[0] != w.kind || ev[1] != w.u0 || ev[2] != w.end || ev[3] != w.first || ev[4] != w.last || ev[7] != w.index)
        return fail("event fields", w.u0, w.end);
      for (; id_at < ev[5]; ++id_at) open_ids.push_back(ids[id_at]);
      if (open_ids != w.ids) return fail("ids of a stretch", w.u0, w.end);
      float got;
      memcpy(&got, &ev[6], 4);
      if (memcmp(&got, &w.neg_sum, 4) != 0) return fail("sum of a stretch", w.u0, w.end);
      open_ids.clear();
      ++counts[w.kind];
    }
    if (n_events > P) return fail("more events than slots", n_events, P);
    for (; id_at < new_count; ++id_at) open_ids.push_back(ids[id_at]);
    // pieces: adjacent, in order, inside the step's consumed rows; reset after every event; the limit where a final ends
    int next_row = 0, e = 0;
    bool reset_due = first_step || pending_reset;
    pending_reset = false;
    for (int p = 0; p < P; ++p) {
      const int* q = &pieces[p * 4];
      if (q[0] == 0 && q[1] == 0 && q[2] == -1 && q[3] == 0) continue;
      if (q[1] > 0 && q[0] != next_row) return fail("pieces are not adjacent", p, q[0]);
      if (q[1] < 0 || next_row + q[1] > n) return fail("a piece outside the consumed rows", p, q[1]);
      if (q[3] != (reset_due ? 1 : 0)) return fail("reset flag of a piece", p, q[3]);
      reset_due = false;
      next_row += q[1];
      if (e < n_events && events[e * 8 + 2] == fed + next_row && (q[1] > 0 || q[2] >= 0)) {   // this piece ends a stretch
        const int kind = events[e * 8];
        if (q[2] != (kind == ep::EV_DISCARD ? -1 : events[e * 8 + 2])) return fail("limit of a closing piece", p, q[2]);
        ++e;
        reset_due = kind != ep::EV_END;
      } else if (q[2] != -1) {
        return fail("limit of an open piece", p, q[2]);
      }
    }
    if (next_row != n) return fail("pieces do not tile the consumed rows", next_row, n);
    if (e < n_events && !(events[e * 8] == ep::EV_DISCARD && finishing)) return fail("an event without its piece", e, n_events);
    pending_reset = reset_due && !finishing;
    if (pending_reset) return fail("a reset left for the next step", fed, n);      // (the walk hands it over as a piece without rows)
    covered += next_row;
    fed += n;
    first_step = false;
    done = finishing;
    if (state[7] != fed) return fail("rows consumed in the record", state[7], fed);
  }
  if (at != want.size()) return fail("events missing", (int)at, (int)want.size());
  if (covered != limit) return fail("rows covered", covered, limit);
  return 0;
}

int main() {
  long counts[5] = {0, 0, 0, 0, 0}, streams = 0;
  const int Rs[3] = {1, 2, 5}, Ls[3] = {1, 3, 7}, Cs[4] = {2, 5, 29, 32}, cuts[5] = {1, 2, 7, 10, 80};
  for (int R : Rs)
    for (int L : Ls)
      for (int M : {L, 9, 40}) {
        if (M < L) continue;
        for (int C : Cs)
          for (int space : {-1, C - 2}) {
            if (space >= 0 && C == 2) continue;
            for (int cut : cuts)
              for (int apart = 0; apart < 2; ++apart) {
                if (check_stream(C, space, R, L, M, 60 + (int)(rnd() % 60), cut, apart != 0, counts)) {
                  printf("  at R=%d L=%d M=%d C=%d space=%d cut=%d apart=%d\n", R, L, M, C, space, cut, apart);
                  return 1;
                }
                ++streams;
              }
          }
      }
  printf("checked %ld streams; events 1/2/3/4: %ld %ld %ld %ld\n", streams, counts[1], counts[2], counts[3], counts[4]);
  if (counts[1] < 100 || counts[2] < 100 || counts[3] < 100 || counts[4] < 100) { printf("too few events of a kind\n"); return 1; }
  printf("all cuts agree\n");
  return 0;
}
