// st_ctc_follow_stream_host as a stand-alone program (its own main, no device): the sizes, bad arguments, a planted script whose
// cursor and events are known in closed form, a script of 1 000 ids (three state blocks) fed in uneven steps against one step per
// 64 rows -- trace, events, record and state bytes --, slots that sit out, a buffer of one event and a script longer than the state,
// for a run under the address and undefined-behaviour sanitizers (tests/test_follow_host.py).  Every buffer is exactly as large as
// the contract says, so a write or a read outside one is the sanitizer's to find.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "speecht_hip.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static std::vector<float> noise(size_t n, unsigned seed) {
  std::vector<float> x(n);
  for (auto& v : x) { seed = seed * 1664525u + 1013904223u; v = ((seed >> 8) % 2000) / 500.f - 2.f; }
  return x;
}

struct Out {
  std::vector<int> trace;
  std::vector<std::pair<int, int>> events;
  std::vector<int32_t> record;
  std::vector<char> state;
  long lost = 0;
};

// one stream (slot `slot` of `slots`, the others without a script) of T rows [T][C] fed in steps of the sizes `cuts` cycles through
static int run(const std::vector<int32_t>& script, const std::vector<int32_t>& starts, int C, const std::vector<float>& x, int T,
               const std::vector<int>& cuts, int K, int max_events, int max_labels, int slots, int slot, Out& out) {
  const size_t sb = st_ctc_follow_stream_state_bytes(max_labels);
  CHECK(sb > 0 && sb % 16 == 0);
  const int max_rows = *std::max_element(cuts.begin(), cuts.end());
  const size_t wb = st_ctc_follow_stream_ws(std::max(max_rows, 1), max_labels, slots);
  CHECK(wb > 0);
  std::vector<double> state(sb * slots / 8), work(wb / 8);
  std::memset(state.data(), 0x5A, sb * slots);
  std::vector<int32_t> offs(slots + 1, 0), woffs(slots + 1, 0);
  for (int s = slot + 1; s <= slots; ++s) { offs[s] = (int32_t)script.size(); woffs[s] = (int32_t)starts.size(); }
  std::vector<int32_t> events((size_t)slots * max_events * 2), result((size_t)slots * 16);
  int at = 0;
  for (size_t i = 0; at < T; ++i) {
    const int n = std::min(cuts[i % cuts.size()], T - at);
    std::vector<int32_t> rows, table((size_t)slots * 4, 0), trace(std::max(n, 1), -9);
    for (int s = 0; s < slots; ++s) table[4 * s + 2] = -1;
    for (int r = 0; r < std::max(n, 1); ++r) { rows.push_back(slot); rows.push_back(at + r); }
    table[4 * slot] = 0; table[4 * slot + 1] = n; table[4 * slot + 3] = at == 0;
    std::vector<float> step(x.begin() + (size_t)at * C, x.begin() + (size_t)(at + n) * C);
    if (step.empty()) step.assign(C, 0.f);
    CHECK(st_ctc_follow_stream_host(step.data(), C, C, rows.data(), table.data(), n, std::max(max_rows, 1), n, slots, script.data(),
                                    offs.data(), starts.data(), woffs.data(), max_labels, K, state.data(), events.data(), max_events,
                                    result.data(), trace.data(), work.data(), wb) == 0);
    const int32_t* rec = &result[16 * (size_t)slot];
    CHECK(rec[0] == at + n && rec[2] == 0 && rec[3] >= 0);
    for (int s = 0; s < slots; ++s)
      if (s != slot) CHECK(result[16 * (size_t)s + 2] == 2 && result[16 * (size_t)s + 1] == -1);
    for (int r = 0; r < n; ++r) out.trace.push_back(trace[r]);
    for (int e = 0; e < std::min(rec[3], max_events); ++e)
      out.events.push_back({events[((size_t)slot * max_events + e) * 2], events[((size_t)slot * max_events + e) * 2 + 1]});
    out.lost += std::max(rec[3] - max_events, 0);
    out.record.assign(rec, rec + 16);
    at += n;
  }
  const char* base = reinterpret_cast<const char*>(state.data());
  out.state.assign(base + sb * slot, base + sb * (slot + 1));
  for (int s = 0; s < slots; ++s)
    if (s != slot)
      for (size_t b = 0; b < sb; ++b) CHECK(base[sb * s + b] == 0x5A);          // a slot without a script keeps its state
  return 0;
}

int main() {
  const int C = 29, SPACE = 27;
  {
    CHECK(st_ctc_follow_stream_state_bytes(1) == 128 + 2 * (896 + 128) * 8 && st_ctc_follow_stream_state_bytes(448) == 128 + 2 * (2 * 896 + 128) * 8);
    CHECK(st_ctc_follow_stream_state_bytes(0) == 0 && st_ctc_follow_stream_state_bytes(28672) == 0 && st_ctc_follow_stream_state_bytes(28671) > 0);
    CHECK(st_ctc_follow_stream_ws(10, 1000, 3) == 10 * 256 + 3 * 64 * 3 * 16 + 3 * 32 + 256 && st_ctc_follow_stream_ws(0, 1, 1) == 0);
  }
  {
    // a planted script without adjacent repeats, one new label per frame: the cursor is 2 t + 1, word j is reached at a_j + K - 1
    const int L = 90, K = 5;
    std::vector<int32_t> script, starts;
    for (int i = 0; i < L; ++i) script.push_back(i % 6 == 5 ? SPACE : (i * 7) % 26);
    for (int i = 0; i < L; ++i)
      if (script[i] != SPACE && (i == 0 || script[i - 1] == SPACE)) starts.push_back(i);
    for (int i = 1; i < L; ++i) CHECK(script[i] != script[i - 1]);
    std::vector<float> x = noise((size_t)L * C, 5);
    for (int t = 0; t < L; ++t) x[(size_t)t * C + script[t]] += 30.f;
    Out whole, cut, one;
    if (run(script, starts, C, x, L, {L}, K, 64, L, 1, 0, whole)) return 1;
    if (run(script, starts, C, x, L, {1, 7, 0, 3}, K, 64, L, 3, 1, cut)) return 1;
    for (int t = 0; t < L; ++t) CHECK(whole.trace[t] == 2 * t + 1);
    size_t e = 0;
    for (size_t j = 0; j < starts.size(); ++j)
      if (starts[j] + K - 1 < L) { CHECK(e < whole.events.size() && whole.events[e] == std::make_pair((int)j, starts[j] + K - 1)); ++e; }
    CHECK(e == whole.events.size() && whole.lost == 0);
    CHECK(cut.trace == whole.trace && cut.events == whole.events && cut.state == whole.state);
    CHECK(std::equal(cut.record.begin() + 4, cut.record.end(), whole.record.begin() + 4) && whole.record[1] == 2 * L - 1);
    // a buffer of one event: the count is true, the rest is lost, nothing is written behind the buffer
    if (run(script, starts, C, x, L, {L}, K, 1, L, 1, 0, one)) return 1;
    CHECK(one.events.size() == 1 && one.lost == (long)whole.events.size() - 1 && one.state == whole.state);
    // a script longer than the state was sized for: a status, the state untouched
    std::vector<double> state(st_ctc_follow_stream_state_bytes(10) / 8), work(st_ctc_follow_stream_ws(L, 10, 1) / 8);
    std::memset(state.data(), 0x5A, state.size() * 8);
    std::vector<int32_t> rows, ev(2), res(16), offs = {0, L}, woffs = {0, (int32_t)starts.size()};
    for (int r = 0; r < L; ++r) { rows.push_back(0); rows.push_back(r); }
    const int32_t table[4] = {0, L, -1, 1};
    auto step = [&](int classes, int max_labels, int confirm, int max_events, int n_rows, int longest, const void* st) {
      return st_ctc_follow_stream_host(x.data(), C, classes, rows.data(), table, n_rows, L, longest, 1, script.data(), offs.data(),
                                       starts.data(), woffs.data(), max_labels, confirm, const_cast<void*>(st), ev.data(), max_events,
                                       res.data(), nullptr, work.data(), work.size() * 8);
    };
    CHECK(step(C, 10, K, 1, L, L, state.data()) == 0 && res[2] == 1 && res[1] == -1 && res[3] == 0);
    for (size_t b = 0; b < state.size() * 8; ++b) CHECK(reinterpret_cast<const char*>(state.data())[b] == 0x5A);
    // bad arguments
    CHECK(step(1, 10, K, 1, L, L, state.data()) != 0 && step(33, 10, K, 1, L, L, state.data()) != 0 && step(C, 0, K, 1, L, L, state.data()) != 0);
    CHECK(step(C, 10, 0, 1, L, L, state.data()) != 0 && step(C, 10, 17, 1, L, L, state.data()) != 0 && step(C, 10, K, 0, L, L, state.data()) != 0);
    CHECK(step(C, 10, K, 1, L + 1, L, state.data()) != 0 && step(C, 10, K, 1, L, L + 1, state.data()) != 0 && step(C, 10, K, 1, L, L, nullptr) != 0);
  }
  {
    // 1 000 ids with repeats over 1 300 noisy rows that spell the script loosely: three state blocks, uneven steps of up to 130 rows
    const int L = 1000, T = 1300, K = 3;
    std::vector<int32_t> script, starts;
    unsigned seed = 9;
    for (int i = 0; i < L; ++i) { seed = seed * 1664525u + 1013904223u; script.push_back(i % 7 == 6 ? SPACE : (int)((seed >> 10) % 26)); }
    for (int i = 0; i < L; ++i)
      if (script[i] != SPACE && (i == 0 || script[i - 1] == SPACE)) starts.push_back(i);
    std::vector<float> x = noise((size_t)T * C, 6);
    for (int t = 0; t < T; ++t) {
      const int u = (int)((long)t * (2 * L) / T);
      x[(size_t)t * C + ((u & 1) ? script[u / 2] : C - 1)] += 4.f;
    }
    Out a, b;
    if (run(script, starts, C, x, T, {64}, K, 512, L, 1, 0, a)) return 1;
    if (run(script, starts, C, x, T, {130, 1, 65, 0, 7, 128}, K, 512, L, 2, 1, b)) return 1;
    CHECK(a.trace == b.trace && a.events == b.events && a.state == b.state && !a.events.empty() && a.lost == 0);
    CHECK(std::equal(a.record.begin() + 4, a.record.end(), b.record.begin() + 4) && a.record[1] == b.record[1]);
    CHECK(*std::max_element(a.trace.begin(), a.trace.end()) > 1792);   // the cursor reaches the third block
    printf("checked a script of %d ids on %d frames in uneven steps\n", L, T);
  }
  return 0;
}
