// st_ctc_spot_stream_plan / st_ctc_spot_stream_host as a stand-alone program (its own main, no device): the packed layouts, bad
// arguments, small streams fed in steps under both packings, and a keyword of 511 ids over a few hundred frames in uneven steps,
// for a run under the address and undefined-behaviour sanitizers (tests/test_ctc_spot_stream_host.py).  Every buffer is exactly
// as large as the contract says, so a write or a read outside one is the sanitizer's to find.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <set>
#include <tuple>
#include <vector>

#include "speecht_hip.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

typedef std::vector<std::vector<int32_t>> Keywords;
typedef std::set<std::tuple<int, int, int, int, long long>> Events;

static std::vector<float> noise(size_t n, unsigned seed) {
  std::vector<float> x(n);
  for (auto& v : x) { seed = seed * 1664525u + 1013904223u; v = ((seed >> 8) % 2000) / 500.f - 2.f; }
  return x;
}

struct Plan {
  std::vector<int32_t> words;
  int n_waves = 0;
  bool ok = false;
};

static Plan make_plan(const Keywords& kws, int C, int pack) {
  std::vector<int32_t> ids = {}, offs = {0};
  for (auto& k : kws) { ids.insert(ids.end(), k.begin(), k.end()); offs.push_back((int32_t)ids.size()); }
  ids.push_back(0);
  Plan p;
  const size_t bytes = st_ctc_spot_stream_plan_bytes(ids.data(), offs.data(), (int)kws.size(), C, pack);
  if (!bytes) return p;
  p.words.resize(bytes / 4);
  p.ok = st_ctc_spot_stream_plan(ids.data(), offs.data(), (int)kws.size(), C, pack, p.words.data(), &p.n_waves) == 0;
  return p;
}

// one stream of T rows [T][C], fed in steps of the sizes `cuts` cycles through, the last of them with the limit: all its events
static int run(const Plan& p, int C, const std::vector<float>& x, int T, const std::vector<int>& cuts, double threshold, int hold,
               int max_events, Events& out, long& lost) {
  const size_t sb = st_ctc_spot_stream_state_bytes(p.words.data());
  CHECK(sb > 0 && sb % 8 == 0);
  std::vector<double> state(sb / 8);
  std::memset(state.data(), 0x5A, sb);
  std::vector<int32_t> events((size_t)max_events * 8), counts(1);
  lost = 0;
  int at = 0;
  for (size_t i = 0;; ++i) {
    const int n = std::min(cuts[i % cuts.size()], T - at);
    std::vector<int32_t> rows;
    for (int r = 0; r < std::max(n, 1); ++r) { rows.push_back(0); rows.push_back(at + r); }
    const int32_t table[4] = {0, n, at + n == T ? T : -1, at == 0};
    std::vector<float> step(x.begin() + (size_t)at * C, x.begin() + (size_t)(at + n) * C);
    if (step.empty()) step.push_back(0.f);
    counts[0] = -7;
    CHECK(st_ctc_spot_stream_host(step.data(), C, C, rows.data(), table, n, 1, p.words.data(), threshold, hold, state.data(),
                                  events.data(), max_events, counts.data()) == 0);
    CHECK(counts[0] >= 0);
    for (int e = 0; e < std::min(counts[0], max_events); ++e) {
      const int32_t* w = &events[(size_t)e * 8];
      long long bits;
      std::memcpy(&bits, w + 4, 8);
      CHECK(w[6] == 0 && w[7] == 0 && (w[3] == 0 || w[3] == 1) && w[1] >= 0 && w[1] < w[2] && w[2] <= T);
      CHECK(out.insert(std::make_tuple(w[0], w[1], w[2], w[3], bits)).second);
    }
    lost += std::max(counts[0] - max_events, 0);
    at += n;
    if (at >= T) return 0;
  }
}

int main() {
  const int C = 29;
  const double ninf = -std::numeric_limits<double>::infinity();
  {
    // the layouts: the header {magic, words, keywords, classes, KPL, waves, pack, first word of the keyword entries}, per wave the
    // descriptors [KPL][64] and the lanes' keywords [64], per keyword {wave, first state, L, 0}
    Plan a = make_plan({std::vector<int32_t>(31, 1)}, C, 1);
    CHECK(a.ok && a.n_waves == 1 && a.words[4] == 1 && a.words[16 + 64 + 61] == 0 && a.words[16 + 64 + 62] == -1);
    Plan b = make_plan({std::vector<int32_t>(31, 1), {2}}, C, 1);
    CHECK(b.ok && b.n_waves == 2 && b.words[b.words[7] + 4] == 1 && b.words[b.words[7] + 5] == 0);
    Plan c = make_plan({std::vector<int32_t>(32, 1)}, C, 1);
    CHECK(c.ok && c.n_waves == 1 && c.words[4] == 2);
    Keywords ones;
    for (int k = 0; k < 21; ++k) ones.push_back({k});
    Plan d = make_plan(ones, C, 1);
    CHECK(d.ok && d.n_waves == 1 && d.words[d.words[7] + 4 * 20 + 1] == 60 && d.words[16 + 64 + 61] == 20);
    ones.push_back({5});
    Plan d1 = make_plan(ones, C, 1), d0 = make_plan(ones, C, 0);
    CHECK(d1.ok && d1.n_waves == 2 && d0.ok && d0.n_waves == 22);
    // "aa": a (enter), the blank between (live, compulsory: the second a has no skip over it), a (end), dead around them
    Plan e = make_plan({{0, 0}}, C, 1);
    CHECK(e.ok && e.words[16] == C - 1 && e.words[17] == (0 | 64 | 128) && e.words[18] == ((C - 1) | 64) && e.words[19] == (0 | 64 | 256));
    CHECK(e.words[20] == C - 1 && e.words[16 + 64 + 3] == 0 && e.words[16 + 64 + 2] == -1);
    // refused: ids outside the labels, empty and too long keywords, offsets that go back, bad classes and pack
    CHECK(!make_plan({{C - 1}}, C, 1).ok && !make_plan({{-1}}, C, 1).ok && !make_plan({{1}, {}}, C, 1).ok);
    CHECK(!make_plan({std::vector<int32_t>(512, 1)}, C, 1).ok && make_plan({std::vector<int32_t>(511, 1)}, C, 1).ok);
    CHECK(!make_plan({{1}}, 33, 1).ok && !make_plan({{0}}, 1, 1).ok && !make_plan({{1}}, C, 2).ok && !make_plan({}, C, 1).ok);
    const int32_t ids[3] = {1, 2, 3}, back[3] = {0, 2, 1};
    int nw = 0;
    std::vector<int32_t> out(4096);
    CHECK(st_ctc_spot_stream_plan_bytes(ids, back, 2, C, 1) == 0 && st_ctc_spot_stream_plan(ids, back, 2, C, 1, out.data(), &nw) != 0);
    CHECK(st_ctc_spot_stream_plan(ids, nullptr, 2, C, 1, out.data(), &nw) != 0 && st_ctc_spot_stream_plan(nullptr, back, 2, C, 1, out.data(), &nw) != 0);
    CHECK(st_ctc_spot_stream_state_bytes(out.data()) == 0 && st_ctc_spot_stream_plan_bind(out.data(), out.data()) != 0);
    CHECK(st_ctc_spot_stream_state_bytes(a.words.data()) == 64 * 32 && st_ctc_spot_stream_state_bytes(c.words.data()) == 64 * 44);
  }
  {
    // small streams under both packings and three cuttings: the same events; a planted reading scores exactly 0 on its span
    const int T = 97;
    const Keywords kws = {{2, 0, 19}, {0}, {7, 7}, {19, 7, 4, 27, 2, 0, 19}};
    std::vector<float> x = noise((size_t)T * C, 3);
    const int planted[5] = {7, C - 1, 7, 7, C - 1};
    for (int i = 0; i < 5; ++i) x[(size_t)(40 + i) * C + planted[i]] = 30.f;
    x[(size_t)39 * C + C - 1] = 30.f;                                // (a blank in front as well: the span is the reading's own)
    Events first;
    for (int pack = 0; pack < 2; ++pack) {
      Plan p = make_plan(kws, C, pack);
      CHECK(p.ok && p.n_waves == (pack ? 1 : 4));
      for (auto& cuts : std::vector<std::vector<int>>{{T}, {1}, {5, 0, 31, 2}}) {
        Events got;
        long lost;
        if (run(p, C, x, T, cuts, ninf, 3, 512, got, lost)) return 1;
        CHECK(lost == 0 && !got.empty());
        if (first.empty()) first = got;
        CHECK(got == first);
      }
      Events exact;
      long lost;
      if (run(p, C, x, T, {9}, 0.0, 2, 8, exact, lost)) return 1;
      CHECK(lost == 0 && exact.count(std::make_tuple(2, 40, 44, 0, 0LL)) == 1);
      // a buffer of one event: the count is true, the rest is lost, nothing is written behind the buffer
      Events one;
      if (run(p, C, x, T, {T}, ninf, 3, 1, one, lost)) return 1;
      CHECK(one.size() == 1 && lost == (long)first.size() - 1);
    }
    // bad arguments of the step
    Plan p = make_plan(kws, C, 1);
    std::vector<double> state(st_ctc_spot_stream_state_bytes(p.words.data()) / 8);
    std::vector<int32_t> events(8), counts(1), rows = {0, 0};
    const int32_t table[4] = {0, 1, -1, 1};
    auto step = [&](const void* plan, int classes, double thr, int hold, int max_events) {
      return st_ctc_spot_stream_host(x.data(), C, classes, rows.data(), table, 1, 1, plan, thr, hold, state.data(), events.data(), max_events,
                                     counts.data());
    };
    CHECK(step(p.words.data(), C, -0.69, 1, 1) == 0);
    CHECK(step(p.words.data(), C, std::nan(""), 1, 1) != 0 && step(p.words.data(), C, 0.1, 1, 1) != 0 && step(p.words.data(), C, -0.69, 0, 1) != 0);
    CHECK(step(p.words.data(), C, -0.69, 1, 0) != 0 && step(p.words.data(), C - 1, -0.69, 1, 1) != 0 && step(nullptr, C, -0.69, 1, 1) != 0);
    std::vector<int32_t> forged = p.words;
    forged[0] += 1;
    CHECK(step(forged.data(), C, -0.69, 1, 1) != 0);
    forged = p.words;
    forged[5] += 1;                                                  // more waves than the block holds
    CHECK(step(forged.data(), C, -0.69, 1, 1) != 0);
  }
  {
    // a keyword of 511 ids (16 states per lane) and a short one beside it over 700 frames whose arg-max spells the long one
    // (threshold 0: only exact readings count -- a looser one lets a worse reading that ends sooner win, as the rule is causal)
    const int T = 700, L = 511;
    Keywords kws(2);
    for (int i = 0; i < L; ++i) kws[0].push_back((i * 5) % 28);
    kws[1] = {5, 10};
    std::vector<float> x = noise((size_t)T * C, 4);
    for (int i = 0; i < L; ++i) x[(size_t)(100 + i) * C + kws[0][i]] = 30.f;
    x[(size_t)99 * C + C - 1] = x[(size_t)(100 + L) * C + C - 1] = 30.f;
    Events a, b;
    long lost;
    Plan p1 = make_plan(kws, C, 1), p0 = make_plan(kws, C, 0);
    CHECK(p1.ok && p0.ok && p1.words[4] == 16 && p1.n_waves == 2 && p0.n_waves == 2);
    if (run(p1, C, x, T, {T}, 0.0, 10, 64, a, lost)) return 1;
    if (run(p0, C, x, T, {37, 1, 200, 0, 3}, 0.0, 10, 64, b, lost)) return 1;
    CHECK(a == b && a.count(std::make_tuple(0, 100, 100 + L, 0, 0LL)) == 1);
    printf("checked a keyword of %d ids on %d frames in uneven steps\n", L, T);
  }
  return 0;
}
