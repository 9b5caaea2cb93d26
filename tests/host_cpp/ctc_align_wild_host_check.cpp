// st_ctc_align_wild_host and st_ctc_align_long_wild_host as a stand-alone program (its own main, no device): small cases, a
// wildcard at each end, bad arguments, and one label of 600 ids across two state blocks with a wildcard on the block edge, for a
// run under the address and undefined-behaviour sanitizers (tests/test_ctc_align_wild_host.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "speecht_hip.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static std::vector<float> noise(size_t n, unsigned seed) {
  std::vector<float> x(n);
  for (auto& v : x) { seed = seed * 1664525u + 1013904223u; v = ((seed >> 8) % 2000) / 250.f - 4.f; }
  return x;
}

// the spans are runs in label order that do not overlap, inside [0, T]
static bool ordered(const std::vector<int32_t>& sp, int L, int T) {
  int prev = 0;
  for (int k = 0; k < L; ++k) {
    if (sp[2 * k] < prev || sp[2 * k + 1] <= sp[2 * k] || sp[2 * k + 1] > T) return false;
    prev = sp[2 * k + 1];
  }
  return true;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main() {
  const int C = 29, W = C;
  {
    // 20 frames: "3 4" planted on frames 2 .. 5, then frames 8 .. 13 spell ids the transcript leaves out, then "5" on 16 .. 17
    const int T = 20, pitch = 32;
    std::vector<float> x = noise((size_t)T * pitch, 1);
    for (int t = 0; t < T; ++t) x[(size_t)t * pitch + C - 1] = 10.f;
    const int cls[20] = {-1, -1, 3, 3, 4, 4, -1, -1, 7, 7, 8, 9, 9, 10, -1, -1, 5, 5, -1, -1};
    for (int t = 0; t < T; ++t) if (cls[t] >= 0) x[(size_t)t * pitch + cls[t]] = 30.f;
    std::vector<float> dense((size_t)T * C);
    for (int t = 0; t < T; ++t) for (int c = 0; c < C; ++c) dense[(size_t)t * C + c] = x[(size_t)t * pitch + c];
    std::vector<int32_t> ids = {3, 4, W, 5}, offs = {0, 4}, lens = {T};
    const int L = 4;
    std::vector<int32_t> spans(2 * L + 2, -7), states(T, -7), lspans(2 * L + 2, -7);
    std::vector<double> fit(L + 1, 7.0), lfit(L + 1, 7.0);
    float score = 7.f;
    double lscore = 7.0;
    int32_t status = -7, lstatus = -7;
    const size_t need = st_ctc_align_ws(1, T, L), lneed = st_ctc_align_long_ws(T, L);
    std::vector<double> ws(need / 8 + 1), lws(lneed / 8 + 1);
    CHECK(st_ctc_align_wild_host(dense.data(), 1, T, C, ids.data(), offs.data(), lens.data(), L, -1.0, spans.data(), states.data(),
                                 &score, &status, fit.data(), ws.data(), need) == 0);
    CHECK(status == 0 && std::isfinite(score) && spans[8] == -7 && fit[4] == 7.0);
    CHECK(spans[0] == 2 && spans[1] == 4 && spans[2] == 4 && spans[3] == 6 && spans[4] == 8 && spans[5] == 14 && spans[6] == 16 &&
          spans[7] == 18);
    CHECK(fit[0] == 0.0 && fit[1] == 0.0 && fit[2] == -6.0 && fit[3] == 0.0);
    CHECK(states[0] == -1 && states[2] == 0 && states[9] == 2 && states[17] == 3 && states[19] == -1);
    CHECK(st_ctc_align_long_wild_host(x.data(), T, C, pitch, ids.data(), L, -1.0, lspans.data(), &lscore, &lstatus, lfit.data(),
                                      lws.data(), lneed) == 0);
    CHECK(lstatus == 0 && (float)lscore == score && lspans[8] == -7 && lfit[4] == 7.0);
    for (int i = 0; i < 2 * L; ++i) CHECK(lspans[i] == spans[i]);
    for (int i = 0; i < L; ++i) CHECK(same_bits(lfit[i], fit[i]));
    // a wildcard at each end, the fit left out; then on the fewest frames (one per label), where every span is one frame
    std::vector<int32_t> ends = {W, 3, 4, W}, eoffs = {0, 4};
    CHECK(st_ctc_align_wild_host(dense.data(), 1, T, C, ends.data(), eoffs.data(), lens.data(), 4, -0.5, spans.data(), nullptr,
                                 &score, &status, nullptr, ws.data(), need) == 0);
    CHECK(status == 0 && spans[0] >= 0 && spans[1] == spans[0] + 1 && spans[1] <= 2 && spans[2] == 2 && spans[5] == 6);
    CHECK(spans[6] == 8 && spans[7] == 18);          // everything the transcript does not read, the planted "5" included
    std::vector<int32_t> four = {4};
    CHECK(st_ctc_align_wild_host(dense.data(), 1, T, C, ends.data(), eoffs.data(), four.data(), 4, -0.5, spans.data(), states.data(),
                                 &score, &status, fit.data(), ws.data(), need) == 0);
    CHECK(status == 0 && spans[0] == 0 && spans[1] == 1 && spans[6] == 3 && spans[7] == 4 && fit[0] == -0.5 && fit[3] == -0.5);
    CHECK(states[4] == -2 && states[T - 1] == -2);
    // one frame short once the wildcards count: refused, NaN fits
    std::vector<int32_t> three = {3};
    CHECK(st_ctc_align_wild_host(dense.data(), 1, T, C, ends.data(), eoffs.data(), three.data(), 4, -0.5, spans.data(), states.data(),
                                 &score, &status, fit.data(), ws.data(), need) == 0);
    CHECK(status == 1 && std::isinf(score) && spans[0] == -1 && spans[7] == -1 && std::isnan(fit[0]) && std::isnan(fit[3]) &&
          fit[4] == 7.0 && states[0] == -2);
    CHECK(st_ctc_align_long_wild_host(x.data(), 3, C, pitch, ends.data(), 4, -0.5, lspans.data(), &lscore, &lstatus, lfit.data(),
                                      lws.data(), lneed) == 0);
    CHECK(lstatus == 1 && std::isinf(lscore) && lspans[0] == -1 && std::isnan(lfit[3]) && lfit[4] == 7.0);
    // an empty label
    CHECK(st_ctc_align_long_wild_host(x.data(), T, C, pitch, nullptr, 0, -1.0, lspans.data(), &lscore, &lstatus, lfit.data(), lws.data(),
                                      lneed) == 0);
    CHECK(lstatus == 0 && std::isfinite(lscore));
    // bad arguments
    std::vector<int32_t> twice = {3, W, W, 5}, outside = {3, C + 1, 4, 5};
#define BATCH(IDS, CLASSES, BIAS, WS, NEED) \
  st_ctc_align_wild_host(dense.data(), 1, T, CLASSES, IDS, offs.data(), lens.data(), L, BIAS, spans.data(), states.data(), &score, \
                         &status, fit.data(), WS, NEED)
#define LONG(IDS, CLASSES, BIAS, WS, NEED) \
  st_ctc_align_long_wild_host(x.data(), T, CLASSES, pitch, IDS, L, BIAS, lspans.data(), &lscore, &lstatus, lfit.data(), WS, NEED)
    CHECK(BATCH(ids.data(), C, -1.0, ws.data(), need) == 0 && LONG(ids.data(), C, -1.0, lws.data(), lneed) == 0);
    CHECK(BATCH(twice.data(), C, -1.0, ws.data(), need) != 0 && LONG(twice.data(), C, -1.0, lws.data(), lneed) != 0);
    CHECK(BATCH(outside.data(), C, -1.0, ws.data(), need) != 0 && LONG(outside.data(), C, -1.0, lws.data(), lneed) != 0);
    CHECK(BATCH(ids.data(), 32, -1.0, ws.data(), need) != 0 && LONG(ids.data(), 32, -1.0, lws.data(), lneed) != 0);
    CHECK(BATCH(ids.data(), 1, -1.0, ws.data(), need) != 0 && LONG(ids.data(), 1, -1.0, lws.data(), lneed) != 0);
    CHECK(BATCH(ids.data(), C, 0.5, ws.data(), need) != 0 && LONG(ids.data(), C, 0.5, lws.data(), lneed) != 0);
    CHECK(BATCH(ids.data(), C, std::nan(""), ws.data(), need) != 0 && LONG(ids.data(), C, std::nan(""), lws.data(), lneed) != 0);
    CHECK(BATCH(ids.data(), C, -INFINITY, ws.data(), need) != 0 && LONG(ids.data(), C, -INFINITY, lws.data(), lneed) != 0);
    CHECK(BATCH(nullptr, C, -1.0, ws.data(), need) != 0 && LONG(nullptr, C, -1.0, lws.data(), lneed) != 0);
    CHECK(BATCH(ids.data(), C, -1.0, nullptr, need) != 0 && LONG(ids.data(), C, -1.0, nullptr, lneed) != 0);
    CHECK(BATCH(ids.data(), C, -1.0, ws.data(), need - 8) != 0 && LONG(ids.data(), C, -1.0, lws.data(), lneed - 8) != 0);
    CHECK(BATCH(ids.data(), C, 0.0, ws.data(), need) == 0 && LONG(ids.data(), C, 0.0, lws.data(), lneed) == 0);
  }
  {
    // one label across two state blocks (1 201 states): state 895 is id 447, the last state the first block owns, and a wildcard;
    // equal ids on both sides of it; on the fewest frames and on more
    const int L = 600;
    std::vector<int32_t> ids;
    for (int i = 0; i < L; ++i) ids.push_back((i * 5) % 28);
    ids[447] = W;
    ids[446] = ids[448];
    ids[100] = W;
    ids[599] = W;
    int rep = 0;
    for (int i = 1; i < L; ++i) rep += ids[i] == ids[i - 1];
    CHECK(rep == 0);
    for (int T : {L, 900}) {
      std::vector<float> x = noise((size_t)T * C, 2 + T);
      std::vector<int32_t> spans(2 * L);
      std::vector<double> fit(L, 7.0);
      double score = 7.0;
      int32_t status = -7;
      const size_t need = st_ctc_align_long_ws(T, L);
      CHECK(need == (size_t)T * (256 + 2 * 224) + 2 * (2 * 896 + 128) * 8 + 512);
      std::vector<double> ws(need / 8, -1.0);
      CHECK(st_ctc_align_long_wild_host(x.data(), T, C, C, ids.data(), L, -1.0, spans.data(), &score, &status, fit.data(), ws.data(),
                                        need) == 0);
      CHECK(status == 0 && std::isfinite(score) && score < 0.0 && ordered(spans, L, T));
      for (int k : {100, 447, 599}) CHECK(fit[k] == -1.0 * (spans[2 * k + 1] - spans[2 * k]));
      for (int k = 0; k < L; ++k) CHECK(fit[k] <= 0.0);
      if (T == L) CHECK(spans[0] == 0 && spans[2 * L - 1] == T && spans[2 * 447] == 447 && fit[447] == -1.0);
      if (T == 900) CHECK(spans[2 * 100 + 1] - spans[2 * 100] + spans[2 * 447 + 1] - spans[2 * 447] + spans[2 * 599 + 1] -
                              spans[2 * 599] > 3);                     // noise: the wildcards soak up frames no label reads
    }
    printf("checked a label of %d ids across two state blocks with a wildcard on the block edge\n", L);
  }
  return 0;
}
