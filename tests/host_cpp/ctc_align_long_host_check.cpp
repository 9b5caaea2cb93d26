// st_ctc_align_long_host as a stand-alone program (its own main, no device): small cases, an empty label, a label that does not
// fit, bad arguments and one label across two state blocks, for a run under the address and undefined-behaviour sanitizers
// (tests/test_ctc_align_long_host.py).
#include <cmath>
#include <cstdio>
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

int main() {
  const int C = 29;
  {
    // "3 3 _ 4" planted on frames 2 .. 5 of 12, read from rows of pitch 32
    const int T = 12, L = 3, pitch = 32;
    std::vector<float> x = noise((size_t)T * pitch, 1);
    for (int t = 0; t < T; ++t) x[(size_t)t * pitch + C - 1] = 10.f;
    const int planted[4] = {3, 3, C - 1, 3};
    for (int i = 0; i < 4; ++i) x[(size_t)(2 + i) * pitch + planted[i]] = 30.f;
    x[(size_t)8 * pitch + 4] = 30.f;
    std::vector<int32_t> ids = {3, 3, 4}, spans(2 * L + 2, -7);
    double score = 7.0;
    int32_t status = -7;
    const size_t need = st_ctc_align_long_ws(T, L);
    CHECK(need == (size_t)T * (256 + 224) + 2 * (896 + 128) * 8 + 512);
    std::vector<double> ws(need / 8);
    CHECK(st_ctc_align_long_host(x.data(), T, C, pitch, ids.data(), L, spans.data(), &score, &status, ws.data(), need) == 0);
    CHECK(status == 0 && std::isfinite(score) && score < 0.0 && spans[6] == -7 && spans[7] == -7);
    CHECK(spans[0] == 2 && spans[1] == 4 && spans[2] == 5 && spans[3] == 6 && spans[4] == 8 && spans[5] == 9);
    // an empty label: no spans, no ids
    score = 7.0;
    CHECK(st_ctc_align_long_host(x.data(), T, C, pitch, nullptr, 0, spans.data(), &score, &status, ws.data(), need) == 0);
    CHECK(status == 0 && std::isfinite(score) && spans[0] == 2);
    // two frames for "3 3": one short
    CHECK(st_ctc_align_long_host(x.data(), 2, C, pitch, ids.data(), 2, spans.data(), &score, &status, ws.data(), need) == 0);
    CHECK(status == 1 && std::isinf(score) && spans[0] == -1 && spans[3] == -1 && spans[4] == 8);
    CHECK(st_ctc_align_long_host(x.data(), 3, C, pitch, ids.data(), 2, spans.data(), &score, &status, ws.data(), need) == 0);
    CHECK(status == 0 && spans[0] == 0 && spans[3] == 3);
    // bad arguments
    CHECK(st_ctc_align_long_host(nullptr, T, C, pitch, ids.data(), L, spans.data(), &score, &status, ws.data(), need) != 0);
    CHECK(st_ctc_align_long_host(x.data(), T, C, pitch, nullptr, L, spans.data(), &score, &status, ws.data(), need) != 0);
    CHECK(st_ctc_align_long_host(x.data(), T, C, pitch, ids.data(), L, spans.data(), &score, &status, nullptr, need) != 0);
    CHECK(st_ctc_align_long_host(x.data(), T, C, pitch, ids.data(), L, spans.data(), &score, &status, ws.data(), need - 8) != 0);
    CHECK(st_ctc_align_long_host(x.data(), T, C, pitch, ids.data(), L, spans.data(), &score, &status, ws.data() + 1, need) != 0);
    CHECK(st_ctc_align_long_host(x.data(), T, 33, 64, ids.data(), L, spans.data(), &score, &status, ws.data(), need) != 0);
    CHECK(st_ctc_align_long_host(x.data(), T, 1, pitch, ids.data(), L, spans.data(), &score, &status, ws.data(), need) != 0);
    CHECK(st_ctc_align_long_host(x.data(), T, C, C - 1, ids.data(), L, spans.data(), &score, &status, ws.data(), need) != 0);
    CHECK(st_ctc_align_long_host(x.data(), 0, C, pitch, ids.data(), L, spans.data(), &score, &status, ws.data(), need) != 0);
    CHECK(st_ctc_align_long_host(x.data(), T, C, pitch, ids.data(), -1, spans.data(), &score, &status, ws.data(), need) != 0);
    CHECK(st_ctc_align_long_host(x.data(), T, C, pitch, ids.data(), 1 << 20, spans.data(), &score, &status, ws.data(), need) != 0);
    CHECK(st_ctc_align_long_ws(0, 3) == 0 && st_ctc_align_long_ws(5, -1) == 0 && st_ctc_align_long_ws(5, 1 << 20) == 0);
  }
  {
    // one label across two state blocks (1 201 states), with repeats around state 896, on the fewest frames and on more
    const int L = 600;
    std::vector<int32_t> ids;
    for (int i = 0; i < L; ++i) ids.push_back((i * 5) % 28);
    ids[447] = ids[448] = ids[449];
    int rep = 0;
    for (int i = 1; i < L; ++i) rep += ids[i] == ids[i - 1];
    CHECK(rep == 2);
    for (int T : {L + rep, 900}) {
      std::vector<float> x = noise((size_t)T * C, 2 + T);
      std::vector<int32_t> spans(2 * L);
      double score = 7.0;
      int32_t status = -7;
      const size_t need = st_ctc_align_long_ws(T, L);
      CHECK(need == (size_t)T * (256 + 2 * 224) + 2 * (2 * 896 + 128) * 8 + 512);
      std::vector<double> ws(need / 8, -1.0);
      CHECK(st_ctc_align_long_host(x.data(), T, C, C, ids.data(), L, spans.data(), &score, &status, ws.data(), need) == 0);
      CHECK(status == 0 && std::isfinite(score) && score < 0.0 && ordered(spans, L, T));
      CHECK(spans[2 * 448] > spans[2 * 447 + 1] && spans[2 * 449] > spans[2 * 448 + 1]);     // a blank between the repeats
      if (T == L + rep) CHECK(spans[0] == 0 && spans[2 * L - 1] == T);
    }
    CHECK(st_ctc_align_long_ws(L + rep - 1, L) > 0);
    printf("checked a label of %d ids across two state blocks\n", L);
  }
  return 0;
}
