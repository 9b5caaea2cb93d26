// st_ctc_spot_host as a stand-alone program (its own main, no device): small batches, jobs outside the tables, bad arguments and
// the longest keyword the lattice holds, for a run under the address and undefined-behaviour sanitizers
// (tests/test_ctc_spot_host.py).
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

int main() {
  const int C = 29;
  {
    const int B = 3, T = 12;
    std::vector<float> x = noise((size_t)B * T * C, 1);
    // utterance 1 reads "3 3 _ 4" on frames 2 .. 5
    const int planted[4] = {3, 3, C - 1, 4};
    for (int i = 0; i < 4; ++i) x[((size_t)1 * T + 2 + i) * C + planted[i]] = 20.f;
    for (int i = 0; i < 3; ++i) x[((size_t)1 * T + 6 + i) * C + 7] = 20.f;
    x[((size_t)1 * T + 1) * C + 9] = 20.f;
    std::vector<int32_t> ids = {3, 4, 5, 5, 5, 5, 5, 5, 5, 6}, offs = {0, 2, 9, 10, 10}, lens = {12, 9, 0};
    // the pairs of utterances 0 and 1, then no frames, an empty keyword, a keyword that needs 13 frames, and pairs outside the tables
    std::vector<int32_t> jobs = {0, 0, 0, 2, 1, 0, 1, 2, 2, 0, 0, 3, 0, 1, 3, 0, -1, 0, 0, 4, 0, -1, 1, 0};
    const int J = (int)jobs.size() / 2;
    std::vector<double> score(J + 1, 7.0), trv((size_t)(J + 1) * T, 7.0);
    std::vector<int32_t> span(2 * (J + 1), -7), status(J + 1, -7), trs((size_t)(J + 1) * T, -7);
    const size_t need = st_ctc_spot_ws(B, T, 7, J);
    CHECK(need == (size_t)B * T * 256 + 512);
    std::vector<double> ws(need / 8);
    CHECK(st_ctc_spot_host(x.data(), B, T, C, lens.data(), ids.data(), offs.data(), 4, 7, jobs.data(), J, score.data(), span.data(),
                           trv.data(), trs.data(), status.data(), ws.data(), need) == 0);
    CHECK(score[J] == 7.0 && span[2 * J] == -7 && status[J] == -7 && trv[(size_t)J * T] == 7.0 && trs[(size_t)J * T] == -7);
    const int want_status[12] = {0, 0, 0, 0, 0, 1, 0, 1, 1, 1, 1, 0};
    for (int j = 0; j < J; ++j) CHECK(status[j] == want_status[j]);
    for (int j : {0, 1, 2, 3, 11}) CHECK(std::isfinite(score[j]) && score[j] <= 0.0 && span[2 * j] >= 0 && span[2 * j] < span[2 * j + 1]);
    CHECK(score[2] == 0.0 && span[4] == 2 && span[5] == 6 && score[11] == 0.0);
    for (int j : {4, 5, 6, 7, 8, 9, 10}) CHECK(std::isinf(score[j]) && span[2 * j] == -1 && span[2 * j + 1] == -1);
    for (int t = 0; t < T; ++t) {
      CHECK(std::isinf(trv[(size_t)5 * T + t]) && trs[(size_t)5 * T + t] == -1);
      if (t >= 9) CHECK(std::isinf(trv[(size_t)2 * T + t]) && trs[(size_t)2 * T + t] == -1);
    }
    CHECK(trv[(size_t)2 * T + 5] == 0.0 && trs[(size_t)2 * T + 5] == 2);
    // without the trace: the same results
    std::vector<double> score2(J, 7.0);
    std::vector<int32_t> span2(2 * J, -7);
    CHECK(st_ctc_spot_host(x.data(), B, T, C, lens.data(), ids.data(), offs.data(), 4, 7, jobs.data(), J, score2.data(), span2.data(),
                           nullptr, nullptr, status.data(), ws.data(), need) == 0);
    for (int j = 0; j < J; ++j) CHECK((score2[j] == score[j]) && span2[2 * j] == span[2 * j] && span2[2 * j + 1] == span[2 * j + 1]);
    // no jobs; then bad arguments
    CHECK(st_ctc_spot_host(x.data(), B, T, C, lens.data(), ids.data(), offs.data(), 4, 7, nullptr, 0, nullptr, nullptr, nullptr, nullptr,
                           nullptr, ws.data(), need) == 0);
    CHECK(st_ctc_spot_host(x.data(), B, T, C, lens.data(), ids.data(), offs.data(), 4, 7, jobs.data(), J, score.data(), span.data(),
                           trv.data(), trs.data(), status.data(), ws.data(), need - 8) != 0);
    CHECK(st_ctc_spot_host(x.data(), B, T, 33, lens.data(), ids.data(), offs.data(), 4, 7, jobs.data(), J, score.data(), span.data(),
                           trv.data(), trs.data(), status.data(), ws.data(), need) != 0);
    CHECK(st_ctc_spot_host(x.data(), B, T, C, lens.data(), ids.data(), offs.data(), 4, 0, jobs.data(), J, score.data(), span.data(),
                           trv.data(), trs.data(), status.data(), ws.data(), need) != 0);
    CHECK(st_ctc_spot_host(x.data(), B, T, C, lens.data(), ids.data(), offs.data(), 4, 512, jobs.data(), J, score.data(), span.data(),
                           trv.data(), trs.data(), status.data(), ws.data(), need) != 0);
    CHECK(st_ctc_spot_host(x.data(), B, T, C, lens.data(), ids.data(), offs.data(), 4, 7, jobs.data(), J, score.data(), span.data(),
                           trv.data(), nullptr, status.data(), ws.data(), need) != 0);
    CHECK(st_ctc_spot_ws(B, T, 512, J) == 0 && st_ctc_spot_ws(B, T, 0, J) == 0 && st_ctc_spot_ws(B, 0, 7, J) == 0);
  }
  {
    // a keyword of 511 ids on 1 200 frames, its lattice lengths wild and sane, and ids outside the classes
    const int T = 1200, L = 511;
    std::vector<float> x = noise((size_t)2 * T * C, 2);
    std::vector<int32_t> ids, offs = {0, L, L + 3}, lens = {T, 1300}, jobs = {0, 0, 1, 0, 0, 1};
    for (int i = 0; i < L; ++i) ids.push_back((i * 5) % 28);
    ids.push_back(-5); ids.push_back(1 << 30); ids.push_back(31);
    std::vector<double> score(3), trv((size_t)3 * T);
    std::vector<int32_t> span(6), status(3), trs((size_t)3 * T);
    const size_t need = st_ctc_spot_ws(2, T, L, 3);
    std::vector<double> ws(need / 8);
    CHECK(st_ctc_spot_host(x.data(), 2, T, C, lens.data(), ids.data(), offs.data(), 2, L, jobs.data(), 3, score.data(), span.data(),
                           trv.data(), trs.data(), status.data(), ws.data(), need) == 0);
    CHECK(status[0] == 0 && status[1] == 1 && status[2] == 0);
    CHECK(std::isfinite(score[0]) && score[0] < 0.0 && span[0] >= 0 && span[1] - span[0] >= L && span[1] <= T);
    int finite = 0;
    for (int t = 0; t < T; ++t) finite += std::isfinite(trv[t]);
    CHECK(finite == T - (L - 1));
    printf("checked a keyword of %d ids on %d frames\n", L, T);
  }
  return 0;
}
