// st_ctc_word_conf_host as a stand-alone program (its own main, no device): small and wild inputs and the largest label the
// lattice holds, for a run under the address and undefined-behaviour sanitizers (tests/test_ctc_conf_host.py).
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
  const int C = 29, S = 27;
  {
    const int B = 3, T = 12;
    std::vector<float> x = noise((size_t)B * T * C, 1);
    std::vector<int32_t> ids = {1, 2, S, 3, 3, 4, 4, 4, S, 5, 6, S, 7}, offs = {0, 5, 10, 13}, lens = {12, 4, 9};
    // the words of utterances 0, 1 (refused) and 2, then spans that are no word runs, outside their label or the batch
    std::vector<int32_t> spans = {0, 0, 2, 0, 3, 5, 1, 0, 3, 1, 4, 5, 2, 0, 1, 2, 2, 3, 0, 3, 2, 0, -1, 2, 0, 0, 6, 7, 0, 1, -1, 0, 1, 0, 2, 3};
    const int W = (int)spans.size() / 3;
    std::vector<double> lp(B + 1, 7.0), lc(W + 1, 7.0);
    std::vector<int32_t> st(B + 1, -7);
    const size_t need = st_ctc_word_conf_ws(B, T, 5, B + W);
    CHECK(need == (size_t)B * T * 256 + (size_t)(B + W) * 8 + 512);
    std::vector<double> ws(need / 8);
    CHECK(st_ctc_word_conf_host(x.data(), B, T, C, ids.data(), offs.data(), lens.data(), 5, S, spans.data(), W, lp.data(), lc.data(),
                                st.data(), ws.data(), need) == 0);
    CHECK(st[0] == 0 && st[1] == 1 && st[2] == 0 && st[3] == -7 && lp[3] == 7.0 && lc[W] == 7.0);
    CHECK(std::isfinite(lp[0]) && lp[0] < 0 && std::isinf(lp[1]) && std::isfinite(lp[2]));
    for (int w : {0, 1, 4, 5}) CHECK(std::isfinite(lc[w]) && lc[w] <= 0.0);
    for (int w : {2, 3, 6, 7, 8, 9, 10}) CHECK(std::isnan(lc[w]));
    CHECK(st_ctc_word_conf_host(x.data(), B, T, C, ids.data(), offs.data(), lens.data(), 5, S, spans.data(), W, lp.data(), lc.data(),
                                st.data(), ws.data(), need - 8) != 0);
    CHECK(st_ctc_word_conf_host(x.data(), B, T, 31, ids.data(), offs.data(), lens.data(), 5, S, spans.data(), W, lp.data(), lc.data(),
                                st.data(), ws.data(), need) != 0);
    CHECK(st_ctc_word_conf_host(x.data(), B, T, C, ids.data(), offs.data(), lens.data(), 5, 28, spans.data(), W, lp.data(), lc.data(),
                                st.data(), ws.data(), need) != 0);
  }
  {
    // 511 labels on 1 200 frames: words of seven letters
    const int T = 1200, L = 511;
    std::vector<float> x = noise((size_t)T * C, 2);
    std::vector<int32_t> ids, offs = {0, L}, lens = {T}, spans;
    for (int i = 0; i < L; ++i) ids.push_back(i % 8 == 7 ? S : (i * 5) % 26);
    for (int i = 0; i < L; i += 8) { spans.push_back(0); spans.push_back(i); spans.push_back(i + 7 < L ? i + 7 : L); }
    const int W = (int)spans.size() / 3;
    std::vector<double> lp(1), lc(W);
    std::vector<int32_t> st(1);
    const size_t need = st_ctc_word_conf_ws(1, T, L, 1 + W);
    std::vector<double> ws(need / 8);
    CHECK(st_ctc_word_conf_host(x.data(), 1, T, C, ids.data(), offs.data(), lens.data(), L, S, spans.data(), W, lp.data(), lc.data(),
                                st.data(), ws.data(), need) == 0);
    CHECK(st[0] == 0 && std::isfinite(lp[0]));
    for (int w = 0; w < W; ++w) CHECK(std::isfinite(lc[w]) && lc[w] <= 0.0);
    printf("checked %d words of a label of %d ids\n", W, L);
  }
  return 0;
}
