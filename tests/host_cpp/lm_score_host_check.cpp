// st_lm_score_prefixes_host as a stand-alone program (its own main, no device): no prefixes, a pitch above every length, ids
// outside 0..27, the longest prefix and models of orders 1 and 5, for a run under the address and undefined-behaviour sanitizers
// (tests/test_lm_score_host.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "speecht_hip.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static const char* kOrder1 =
    "\\data\\\nngram 1=6\n\n\\1-grams:\n-1.0\t</s>\n-99\t<s>\n-2.0\t<unk>\n-0.5\tthe\n-0.75\tcat\n-1.5\tit's\n\n\\end\\\n";

// an order-5 model over {a, b, ab}: every order holds one n-gram that continues the one below, with backoffs on the way
static const char* kOrder5 =
    "\\data\\\nngram 1=6\nngram 2=3\nngram 3=2\nngram 4=1\nngram 5=1\n\n"
    "\\1-grams:\n-1.0\t</s>\n-99\t<s>\t-0.25\n-2.0\t<unk>\t-0.125\n-0.5\ta\t-0.5\n-0.75\tb\t-0.375\n-1.25\tab\t-0.0625\n\n"
    "\\2-grams:\n-0.25\t<s> a\t-0.5\n-0.375\ta b\t-0.25\n-0.625\tb </s>\n\n"
    "\\3-grams:\n-0.125\t<s> a b\t-0.75\n-0.3125\ta b ab\t-0.125\n\n"
    "\\4-grams:\n-0.0625\t<s> a b ab\t-1.0\n\n"
    "\\5-grams:\n-0.03125\t<s> a b ab a\n\n\\end\\\n";

static std::vector<int32_t> ids_of(const char* text) {
  std::vector<int32_t> v;
  for (const char* c = text; *c; ++c) v.push_back(*c == ' ' ? 27 : (*c == '\'' ? 26 : *c - 'a'));
  return v;
}

int main() {
  char err[256];
  void *lm1 = nullptr, *lm5 = nullptr;
  CHECK(st_lm_create_arpa(kOrder1, strlen(kOrder1), &lm1, err, sizeof err) == 0);
  CHECK(st_lm_create_arpa(kOrder5, strlen(kOrder5), &lm5, err, sizeof err) == 0);
  {
    // n = 0: valid, nothing is read or written (null outputs)
    CHECK(st_lm_score_prefixes_host(lm1, nullptr, 1, nullptr, 0, nullptr, nullptr, nullptr) == 0);
    CHECK(st_lm_score_prefixes_host(nullptr, nullptr, 1, nullptr, 0, nullptr, nullptr, nullptr) != 0);
    CHECK(st_lm_score_prefixes_host(lm1, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr) != 0);
  }
  {
    // order 1, pitch > len: the ids beyond a prefix's length (poisoned here) are never read
    const char* texts[] = {"", "the cat", " the", "the  cat", "the cat ", "zq", "it's", " "};
    const int n = 8, pitch = 12;
    std::vector<int32_t> ids((size_t)n * pitch, 1 << 30), lens(n);
    for (int i = 0; i < n; ++i) {
      std::vector<int32_t> v = ids_of(texts[i]);
      lens[i] = (int32_t)v.size();
      for (size_t k = 0; k < v.size(); ++k) ids[(size_t)i * pitch + k] = v[k];
    }
    std::vector<double> g(n + 1, 7.0);
    std::vector<int32_t> nw(n + 1, -7), nv(n + 1, -7);
    CHECK(st_lm_score_prefixes_host(lm1, ids.data(), pitch, lens.data(), n, g.data(), nw.data(), nv.data()) == 0);
    CHECK(g[n] == 7.0 && nw[n] == -7 && nv[n] == -7);
    const double want_g[8] = {-1.0, -2.25, -3.5, -4.25, -2.25, -3.0, -2.5, -3.0};
    const int want_w[8] = {0, 2, 2, 3, 2, 1, 1, 1}, want_v[8] = {0, 2, 1, 2, 2, 0, 1, 0};
    for (int i = 0; i < n; ++i) CHECK(g[i] == want_g[i] && nw[i] == want_w[i] && nv[i] == want_v[i]);
    // a bad id inside a prefix's length: ST_EINVAL, nothing written; a length outside 0..pitch likewise
    std::vector<double> g2(n, 7.0);
    for (int32_t bad : {28, -1, 1 << 30}) {
      std::vector<int32_t> ids2 = ids;
      ids2[(size_t)3 * pitch + 2] = bad;
      CHECK(st_lm_score_prefixes_host(lm1, ids2.data(), pitch, lens.data(), n, g2.data(), nw.data(), nv.data()) != 0);
      CHECK(g2[0] == 7.0 && g2[n - 1] == 7.0);
    }
    std::vector<int32_t> lens2 = lens;
    lens2[5] = pitch + 1;
    CHECK(st_lm_score_prefixes_host(lm1, ids.data(), pitch, lens2.data(), n, g2.data(), nw.data(), nv.data()) != 0);
    lens2[5] = -1;
    CHECK(st_lm_score_prefixes_host(lm1, ids.data(), pitch, lens2.data(), n, g2.data(), nw.data(), nv.data()) != 0);
    CHECK(st_lm_score_prefixes_host(lm1, ids.data(), pitch, lens.data(), n, nullptr, nw.data(), nv.data()) != 0);
  }
  {
    // order 5: the context grows to four words and then drops its oldest; every backoff level is walked
    const char* texts[] = {"a b ab a", "a b ab a b", "b", "ab ab"};
    const int n = 4, pitch = 16;
    std::vector<int32_t> ids((size_t)n * pitch, -9), lens(n);
    for (int i = 0; i < n; ++i) {
      std::vector<int32_t> v = ids_of(texts[i]);
      lens[i] = (int32_t)v.size();
      for (size_t k = 0; k < v.size(); ++k) ids[(size_t)i * pitch + k] = v[k];
    }
    std::vector<double> g(n);
    std::vector<int32_t> nw(n), nv(n);
    CHECK(st_lm_score_prefixes_host(lm5, ids.data(), pitch, lens.data(), n, g.data(), nw.data(), nv.data()) == 0);
    // <s> a | <s> a b | <s> a b ab | <s> a b ab a | </s> after (a b ab a): no 5-gram, no 4-gram context listed -> unigram + bo(a)
    CHECK(g[0] == -0.25 + -0.125 + -0.0625 + -0.03125 + (-1.0 + -0.5));
    CHECK(nw[0] == 4 && nv[0] == 4 && nw[1] == 5 && nw[2] == 1 && nw[3] == 2 && nv[3] == 2);
    // b | <s>: bo(<s>) + p(b); </s> | <s> b: the bigram (b </s>)
    CHECK(g[2] == (-0.75 + -0.25) + -0.625);
    CHECK(std::isfinite(g[1]) && std::isfinite(g[3]));
  }
  {
    // the longest prefix a beam search can return on 30 s of audio (1 501 output frames), alone and with a pitch to match
    const int L = 1501;
    std::vector<int32_t> ids(L), len = {L};
    for (int i = 0; i < L; ++i) ids[i] = (i % 4 == 3) ? 27 : (i % 3);
    double g1 = 0, g5 = 0;
    int32_t nw = 0, nv = 0;
    CHECK(st_lm_score_prefixes_host(lm1, ids.data(), L, len.data(), 1, &g1, &nw, &nv) == 0);
    CHECK(nw == 376 && nv == 0 && g1 == -2.0 * 376 - 1.0);
    CHECK(st_lm_score_prefixes_host(lm5, ids.data(), L, len.data(), 1, &g5, &nw, &nv) == 0);
    CHECK(nw == 376 && std::isfinite(g5) && g5 < 0.0);
    printf("checked a prefix of %d ids at orders 1 and 5\n", L);
  }
  CHECK(st_lm_destroy(lm1) == 0 && st_lm_destroy(lm5) == 0);
  return 0;
}
