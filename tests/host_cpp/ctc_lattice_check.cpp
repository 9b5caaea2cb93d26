// Exhaustive host check of the host-usable half of speecht_amd/csrc/ctc_lattice.h: the states-per-lane dispatch list, the
// state predicates (class, skip from below, skip to above) and the refusal rule, each against a direct restatement of its
// definition.  Built from the header alone and run by tests/test_ctc_lattice_host.py with g++.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ctc_lattice.h"

static unsigned rng_state = 12345u;
static unsigned rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

#define CHECK(c, ...) do { if (!(c)) { printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

static int check_kpl() {
  const int list[] = {1, 2, 3, 4, 5, 6, 8, 10, 12, 16};
  for (int L = -1; L <= 512; ++L) {
    int want = -1;
    if (L >= 0) for (int k : list) if (64 * k >= 2 * L + 1) { want = k; break; }
    CHECK(st::lattice_kpl(L) == want, "lattice_kpl(%d) = %d, want %d", L, st::lattice_kpl(L), want);
    CHECK((L >= 0 && L <= 511) == (want > 0), "list does not cover L = %d", L);
    int got = -1, calls = 0;
    st::dispatch_kpl(want, [&](auto k) { got = k(); ++calls; });
    CHECK(want < 0 ? calls == 0 : (calls == 1 && got == want), "dispatch_kpl(%d) reached %d, %d times", want, got, calls);
  }
  return 0;
}

static int check_string(const std::vector<int>& lab, int blank) {
  const int L = (int)lab.size(), U = 2 * L + 1;
  for (int u = 0; u < U; ++u) {
    const bool label = u % 2 == 1;
    const int i = u / 2;                                      // label index of an odd state
    const int cls = label ? lab[i] : blank;
    const bool below = label && i >= 1 && lab[i] != lab[i - 1];
    const bool above = label && i + 1 < L && lab[i + 1] != lab[i];
    CHECK(st::lattice_class(u, lab.data(), blank) == cls, "class of state %d (L %d)", u, L);
    CHECK(st::lattice_skip_from_below(u, lab.data()) == below, "skip from below of state %d (L %d)", u, L);
    CHECK(st::lattice_skip_to_above(u, U, lab.data()) == above, "skip to above of state %d (L %d)", u, L);
  }
  int rep = 0;
  for (int i = 1; i < L; ++i) rep += lab[i] == lab[i - 1];
  const int fit = L + rep, UP = 64 * st::lattice_kpl(L);
  for (int Tb : {0, fit - 1, fit, fit + 1, fit + 70}) {
    if (Tb < 0) continue;
    const int T = fit + 70;
    CHECK(st::lattice_refused(L, rep, Tb, T, UP) == (fit > Tb), "refused(L %d, rep %d, Tb %d)", L, rep, Tb);
  }
  CHECK(st::lattice_refused(L, rep, fit + 1, fit, UP), "Tb > T accepted");
  CHECK(st::lattice_refused(L, rep, -1, fit + 70, UP), "Tb < 0 accepted");
  if (UP > 64) CHECK(st::lattice_refused(L, rep, fit, fit, UP - 64) == (U > UP - 64), "U > UP (L %d)", L);
  return 0;
}

int main() {
  if (check_kpl()) return 1;
  CHECK(!st::lattice_refused(0, 0, 0, 5, 64), "the empty label over no frames is valid");
  CHECK(st::lattice_refused(-1, 0, 5, 5, 64) && st::lattice_refused(-3, 0, 0, 5, 1024), "a negative label length is refused");
  const st_tensor3 t{nullptr, 3, 50, 29, 2, 60, 32};
  const st::RowMap m = st::row_map(t);
  CHECK(m.off(0, 0) == 2 * 32 && m.off(2, 7) == (2L * 60 + 2 + 7) * 32, "row_map");
  int n = 0;
  for (int symbols : {2, 3, 28})
    for (int k : {1, 2, 3, 4, 5, 6, 8, 10, 12, 16})
      for (int rep = 0; rep < 10; ++rep) {
        // a label that fills dispatch k (shorter ones in later repeats), repeats forced at the labels of the lane-crossing states
        const int L = rep == 0 ? 32 * k - 1 : (int)(rnd() % (32 * k));
        std::vector<int> lab(L);
        for (int& v : lab) v = (int)(rnd() % symbols);
        for (int j = 1; j < 64; ++j)
          for (int d : {-1, 1}) {
            const int i = (k * j + d) / 2;             // label of state k j +- 1, either side of a lane edge
            if (i >= 1 && i < L) lab[i] = lab[i - 1];
          }
        if (check_string(lab, symbols)) { printf("FAILED symbols=%d k=%d rep=%d\n", symbols, k, rep); return 1; }
        ++n;
      }
  if (check_string({}, 28) || check_string({5}, 28) || check_string({5, 5}, 28)) return 1;
  printf("checked lattice_kpl for L = -1..512 and %d label strings\n", n + 3);
  return 0;
}
