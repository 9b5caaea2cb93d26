// st_spec_augment_host / st_spec_augment_plan_host as a stand-alone program (its own main, no device): the lengths around the
// warp's threshold, a single frame, a single utterance, 13 channels, masks wider than the utterance, eight masks of each kind and
// bad arguments, into destination buffers with not one float to spare, for a run under the address and undefined-behaviour
// sanitizers (tests/test_spec_augment_host.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "speecht_hip.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static std::vector<float> noise(size_t n, unsigned seed) {
  std::vector<float> x(n);
  for (auto& v : x) { seed = seed * 1664525u + 1013904223u; v = ((seed >> 8) % 2000) / 250.f - 4.f + 0.001f; }
  return x;
}

struct Policy { int W, F, mF, T, mT, q; };

// one batch through the host form into an exactly sized padded buffer; checks what must hold whatever was drawn
static int run(int B, int T, int C, const std::vector<int32_t>& lens, const Policy& p, uint64_t seed, int halo, int tail, long* zeros) {
  const int c_pitch = (C + 15) / 16 * 16, t_pitch = halo + T + tail, words = 2 + 2 * (p.mF + p.mT);
  std::vector<float> x = noise((size_t)B * T * C, (unsigned)(seed + T));
  std::vector<float> out((size_t)B * t_pitch * c_pitch, 7.f);
  std::vector<int64_t> ids(B);
  for (int b = 0; b < B; ++b) ids[b] = (int64_t)(0x9E3779B97F4A7C15ull * (uint64_t)(b + 1) + seed);
  std::vector<int32_t> plan((size_t)B * words, -7), plan2((size_t)B * words, -7);
  st_tensor3 dst = {out.data(), B, T, C, halo, t_pitch, c_pitch};
  CHECK(st_spec_augment_host(x.data(), B, T, C, lens.data(), ids.data(), seed, p.W, p.F, p.mF, p.T, p.mT, p.q, &dst, plan.data()) == 0);
  CHECK(st_spec_augment_plan_host(lens.data(), ids.data(), B, C, seed, p.W, p.F, p.mF, p.T, p.mT, p.q, plan2.data()) == 0);
  CHECK(plan == plan2);
  for (int b = 0; b < B; ++b) {
    const int32_t* pl = &plan[(size_t)b * words];
    const int L = lens[b];
    const bool warps = p.W > 0 && L >= 2 * p.W + 2;
    if (warps) CHECK(pl[0] >= p.W + 1 && pl[0] <= L - p.W - 1 && pl[1] >= -p.W && pl[1] <= p.W);
    else CHECK(pl[0] == 0 && pl[1] == 0);
    for (int k = 0; k < p.mF; ++k) CHECK(pl[2 + 2 * k] >= 0 && pl[3 + 2 * k] >= 0 && pl[3 + 2 * k] <= p.F && pl[2 + 2 * k] + pl[3 + 2 * k] <= C);
    for (int k = 0; k < p.mT; ++k) {
      const int32_t* m = pl + 2 + 2 * p.mF + 2 * k;
      CHECK(m[0] >= 0 && m[1] >= 0 && m[1] <= p.T && m[1] <= (int)(((int64_t)p.q * L) >> 16) && m[0] + m[1] <= L);
    }
    for (int r = 0; r < t_pitch; ++r)
      for (int c = 0; c < c_pitch; ++c) {
        const float v = out[((size_t)b * t_pitch + r) * c_pitch + c];
        const int t = r - halo;
        if (t < 0 || t >= T || c >= C) { CHECK(v == 7.f); continue; }                    // halo rows and pad channels: not touched
        CHECK(std::isfinite(v) && std::fabs(v) <= 4.01f);                                // a value between two source values, or 0
        if (t >= L) CHECK(v == x[((size_t)b * T + t) * C + c]);
        else if (!warps && v != 0.f) CHECK(v == x[((size_t)b * T + t) * C + c]);
        if (v == 0.f) ++*zeros;
      }
  }
  return 0;
}

int main() {
  long zeros = 0;
  const Policy ld_small = {4, 5, 2, 6, 2, 65536}, warp = {4, 0, 0, 0, 0, 65536}, masks = {0, 5, 8, 6, 8, 65536};
  const Policy wide = {3, 1000, 8, 1000, 8, 65536}, tiny_ratio = {2, 3, 1, 50, 3, 655}, none = {0, 0, 0, 0, 0, 65536};
  int cases = 0;
  for (const Policy& p : {ld_small, warp, masks, wide, tiny_ratio, none})
    for (int C : {80, 13, 128, 1}) {
      const int W = p.W;
      // lengths 1, 2, 2W+1, 2W+2, 2W+3 and the whole padded length in one batch
      const std::vector<int32_t> lens = {1, 2, 2 * W + 1, 2 * W + 2, 2 * W + 3, 37, 0};
      if (run(7, 37, C, lens, p, 1000 + cases, 3, 2, &zeros)) return 1;
      if (run(1, 37, C, {20}, p, 2000 + cases, 0, 0, &zeros)) return 1;            // B = 1, no halo at all
      if (run(2, 1, C, {1, 0}, p, 3000 + cases, 1, 0, &zeros)) return 1;           // T = 1
      cases += 3;
    }
  CHECK(zeros > 1000);
  {
    // the identity policy is the copy; bad arguments are refused and write nothing
    const int B = 2, T = 5, C = 13;
    std::vector<float> x = noise((size_t)B * T * C, 5), out((size_t)B * T * 16, 7.f);
    std::vector<int32_t> lens = {5, 3}, plan(B * 34, -7);
    std::vector<int64_t> ids = {1, 2};
    st_tensor3 dst = {out.data(), B, T, C, 0, T, 16};
    CHECK(st_spec_augment_host(x.data(), B, T, C, lens.data(), ids.data(), 1, 0, 0, 0, 0, 0, 0, &dst, nullptr) == 0);
    for (int b = 0; b < B; ++b)
      for (int t = 0; t < T; ++t) CHECK(std::memcmp(&out[((size_t)b * T + t) * 16], &x[((size_t)b * T + t) * C], C * sizeof(float)) == 0);
    std::vector<float> before = out;
    lens[1] = 6;
    CHECK(st_spec_augment_host(x.data(), B, T, C, lens.data(), ids.data(), 1, 1, 1, 1, 1, 1, 65536, &dst, plan.data()) != 0);
    lens[1] = -1;
    CHECK(st_spec_augment_host(x.data(), B, T, C, lens.data(), ids.data(), 1, 1, 1, 1, 1, 1, 65536, &dst, plan.data()) != 0);
    CHECK(st_spec_augment_plan_host(lens.data(), ids.data(), B, C, 1, 1, 1, 1, 1, 1, 65536, plan.data()) != 0);
    lens[1] = 3;
    CHECK(st_spec_augment_host(x.data(), B, T, C, lens.data(), ids.data(), 1, 1, 1, 9, 1, 1, 65536, &dst, plan.data()) != 0);
    CHECK(st_spec_augment_host(x.data(), B, T, C, lens.data(), ids.data(), 1, 1, 1, 1, 1, 9, 65536, &dst, plan.data()) != 0);
    CHECK(st_spec_augment_host(x.data(), B, T, C, lens.data(), ids.data(), 1, -1, 1, 1, 1, 1, 65536, &dst, plan.data()) != 0);
    CHECK(st_spec_augment_host(x.data(), B, T, C, lens.data(), ids.data(), 1, 1, 1, 1, 1, 1, 65537, &dst, plan.data()) != 0);
    CHECK(st_spec_augment_host(x.data(), 0, T, C, lens.data(), ids.data(), 1, 1, 1, 1, 1, 1, 65536, &dst, plan.data()) != 0);
    CHECK(st_spec_augment_host(x.data(), B, T, 12, lens.data(), ids.data(), 1, 1, 1, 1, 1, 1, 65536, &dst, plan.data()) != 0);
    CHECK(st_spec_augment_host(nullptr, B, T, C, lens.data(), ids.data(), 1, 1, 1, 1, 1, 1, 65536, &dst, plan.data()) != 0);
    CHECK(st_spec_augment_f32(x.data(), B, T, C, lens.data(), ids.data(), 1, 1, 1, 9, 1, 1, 65536, &dst, plan.data(), nullptr) != 0);
    CHECK(out == before);
    for (int32_t v : plan) CHECK(v == -7);
  }
  printf("checked %d batches through the host form\n", cases);
  return 0;
}
