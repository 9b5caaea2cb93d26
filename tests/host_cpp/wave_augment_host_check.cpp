// st_wave_augment_host / st_wave_augment_plan_host as a stand-alone program (its own main, no device): utterances of 1, 2, 2H - 1,
// 255, 256, 257, 513, 3 001 and 70 000 samples at six speeds and the three-speed policy, with and without a bank of clips of 1, 700
// and 50 000 samples, into input, output and bank buffers with not one float to spare, and bad arguments -- for a run under the
// address and undefined-behaviour sanitizers (tests/test_wave_augment_host.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "speecht_hip.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

struct Plan {                                          // the record of include/speecht_hip.h
  int64_t M, offset;
  double lin;
  int32_t speed, noisy, clip, snr_centi;
};
static_assert(sizeof(Plan) == 40, "plan record");

static std::vector<float> noise(size_t n, unsigned seed) {
  std::vector<float> x(n);
  for (auto& v : x) { seed = seed * 1664525u + 1013904223u; v = ((seed >> 8) % 2000) / 1000.f - 1.f + 0.0005f; }
  return x;
}

static int half_width(int num, int den) { return num <= den ? 16 : (16 * num + den - 1) / den; }

// any table of the right shape will do here: a Hann-windowed sinc with rows that sum to one
static void append_table(std::vector<float>& t, int num, int den) {
  const int H = half_width(num, den);
  const double fc = 0.85 * (num > den ? (double)den / num : 1.0), pi = 3.14159265358979323846;
  for (int phi = 0; phi < den; ++phi) {
    std::vector<double> row(2 * H);
    double sum = 0;
    for (int k = 0; k < 2 * H; ++k) {
      const double tau = (k - H + 1) - (double)phi / den, a = pi * fc * tau;
      row[k] = (a == 0 ? 1.0 : std::sin(a) / a) * fc * (0.5 + 0.5 * std::cos(pi * tau / H));
      sum += row[k];
    }
    for (double v : row) t.push_back((float)(v / sum));
  }
}

static int run(const std::vector<int32_t>& speeds, int q16, bool with_bank, uint64_t seed, int64_t min_samples, long* noisy_seen,
               long* replaced_seen) {
  const int n_speeds = (int)speeds.size() / 2;
  int H = 0;
  std::vector<float> tables;
  for (int s = 0; s < n_speeds; ++s) {
    append_table(tables, speeds[2 * s], speeds[2 * s + 1]);
    H = half_width(speeds[2 * s], speeds[2 * s + 1]);
  }
  const std::vector<int64_t> lens = {1, 2, 2 * H - 1, 255, 256, 257, 513, 3001, 70000};
  const int n = (int)lens.size();
  std::vector<int64_t> in_off(n + 1, 0), out_off(n + 1, 0), ids(n), clip_lens = {1, 700, 50000}, clip_off = {0, 1, 701, 50701};
  for (int u = 0; u < n; ++u) { in_off[u + 1] = in_off[u] + lens[u]; ids[u] = (int64_t)(0x9E3779B97F4A7C15ull * (uint64_t)(u + 1) + seed); }
  const std::vector<float> x = noise((size_t)in_off[n], (unsigned)seed), bank = noise(50701, 77u);
  std::vector<Plan> plan(n);
  const int n_clips = with_bank ? 3 : 0;
  CHECK(st_wave_augment_plan_host(lens.data(), ids.data(), n, seed, speeds.data(), n_speeds, q16, 500, 2500, with_bank ? clip_lens.data() : nullptr,
                                  n_clips, min_samples, plan.data()) == 0);
  for (int u = 0; u < n; ++u) {
    const Plan& p = plan[u];
    CHECK(p.speed >= -1 && p.speed < n_speeds);
    const int num = p.speed < 0 ? 1 : speeds[2 * p.speed], den = p.speed < 0 ? 1 : speeds[2 * p.speed + 1];
    CHECK(p.M == (lens[u] * den + num - 1) / num);
    CHECK(p.speed < 0 || p.M > min_samples);
    *replaced_seen += p.speed < 0;
    if (p.noisy) {
      CHECK(with_bank && p.clip >= 0 && p.clip < 3 && p.offset >= 0 && p.offset < clip_lens[p.clip] && p.snr_centi >= 500 && p.snr_centi <= 2500);
      CHECK(std::fabs(p.lin - std::pow(10.0, p.snr_centi / 1000.0)) <= 1e-12 * p.lin);
      ++*noisy_seen;
    }
    out_off[u + 1] = out_off[u] + p.M;                 // packed: an output one sample too long lands in its neighbour or past the end
  }
  std::vector<float> out((size_t)out_off[n], 7.f), again((size_t)out_off[n], 9.f);
  std::vector<double> sums(2 * n, -1.0);
  CHECK(st_wave_augment_host(x.data(), in_off.data(), n, plan.data(), speeds.data(), n_speeds, tables.data(), with_bank ? bank.data() : nullptr,
                             with_bank ? clip_off.data() : nullptr, n_clips, out.data(), out_off.data(), sums.data()) == 0);
  for (float v : out) CHECK(std::isfinite(v) && std::fabs(v) <= 40.f);
  for (int u = 0; u < n; ++u) {
    CHECK((sums[2 * u] > 0) == (plan[u].noisy != 0) && (sums[2 * u + 1] > 0) == (plan[u].noisy != 0));
    const int sp = plan[u].speed;
    if (!plan[u].noisy && (sp < 0 || speeds[2 * sp] == speeds[2 * sp + 1]))
      CHECK(std::memcmp(&out[out_off[u]], &x[in_off[u]], sizeof(float) * lens[u]) == 0);
  }
  // one utterance alone gives the bits it had in the batch
  for (int u = 0; u < n; u += 4) {
    const int64_t io[2] = {0, lens[u]}, oo[2] = {0, plan[u].M};
    CHECK(st_wave_augment_host(&x[in_off[u]], io, 1, &plan[u], speeds.data(), n_speeds, tables.data(), with_bank ? bank.data() : nullptr,
                               with_bank ? clip_off.data() : nullptr, n_clips, &again[out_off[u]], oo, nullptr) == 0);
    CHECK(std::memcmp(&again[out_off[u]], &out[out_off[u]], sizeof(float) * plan[u].M) == 0);
  }
  return 0;
}

int main() {
  long noisy = 0, replaced = 0;
  const std::vector<std::vector<int32_t>> single = {{11, 10}, {9, 10}, {32, 31}, {7, 8}, {2, 1}, {1, 2}};
  for (const auto& s : single) {
    CHECK(run(s, 0, false, 3, 0, &noisy, &replaced) == 0);
    CHECK(run(s, 65536, true, 4, 256, &noisy, &replaced) == 0);
  }
  CHECK(run({9, 10, 1, 1, 11, 10}, 32768, true, 5, 256, &noisy, &replaced) == 0);
  CHECK(noisy > 50 && replaced > 20);

  // bad arguments: a status and a message, nothing read or written
  const int64_t len1[1] = {100}, id1[1] = {0}, off[2] = {0, 100}, clip_bad[2] = {0, 0};
  const int32_t good[2] = {9, 10}, unreduced[2] = {18, 20}, slow[2] = {1, 3}, big[2] = {33, 32};
  Plan p;
  CHECK(st_wave_augment_plan_host(len1, id1, 1, 0, unreduced, 1, 0, 0, 0, nullptr, 0, 0, &p) != 0);
  CHECK(st_wave_augment_plan_host(len1, id1, 1, 0, slow, 1, 0, 0, 0, nullptr, 0, 0, &p) != 0);
  CHECK(st_wave_augment_plan_host(len1, id1, 1, 0, big, 1, 0, 0, 0, nullptr, 0, 0, &p) != 0);
  CHECK(st_wave_augment_plan_host(len1, id1, 1, 0, good, 1, 100, 0, 0, nullptr, 0, 0, &p) != 0);        // noise without a bank
  CHECK(st_wave_augment_plan_host(len1, id1, 1, 0, good, 1, 0, 0, 0, nullptr, 0, 0, nullptr) != 0);
  CHECK(std::strlen(st_last_error()) > 0);
  CHECK(st_wave_augment_plan_host(len1, id1, 1, 0, good, 1, 0, 0, 0, nullptr, 0, 0, &p) == 0 && p.M == 112 && p.speed == 0);
  std::vector<float> x = noise(100, 1), tab, out(112, 7.f);
  append_table(tab, 9, 10);
  const int64_t out_short[2] = {0, 111}, out_ok[2] = {0, 112};
  CHECK(st_wave_augment_host(x.data(), off, 1, &p, good, 1, tab.data(), nullptr, nullptr, 0, out.data(), out_short, nullptr) != 0);
  Plan q = p;
  q.speed = 1;
  CHECK(st_wave_augment_host(x.data(), off, 1, &q, good, 1, tab.data(), nullptr, nullptr, 0, out.data(), out_ok, nullptr) != 0);
  q = p;
  q.noisy = 1;                                         // a noisy plan without a bank, and with an empty clip
  CHECK(st_wave_augment_host(x.data(), off, 1, &q, good, 1, tab.data(), nullptr, nullptr, 0, out.data(), out_ok, nullptr) != 0);
  CHECK(st_wave_augment_host(x.data(), off, 1, &q, good, 1, tab.data(), x.data(), clip_bad, 1, out.data(), out_ok, nullptr) != 0);
  for (float v : out) CHECK(v == 7.f);
  CHECK(st_wave_augment_ws(0, 100) == 0 && st_wave_augment_ws(2, 257) == 2 * 2 * 2 * sizeof(double));
  printf("checked %ld noisy and %ld replaced plans over the edge lengths\n", noisy, replaced);
  return 0;
}
