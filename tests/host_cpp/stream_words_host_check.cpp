// st_ctc_align_ring_host / st_ctc_word_conf_ring_host as a stand-alone program (its own main, no device), for a run under the address
// and undefined-behaviour sanitizers (tests/test_stream_words_host.py).  A host ring of exactly st_stream_keep_rows(M, max_rows) rows
// per stream is filled by the keep rule -- written out here on its own, not through csrc/stream_ring.h -- from streams whose frames
// wrap it several times; after every frame the last rows of every stream are a job, so that jobs start at every ring offset, and each
// is held to st_ctc_align_host / st_ctc_word_conf_host on the dense rows: spans, states, score bits, status, log_prob / log_conf bits.
// Then a job of exactly max_rows rows, jobs of 0 rows and the jobs the ring cannot serve.  Every buffer is exactly as large as the
// contract says, so a write or a read outside one is the sanitizer's to find.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "speecht_hip.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

struct alignas(16) Q { char b[16]; };

static unsigned g_seed = 12345u;
static unsigned rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

struct Labels {
  std::vector<int32_t> ids, offs = {0}, spans;      // CSR over the jobs; word spans {job, first, one past the last}
  int max_len = 0;
  void add(const std::vector<int32_t>& l, int space) {
    const int job = (int)offs.size() - 1;
    int start = -1;
    for (int k = 0; k <= (int)l.size(); ++k) {
      const bool sp = k == (int)l.size() || l[k] == space;
      if (!sp && start < 0) start = k;
      if (sp && start >= 0) { spans.insert(spans.end(), {job, start, k}); start = -1; }
    }
    ids.insert(ids.end(), l.begin(), l.end());
    offs.push_back((int32_t)ids.size());
    max_len = std::max(max_len, (int)l.size());
  }
  int n_words() const { return (int)spans.size() / 3; }
};

struct Result {
  std::vector<int32_t> spans, states, status, cstatus;
  std::vector<float> score;
  std::vector<double> log_prob, log_conf;
};

static bool same_bits(const void* a, const void* b, size_t n) { return std::memcmp(a, b, n) == 0; }

// the two dense host forms on a batch of one utterance of n rows [n][C]
static int dense(const std::vector<float>& x, int n, int C, int space, const std::vector<int32_t>& label, Result& r) {
  Labels lab;
  lab.add(label, space);
  std::vector<int32_t> ids = lab.ids;
  ids.push_back(0);
  const int frames = std::max(n, 1);
  std::vector<float> rows(x);
  rows.resize((size_t)frames * C, 0.f);
  const int32_t len[1] = {n};
  r.spans.assign(2 * label.size() + 2, -9);
  r.states.assign(frames, -9);
  r.status.assign(1, -9);
  r.cstatus.assign(1, -9);
  r.score.assign(1, 9.f);
  std::vector<Q> ws((st_ctc_align_ws(1, frames, lab.max_len) + 15) / 16);
  CHECK(st_ctc_align_host(rows.data(), 1, frames, C, ids.data(), lab.offs.data(), len, lab.max_len, r.spans.data(), r.states.data(),
                          r.score.data(), r.status.data(), ws.data(), ws.size() * 16) == 0);
  const int W = lab.n_words();
  r.log_prob.assign(1, 9.0);
  r.log_conf.assign(W + 1, 9.0);
  std::vector<int32_t> spans = lab.spans;
  spans.resize(3 * W + 3, 0);
  std::vector<Q> ws2((st_ctc_word_conf_ws(1, frames, lab.max_len, 1 + W) + 15) / 16);
  CHECK(st_ctc_word_conf_host(rows.data(), 1, frames, C, ids.data(), lab.offs.data(), len, lab.max_len, space, spans.data(), W,
                              r.log_prob.data(), r.log_conf.data(), r.cstatus.data(), ws2.data(), ws2.size() * 16) == 0);
  return 0;
}

// the two ring host forms on a batch of jobs
static int ring_forms(const std::vector<float>& ring, int S, int cap, int C, int space, const std::vector<int32_t>& jobs, int max_rows,
                      const Labels& lab, Result& r) {
  const int J = (int)jobs.size() / 3, W = lab.n_words();
  std::vector<int32_t> ids = lab.ids, spans = lab.spans;
  ids.push_back(0);
  spans.resize(3 * W + 3, 0);
  r.spans.assign(2 * lab.ids.size() + 2, -9);
  r.states.assign((size_t)J * max_rows, -9);
  r.status.assign(J, -9);
  r.cstatus.assign(J, -9);
  r.score.assign(J, 9.f);
  r.log_prob.assign(J, 9.0);
  r.log_conf.assign(W + 1, 9.0);
  std::vector<Q> ws((st_ctc_align_ws(J, max_rows, lab.max_len) + 15) / 16);
  CHECK(st_ctc_align_ring_host(ring.data(), S, cap, C, jobs.data(), J, max_rows, ids.data(), lab.offs.data(), lab.max_len, r.spans.data(),
                               r.states.data(), r.score.data(), r.status.data(), ws.data(), ws.size() * 16) == 0);
  std::vector<Q> ws2((st_ctc_word_conf_ws(J, max_rows, lab.max_len, J + W) + 15) / 16);
  CHECK(st_ctc_word_conf_ring_host(ring.data(), S, cap, C, jobs.data(), J, max_rows, ids.data(), lab.offs.data(), lab.max_len, space,
                                   spans.data(), W, r.log_prob.data(), r.log_conf.data(), r.cstatus.data(), ws2.data(),
                                   ws2.size() * 16) == 0);
  return 0;
}

int main() {
  const int S = 3, M = 9, PASS = 5, C = 6, space = 4, T = 130;
  CHECK(st_stream_keep_rows(0, 4) == 0 && st_stream_keep_rows(4, 0) == 0 && st_stream_keep_rows(-1, -1) == 0);
  const int cap = st_stream_keep_rows(M, PASS);
  CHECK(cap == M + PASS);
  std::vector<std::vector<float>> x(S, std::vector<float>((size_t)T * C));
  for (auto& s : x) for (auto& v : s) v = (rnd() % 4000) / 500.f - 4.f;
  std::vector<float> ring((size_t)S * cap * 32, NAN);
  std::set<int> offsets;
  long jobs_checked = 0, refused = 0, words = 0;
  for (int f = 0; f < T; ++f) {
    for (int s = 0; s < S; ++s)      // the keep rule: frame f of stream s to ring[s][f % cap], columns below C
      for (int c = 0; c < C; ++c) ring[((size_t)s * cap + f % cap) * 32 + c] = x[s][(size_t)f * C + c];
    const int n = 1 + f % M;         // the last n rows of every stream: [f + 1 - n, f + 1), n = M among them
    if (f + 1 - n < 0) continue;
    std::vector<int32_t> jobs;
    std::vector<std::vector<int32_t>> labels;
    Labels lab;
    for (int s = 0; s < S; ++s) {
      jobs.insert(jobs.end(), {s, f + 1 - n, n});
      std::vector<int32_t> l(rnd() % (n + 1));          // (some too long for their rows once repeats count: refused)
      for (auto& id : l) id = (int32_t)(rnd() % (C - 1));
      labels.push_back(l);
      lab.add(l, space);
    }
    offsets.insert((f + 1 - n) % cap);
    Result got;
    if (ring_forms(ring, S, cap, C, space, jobs, M, lab, got)) return 1;
    int word = 0;
    for (int s = 0; s < S; ++s) {
      Result want;
      const int u0 = f + 1 - n, L = (int)labels[s].size();
      if (dense(std::vector<float>(x[s].begin() + (size_t)u0 * C, x[s].begin() + (size_t)(u0 + n) * C), n, C, space, labels[s], want))
        return 1;
      CHECK(got.status[s] == want.status[0] && got.cstatus[s] == want.cstatus[0] && got.status[s] == got.cstatus[s]);
      CHECK(same_bits(&got.score[s], &want.score[0], 4) && same_bits(&got.log_prob[s], &want.log_prob[0], 8));
      CHECK(same_bits(&got.spans[2 * lab.offs[s]], want.spans.data(), 8 * L));
      CHECK(same_bits(&got.states[(size_t)s * M], want.states.data(), 4 * n));
      for (int t = n; t < M; ++t) CHECK(got.states[(size_t)s * M + t] == -2);
      int W = 0;
      for (int w = 0; w < lab.n_words(); ++w) W += lab.spans[3 * w] == s;
      CHECK(same_bits(&got.log_conf[word], want.log_conf.data(), 8 * W));
      if (got.status[s] == 0) for (int w = 0; w < W; ++w) CHECK(got.log_conf[word + w] <= 0.0);
      word += W;
      words += got.status[s] == 0 ? W : 0;
      refused += got.status[s] != 0;
      ++jobs_checked;
    }
    CHECK(got.spans[2 * lab.ids.size()] == -9 && got.log_conf[lab.n_words()] == 9.0);     // nothing behind the outputs
  }
  CHECK((int)offsets.size() == cap);                    // a job has started at every ring offset 0 .. cap - 1
  CHECK(jobs_checked > 250 && refused > 5 && words > 100);
  printf("checked %ld jobs (%ld words, %ld refused) starting at all %d ring offsets, the ring wrapped %d times\n", jobs_checked, words,
         refused, cap, T / cap);

  // jobs of 0 rows (an empty label: the empty path; a label: refused) and the jobs the ring cannot serve: a status, nothing read
  {
    const int f = T - 1;
    std::vector<int32_t> jobs = {0, f, 0, 1, f, 0, -1, f - 3, 3, S, f - 3, 3, 2, -1, 3, 2, f - 3, -1, 2, f - 3, M + 1, 1, f - 3, 4};
    Labels lab;
    const std::vector<int32_t> one = {1, space, 2};
    lab.add({}, space);
    for (int j = 1; j < 7; ++j) lab.add(one, space);
    lab.add({1}, space);
    Result got;
    if (ring_forms(ring, S, cap, C, space, jobs, M, lab, got)) return 1;
    CHECK(got.status[0] == 0 && got.cstatus[0] == 0 && got.score[0] == 0.f && got.log_prob[0] == 0.0);
    for (int j = 1; j < 7; ++j) {
      CHECK(got.status[j] != 0 && got.cstatus[j] != 0 && got.score[j] == -INFINITY && got.log_prob[j] == -INFINITY);
      for (int i = 0; i < 6; ++i) CHECK(got.spans[2 * lab.offs[j] + i] == -1);
      for (int t = 0; t < M; ++t) CHECK(got.states[(size_t)j * M + t] == -2);
      CHECK(std::isnan(got.log_conf[2 * (j - 1)]) && std::isnan(got.log_conf[2 * (j - 1) + 1]));
    }
    Result want;                                          // the good job beside them is not disturbed
    if (dense(std::vector<float>(x[1].begin() + (size_t)(f - 3) * C, x[1].begin() + (size_t)(f + 1) * C), 4, C, space, {1}, want)) return 1;
    CHECK(got.status[7] == 0 && same_bits(&got.score[7], &want.score[0], 4) && same_bits(&got.log_prob[7], &want.log_prob[0], 8));
    CHECK(same_bits(&got.spans[2 * lab.offs[7]], want.spans.data(), 8) && same_bits(&got.log_conf[12], want.log_conf.data(), 8));
    printf("checked jobs of 0 rows and the jobs the ring cannot serve\n");
  }

  // bad arguments are refused
  {
    const int32_t job[3] = {0, 0, 1}, ids[2] = {1, 0}, offs[2] = {0, 1};
    int32_t spans[2], status[1];
    float score[1];
    double lp[1];
    std::vector<Q> ws((st_ctc_align_ws(1, 1, 1) + 15) / 16);
    CHECK(st_ctc_align_ring_host(nullptr, S, cap, C, job, 1, 1, ids, offs, 1, spans, nullptr, score, status, ws.data(), ws.size() * 16) != 0);
    CHECK(st_ctc_align_ring_host(ring.data(), S, 0, C, job, 1, 1, ids, offs, 1, spans, nullptr, score, status, ws.data(), ws.size() * 16) != 0);
    CHECK(st_ctc_align_ring_host(ring.data(), S, cap, 33, job, 1, 1, ids, offs, 1, spans, nullptr, score, status, ws.data(), ws.size() * 16) != 0);
    CHECK(st_ctc_align_ring_host(ring.data(), S, cap, C, job, 1, 1, ids, offs, 1, spans, nullptr, score, status, ws.data(), 16) != 0);
    CHECK(st_ctc_word_conf_ring_host(ring.data(), S, cap, 31, job, 1, 1, ids, offs, 1, space, nullptr, 0, lp, nullptr, status, ws.data(),
                                     ws.size() * 16) != 0);
    CHECK(st_ctc_word_conf_ring_host(ring.data(), S, cap, C, nullptr, 1, 1, ids, offs, 1, space, nullptr, 0, lp, nullptr, status, ws.data(),
                                     ws.size() * 16) != 0);
    printf("checked the refusals\n");
  }
  return 0;
}
