// Word n-gram language model tables for the LM-scored CTC beam search (lm.hip, ctc_beam.hip): an ARPA file parsed from a
// memory buffer into
//   - word ids: <unk> = 0, <s> = 1, </s> = 2, then the unigrams in file order (words lowercased);
//   - unigrams: a dense array {log10 p, log10 backoff} indexed by word id;
//   - one open-addressing hash per order n >= 2, slot = {ids[5], log10 p, log10 backoff, pad} (32 B), the full id tuple stored
//     for verification, linear probing, load factor <= 1/2;
//   - a character trie over the words spelled in [a-z'] (labels 0..26), children of a node contiguous in label order:
//     node = {27-bit child mask, first child, lowest unigram log10 p of the words below, terminal word id or -1} (16 B),
//     child c at first + popcount(mask & ((1 << c) - 1)).
// Plain C++ (g++ compiles it alone); the lookups are host + device functions shared by the host query and the kernel.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define ST_LM_HD __host__ __device__ __forceinline__
#else
#define ST_LM_HD inline
#endif

namespace stlm {

constexpr int kMaxOrder = 5;
constexpr int kLetters = 27;             // a-z, apostrophe: the labels that spell a word (vocabulary.py); 27 = space
constexpr int kUnk = 0, kBos = 1, kEos = 2;
constexpr float kMissingSpecialLogp = -100.f;   // <unk> / <s> / </s> absent from the unigrams (KenLM substitutes -100 for <unk>)

struct TrieNode {
  uint32_t mask;      // bit c: child with label c exists
  int32_t first;      // index of the first child
  float min_logp;     // lowest unigram log10 p among the words with this prefix
  int32_t word;       // word id spelled by the path to this node, -1 if none
};
static_assert(sizeof(TrieNode) == 16, "trie node is 16 B");

struct Slot {
  int32_t ids[kMaxOrder];   // ids[0] == -1: empty
  float logp, bo;
  int32_t pad;
};
static_assert(sizeof(Slot) == 32, "n-gram slot is 32 B");

// the tables as one set of (host or device) pointers
struct View {
  const TrieNode* trie;
  const float* uni;                        // [words][2] = {log10 p, log10 backoff}
  const Slot* tab[kMaxOrder + 1];          // tab[n] for n = 2..order
  uint32_t cap_mask[kMaxOrder + 1];        // capacity - 1 (power of two)
  int order;
  int words;
};

ST_LM_HD uint32_t ngram_hash(const int32_t* ids, int n) {
  uint64_t h = 0x9E3779B97F4A7C15ull * (uint64_t)n;
  for (int i = 0; i < n; ++i) {
    h = (h ^ (uint32_t)ids[i]) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 29;
  }
  return (uint32_t)(h ^ (h >> 32));
}

// n-gram (ids[0..n-1]), 2 <= n <= order: its slot, or nullptr
ST_LM_HD const Slot* find(const View& v, const int32_t* ids, int n) {
  const Slot* tab = v.tab[n];
  const uint32_t m = v.cap_mask[n];
  for (uint32_t i = ngram_hash(ids, n) & m;; i = (i + 1) & m) {
    const Slot* s = tab + i;
    if (s->ids[0] < 0) return nullptr;
    bool eq = true;
    for (int k = 0; k < n; ++k) eq = eq && s->ids[k] == ids[k];
    if (eq) return s;
  }
}

// log10 p(w | ctx) with ARPA backoff: ctx = the last n_ctx word ids (oldest first, n_ctx <= order - 1).  Every probe is known up
// front (the longest listed n-gram ending in w wins, plus the backoffs of the longer contexts, a missing backoff counting 0), so
// on the device they are one round of independent loads.
ST_LM_HD float score(const View& v, const int32_t* ctx, int n_ctx, int32_t w) {
  int32_t key[kMaxOrder];
  float r = v.uni[2 * w];
  for (int k = 1; k <= n_ctx && k < v.order; ++k) {
    // context suffix of length k: ctx[n_ctx - k .. n_ctx - 1]
    for (int i = 0; i < k; ++i) key[i] = ctx[n_ctx - k + i];
    key[k] = w;
    const Slot* hit = find(v, key, k + 1);
    float bo = 0.f;
    if (k == 1) bo = v.uni[2 * key[0] + 1];
    else if (const Slot* c = find(v, key, k)) bo = c->bo;
    r = hit ? hit->logp : r + bo;
  }
  return r;
}

}  // namespace stlm

// ---- host side: the parser and the table builder ---------------------------------------------------------------------------
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

namespace stlm {

struct HostTables {
  int order = 0;
  long long counts[kMaxOrder + 1] = {};       // \data\ counts
  long long skipped_words = 0;                // unigrams spelled outside [a-z']: in the n-grams, unreachable from the trie
  std::vector<std::string> words;             // by id
  std::unordered_map<std::string, int32_t> id_of;   // word -> id
  std::vector<float> uni;                     // [words][2]
  std::vector<Slot> tab[kMaxOrder + 1];
  std::vector<TrieNode> trie;

  View view() const {
    View v{};
    v.trie = trie.data();
    v.uni = uni.data();
    for (int n = 2; n <= order; ++n) {
      v.tab[n] = tab[n].data();
      v.cap_mask[n] = (uint32_t)tab[n].size() - 1u;
    }
    v.order = order;
    v.words = (int)words.size();
    return v;
  }
};

namespace detail {

struct Lines {
  const char* p;
  const char* end;
  long line = 0;
  // next line without its end-of-line characters; false at the end of the buffer
  bool next(const char*& b, const char*& e) {
    if (p >= end) return false;
    b = p;
    const char* nl = static_cast<const char*>(memchr(p, '\n', (size_t)(end - p)));
    e = nl ? nl : end;
    p = nl ? nl + 1 : end;
    while (e > b && (e[-1] == '\r' || e[-1] == ' ' || e[-1] == '\t')) --e;
    ++line;
    return true;
  }
};

inline bool blank_line(const char* b, const char* e) {
  for (; b < e; ++b)
    if (*b != ' ' && *b != '\t') return false;
  return true;
}

// whitespace-separated fields of [b, e)
inline int split(const char* b, const char* e, std::vector<std::string>& out) {
  out.clear();
  while (b < e) {
    while (b < e && (*b == ' ' || *b == '\t')) ++b;
    const char* s = b;
    while (b < e && *b != ' ' && *b != '\t') ++b;
    if (b > s) out.emplace_back(s, b);
  }
  return (int)out.size();
}

inline bool parse_float(const std::string& s, float& out) {
  char* endp = nullptr;
  const double d = strtod(s.c_str(), &endp);        // through double, like the Python restatement: float(text) -> float32
  if (endp == s.c_str() || *endp != '\0') return false;
  out = (float)d;
  return true;
}

inline int label_of(char ch) {
  if (ch >= 'a' && ch <= 'z') return ch - 'a';
  if (ch == '\'') return 26;
  return -1;
}

}  // namespace detail

// Parses an ARPA model.  Returns false with a message (line number included) on a format error.
inline bool parse_arpa(const char* text, size_t bytes, HostTables& t, std::string& err) {
  using namespace detail;
  Lines in{text, text + bytes};
  const char *b, *e;
  char msg[256];
  auto fail = [&](const char* what) {
    char line[320];
    snprintf(line, sizeof line, "ARPA line %ld: %s", in.line, what);
    err = line;
    return false;
  };
  // header: skip to \data\ ;
  bool found = false;
  while (in.next(b, e)) {
    if (std::string(b, e) == "\\data\\") { found = true; break; }
  }
  if (!found) return fail("no \\data\\ section");
  while (in.next(b, e)) {
    if (blank_line(b, e)) {
      if (t.order > 0) break;
      continue;
    }
    if (*b == '\\' && t.order > 0) {          // the first section header right after the counts: give the line back
      in.p = b;
      --in.line;
      break;
    }
    int n = 0;
    long long c = 0;
    std::string s(b, e);
    if (sscanf(s.c_str(), "ngram %d=%lld", &n, &c) != 2) return fail("expected 'ngram N=count'");
    if (n != t.order + 1) return fail("n-gram orders in \\data\\ must be 1, 2, ... in turn");
    if (n > kMaxOrder) return fail("orders above 5 are not supported");
    if (c < 0 || c >= (1ll << 30)) return fail("bad n-gram count");
    t.order = n;
    t.counts[n] = c;
  }
  if (t.order == 0) return fail("no n-gram counts in \\data\\");
  if (t.counts[1] <= 0) return fail("no unigrams");

  t.words = {"<unk>", "<s>", "</s>"};
  t.uni.assign(6, 0.f);
  bool special_seen[3] = {false, false, false};
  std::unordered_map<std::string, int32_t>& id_of = t.id_of;
  id_of.reserve((size_t)t.counts[1] * 2 + 8);
  for (int i = 0; i < 3; ++i) id_of[t.words[i]] = i;
  for (int n = 2; n <= t.order; ++n) {
    size_t cap = 16;
    while (cap < (size_t)t.counts[n] * 2) cap <<= 1;
    Slot empty{};
    for (int k = 0; k < kMaxOrder; ++k) empty.ids[k] = -1;
    empty.logp = empty.bo = 0.f;
    t.tab[n].assign(cap, empty);
  }

  std::vector<std::string> f;
  for (int n = 1; n <= t.order; ++n) {
    char head[32];
    snprintf(head, sizeof head, "\\%d-grams:", n);
    // the section header, after blank lines
    for (;;) {
      if (!in.next(b, e)) return fail("file ends before the n-gram section");
      if (blank_line(b, e)) continue;
      if (std::string(b, e) != head) {
        snprintf(msg, sizeof msg, "expected '%s'", head);
        return fail(msg);
      }
      break;
    }
    long long seen = 0;
    for (;;) {
      if (!in.next(b, e)) return fail("file ends inside an n-gram section");
      if (blank_line(b, e)) {
        if (seen == t.counts[n]) break;
        continue;
      }
      if (*b == '\\') {
        if (seen != t.counts[n]) {
          snprintf(msg, sizeof msg, "%lld %d-grams listed, \\data\\ says %lld", seen, n, t.counts[n]);
          return fail(msg);
        }
        in.p = b;                 // give the line back: it is the next header
        --in.line;
        break;
      }
      if (seen == t.counts[n]) {
        snprintf(msg, sizeof msg, "more %d-grams than the %lld \\data\\ announces", n, t.counts[n]);
        return fail(msg);
      }
      const int nf = split(b, e, f);
      if (nf != n + 1 && nf != n + 2) return fail("expected 'log10p w1 .. wn [backoff]'");
      float logp = 0.f, bo = 0.f;
      if (!parse_float(f[0], logp)) return fail("bad probability");
      if (nf == n + 2 && !parse_float(f[n + 1], bo)) return fail("bad backoff");
      if (n == 1) {
        std::string w = f[1];
        for (char& ch : w) ch = (char)tolower((unsigned char)ch);
        int32_t id;
        auto it = id_of.find(w);
        if (it != id_of.end()) {
          if (it->second > kEos || special_seen[it->second]) return fail("word listed twice (after lowercasing)");
          special_seen[it->second] = true;
          id = it->second;
        } else {
          id = (int32_t)t.words.size();
          id_of.emplace(w, id);
          t.words.push_back(w);
          t.uni.push_back(0.f);
          t.uni.push_back(0.f);
        }
        t.uni[2 * id] = logp;
        t.uni[2 * id + 1] = bo;
      } else {
        Slot s{};
        for (int k = 0; k < kMaxOrder; ++k) s.ids[k] = -1;
        for (int k = 0; k < n; ++k) {
          std::string w = f[1 + k];
          for (char& ch : w) ch = (char)tolower((unsigned char)ch);
          auto it = id_of.find(w);
          if (it == id_of.end()) return fail("n-gram word missing from the unigrams");
          s.ids[k] = it->second;
        }
        s.logp = logp;
        s.bo = bo;
        std::vector<Slot>& tab = t.tab[n];
        const uint32_t m = (uint32_t)tab.size() - 1u;
        for (uint32_t i = ngram_hash(s.ids, n) & m;; i = (i + 1) & m) {
          if (tab[i].ids[0] < 0) { tab[i] = s; break; }
          if (std::equal(s.ids, s.ids + n, tab[i].ids)) return fail("n-gram listed twice");
        }
      }
      ++seen;
    }
  }
  // \end\ after blank lines
  for (;;) {
    if (!in.next(b, e)) return fail("missing \\end\\");
    if (blank_line(b, e)) continue;
    if (std::string(b, e) != "\\end\\") return fail("expected \\end\\");
    break;
  }
  for (int i = 0; i < 3; ++i)
    if (!special_seen[i]) t.uni[2 * i] = kMissingSpecialLogp;

  // character trie over the words spelled in [a-z']: a pointer trie, then laid out breadth first (children contiguous)
  struct Build {
    int32_t child[kLetters];
    int32_t word;
    float min_logp;
  };
  std::vector<Build> bt(1);
  auto fresh = [&]() {
    Build x;
    for (int c = 0; c < kLetters; ++c) x.child[c] = -1;
    x.word = -1;
    x.min_logp = INFINITY;
    return x;
  };
  bt[0] = fresh();
  t.skipped_words = 0;
  for (int32_t id = kEos + 1; id < (int32_t)t.words.size(); ++id) {
    const std::string& w = t.words[id];
    bool ok = !w.empty();
    for (char ch : w) ok = ok && label_of(ch) >= 0;
    if (!ok) { ++t.skipped_words; continue; }
    const float lp = t.uni[2 * id];
    int32_t node = 0;
    bt[0].min_logp = std::min(bt[0].min_logp, lp);
    for (char ch : w) {
      const int c = label_of(ch);
      if (bt[node].child[c] < 0) {
        bt[node].child[c] = (int32_t)bt.size();
        bt.push_back(fresh());
      }
      node = bt[node].child[c];
      bt[node].min_logp = std::min(bt[node].min_logp, lp);
    }
    bt[node].word = id;
  }
  // breadth-first numbering: node i's children get consecutive indices in label order
  std::vector<int32_t> order_bfs{0}, new_index(bt.size(), -1);
  new_index[0] = 0;
  for (size_t q = 0; q < order_bfs.size(); ++q) {
    const Build& x = bt[order_bfs[q]];
    for (int c = 0; c < kLetters; ++c) {
      if (x.child[c] >= 0) {
        new_index[x.child[c]] = (int32_t)order_bfs.size();
        order_bfs.push_back(x.child[c]);
      }
    }
  }
  t.trie.resize(bt.size());
  for (size_t q = 0; q < order_bfs.size(); ++q) {
    const Build& x = bt[order_bfs[q]];
    TrieNode nd{0u, 0, x.min_logp == INFINITY ? 0.f : x.min_logp, x.word};
    int32_t first = -1;
    for (int c = 0; c < kLetters; ++c) {
      if (x.child[c] >= 0) {
        nd.mask |= 1u << c;
        if (first < 0) first = new_index[x.child[c]];
      }
    }
    nd.first = first < 0 ? 0 : first;
    t.trie[q] = nd;
  }
  return true;
}

// device bytes of the tables (one allocation: trie | unigrams | the hash of each order, each part 256-B aligned)
inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }
inline size_t device_bytes(const HostTables& t) {
  size_t n = align256(t.trie.size() * sizeof(TrieNode)) + align256(t.uni.size() * sizeof(float));
  for (int k = 2; k <= t.order; ++k) n += align256(t.tab[k].size() * sizeof(Slot));
  return n;
}

// what a handle of the C ABI (st_lm_*) holds: the host tables and one device copy per device they were uploaded to
struct DeviceCopy {
  int device;
  void* dev;                  // one allocation on `device` (device_bytes(host))
  View view;                  // the tables' pointers into it
};
struct Model {
  HostTables host;
  std::vector<DeviceCopy> copies;
  const DeviceCopy* on(int device) const {
    for (const DeviceCopy& c : copies)
      if (c.device == device) return &c;
    return nullptr;
  }
};

}  // namespace stlm
