// Sentence score of a label prefix under a word n-gram model (lm_score.hip: st_lm_score_prefixes_f64 / _host): what the
// LM-scored beam search adds to a final entry, without its weights -- G = the sum of the log10 n-gram probabilities of the
// prefix's words plus </s>, and the two counts the word bonuses multiply (tests/nbest_oracle.py::sentence_score, equal to
// lm_oracle.Scorer(lm, 0, 0): state(p)[3] + end_delta(p)).  One function for host and device, every step in the same order, so the
// two forms are bit-identical.
#pragma once

#include "lm_tables.h"

namespace stlm {

constexpr int kSpaceLabel = 27;            // vocabulary.SPACE_ID: the ids of a prefix are a-z ' (0..26) and space

// stlm::score with the backoff sum in double: log10 p(w | ctx) = the longest listed n-gram ending in w, plus the backoffs of the
// longer contexts (float32 table values, added in double from the shortest context up)
ST_LM_HD double score_f64(const View& v, const int32_t* ctx, int n_ctx, int32_t w) {
  int32_t key[kMaxOrder];
  double r = (double)v.uni[2 * w];
  for (int k = 1; k <= n_ctx && k < v.order; ++k) {
    for (int i = 0; i < k; ++i) key[i] = ctx[n_ctx - k + i];
    key[k] = w;
    const Slot* hit = find(v, key, k + 1);
    float bo = 0.f;
    if (k == 1) bo = v.uni[2 * key[0] + 1];
    else if (const Slot* c = find(v, key, k)) bo = c->bo;
    r = hit ? (double)hit->logp : r + (double)bo;
  }
  return r;
}

// ids[0..len-1] cut at every space into words: an empty run (a leading space, two spaces in a row) is a word and scores as <unk>;
// the trailing run counts only if it is non-empty.  The context starts as <s> (order > 1) and keeps the last order - 1 words.  A
// word the trie spells (a unigram in [a-z']) scores as itself and counts in n_valid, any other as <unk>.  The table values are
// float32; they are summed in double in word order, </s> last.  Returns false on an id outside 0..27 (nothing is written).
ST_LM_HD bool score_prefix(const View& v, const int32_t* ids, int len, double* g, int32_t* n_words, int32_t* n_valid) {
  const int cap = v.order - 1;
  int32_t ctx[kMaxOrder - 1] = {kBos, 0, 0, 0};
  int nc = cap < 1 ? cap : 1;
  int node = 0;                            // trie node of the incomplete word, -1 once it has left the vocabulary
  bool open = false;                       // the incomplete word holds a letter
  double sum = 0.0;
  int32_t words = 0, valid = 0;
  auto close_word = [&]() {
    const int32_t spelled = node >= 0 ? v.trie[node].word : -1;
    const int32_t w = spelled >= 0 ? spelled : kUnk;
    sum += score_f64(v, ctx, nc, w);
    ++words;
    valid += spelled >= 0 ? 1 : 0;
    if (cap > 0) {
      if (nc == cap) {
        for (int i = 0; i + 1 < cap; ++i) ctx[i] = ctx[i + 1];
        ctx[cap - 1] = w;
      } else {
        ctx[nc++] = w;
      }
    }
    node = 0;
    open = false;
  };
  for (int i = 0; i < len; ++i) {
    const int32_t c = ids[i];
    if (c < 0 || c > kSpaceLabel) return false;
    if (c == kSpaceLabel) {
      close_word();
    } else {
      if (node >= 0) {
        const TrieNode nd = v.trie[node];
        node = ((nd.mask >> c) & 1u) ? nd.first + __builtin_popcount(nd.mask & ((1u << c) - 1u)) : -1;
      }
      open = true;
    }
  }
  if (open) close_word();
  sum += score_f64(v, ctx, nc, kEos);
  *g = sum;
  *n_words = words;
  *n_valid = valid;
  return true;
}

}  // namespace stlm
