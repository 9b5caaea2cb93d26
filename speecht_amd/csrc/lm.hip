// Word n-gram language model handles of the C ABI (st_lm_*): ARPA text -> host tables (lm_tables.h) -> one allocation per
// device that the LM-scored beam search (ctc_beam.hip, st_ctc_beam_search_decode_lm) reads on that device.
#include <string.h>

#include <new>
#include <string>

#include "lm_tables.h"
#include "st_common.h"

extern "C" {

int st_lm_create_arpa(const char* text, size_t bytes, void** handle, char* err, size_t errlen) {
  ST_REQUIRE(text && handle, "st_lm_create_arpa: null argument");
  *handle = nullptr;
  stlm::Model* m = new (std::nothrow) stlm::Model();
  ST_REQUIRE(m, "st_lm_create_arpa: out of host memory");
  std::string msg;
  bool ok = false;
  try {
    ok = stlm::parse_arpa(text, bytes, m->host, msg);
  } catch (const std::bad_alloc&) {
    msg = "out of host memory while building the tables";
  }
  if (!ok) {
    if (err && errlen) {
      strncpy(err, msg.c_str(), errlen - 1);
      err[errlen - 1] = '\0';
    }
    st::set_error("%s", msg.c_str());
    delete m;
    return ST_EINVAL;
  }
  *handle = m;
  return ST_OK;
}

// counts: order + 1 entries (counts[n] = n-grams of order n, counts[0] = word ids incl. <unk> <s> </s>)
int st_lm_info(void* handle, int* order, int64_t* counts, int64_t* skipped_words, int64_t* trie_nodes, size_t* device_bytes) {
  ST_REQUIRE(handle, "st_lm_info: null handle");
  const stlm::HostTables& t = static_cast<stlm::Model*>(handle)->host;
  if (order) *order = t.order;
  if (counts) {
    counts[0] = (int64_t)t.words.size();
    for (int n = 1; n <= t.order; ++n) counts[n] = t.counts[n];
  }
  if (skipped_words) *skipped_words = t.skipped_words;
  if (trie_nodes) *trie_nodes = (int64_t)t.trie.size();
  if (device_bytes) *device_bytes = stlm::device_bytes(t);
  return ST_OK;
}

// copies the tables to the device of `stream` (null: the current device), once per device: a handle serves engines on several
// devices, and the decoder takes the copy on its stream's device
int st_lm_upload(void* handle, void* stream) {
  ST_REQUIRE(handle, "st_lm_upload: null handle");
  stlm::Model* m = static_cast<stlm::Model*>(handle);
  hipStream_t s = st::as_stream(stream);
  int device = -1;
  hipError_t e = hipStreamGetDevice(s, &device);
  if (e != hipSuccess) {
    st::set_error("st_lm_upload: hipStreamGetDevice: %s", hipGetErrorString(e));
    return ST_ELAUNCH;
  }
  if (m->on(device)) return ST_OK;
  int prev = -1;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(device);
  const stlm::HostTables& t = m->host;
  const size_t bytes = stlm::device_bytes(t);
  void* dev = nullptr;
  e = hipMalloc(&dev, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    (void)hipSetDevice(prev);
    st::set_error("st_lm_upload: hipMalloc of %zu bytes on device %d failed", bytes, device);
    return ST_ELAUNCH;
  }
  char* p = static_cast<char*>(dev);
  stlm::View v{};
  v.order = t.order;
  v.words = (int)t.words.size();
  e = hipMemcpyAsync(p, t.trie.data(), t.trie.size() * sizeof(stlm::TrieNode), hipMemcpyHostToDevice, s);
  v.trie = reinterpret_cast<const stlm::TrieNode*>(p);
  p += stlm::align256(t.trie.size() * sizeof(stlm::TrieNode));
  if (e == hipSuccess) e = hipMemcpyAsync(p, t.uni.data(), t.uni.size() * sizeof(float), hipMemcpyHostToDevice, s);
  v.uni = reinterpret_cast<const float*>(p);
  p += stlm::align256(t.uni.size() * sizeof(float));
  for (int n = 2; n <= t.order; ++n) {
    if (e == hipSuccess) e = hipMemcpyAsync(p, t.tab[n].data(), t.tab[n].size() * sizeof(stlm::Slot), hipMemcpyHostToDevice, s);
    v.tab[n] = reinterpret_cast<const stlm::Slot*>(p);
    v.cap_mask[n] = (uint32_t)t.tab[n].size() - 1u;
    p += stlm::align256(t.tab[n].size() * sizeof(stlm::Slot));
  }
  // the host tables must outlive the copies (pageable sources: the copies may still read them after the call returns)
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    st::set_error("st_lm_upload: %s", hipGetErrorString(e));
    (void)hipFree(dev);
    (void)hipSetDevice(prev);
    return ST_ELAUNCH;
  }
  (void)hipSetDevice(prev);
  m->copies.push_back(stlm::DeviceCopy{device, dev, v});
  return ST_OK;
}

int st_lm_word_id(void* handle, const char* word, int32_t* id) {
  ST_REQUIRE(handle && word && id, "st_lm_word_id: null argument");
  const stlm::HostTables& t = static_cast<stlm::Model*>(handle)->host;
  std::string w(word);
  for (char& ch : w) ch = (char)tolower((unsigned char)ch);
  const auto it = t.id_of.find(w);
  *id = it == t.id_of.end() ? stlm::kUnk : it->second;
  return ST_OK;
}

// log10 p(word | ctx) through the host tables -- the lookup the kernel runs (stlm::score), reachable without a GPU
int st_lm_query_host(void* handle, const int32_t* ctx, int n, int32_t word, float* logp) {
  ST_REQUIRE(handle && logp && (ctx || n == 0), "st_lm_query_host: null argument");
  const stlm::HostTables& t = static_cast<stlm::Model*>(handle)->host;
  ST_REQUIRE(n >= 0 && n < stlm::kMaxOrder, "st_lm_query_host: context of 0..%d words, got %d", stlm::kMaxOrder - 1, n);
  ST_REQUIRE(word >= 0 && word < (int32_t)t.words.size(), "st_lm_query_host: word id %d out of range", word);
  for (int i = 0; i < n; ++i)
    ST_REQUIRE(ctx[i] >= 0 && ctx[i] < (int32_t)t.words.size(), "st_lm_query_host: context id %d out of range", ctx[i]);
  const int used = n < t.order - 1 ? n : t.order - 1;        // the last order - 1 words
  *logp = stlm::score(t.view(), ctx + (n - used), used, word);
  return ST_OK;
}

// the trie node spelled by `prefix` (labels a-z, '): node index or -1, its lowest unigram log10 p and terminal word id
int st_lm_trie_lookup(void* handle, const char* prefix, int32_t* node, float* min_logp, int32_t* word) {
  ST_REQUIRE(handle && prefix && node && min_logp && word, "st_lm_trie_lookup: null argument");
  const stlm::HostTables& t = static_cast<stlm::Model*>(handle)->host;
  int32_t k = 0;
  for (const char* c = prefix; *c && k >= 0; ++c) {
    const int l = stlm::detail::label_of(*c);
    const stlm::TrieNode& nd = t.trie[k];
    k = (l >= 0 && ((nd.mask >> l) & 1u)) ? nd.first + __builtin_popcount(nd.mask & ((1u << l) - 1u)) : -1;
  }
  *node = k;
  *min_logp = k >= 0 ? t.trie[k].min_logp : 0.f;
  *word = k >= 0 ? t.trie[k].word : -1;
  return ST_OK;
}

int st_lm_destroy(void* handle) {
  if (!handle) return ST_OK;
  stlm::Model* m = static_cast<stlm::Model*>(handle);
  int prev = -1;
  (void)hipGetDevice(&prev);
  for (const stlm::DeviceCopy& c : m->copies) {
    (void)hipSetDevice(c.device);
    (void)hipFree(c.dev);
  }
  if (!m->copies.empty()) (void)hipSetDevice(prev);
  delete m;
  return ST_OK;
}

}  // extern "C"
