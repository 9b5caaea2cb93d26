// Sentence scores of label prefixes under a word n-gram model (st_lm_score_prefixes_f64 / _host): the LM part of an N-best
// hypothesis' score -- G and the two word counts of lm_score_core.h -- so that a list can be re-ranked under other weights or
// another model without searching again (speecht_amd/nbest.py).
//
// Mapping: ONE lane per prefix -- the trie walk and the n-gram queries of a prefix are sequential, the prefixes are the parallel
// axis -- in a plain grid of 256-thread blocks.  A few thousand dependent table reads per prefix; nothing here is tuned.
#include "lm_score_core.h"
#include "st_common.h"

namespace {

__global__ __launch_bounds__(256) void lm_score_prefixes_kernel(stlm::View v, const int32_t* __restrict__ ids, int pitch,
                                                                const int32_t* __restrict__ lens, int n, double* __restrict__ g,
                                                                int32_t* __restrict__ n_words, int32_t* __restrict__ n_valid) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int len = lens[i];
  double sum = 0.0;
  int32_t words = 0, valid = 0;
  // a length outside 0..pitch or an id outside 0..27: the prefix is marked (NaN, -1, -1); the host form refuses the call instead
  if (len < 0 || len > pitch || !stlm::score_prefix(v, ids + (size_t)i * pitch, len, &sum, &words, &valid)) {
    sum = __longlong_as_double(0x7FF8000000000000ll);
    words = valid = -1;
  }
  g[i] = sum;
  n_words[i] = words;
  n_valid[i] = valid;
}

}  // namespace

extern "C" {

int st_lm_score_prefixes_f64(void* lm, const int32_t* ids, int pitch, const int32_t* lens, int n, double* g, int32_t* n_words,
                             int32_t* n_valid, void* stream) {
  ST_REQUIRE(lm, "LM sentence scores: null model");
  ST_REQUIRE(n >= 0 && pitch >= 1, "LM sentence scores: n >= 0 and pitch >= 1, got %d and %d", n, pitch);
  if (n == 0) return ST_OK;
  ST_REQUIRE(ids && lens && g && n_words && n_valid, "LM sentence scores: null argument");
  const stlm::Model* m = static_cast<const stlm::Model*>(lm);
  int device = -1;
  if (hipStreamGetDevice(st::as_stream(stream), &device) != hipSuccess) {
    st::set_error("LM sentence scores: hipStreamGetDevice failed");
    return ST_ELAUNCH;
  }
  const stlm::DeviceCopy* copy = m->on(device);
  ST_REQUIRE(copy, "LM sentence scores: the language model is not on device %d (st_lm_upload with a stream of that device)", device);
  st::trace("lm_score_prefixes n=%d pitch=%d order=%d", n, pitch, copy->view.order);
  hipLaunchKernelGGL(lm_score_prefixes_kernel, dim3(st::ceil_div(n, 256)), dim3(256), 0, st::as_stream(stream), copy->view, ids, pitch,
                     lens, n, g, n_words, n_valid);
  return st::check_launch("lm_score_prefixes");
}

int st_lm_score_prefixes_host(void* lm, const int32_t* ids, int pitch, const int32_t* lens, int n, double* g, int32_t* n_words,
                              int32_t* n_valid) {
  ST_REQUIRE(lm, "LM sentence scores: null model");
  ST_REQUIRE(n >= 0 && pitch >= 1, "LM sentence scores: n >= 0 and pitch >= 1, got %d and %d", n, pitch);
  if (n == 0) return ST_OK;
  ST_REQUIRE(ids && lens && g && n_words && n_valid, "LM sentence scores: null argument");
  const stlm::View v = static_cast<const stlm::Model*>(lm)->host.view();
  // every prefix is checked before anything is written
  for (int i = 0; i < n; ++i) {
    ST_REQUIRE(lens[i] >= 0 && lens[i] <= pitch, "LM sentence scores: prefix %d has length %d, outside 0..pitch = %d", i, lens[i], pitch);
    for (int k = 0; k < lens[i]; ++k) {
      const int32_t c = ids[(size_t)i * pitch + k];
      ST_REQUIRE(c >= 0 && c <= stlm::kSpaceLabel, "LM sentence scores: prefix %d holds id %d at %d, outside 0..27", i, c, k);
    }
  }
  for (int i = 0; i < n; ++i) stlm::score_prefix(v, ids + (size_t)i * pitch, lens[i], g + i, n_words + i, n_valid + i);
  return ST_OK;
}

}  // extern "C"
