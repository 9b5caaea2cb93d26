// Exact Levenshtein distances of (expected, decoded) id-sequence pairs on gfx950, letters and words: what the evaluation's
// `editdistance.eval(expected_str, decoded_str)` and `editdistance.eval(expected_str.split(), decoded_str.split())` give for the
// ids 0..27 of vocabulary.py (a-z ' space).  The LM weight search scores every candidate of a generation with it, on the
// decodings the multi-candidate beam search left on the device.
//
// Mapping: ONE wavefront per pair.  Both sequences go to LDS (16-bit), then:
//  - the dynamic programme D[i][j] runs as a systolic sweep: lane l owns row r0 + l + 1 of a band of 64 rows and computes
//    column j at step j + l, so each step is one min of three on every lane; D[i-1][j] arrives from lane l - 1 by one
//    cross-lane move, the band's last row goes to an LDS row that the next band's lane 0 reads (distances fit 16 bits);
//  - words are maximal runs of ids other than space (27) -- `str.split()` on ids_to_sentence for ids 0..27 -- found with two
//    ballots per 64 ids, and every word is replaced by the index of the first word (of either sequence) EQUAL to it, compared
//    letter by letter; the word distance is then the same sweep over those indices.  Equality is exact, never a hash.
// A pair holding an id outside 0..27 (which ids_to_sentence may map to whitespace) or a sequence longer than kMaxLen gets
// -1 in both results: the caller scores it on the host.
#include <stdint.h>

#include "st_common.h"

namespace {

constexpr int kMaxLen = 4096;          // letters per sequence (ST_EDIT_DISTANCE_MAX_LEN)
constexpr int kMaxWords = kMaxLen / 2; // a sequence of n letters holds at most ceil(n / 2) words
constexpr int kSpaceId = 27;

// Levenshtein distance of x[0..n) and y[0..m) (LDS), wave-uniform result; `row` holds m + 1 entries
__device__ int lev_wave(const uint16_t* x, int n, const uint16_t* y, int m, uint16_t* row) {
  const int lane = threadIdx.x;
  if (n == 0) return m;
  if (m == 0) return n;
  for (int j = lane; j <= m; j += 64) row[j] = (uint16_t)j;       // D[0][j]
  __syncthreads();
  int result = 0;
  for (int r0 = 0; r0 < n; r0 += 64) {
    const int i = r0 + lane + 1;                                   // this lane's row of D
    const int last = min(63, n - r0 - 1);                          // the band's last live lane
    const bool live = lane <= last;
    const int xi = live ? x[i - 1] : -1;
    int left = i, diag = i - 1, cur = 0;                           // D[i][j-1], D[i-1][j-1], D[i][j]
    for (int s = 0; s < m + last; ++s) {
      const int j = s - lane + 1;
      const int from_above = __shfl_up(cur, 1, 64);                // lane - 1's D[i-1][j] (its column j was the step before)
      const bool in = live && j >= 1 && j <= m;
      const int up = lane == 0 ? (in ? (int)row[j] : 0) : from_above;
      if (in) {
        cur = min(min(up, left) + 1, diag + (xi != (int)y[j - 1] ? 1 : 0));
        diag = up;
        left = cur;
        if (lane == 63) row[j] = (uint16_t)cur;                    // D[r0 + 64][j] for the next band (read at its step j - 1)
      }
    }
    __syncthreads();
    if (r0 + 64 >= n) result = __shfl(cur, last, 64);             // D[n][m]
  }
  return result;
}

// the words of ch[base .. base + len): start offsets (absolute) and lengths from word index `first` on; returns their number
__device__ int words_of(const uint16_t* ch, int base, int len, uint16_t* wstart, uint16_t* wlen, int first) {
  const int lane = threadIdx.x;
  int n = 0, n_end = 0;                             // starts and ends so far (they differ while a word spans two chunks)
  for (int i0 = 0; i0 < len; i0 += 64) {
    const int i = i0 + lane;
    const bool in = i < len;
    const int c = in ? ch[base + i] : kSpaceId;
    const int prev = (in && i > 0) ? ch[base + i - 1] : kSpaceId;
    const int next = (in && i + 1 < len) ? ch[base + i + 1] : kSpaceId;
    const bool is_start = c != kSpaceId && prev == kSpaceId;
    const bool is_end = c != kSpaceId && next == kSpaceId;
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long ms = __ballot(is_start), me = __ballot(is_end);
    if (is_start) wstart[first + n + __popcll(ms & below)] = (uint16_t)(base + i);
    __syncthreads();
    // the k-th end closes the k-th start; a word may have started in an earlier chunk
    const int ne = n_end + __popcll(me & below);
    if (is_end) wlen[first + ne] = (uint16_t)(base + i + 1 - wstart[first + ne]);
    n += __popcll(ms);
    n_end += __popcll(me);
    __syncthreads();
  }
  return n;
}

__global__ __launch_bounds__(64) void edit_distance_kernel(const int32_t* __restrict__ expected, int expected_rows, int expected_pitch,
                                                           const int32_t* __restrict__ expected_lens, const int32_t* __restrict__ decoded,
                                                           int decoded_rows, int decoded_pitch, const int32_t* __restrict__ decoded_lens,
                                                           const int32_t* __restrict__ pairs, int32_t* __restrict__ out) {
  __shared__ uint16_t ch[2 * kMaxLen];              // expected at 0, decoded at kMaxLen
  __shared__ uint16_t row[kMaxLen + 1];
  __shared__ uint16_t wstart[2 * kMaxWords], wlen[2 * kMaxWords], wid[2 * kMaxWords];
  const int lane = threadIdx.x, q = blockIdx.x;
  const int ra = pairs[2 * q], rb = pairs[2 * q + 1];
  const bool rows_ok = ra >= 0 && ra < expected_rows && rb >= 0 && rb < decoded_rows;
  const int la = rows_ok ? expected_lens[ra] : -1, lb = rows_ok ? decoded_lens[rb] : -1;
  if (!rows_ok || la < 0 || lb < 0 || la > min(expected_pitch, kMaxLen) || lb > min(decoded_pitch, kMaxLen)) {
    if (lane == 0) { out[2 * q] = -1; out[2 * q + 1] = -1; }
    return;
  }
  bool bad = false;
  const int32_t* a = expected + (long)ra * expected_pitch;
  const int32_t* b = decoded + (long)rb * decoded_pitch;
  for (int i = lane; i < la; i += 64) {
    const int v = a[i];
    bad |= v < 0 || v > kSpaceId;
    ch[i] = (uint16_t)v;
  }
  for (int i = lane; i < lb; i += 64) {
    const int v = b[i];
    bad |= v < 0 || v > kSpaceId;
    ch[kMaxLen + i] = (uint16_t)v;
  }
  if (__ballot(bad)) {
    if (lane == 0) { out[2 * q] = -1; out[2 * q + 1] = -1; }
    return;
  }
  __syncthreads();
  const int letters = lev_wave(ch, la, ch + kMaxLen, lb, row);
  const int na = words_of(ch, 0, la, wstart, wlen, 0);
  const int nb = words_of(ch, kMaxLen, lb, wstart, wlen, na);
  // every word -> the index of the first word equal to it (lane-parallel over the words)
  for (int w = lane; w < na + nb; w += 64) {
    const int sw = wstart[w], lw = wlen[w];
    int k = 0;
    for (; k < w; ++k) {
      if (wlen[k] != lw) continue;
      const int sk = wstart[k];
      int t = 0;
      while (t < lw && ch[sk + t] == ch[sw + t]) ++t;
      if (t == lw) break;
    }
    wid[w] = (uint16_t)k;
  }
  __syncthreads();
  const int words = lev_wave(wid, na, wid + na, nb, row);
  if (lane == 0) { out[2 * q] = letters; out[2 * q + 1] = words; }
}

}  // namespace

extern "C" {

int st_edit_distance_max_len(void) { return kMaxLen; }

int st_edit_distance_pairs(const int32_t* expected, int expected_rows, int expected_pitch, const int32_t* expected_lens,
                           const int32_t* decoded, int decoded_rows, int decoded_pitch, const int32_t* decoded_lens,
                           const int32_t* pairs, int n_pairs, int32_t* distances, void* stream) {
  ST_REQUIRE(expected_rows >= 0 && expected_pitch >= 0 && decoded_rows >= 0 && decoded_pitch >= 0 && n_pairs >= 0,
             "edit distance: negative rows, pitch or pair count (%d, %d, %d, %d, %d)", expected_rows, expected_pitch, decoded_rows,
             decoded_pitch, n_pairs);
  if (n_pairs == 0) return ST_OK;
  ST_REQUIRE(expected && expected_lens && decoded && decoded_lens && pairs && distances, "edit distance: null argument");
  st::trace("edit_distance pairs=%d", n_pairs);
  hipLaunchKernelGGL(edit_distance_kernel, dim3(n_pairs), dim3(64), 0, st::as_stream(stream), expected, expected_rows, expected_pitch,
                     expected_lens, decoded, decoded_rows, decoded_pitch, decoded_lens, pairs, distances);
  return st::check_launch("edit_distance");
}

}  // extern "C"
