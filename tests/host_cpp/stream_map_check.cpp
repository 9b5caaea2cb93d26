// The index arithmetic of streaming recognition (speecht_amd/csrc/stream_map.h) against a brute-force enumeration of receptive
// fields, on the host: for every layer geometry of the model and every number of input frames up to 260, open and finished,
// the outputs that are ready and the first input frame still needed; then whole streams fed in chunks through the eleven
// layers, every output frame emitted exactly once and no emitted row reading a frame that was dropped.
// Built and run by tests/test_stream_map_host.py under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <vector>

#include "stream_map.h"

namespace sm = st::stream_map;

static long same_pad_left(long T, int width, int stride) {      // SAME padding as the convolution defines it
  const long t_out = (T + stride - 1) / stride;
  long total = (t_out - 1) * stride + width - T;
  if (total < 0) total = 0;
  return total / 2;
}

static int check_layer(int width, int stride) {
  if (!sm::pad_left_fixed(width, stride)) { printf("padding of (%d, %d) depends on the length\n", width, stride); return 1; }
  const int pl = sm::pad_left(width, stride);
  for (long n = 0; n <= 260; ++n) {
    if (n > 0 && same_pad_left(n, width, stride) != pl) { printf("pad_left(%d, %d) != SAME at T=%ld\n", width, stride, n); return 1; }
    for (int fin = 0; fin < 2; ++fin) {
      long ready = 0;
      for (long j = 0; j <= n + 1; ++j) {
        long last = 0;
        for (int w = 0; w < width; ++w) last = j * stride - pl + w;     // the field's last frame
        const bool ok = fin ? j < (n + stride - 1) / stride : last <= n - 1;
        if (ok) { if (j != ready) { printf("ready outputs are not a prefix\n"); return 1; } ++ready; }
      }
      if (sm::ready_count(n, width, stride, fin) != ready) {
        printf("ready_count(%ld, %d, %d, %d) = %ld, enumeration %ld\n", n, width, stride, fin, sm::ready_count(n, width, stride, fin), ready);
        return 1;
      }
      long need = ready * stride - pl;                                   // first frame of the next output's field
      if (need < 0) need = 0;
      if (sm::retain_from(ready, width, stride) != need || sm::first_tap(ready, width, stride) > need) { printf("retain_from\n"); return 1; }
      for (long e = 0; e <= ready + 1; ++e)
        if (sm::emit_count(n, e, width, stride, fin) != (ready > e ? ready - e : 0)) { printf("emit_count\n"); return 1; }
    }
  }
  return 0;
}

int main() {
  const int geo[11][2] = {{48, 2}, {7, 1}, {7, 1}, {7, 1}, {7, 1}, {7, 1}, {7, 1}, {7, 1}, {32, 1}, {1, 1}, {1, 1}};
  const int shapes[7][2] = {{48, 2}, {7, 1}, {32, 1}, {1, 1}, {6, 2}, {4, 2}, {2, 1}};
  for (auto& g : shapes)
    if (check_layer(g[0], g[1])) return 1;
  if (sm::pad_left_fixed(5, 3) || sm::pad_left_fixed(3, 2) || sm::pad_left_fixed(1, 2)) { printf("pad_left_fixed accepts a length-dependent padding\n"); return 1; }
  long streams = 0, first_row_at = -1;
  for (int chunk : {1, 7, 20, 64})
    for (long T = 1; T <= 260; ++T) {
      long n[11] = {0}, e[11] = {0};
      std::vector<std::vector<int>> seen(11);
      long fed = 0;
      for (;;) {
        long add = T - fed < chunk ? T - fed : chunk;
        const bool fin = add == 0;
        fed += add;
        for (int l = 0; l < 11; ++l) {
          const int w = geo[l][0], s = geo[l][1];
          const long base = sm::retain_from(e[l], w, s);
          n[l] += add;
          const long count = sm::emit_count(n[l], e[l], w, s, fin);
          for (long j = e[l]; j < e[l] + count; ++j) {
            const long a = sm::first_tap(j, w, s), b = a + w - 1;
            if (!fin && b > n[l] - 1) { printf("row emitted before its context\n"); return 1; }
            if (a >= 0 && a < n[l] && a < base) { printf("row reads a dropped frame\n"); return 1; }
            if ((long)seen[l].size() != j) { printf("output emitted out of order\n"); return 1; }
            seen[l].push_back(1);
          }
          if (l == 10 && count > 0 && chunk == 1 && T == 260 && first_row_at < 0) first_row_at = fed;
          e[l] += count;
          add = count;
        }
        if (fin) break;
      }
      long t = T;
      for (int l = 0; l < 11; ++l) {
        t = (t + geo[l][1] - 1) / geo[l][1];
        if ((long)seen[l].size() != t) { printf("T=%ld layer %d: %zu outputs, %ld expected\n", T, l, seen[l].size(), t); return 1; }
      }
      if (sm::decode_limit(T) != T / 2) return 1;
      ++streams;
    }
  printf("checked %ld streams; first logits row after %ld input frames\n", streams, first_row_at);
  return 0;
}
