// Tap selection of resampy's "kaiser_best" band-limited interpolation, as audio_io.resample_kaiser_best restates it, shared
// by the gfx950 kernel and the host form of csrc/resample.hip (st_resample_kaiser_f32 / st_resample_kaiser_host).  Every
// quantity here is the float64 expression of the numpy code, in the same order, so that the device picks exactly the host's
// taps and forms exactly the host's filter weights; only the rounding of the per-wing sums may differ.
//
//   t = i / ratio;  n = int(t);  frac = scale * (t - n)   (wing 1: scale - frac)
//   index_frac = frac * 512;  offset = int(index_frac);  eta = index_frac - offset
//   taps = min((nwin - offset) // index_step, wing 0 ? n + 1 : n_orig - n - 1)
//   tap k: table index offset + k * index_step, source sample n - k (wing 0) or n + k + 1 (wing 1)
//   weight = win[idx] + eta * delta[idx]   with win scaled by ratio and delta = diff(win) when ratio < 1
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define ST_RS_HD __host__ __device__ __forceinline__
#else
#define ST_RS_HD inline
#endif

namespace st {

constexpr int RS_NUM_TABLE = 512;                    // table entries per zero crossing (precision 9)
constexpr int RS_NUM_ZEROS = 64;
constexpr int64_t RS_NWIN = (int64_t)RS_NUM_TABLE * RS_NUM_ZEROS + 1;   // 32 769 entries of the right half window

struct RsParams {
  double ratio, scale;                               // sr_new / sr_orig, min(1, ratio)
  int64_t index_step;                                // int(scale * 512)
};

ST_RS_HD RsParams rs_params(int sr_orig, int sr_new) {
  RsParams p;
  p.ratio = (double)sr_new / (double)sr_orig;
  p.scale = p.ratio < 1.0 ? p.ratio : 1.0;
  p.index_step = (int64_t)(p.scale * RS_NUM_TABLE);
  return p;
}

struct RsWing {
  int64_t n;                                         // floor of the output's time in source samples
  int64_t offset;                                    // table index of tap 0
  double eta;                                        // linear-interpolation fraction between table entries
  int64_t count;                                     // taps (<= 0: none)
};

ST_RS_HD RsWing rs_wing(const RsParams& p, int64_t i, int64_t n_orig, int wing) {
#pragma clang fp contract(off)
  RsWing w;
  const double t = (double)i / p.ratio;
  w.n = (int64_t)t;
  double frac = p.scale * (t - (double)w.n);
  if (wing) frac = p.scale - frac;
  const double index_frac = frac * (double)RS_NUM_TABLE;
  w.offset = (int64_t)index_frac;
  w.eta = index_frac - (double)w.offset;
  const int64_t limit = (RS_NWIN - w.offset) / p.index_step;
  const int64_t avail = wing == 0 ? w.n + 1 : n_orig - w.n - 1;
  w.count = limit < avail ? limit : avail;
  return w;
}

// weight of table entry k (k < RS_NWIN); win: the unscaled window (audio_io._kaiser_best_filter)
ST_RS_HD double rs_weight(const double* win, int64_t k, double eta, double ratio) {
#pragma clang fp contract(off)
  const double a = win[k];
  const double b = k + 1 < RS_NWIN ? win[k + 1] : a;          // delta[-1] = 0
  if (ratio < 1.0) {
    const double as = a * ratio, bs = b * ratio;
    return as + eta * (bs - as);
  }
  return a + eta * (b - a);
}

// output sample i (< the resampled length int(n_orig * ratio)) of a signal of n_orig samples whose sample j is src(j): the two
// wings' sums, added as the host adds them (sum of wing 0, then + sum of wing 1); the taps in order, product rounded before the
// add.  Only where sample j is read from differs between the callers (a whole signal in memory; a live stream's staged window).
template <class Src>
ST_RS_HD double rs_output_src(const Src& src, int64_t n_orig, const RsParams& p, int64_t i, const double* win) {
#pragma clang fp contract(off)
  double out = 0.0;
  for (int wing = 0; wing < 2; ++wing) {
    const RsWing w = rs_wing(p, i, n_orig, wing);
    double acc = 0.0;
    if (w.n >= 0 && w.n < n_orig) {                  // always true for i < int(n_orig * ratio); keeps every read in bounds
      for (int64_t k = 0; k < w.count; ++k) {
        const double wt = rs_weight(win, w.offset + k * p.index_step, w.eta, p.ratio);
        acc += wt * (double)src(wing == 0 ? w.n - k : w.n + k + 1);
      }
    }
    out += acc;
  }
  return out;
}

struct RsSignal {                                    // the signal y[0 .. n_orig) in memory
  const float* y;
  ST_RS_HD float operator()(int64_t j) const { return y[j]; }
};

ST_RS_HD double rs_output(const float* y, int64_t n_orig, const RsParams& p, int64_t i, const double* win) {
  return rs_output_src(RsSignal{y}, n_orig, p, i, win);
}

}  // namespace st
