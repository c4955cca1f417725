// One output frame of the linear contour fit (ss_contour_fit; definition: `contour_fit` in stylesinger_amd/pitch.py), shared by the fit kernel
// (pitch_fit.hip) and the items ss_contour_align does not align (contour_align.hip): both run this arithmetic, so their results are bit-identical.
#pragma once
#include "common.h"

// f = the item's n_c > 0 source frames in Hz (0 = unvoiced), t < n_t the output frame, scale = fl(2^(shift / 12)). Source position
// s = (t + 0.5) n_c / n_t - 0.5 clamped to [0, n_c - 1], held as the exact fraction num / den, den = 2 n_t (pitch_fit.hip's header comment).
__device__ __forceinline__ float ss_contour_fit_frame(const float* __restrict__ f, int n_c, int n_t, int t, float scale) {
  float v = 0.f;
  const int64_t den = 2 * (int64_t)n_t;
  int64_t num = (2 * (int64_t)t + 1) * n_c - n_t;
  const int64_t hi = (int64_t)(n_c - 1) * den;
  num = num < 0 ? 0 : (num > hi ? hi : num);
  const int i0 = (int)(num / den);
  const int64_t rem = num - (int64_t)i0 * den;
  const int i1 = i0 + 1 < n_c ? i0 + 1 : n_c - 1;
  const float a = f[i0], c = f[i1];
  const float near = 2 * rem >= den ? c : a;
  if (near > 0.f) {
    if (rem == 0 || !(a > 0.f && c > 0.f)) {
      v = near;   // rem == 0: near is a = the source sample itself
    } else {
      const float fr = (float)((double)rem / (double)den);
      const float la = log2f(a), lc = log2f(c);
      v = exp2f(la + fr * (lc - la));
    }
    v *= scale;
  }
  return v;
}
