// A caller's pitch contour fitted to the frame count of a score (input producer of forward(pitch_hz=...)): the contour is in Hz on a frame grid of its
// own (edited, tracked from a guide vocal, ...), the score's frame count is only known inside forward (durations are predicted), so the fit runs on
// the device from device lengths - no host sync. The float64 definition is `contour_fit` in stylesinger_amd/pitch.py; this kernel is its fp32 form.
//
// Output frame t of an item sits at source position s = (t + 0.5) * n_c / n_t - 0.5 clamped to [0, n_c - 1] (frame centres of both grids on a common
// time axis). s is kept as an exact integer fraction num / den, den = 2 n_t: i0 = num / den, fr = (num % den) / den, i1 = min(i0 + 1, n_c - 1), and
// the nearest source frame is i1 where 2 (num % den) >= den, else i0.
//   voiced iff the NEAREST source frame is voiced (> 0 Hz); unvoiced frames and frames t >= n_t are written as 0;
//   value = exp2((1 - fr) log2 f[i0] + fr log2 f[i1]) when both neighbours are voiced, else the nearest frame's value (the voiced neighbour);
//   times 2^(shift / 12). fr == 0 takes the source sample itself (no log2 / exp2 round trip): with shift == 0, n_c == n_t is a bit-exact copy.
// One thread per output frame, plain vector loads and stores, no atomics: an item's frames do not depend on B, T, Lc or the other items.
#include "common.h"
#include "pitch_fit.h"
#include "../../include/stylesinger_hip.h"

namespace {

constexpr int PF_THREADS = 256;

__global__ __launch_bounds__(PF_THREADS) void contour_fit_kernel(const float* __restrict__ f0_hz, int64_t ldc, int Lc, const int32_t* __restrict__ lens_c,
                                                                 const int32_t* __restrict__ lens_t, float scale, float* __restrict__ out, int64_t ldo,
                                                                 int T) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * PF_THREADS + threadIdx.x;
  if (t >= T) return;
  const int n_c = ss_uniform_len(lens_c, b, Lc), n_t = ss_uniform_len(lens_t, b, T);   // clamped to [0, Lc] / [0, T]
  const float v = (t < n_t && n_c > 0) ? ss_contour_fit_frame(f0_hz + (int64_t)b * ldc, n_c, n_t, t, scale) : 0.f;
  out[(int64_t)b * ldo + t] = v;
}

}  // namespace

extern "C" int ss_contour_fit(const float* f0_hz, int64_t ldc, int Lc, const int32_t* lens_c, const int32_t* lens_t, float shift_semitones, float* out,
                              int64_t ldo, int T, int B, void* stream) {
  SS_CHECK_ARG(f0_hz && lens_c && lens_t && out, "ss_contour_fit: null pointer");
  SS_CHECK_ARG(B > 0 && B <= 65535 && Lc > 0 && T > 0 && ldc >= Lc && ldo >= T, "ss_contour_fit: bad dims (B=%d Lc=%d T=%d ldc=%lld ldo=%lld)", B, Lc, T,
               (long long)ldc, (long long)ldo);
  SS_CHECK_ARG(shift_semitones >= -48.f && shift_semitones <= 48.f, "ss_contour_fit: shift of %g semitones outside +-48", (double)shift_semitones);
  SS_CHECK_ARG(f0_hz != out, "ss_contour_fit: input and output must not alias");
  const float scale = (float)exp2((double)shift_semitones / 12.0);   // shift 0 -> exactly 1
  hipLaunchKernelGGL(contour_fit_kernel, dim3((unsigned)((T + PF_THREADS - 1) / PF_THREADS), (unsigned)B), dim3(PF_THREADS), 0, (hipStream_t)stream,
                     f0_hz, ldc, Lc, lens_c, lens_t, scale, out, ldo, T);
  SS_CHECK_LAUNCH("ss_contour_fit");
  return SS_OK;
}
