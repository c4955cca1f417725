// Pitch post-processing around the f0 sampler: the dyn_clip bounds it samples inside, and the merge / denorm / coarse step after it - for the two
// predictors or for a given contour. Elementwise launches, no workspace.
#include "common.h"
#include "../../include/stylesinger_hip.h"

namespace {

// dyn_clip bounds from MIDI (stylesinger.py:274-283)
__global__ void f0_bounds_kernel(const int64_t* __restrict__ midi, float* __restrict__ lo, float* __restrict__ hi, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float m = (float)midi[i];
  auto nb = [](float note) {
    float hz = powf(2.0f, (note - 69.0f) / 12.0f) * 440.0f;
    float x = log2f(hz);
    if (x > 10.0f) x = 10.0f;
    float v = (x - 6.0f) / (10.0f - 6.0f) * 2.0f - 1.0f;
    return fminf(fmaxf(v, -1.0f), 1.0f);
  };
  lo[i] = nb(m - 3.0f);
  hi[i] = nb(m + 3.0f);
}

// f0_to_coarse (utils/pitch_utils.py:22-31): Hz -> pitch embedding row; shared by the predicted and the given-contour kernels
__device__ __forceinline__ int64_t f0_to_coarse(float hz) {
  // utils/pitch_utils.py:17-18: numpy float64 constants, cast to fp32 when they meet the tensor
  const float f0_mel_min = (float)77.75496616579426;          // 1127*ln(1+50/700)
  const float f0_mel_span = (float)986.6532669978451;         // 1127*ln(1+1100/700) - f0_mel_min
  float mel = 1127.0f * logf(1.0f + hz / 700.0f);
  if (mel > 0.0f) mel = (mel - f0_mel_min) * 254.0f / f0_mel_span + 1.0f;
  if (mel <= 1.0f) mel = 1.0f;
  if (mel > 255.0f) mel = 255.0f;
  return (int64_t)(mel + 0.5f);
}

// merge of the two predictors + denorm + coarse (stylesinger.py:230-246,286-311; pitch_utils.py:22-31,65-78)
__global__ void pitch_post_kernel(const float* __restrict__ f0_a, const int32_t* __restrict__ uv_a,
                                  const float* __restrict__ f0_b, const int32_t* __restrict__ uv_b,
                                  const int64_t* __restrict__ midi, const int64_t* __restrict__ mel2ph,
                                  float* __restrict__ pitch_pred, float* __restrict__ f0_denorm,
                                  int64_t* __restrict__ coarse, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool rest = midi[i] == 0;
  const float ua = rest ? 1.0f : (float)(uv_a[i] != 0), ub = rest ? 1.0f : (float)(uv_b[i] != 0);
  const float fa = (f0_a[i] + 1.0f) / 2.0f * (10.0f - 6.0f) + 6.0f;
  const float fb = (f0_b[i] + 1.0f) / 2.0f * (10.0f - 6.0f) + 6.0f;
  const float f = fb / 2.0f + fa / 2.0f;  // pitch_domain_specific/2 + pitch_domain_agnostic/2
  const float u = ub / 2.0f + ua / 2.0f;
  pitch_pred[(int64_t)i * 2 + 0] = f;
  pitch_pred[(int64_t)i * 2 + 1] = u;
  float hz = exp2f(f);
  if (u > 0.0f) hz = 0.0f;
  if (mel2ph[i] == 0) hz = 0.0f;
  f0_denorm[i] = hz;
  coarse[i] = f0_to_coarse(hz);
}

// A GIVEN contour instead of the two predictors (the f0 is not None branch of stylesinger.py:230-241 with add_gmdiff_pitch's :301-311: both
// "predictors" return cat(f0, uv) unchanged, so pitch_pred = (f0/2 + f0/2, uv/2 + uv/2)); then denorm_f0 + f0_to_coarse as above. The note-rest rule
// (uv[midi == 0] = 1, :288,296) sits in the predicted branch only: the reference does not apply it to a given contour, and neither does this kernel.
__global__ void pitch_given_kernel(const float* __restrict__ f0_log2, const float* __restrict__ uv, const int64_t* __restrict__ mel2ph,
                                   float* __restrict__ pitch_pred, float* __restrict__ f0_denorm, int64_t* __restrict__ coarse, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float f = f0_log2[i] / 2.0f + f0_log2[i] / 2.0f;
  const float u = uv[i] / 2.0f + uv[i] / 2.0f;
  pitch_pred[(int64_t)i * 2 + 0] = f;
  pitch_pred[(int64_t)i * 2 + 1] = u;
  float hz = exp2f(f);
  if (u > 0.0f) hz = 0.0f;
  if (mel2ph[i] == 0) hz = 0.0f;
  f0_denorm[i] = hz;
  coarse[i] = f0_to_coarse(hz);
}

}  // namespace

extern "C" int ss_f0_bounds(const int64_t* midi, float* lo, float* hi, int n, void* stream) {
  SS_CHECK_ARG(midi && lo && hi && n > 0, "ss_f0_bounds: bad args");
  hipLaunchKernelGGL(f0_bounds_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, midi, lo, hi, n);
  SS_CHECK_LAUNCH("ss_f0_bounds");
  return SS_OK;
}

extern "C" int ss_pitch_post(const float* f0_a, const int32_t* uv_a, const float* f0_b, const int32_t* uv_b,
                             const int64_t* midi, const int64_t* mel2ph, float* pitch_pred, float* f0_denorm,
                             int64_t* pitch_coarse, int n, void* stream) {
  SS_CHECK_ARG(f0_a && uv_a && f0_b && uv_b && midi && mel2ph && pitch_pred && f0_denorm && pitch_coarse && n > 0,
               "ss_pitch_post: bad args");
  hipLaunchKernelGGL(pitch_post_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, f0_a, uv_a, f0_b, uv_b,
                     midi, mel2ph, pitch_pred, f0_denorm, pitch_coarse, n);
  SS_CHECK_LAUNCH("ss_pitch_post");
  return SS_OK;
}

extern "C" int ss_pitch_given(const float* f0_log2, const float* uv, const int64_t* mel2ph, float* pitch_pred, float* f0_denorm,
                              int64_t* pitch_coarse, int n, void* stream) {
  SS_CHECK_ARG(f0_log2 && uv && mel2ph && pitch_pred && f0_denorm && pitch_coarse, "ss_pitch_given: null pointer");
  SS_CHECK_ARG(n > 0, "ss_pitch_given: n=%d must be positive", n);
  hipLaunchKernelGGL(pitch_given_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, f0_log2, uv, mel2ph, pitch_pred,
                     f0_denorm, pitch_coarse, n);
  SS_CHECK_LAUNCH("ss_pitch_given");
  return SS_OK;
}
