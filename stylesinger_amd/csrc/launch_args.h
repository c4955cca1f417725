// Host-side helpers that fill the launch-argument structs (ss_conv_gemm_args / ss_gemm_bf16_args) of the denoiser stack, the samplers and the vocoder.
#pragma once
#include "common.h"
#include "../../include/stylesinger_hip.h"

inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
inline int round_up32(int x) { return (x + 31) / 32 * 32; }
// 256-thread blocks of a grid-stride elementwise launch over n elements
inline int grid_for(int64_t n) {
  int64_t g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

// what a launch of either argument struct starts from
template <class Args> inline Args zeroed_args(int B, int T, const int32_t* lens) {
  Args a;
  memset(&a, 0, sizeof(a));
  a.B = B;
  a.T = T;
  a.lens = lens;
  a.ntaps = 1;
  a.post_scale = 1.0f;
  a.mask_rows = 1;
  return a;
}
inline ss_conv_gemm_args base_args(int B, int T, const int32_t* lens) {
  ss_conv_gemm_args a = zeroed_args<ss_conv_gemm_args>(B, T, lens);
  a.a_scale = 1.0f;
  a.a_lrelu = 1.0f;
  a.pre_scale = 1.0f;
  return a;
}
inline ss_gemm_bf16_args base_args_h(const ss_wavenet* net, int B, int T, const int32_t* lens) {
  ss_gemm_bf16_args a = zeroed_args<ss_gemm_bf16_args>(B, T, lens);
  if (net->n_groups > 1) a.group_size = B / net->n_groups;
  return a;
}
// the A operand / the output / the residual operand of a launch (either argument struct) as [B][T][ld] rows
template <class Args, class P> inline void set_a(Args& a, P* p, int ld, int T) {
  a.A = p;
  a.lda = ld;
  a.a_batch_stride = (int64_t)T * ld;
}
template <class Args, class P> inline void set_c(Args& a, P* p, int ld, int T) {
  a.C = p;
  a.ldc = ld;
  a.c_batch_stride = (int64_t)T * ld;
}
template <class Args, class P> inline void set_r(Args& a, P* p, int ld, int T) {
  a.R = p;
  a.ldr = ld;
  a.r_batch_stride = (int64_t)T * ld;
}
// the three taps of a k = 3 conv of dilation d
template <class Args> inline void set_taps3(Args& a, int d) {
  a.ntaps = 3;
  a.tap_off[0] = -d;
  a.tap_off[1] = 0;
  a.tap_off[2] = d;
}
// paired nets: item b runs net b / group_size, whose weights / bias / A-operand bias live gs_* floats further
inline void set_groups(ss_conv_gemm_args& a, const ss_wavenet* net, int B, int64_t gs_w, int64_t gs_bias, int64_t gs_a_bias = 0) {
  if (net->n_groups <= 1) return;
  a.group_size = B / net->n_groups;
  a.w_group_stride = gs_w;
  a.bias_group_stride = gs_bias;
  a.a_bias_group_stride = gs_a_bias;
}
