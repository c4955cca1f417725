// The joint f0 / uv sampler: GaussianMultinomialDiffusion.sample (modules/diff/gaussian_multinomial_diffusion.py:922-942) with DDiffNet
// (net.py:215-266) over the residual stack of wavenet_stack.hip - the ancestral loop and the strided one, one tail launch per network evaluation.
#include "wavenet_stack.h"
#include "launch_args.h"
#include <cmath>
#include <vector>

using namespace ss_stack;

namespace {

// ---------------------------------------------------------------------------------------------
// f0 net input: x[:, :C/2] = w*f0 + b ; x[:, C/2:] = uv_embed[uv]   (net.py:249-252)
// ---------------------------------------------------------------------------------------------
__global__ void f0_input_kernel(const float* __restrict__ f0, const int32_t* __restrict__ uv,
                                const float* __restrict__ w_in, const float* __restrict__ b_in,
                                const float* __restrict__ uv_embed, float* __restrict__ X, int B, int T, int C,
                                const int32_t* __restrict__ lens, int group_size, int64_t gs_w, int64_t gs_b, int64_t gs_e) {
  const int half = C / 2;
  const int64_t total = (int64_t)B * T * C;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const int64_t r = i / C;
    const int b = (int)(r / T), t = (int)(r % T);
    const int g = group_size > 0 ? b / group_size : 0;
    float v;
    if (c < half) v = w_in[g * gs_w + c] * f0[r] + b_in[g * gs_b + c];
    else v = uv_embed[g * gs_e + (uv[r] != 0 ? 1 : 0) * half + (c - half)];
    if (lens && t >= lens[b]) v = 0.f;
    X[i] = v;
  }
}

__device__ __forceinline__ float log_add_exp(float a, float b) {
  const float m = fmaxf(a, b);
  return m + logf(expf(a - m) + expf(b - m));
}

// One reverse step of the joint sampler for one frame (gaussian_p_sample :326-333, p_sample :410-413,
// q_posterior :374-397, log_sample_categorical :447-452): (eps, l0, l1) = the network's three outputs for frame i = (b, t).
// `time` = the network time of the step: it addresses the Philox draw (the tape rows arrive already offset by it). `final_step` = the
// transition ends at x_0. The ancestral loop has final_step == (time == 0); a strided list (ss_f0diff_sample_strided) jumps time -> s with the
// coefficients of that gap in the same fields of F0StepCoef: alpha_{t|s} for alpha_t, cumprod alpha_s for cumprod alpha_{t-1}.
struct F0StepCoef {
  float recip, recipm1, c1, c2, sigma, log_alpha_t, log_1m_alpha_t, log_cp_tm1, log_1m_cp_tm1;
};
__device__ __forceinline__ void f0_update_row(float eps, float l0, float l1, int64_t i, int b, int t, int T, float& f0v, int32_t& uvv, float lo, float hi,
                                              const float* __restrict__ noise, const float* __restrict__ gumbel_u, const SsPhilox& rng, int time,
                                              bool final_step, const F0StepCoef& k) {
  const float LOG2 = 0.69314718055994530942f;
  const float LOG_TINY = -69.07755278982137f;  // log(1e-30) as torch computes log(clamp(onehot, 1e-30))
  float z = 0.f, u0, u1;
  if (noise) z = noise[i];
  if (gumbel_u) {
    u0 = gumbel_u[((int64_t)b * 2 + 0) * T + t];
    u1 = gumbel_u[((int64_t)b * 2 + 1) * T + t];
  }
  if (!noise || !gumbel_u) {
    uint32_t o[4];
    rng.gen((uint32_t)t, (uint32_t)b, (uint32_t)time, 0x46305556u, o);  // counter = (frame, item): invariant to T padding
    float z0, z1;
    ss_boxmuller(o[0], o[1], z0, z1);
    if (!noise) z = z0;
    if (!gumbel_u) {
      u0 = (float)(o[2] >> 8) * (1.0f / 16777216.0f);  // [0,1) like torch.rand
      u1 = (float)(o[3] >> 8) * (1.0f / 16777216.0f);
    }
  }
  // ---- Gaussian f0 ----
  const float x = f0v;
  float x0 = k.recip * x - k.recipm1 * eps;
  x0 = fminf(fmaxf(x0, lo), hi);
  const float mean = k.c1 * x0 + k.c2 * x;
  f0v = mean + k.sigma * z;
  // ---- multinomial uv ----
  const int cls = uvv != 0 ? 1 : 0;
  const float lx0 = cls == 0 ? 0.f : LOG_TINY, lx1 = cls == 1 ? 0.f : LOG_TINY;
  // log_softmax
  const float m = fmaxf(l0, l1);
  const float lse = logf(expf(l0 - m) + expf(l1 - m));
  const float p0 = (l0 - m) - lse, p1 = (l1 - m) - lse;
  float ev0, ev1;
  if (final_step) {   // the transition to x_0: no prior term (the reference's t == 0 row)
    ev0 = p0;
    ev1 = p1;
  } else {
    ev0 = log_add_exp(p0 + k.log_cp_tm1, k.log_1m_cp_tm1 - LOG2);
    ev1 = log_add_exp(p1 + k.log_cp_tm1, k.log_1m_cp_tm1 - LOG2);
  }
  const float un0 = ev0 + log_add_exp(lx0 + k.log_alpha_t, k.log_1m_alpha_t - LOG2);
  const float un1 = ev1 + log_add_exp(lx1 + k.log_alpha_t, k.log_1m_alpha_t - LOG2);
  const float mm = fmaxf(un0, un1);
  const float nlse = mm + logf(expf(un0 - mm) + expf(un1 - mm));
  const float q0 = un0 - nlse, q1 = un1 - nlse;
  const float g0 = -logf(-logf(u0 + 1e-30f) + 1e-30f);
  const float g1 = -logf(-logf(u1 + 1e-30f) + 1e-30f);
  uvv = (g1 + q1) > (g0 + q0) ? 1 : 0;  // argmax, first max wins ties
}

// The tail of an f0 network evaluation in ONE launch (round 4): output projection (C -> 3: a GEMV per frame, not matrix-core work - it ran on a
// 128x32 MFMA tile with 29 dead columns), the joint sampler update, and the NEXT evaluation's input row x[:, :C/2] = w*f0 + b ;
// x[:, C/2:] = uv_embed[uv] (net.py:249-252): 3 launches per step -> 1. 16 lanes per frame: lane j owns the float4s j, j + 16, ... of the row.
__global__ __launch_bounds__(256) void f0_tail_kernel(const SkipSrc src, int64_t gs_bskip, const float* __restrict__ w_final, const float* __restrict__ b_final,
                                                      float* __restrict__ f0, int32_t* __restrict__ uv, const float* __restrict__ lo,
                                                      const float* __restrict__ hi, const float* __restrict__ noise,
                                                      const float* __restrict__ gumbel_u, uint64_t seed, const uint64_t* __restrict__ seed_dev, int time,
                                                      int final_step, int B, int T, int C, F0StepCoef k, const float* __restrict__ w_in, const float* __restrict__ b_in,
                                                      const float* __restrict__ uv_embed, float* __restrict__ X, const int32_t* __restrict__ lens,
                                                      int group_size, int64_t gs_wf, int64_t gs_bf, int64_t gs_w, int64_t gs_b, int64_t gs_e) {
  const int64_t n = (int64_t)B * T;
  const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (i >= n) return;   // whole 16-lane groups leave together
  const int j = threadIdx.x & 15;
  const int b = (int)(i / T), t = (int)(i % T);
  const int g = group_size > 0 ? b / group_size : 0;
  const float* W = w_final + g * gs_wf;   // packed rows [n][Kp = C]
  const float* bsk = src.bias ? src.bias + g * gs_bskip : nullptr;
  const bool masked = lens && t >= lens[b];
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int q = j; q < C / 4; q += 16) {
    const float4 gv = skip_load4(src, bsk, i, C, 4 * q, masked);
    const float4 w0 = *reinterpret_cast<const float4*>(W + 4 * q), w1 = *reinterpret_cast<const float4*>(W + C + 4 * q),
                 w2 = *reinterpret_cast<const float4*>(W + 2 * C + 4 * q);
    a0 = fmaf(gv.w, w0.w, fmaf(gv.z, w0.z, fmaf(gv.y, w0.y, fmaf(gv.x, w0.x, a0))));
    a1 = fmaf(gv.w, w1.w, fmaf(gv.z, w1.z, fmaf(gv.y, w1.y, fmaf(gv.x, w1.x, a1))));
    a2 = fmaf(gv.w, w2.w, fmaf(gv.z, w2.z, fmaf(gv.y, w2.y, fmaf(gv.x, w2.x, a2))));
  }
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) {   // butterfly over the 16 lanes of the frame: every lane ends with the same three sums
    a0 += __shfl_xor(a0, o, 16);
    a1 += __shfl_xor(a1, o, 16);
    a2 += __shfl_xor(a2, o, 16);
  }
  const float* bf = b_final + g * gs_bf;
  const SsPhilox rng(seed + (seed_dev ? seed_dev[0] : 0ull));
  float f0v = f0[i];
  int32_t uvv = uv[i];
  // padded frames: eps / logits = 0 as the row-masked projection GEMM wrote them before this kernel replaced it (not 0 + b_final)
  f0_update_row(masked ? 0.f : a0 + bf[0], masked ? 0.f : a1 + bf[1], masked ? 0.f : a2 + bf[2], i, b, t, T, f0v, uvv, lo[i], hi[i], noise, gumbel_u, rng,
                time, final_step != 0, k);
  if (j == 0) {
    f0[i] = f0v;
    uv[i] = uvv;
  }
  if (X) {   // the next evaluation's input row (exactly f0_input_kernel's values)
    const int half = C / 2;
    const bool pad = lens && t >= lens[b];
    float* Xr = X + i * C;
    for (int q = j; q < C / 4; q += 16) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 4 * q + e;
        v[e] = c < half ? w_in[g * gs_w + c] * f0v + b_in[g * gs_b + c] : uv_embed[g * gs_e + (uvv != 0 ? 1 : 0) * half + (c - half)];
        if (pad) v[e] = 0.f;
      }
      *reinterpret_cast<float4*>(Xr + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

// the input row of a call's first evaluation; every later one is written by the previous step's tail kernel
int f0_first_input(const ss_wavenet* net, const float* f0, const int32_t* uv, const int32_t* lens, int B, int T, const WsLayout& w, hipStream_t stream) {
  const int C = net->C;
  const int gsz = net->n_groups > 1 ? B / net->n_groups : 0;
  hipLaunchKernelGGL(f0_input_kernel, dim3(grid_for((int64_t)B * T * C)), dim3(256), 0, stream, f0, uv, net->w_in, net->b_in, net->uv_embed, w.X, B, T, C,
                     lens, gsz, net->gs_w_in, net->gs_b_in, net->gs_uv_embed);
  SS_CHECK_LAUNCH("f0_input_kernel");
  return SS_OK;
}

// One evaluation of the f0 net at network time t (evaluation `eval` of its loop) and the joint update with the coefficients k of the transition
// that leaves t; noise_t / gumbel_t = the tape rows of time t (or NULL -> Philox at counter t); write_x: also the next evaluation's input row.
// Every stack form resolve_form returns ends here: run_residual_stack leaves relu(skip) in G or as split-K slices, f0_tail_kernel takes either.
int f0_step(const ss_wavenet* net, const StackForm& sf, float* f0, int32_t* uv, const float* lo, const float* hi, const int32_t* lens, int B, int T,
            const WsLayout& w, int t, int eval, bool final_step, const F0StepCoef& k, const float* noise_t, const float* gumbel_t, uint64_t seed,
            const uint64_t* seed_dev, bool write_x, hipStream_t stream) {
  const int C = net->C;
  const int64_t n = (int64_t)B * T;
  const int gsz = net->n_groups > 1 ? B / net->n_groups : 0;
  SS_PROPAGATE(run_residual_stack(net, sf, t, eval, lens, B, T, w, stream, true));
  // partials_ok: the skip GEMM left its split-K slices in w.KP and the tail kernel adds them
  const SkipSrc src = skip_src(net, sf, w, B, T);
  // output projection (C -> 3) + joint sampler update + the next evaluation's input row, one launch (f0_tail_kernel)
  hipLaunchKernelGGL(f0_tail_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, stream, src, net->gs_b_skipall, net->w_final, net->b_final, f0, uv, lo, hi,
                     noise_t, gumbel_t, seed, seed_dev, t, final_step ? 1 : 0, B, T, C, k, net->w_in, net->b_in, net->uv_embed, write_x ? w.X : nullptr, lens,
                     gsz, net->gs_w_final, net->gs_b_final, net->gs_w_in, net->gs_b_in, net->gs_uv_embed);
  SS_CHECK_LAUNCH("f0_tail_kernel");
  return SS_OK;
}

// what both f0 entry points (`who`) ask of the net beyond open_sampler: the 1 -> 3 DDiffNet, C a multiple of 64, one net or a pair
int open_f0_sampler(const char* who, const ss_wavenet* net, int B, int T, const float* cond, const int32_t* lens, void* ws, int64_t ws_bytes, int do_precompute,
                    hipStream_t stream, SamplerCtx& s) {
  SS_CHECK_ARG(net->out_dim == 3 && net->in_dim == 1, "%s: net must be the 1->3 DDiffNet", who);
  return open_sampler(who, net, B, T, cond, lens, ws, ws_bytes, 64, true, do_precompute != 0, stream, s);
}

}  // namespace

extern "C" int ss_f0diff_sample(const ss_wavenet* net, float* f0, int32_t* uv, const float* cond, const float* lo,
                                const float* hi, const int32_t* lens, int B, int T, const float* noise,
                                const float* gumbel_u, uint64_t seed, const uint64_t* seed_dev, int step_lo, int step_hi,
                                int do_precompute, void* ws, int64_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SS_CHECK_ARG(net && f0 && uv && cond && lo && hi && ws, "ss_f0diff_sample: null pointer");
  SS_CHECK_ARG(0 <= step_lo && step_lo <= step_hi && step_hi <= net->steps, "ss_f0diff_sample: bad step range");
  SamplerCtx s;
  SS_PROPAGATE(open_f0_sampler("ss_f0diff_sample", net, B, T, cond, lens, ws, ws_bytes, do_precompute, stream, s));
  const int64_t n = (int64_t)B * T;
  for (int t = step_hi - 1; t >= step_lo; --t) {
    if (t == step_hi - 1) SS_PROPAGATE(f0_first_input(net, f0, uv, lens, B, T, s.w, stream));
    const int tm1 = t > 0 ? t - 1 : 0;
    const F0StepCoef k = {net->sqrt_recip_ac[t], net->sqrt_recipm1_ac[t], net->post_c1[t], net->post_c2[t],
                          t > 0 ? expf(0.5f * net->post_logvar[t]) : 0.0f, net->log_alpha[t], net->log_1m_alpha[t],
                          net->log_cumprod_alpha[tm1], net->log_1m_cumprod_alpha[tm1]};
    SS_PROPAGATE(f0_step(net, s.sf, f0, uv, lo, hi, lens, B, T, s.w, t, net->steps - 1 - t, t == 0, k, noise ? noise + (int64_t)t * n : nullptr,
                         gumbel_u ? gumbel_u + (int64_t)t * n * 2 : nullptr, seed, seed_dev, t > step_lo, stream));
  }
  return SS_OK;
}

// ---------------------------------------------------------------------------------------------
// Strided joint f0 / uv sampler: network times ts[0] > ts[1] > ... ; the transition t -> s (s = the next entry; "final" = x_0 after the last,
// cumprod alpha = 1, Lambda = 0). With a_i = 1 - beta_i, ac = cumprod(a), Lambda = cumsum(log a), all in double:
//   Gaussian half (the DDIM family of ss_meldiff_sample_ddim, the dyn_clip clamp on x0 kept; ddim_coef):
//     sigma = eta sqrt((1 - ac_s)/(1 - ac_t)) sqrt(1 - ac_t/ac_s), c2 = sqrt(max(1 - ac_s - sigma^2, 0)/(1 - ac_t)), c1 = sqrt(ac_s) - c2 sqrt(ac_t)
//   multinomial half: the posterior q(x_s | x_t, x0) ~ q(x_t | x_s) q(x_s | x0) of the uniform-transition chain over the gap, i.e. f0_update_row
//     with alpha_{t|s} = ac_t/ac_s (log: Lambda_t - Lambda_s) for alpha_t and ac_s (log: Lambda_s) for ac_{t-1}; log(1 - .) in multinomial_schedule's
//     1e-40 form; the final transition takes no prior term.
// Stride 1 with eta = 1 is the reference's own step (posterior_mean_coef1/2, posterior variance, log_alpha, log_cumprod_alpha[t-1]).
// ---------------------------------------------------------------------------------------------
namespace {
struct F0Schedule {
  std::vector<double> ac, lam;   // cumprod(1 - beta), cumsum(log(1 - beta))
};
// false: a beta that is not finite or not inside (0, 1) (bad = its index)
bool f0_schedule(const double* betas, int steps, F0Schedule& sc, int& bad) {
  sc.ac.resize(steps);
  sc.lam.resize(steps);
  double p = 1.0, l = 0.0;
  for (int i = 0; i < steps; ++i) {
    const double b = betas[i];
    if (!(std::isfinite(b) && b > 0.0 && b < 1.0)) {
      bad = i;
      return false;
    }
    p *= 1.0 - b;
    l += log(1.0 - b);
    sc.ac[i] = p;
    sc.lam[i] = l;
  }
  return true;
}
F0StepCoef f0_strided_coef(const F0Schedule& sc, int t, int s, double eta) {
  const double ac_t = sc.ac[t], ac_s = s >= 0 ? sc.ac[s] : 1.0;
  const double lam_t = sc.lam[t], lam_s = s >= 0 ? sc.lam[s] : 0.0;
  const DdimCoef g = ddim_coef(ac_t, ac_s, eta);
  const double la = lam_t - lam_s;
  F0StepCoef k;
  k.recip = (float)sqrt(1.0 / ac_t);
  k.recipm1 = (float)sqrt(1.0 / ac_t - 1.0);
  k.c1 = (float)g.c1;
  k.c2 = (float)g.c2;
  k.sigma = (float)g.sigma;
  k.log_alpha_t = (float)la;
  k.log_1m_alpha_t = (float)log(1.0 - exp(la) + 1e-40);
  k.log_cp_tm1 = (float)lam_s;
  k.log_1m_cp_tm1 = (float)log(1.0 - exp(lam_s) + 1e-40);
  return k;
}
}  // namespace

extern "C" int ss_f0_strided_coef(const double* betas, int steps, int t, int s, float eta, float* out9) {
  SS_CHECK_ARG(betas && out9, "ss_f0_strided_coef: null pointer");
  SS_CHECK_ARG(steps >= 1, "ss_f0_strided_coef: steps=%d must be positive", steps);
  SS_CHECK_ARG(0 <= t && t < steps && -1 <= s && s < t, "ss_f0_strided_coef: transition %d -> %d: need -1 <= s < t < steps=%d (s = -1: final)", t, s, steps);
  SS_CHECK_ARG(eta >= 0.0f && eta <= 1.0f, "ss_f0_strided_coef: eta=%g outside [0, 1]", (double)eta);
  F0Schedule sc;
  int bad = 0;
  SS_CHECK_ARG(f0_schedule(betas, steps, sc, bad), "ss_f0_strided_coef: betas[%d]=%g is not a finite value inside (0, 1)", bad, betas[bad]);
  const F0StepCoef k = f0_strided_coef(sc, t, s, (double)eta);
  const float v[9] = {k.recip, k.recipm1, k.c1, k.c2, k.sigma, k.log_alpha_t, k.log_1m_alpha_t, k.log_cp_tm1, k.log_1m_cp_tm1};
  for (int i = 0; i < 9; ++i) out9[i] = v[i];
  return SS_OK;
}

extern "C" int ss_f0diff_sample_strided(const ss_wavenet* net, float* f0, int32_t* uv, const float* cond, const float* lo, const float* hi,
                                        const int32_t* lens, int B, int T, const int32_t* ts, int n_ts, int i_lo, int i_hi, const double* betas,
                                        float eta, const float* noise, const float* gumbel_u, uint64_t seed, const uint64_t* seed_dev,
                                        int do_precompute, void* ws, int64_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SS_CHECK_ARG(net && f0 && uv && cond && lo && hi && ws && ts && betas, "ss_f0diff_sample_strided: null pointer");
  SS_CHECK_ARG(n_ts >= 1, "ss_f0diff_sample_strided: n_ts=%d must be positive", n_ts);
  SS_CHECK_ARG(net->steps >= 1, "ss_f0diff_sample_strided: net has no schedule (steps=%d)", net->steps);
  for (int i = 0; i < n_ts; ++i)
    SS_CHECK_ARG(ts[i] >= 0 && ts[i] < net->steps && (i == 0 || ts[i] < ts[i - 1]),
                 "ss_f0diff_sample_strided: ts must be strictly decreasing in [0, steps=%d) (ts[%d]=%d)", net->steps, i, ts[i]);
  SS_CHECK_ARG(0 <= i_lo && i_lo <= i_hi && i_hi <= n_ts, "ss_f0diff_sample_strided: bad position range [%d, %d) of %d", i_lo, i_hi, n_ts);
  SS_CHECK_ARG(eta >= 0.0f && eta <= 1.0f, "ss_f0diff_sample_strided: eta=%g outside [0, 1]", (double)eta);
  F0Schedule sc;
  int bad = 0;
  SS_CHECK_ARG(f0_schedule(betas, net->steps, sc, bad), "ss_f0diff_sample_strided: betas[%d]=%g is not a finite value inside (0, 1)", bad, betas[bad]);
  SamplerCtx s;
  SS_PROPAGATE(open_f0_sampler("ss_f0diff_sample_strided", net, B, T, cond, lens, ws, ws_bytes, do_precompute, stream, s));
  const int64_t n = (int64_t)B * T;
  const bool draw = eta > 0.0f;   // eta = 0: sigma = 0 on every transition and the Gaussian tape is never read
  for (int i = i_lo; i < i_hi; ++i) {
    if (i == i_lo) SS_PROPAGATE(f0_first_input(net, f0, uv, lens, B, T, s.w, stream));
    const int t = ts[i];
    const bool final_step = i + 1 == n_ts;   // the list's last entry, wherever the call is cut
    const F0StepCoef k = f0_strided_coef(sc, t, final_step ? -1 : ts[i + 1], (double)eta);
    // evaluation i of the loop; tape rows and the Philox counter are those of network time t
    SS_PROPAGATE(f0_step(net, s.sf, f0, uv, lo, hi, lens, B, T, s.w, t, i, final_step, k, (draw && noise) ? noise + (int64_t)t * n : nullptr,
                         gumbel_u ? gumbel_u + (int64_t)t * n * 2 : nullptr, seed, seed_dev, i + 1 < i_hi, stream));
  }
  return SS_OK;
}
