// The mel samplers: DiffusionDecoder.forward (modules/diff/shallow_diffusion_tts.py:285-307) with DiffNet (modules/diff/net.py:81-130) over the
// residual stack of wavenet_stack.hip - the ancestral loop, the ProDiff teacher, the strided (DDIM-family) and the PLMS loop, and the q_sample /
// denorm launches at their two ends.
#include "wavenet_stack.h"
#include "launch_args.h"

using namespace ss_stack;

namespace {

// q_sample of the normalised coarse mel
__global__ void mel_qsample_kernel(const float* __restrict__ mel, const float* __restrict__ smin,
                                   const float* __restrict__ smax, float sa, float s1, const float* __restrict__ noise,
                                   uint64_t seed, const uint64_t* __restrict__ seed_dev, float* __restrict__ x, int64_t rows,
                                   int T, int M) {
  const SsPhilox rng(seed + (seed_dev ? seed_dev[0] : 0ull));
  const int64_t n = rows * M;
  const int64_t per_item = (int64_t)T * M;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % M);
    const float xs = (mel[i] - smin[c]) / (smax[c] - smin[c]) * 2.0f - 1.0f;
    float z;
    if (noise) z = noise[i];
    else {
      uint32_t o[4];
      rng.gen((uint32_t)(i % per_item), (uint32_t)(i / per_item), 0xffffffffu, 0x4d454c44u, o);  // (element of item, item)
      float z1;
      ss_boxmuller(o[0], o[1], z, z1);
    }
    x[i] = sa * xs + s1 * z;
  }
}

__global__ void mel_denorm_kernel(const float* __restrict__ x, const float* __restrict__ smin,
                                  const float* __restrict__ smax, float* __restrict__ mel, int B, int T, int M,
                                  const int32_t* __restrict__ lens, int32_t* __restrict__ nonfinite) {
  const int64_t n = (int64_t)B * T * M;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % M);
    const int64_t r = i / M;
    const int b = (int)(r / T), t = (int)(r % T);
    float v = (x[i] + 1.0f) / 2.0f * (smax[c] - smin[c]) + smin[c];
    if (lens && t >= lens[b]) v = 0.f;
    else if (nonfinite && !isfinite(v)) atomicOr(nonfinite, 1);   // a valid frame left the number range (fp16 modes: the stream overflowed)
    mel[i] = v;
  }
}

// x_in -> w.X = relu(input_projection(x_in))  (net.py:114-116)
int mel_input_proj(const ss_wavenet* net, const float* x_in, const int32_t* lens, int B, int T, const WsLayout& w, hipStream_t stream) {
  const int C = net->C, M = net->in_dim;
  ss_conv_gemm_args a = base_args(B, T, lens);
  set_a(a, x_in, M, T);
  a.Cin = M;
  a.W = net->w_in;
  a.N = C;
  a.Np = round_up32(C);
  a.Kp = round_up32(M);
  a.epi = SS_EPI_STORE;
  a.bias = net->b_in;
  a.act = SS_ACT_RELU;
  set_c(a, w.X, C, T);
  return ss_conv_gemm(&a, stream);
}

// The tail of a mel network evaluation for SMALL launches (one short utterance: the B = 1 latency shape) in ONE launch: output projection
// (C -> M), the DDPM posterior step on x (shallow_diffusion_tts.py:130-162; same tape / Philox counters as the SS_EPI_DDPM epilogue) and the
// NEXT evaluation's input projection relu(W_in x + b) - two 16-20 us MFMA launches of 24-48 workgroups become one ~8 us VALU launch. Exact
// fp32 FMAs; only the summation order over K differs from the matrix-core form. MTR = 2 frames per workgroup.
__global__ __launch_bounds__(256) void mel_tail_kernel(const SkipSrc src, const float* __restrict__ Wf, const float* __restrict__ bf,
                                                       float* __restrict__ x, const float* __restrict__ noise, uint64_t seed,
                                                       const uint64_t* __restrict__ seed_dev, uint32_t step, float recip, float recipm1, float c1,
                                                       float c2, float sigma, const float* __restrict__ Win, const float* __restrict__ bin,
                                                       float* __restrict__ X, const int32_t* __restrict__ lens, int B, int T, int C, int M, int Kp_in) {
  extern __shared__ __attribute__((aligned(16))) float smem_mt[];
  float* gs = smem_mt;            // [MTR][C]
  float* xs = smem_mt + MTR * C;    // [MTR][Kp_in] (zero padded beyond M)
  const int64_t n_rows = (int64_t)B * T, r0 = (int64_t)blockIdx.x * MTR;
  const int tid = threadIdx.x, C4 = C / 4;
  for (int idx = tid; idx < MTR * C4; idx += 256) {
    const int row = idx / C4, q = idx - row * C4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + row < n_rows) {
      const int64_t i = r0 + row;
      v = skip_load4(src, src.bias, i, C, 4 * q, lens && (int)(i % T) >= lens[i / T]);
    }
    *reinterpret_cast<float4*>(gs + row * C + 4 * q) = v;
  }
  for (int idx = tid; idx < MTR * Kp_in; idx += 256) xs[idx] = 0.f;
  __syncthreads();
  const SsPhilox rng(seed + (seed_dev ? seed_dev[0] : 0ull));
  for (int idx = tid; idx < MTR * M; idx += 256) {
    const int row = idx / M, n = idx - row * M;
    const int64_t i = r0 + row;
    if (i >= n_rows) continue;
    const float* wr = Wf + (int64_t)n * C;
    const float* gr = gs + row * C;
    float acc = 0.f;
#pragma unroll 8
    for (int q = 0; q < C4; ++q) {
      const float4 wv = *reinterpret_cast<const float4*>(wr + 4 * q), gv = *reinterpret_cast<const float4*>(gr + 4 * q);
      acc = fmaf(gv.w, wv.w, fmaf(gv.z, wv.z, fmaf(gv.y, wv.y, fmaf(gv.x, wv.x, acc))));
    }
    const float eps = acc + bf[n];
    const int b = (int)(i / T), t = (int)(i % T);
    const float xv = x[i * M + n];
    float z = 0.f;
    if (sigma != 0.f) {
      if (noise) z = noise[i * M + n];
      else {
        float z4[4];   // exactly the SS_EPI_DDPM epilogue's draw: output t & 3 of the block of frames 4 (t >> 2) .. + 3 of this bin
        ss_mel_draw4(rng, (uint32_t)(t >> 2), (uint32_t)M, (uint32_t)n, (uint32_t)b, step, z4);
        z = z4[t & 3];
      }
    }
    float xn = ss_ddpm_update(xv, eps, recip, recipm1, c1, c2, sigma, z, 0);   // the epilogue's update, rounding for rounding
    if (lens && t >= lens[b]) xn = 0.f;
    x[i * M + n] = xn;
    xs[row * Kp_in + n] = xn;
  }
  if (!X) return;   // block-uniform
  __syncthreads();
  const int K4 = Kp_in / 4;   // W_in is packed [C][Kp_in], zero filled beyond M
  for (int c = tid; c < C; c += 256) {
    float acc[MTR];
#pragma unroll
    for (int r = 0; r < MTR; ++r) acc[r] = 0.f;
    const float* wr = Win + (int64_t)c * Kp_in;
#pragma unroll 8
    for (int q = 0; q < K4; ++q) {
      const float4 wv = *reinterpret_cast<const float4*>(wr + 4 * q);
#pragma unroll
      for (int r = 0; r < MTR; ++r) {
        const float4 xv = *reinterpret_cast<const float4*>(xs + r * Kp_in + 4 * q);
        acc[r] = fmaf(xv.w, wv.w, fmaf(xv.z, wv.z, fmaf(xv.y, wv.y, fmaf(xv.x, wv.x, acc[r]))));
      }
    }
    const float bc = bin[c];
#pragma unroll
    for (int r = 0; r < MTR; ++r) {
      const int64_t i = r0 + r;
      if (i >= n_rows) continue;
      const int b = (int)(i / T), t = (int)(i % T);
      float v = fmaxf(acc[r] + bc, 0.f);
      if (lens && t >= lens[b]) v = 0.f;
      X[i * C + c] = v;
    }
  }
}

// One network evaluation DiffNet(x_in, t, cond) up to its output projection: x_in -> relu(input_projection) -> residual stack -> the arguments of
// eps = output_projection(.) into out [B][T][M], whose epilogue the caller chooses  (net.py:114-130). eval: see run_residual_stack
int mel_net_body(const ss_wavenet* net, const StackForm& sf, const float* x_in, float* out, const int32_t* lens, int B, int T, const WsLayout& w,
                 int t, int eval, hipStream_t stream, ss_conv_gemm_args& f) {
  const int C = net->C, M = net->in_dim;
  SS_PROPAGATE(mel_input_proj(net, x_in, lens, B, T, w, stream));
  SS_PROPAGATE(run_residual_stack(net, sf, t, eval, lens, B, T, w, stream));
  f = base_args(B, T, lens);
  set_a(f, w.G, C, T);
  f.Cin = C;
  f.W = net->w_final;
  f.N = M;
  f.Np = round_up32(M);
  f.Kp = round_up32(C);
  f.bias = net->b_final;
  set_c(f, out, M, T);
  return SS_OK;
}

// eps_out [B][T][M] = DiffNet(x_in, t, cond)  (plain output projection, for samplers that keep a history of eps)
int mel_eps(const ss_wavenet* net, const StackForm& sf, const float* x_in, float* eps_out, const int32_t* lens, int B, int T, const WsLayout& w,
            int t, int eval, hipStream_t stream) {
  ss_conv_gemm_args f;
  SS_PROPAGATE(mel_net_body(net, sf, x_in, eps_out, lens, B, T, w, t, eval, stream, f));
  f.epi = SS_EPI_STORE;
  f.mask_rows = 0;
  return ss_conv_gemm(&f, stream);
}

// One reverse step of the mel net at network time `t` with explicit update coefficients
//   x0 = clamp(recip*x - recipm1*eps, -1, 1) ; x <- c1*x0 + c2*x + sigma*z
int mel_step(const ss_wavenet* net, const StackForm& sf, float* x, const int32_t* lens, int B, int T, const WsLayout& w, int t, int eval,
             float recip, float recipm1, float c1, float c2, float sigma, const float* noise_t, uint64_t seed,
             const uint64_t* seed_dev, uint32_t step_id, hipStream_t stream, int x0_pred = 0) {
  ss_conv_gemm_args f;
  SS_PROPAGATE(mel_net_body(net, sf, x, x, lens, B, T, w, t, eval, stream, f));
  f.epi = SS_EPI_DDPM;   // eps = output_projection(.) fused with the posterior step (shallow_diffusion_tts.py:130-162)
  f.ddpm_recip = recip;
  f.ddpm_recipm1 = recipm1;
  f.ddpm_c1 = c1;
  f.ddpm_c2 = c2;
  f.ddpm_sigma = sigma;
  f.noise = noise_t;
  f.seed = seed;
  f.seed_dev = seed_dev;
  f.step = step_id;
  f.ddpm_x0_pred = x0_pred;
  return ss_conv_gemm(&f, stream);
}

}  // namespace

extern "C" int ss_meldiff_sample(const ss_wavenet* net, float* x, const float* cond, const int32_t* lens, int B, int T,
                                 const float* noise, uint64_t seed, const uint64_t* seed_dev, int step_lo, int step_hi,
                                 int do_precompute, void* ws, int64_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SS_CHECK_ARG(net && x && cond && ws, "ss_meldiff_sample: null pointer");
  SS_CHECK_ARG(0 <= step_lo && step_lo <= step_hi && step_hi <= net->steps, "ss_meldiff_sample: bad step range");
  SamplerCtx s;
  SS_PROPAGATE(open_sampler("ss_meldiff_sample", net, B, T, cond, lens, ws, ws_bytes, 32, false, do_precompute != 0, stream, s));
  const StackForm& sf = s.sf;
  const WsLayout& w = s.w;
  const int M = net->in_dim, C = net->C;
  const int Kp_in = round_up32(M);
  for (int t = step_hi - 1; t >= step_lo; --t) {
    const int eval = net->steps - 1 - t;   // evaluation index of the whole loop, whatever [step_lo, step_hi) this call covers
    const float sigma = t > 0 ? expf(0.5f * net->post_logvar[t]) : 0.0f;
    const float* noise_t = noise ? noise + (int64_t)t * B * T * M : nullptr;
    if (!sf.mel_tail) {
      SS_PROPAGATE(mel_step(net, sf, x, lens, B, T, w, t, eval, net->sqrt_recip_ac[t], net->sqrt_recipm1_ac[t], net->post_c1[t], net->post_c2[t], sigma, noise_t,
                            seed, seed_dev, (uint32_t)t, stream));
      continue;
    }
    // launches that leave most CUs idle (one short utterance): the two small projections around the sampler update run as ONE VALU launch
    if (t == step_hi - 1) SS_PROPAGATE(mel_input_proj(net, x, lens, B, T, w, stream));   // later evaluations get their input from the tail kernel
    SS_PROPAGATE(run_residual_stack(net, sf, t, eval, lens, B, T, w, stream, true));
    const SkipSrc src = skip_src(net, sf, w, B, T);
    hipLaunchKernelGGL(mel_tail_kernel, dim3((unsigned)(((int64_t)B * T + MTR - 1) / MTR)), dim3(256), (size_t)(MTR * C + MTR * Kp_in) * 4, stream, src, net->w_final,
                       net->b_final, x, noise_t, seed, seed_dev, (uint32_t)t, net->sqrt_recip_ac[t], net->sqrt_recipm1_ac[t], net->post_c1[t],
                       net->post_c2[t], sigma, net->w_in, net->b_in, t > step_lo ? w.X : nullptr, lens, B, T, C, M, Kp_in);
    SS_CHECK_LAUNCH("mel_tail_kernel");
  }
  return SS_OK;
}

// ProDiff teacher sampler: same launches as ss_meldiff_sample, the final GEMM's epilogue takes the network output as x0.
extern "C" int ss_prodiff_sample(const ss_wavenet* net, float* x, const float* cond, const int32_t* lens, int B, int T,
                                 const float* noise, uint64_t seed, const uint64_t* seed_dev, int n_steps, const float* c1,
                                 const float* c2, const float* sigma, int do_precompute, void* ws, int64_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SS_CHECK_ARG(net && x && cond && ws && c1 && c2 && sigma, "ss_prodiff_sample: null pointer");
  SS_CHECK_ARG(n_steps >= 1 && n_steps <= net->steps, "ss_prodiff_sample: n_steps=%d outside [1, %d]", n_steps, net->steps);
  SamplerCtx s;
  SS_PROPAGATE(open_sampler("ss_prodiff_sample", net, B, T, cond, lens, ws, ws_bytes, 32, false, do_precompute != 0, stream, s));
  const int M = net->in_dim;
  for (int t = n_steps - 1; t >= 0; --t) {
    SS_PROPAGATE(mel_step(net, s.sf, x, lens, B, T, s.w, t, n_steps - 1 - t, 0.0f, 0.0f, c1[t], c2[t], t > 0 ? sigma[t] : 0.0f,
                          noise ? noise + (int64_t)t * B * T * M : nullptr, seed, seed_dev, (uint32_t)t, stream, 1));
  }
  return SS_OK;
}

// Strided sampler (DDIM family, Song et al. 2021 eq. 12 / 16) over the SAME denoiser: visits network times ts[0] > ts[1] > ... and jumps
// x_{ts[i]} -> x_{ts[i+1]} (-> x_0 after the last).  With x0 = clamp(...), eps' = (x - sqrt(ac_t) x0)/sqrt(1-ac_t) and
//   sigma = eta * sqrt((1-ac_prev)/(1-ac_t)) * sqrt(1 - ac_t/ac_prev):
//   x_prev = sqrt(ac_prev) x0 + sqrt(1-ac_prev-sigma^2) eps' + sigma z = c1 x0 + c2 x + sigma z,
//   c2 = sqrt((1-ac_prev-sigma^2)/(1-ac_t)), c1 = sqrt(ac_prev) - c2 sqrt(ac_t)   (ddim_coef)
// i.e. the DDPM epilogue with other coefficients.  eta = 0 is the deterministic sampler of BASELINE config 5 (the reference has none);
// eta = 1 with ts = K-1 ... 0 IS the reference's ancestral p_sample (shallow_diffusion_tts.py:136-162: c1, c2 become
// posterior_mean_coef1/2 and sigma^2 the posterior variance), which is how this entry point is pinned to the reference
// (golden acoustic_t64_s100).  The schedule comes in DOUBLE precision (1 - ac_prev loses its digits in a float table at small t).
extern "C" int ss_meldiff_sample_ddim(const ss_wavenet* net, float* x, const float* cond, const int32_t* lens, int B, int T,
                                      const int32_t* ts, int n_ts, const double* alphas_cumprod, float eta, const float* noise,
                                      uint64_t seed, const uint64_t* seed_dev, int do_precompute, void* ws, int64_t ws_bytes,
                                      void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SS_CHECK_ARG(net && x && cond && ws && ts && alphas_cumprod && n_ts > 0, "ss_meldiff_sample_ddim: null pointer");
  SS_CHECK_ARG(eta >= 0.0f && eta <= 1.0f, "ss_meldiff_sample_ddim: eta=%g outside [0, 1]", (double)eta);
  for (int i = 0; i < n_ts; ++i)
    SS_CHECK_ARG(ts[i] >= 0 && ts[i] < net->steps && (i == 0 || ts[i] < ts[i - 1]), "ss_meldiff_sample_ddim: ts must be strictly decreasing in [0,steps)");
  SamplerCtx s;
  SS_PROPAGATE(open_sampler("ss_meldiff_sample_ddim", net, B, T, cond, lens, ws, ws_bytes, 1, false, do_precompute != 0, stream, s));
  const int M = net->in_dim;
  for (int i = 0; i < n_ts; ++i) {
    const int t = ts[i];
    const DdimCoef k = ddim_coef(alphas_cumprod[t], (i + 1 < n_ts) ? alphas_cumprod[ts[i + 1]] : 1.0, (double)eta);
    const bool draw = eta > 0.0f;  // like p_sample, a stochastic run draws at every step (sigma = 0 on the last)
    SS_PROPAGATE(mel_step(net, s.sf, x, lens, B, T, s.w, t, i, net->sqrt_recip_ac[t], net->sqrt_recipm1_ac[t], (float)k.c1, (float)k.c2, (float)k.sigma,
                          (draw && noise) ? noise + (int64_t)t * B * T * M : nullptr, seed, draw ? seed_dev : nullptr, (uint32_t)t, stream));
  }
  return SS_OK;
}

// ---------------------------------------------------------------------------------------------
// DPM-Solver++ multistep sampler (Lu et al. 2022, "DPM-Solver++", Algorithm 2: data prediction, 2M) over the strided list of the DDIM entry.
// With alpha = sqrt(ac), sigma = sqrt(1 - ac), lambda = log(alpha / sigma), h = lambda_s - lambda_t and x0_i the clamped x0 prediction at ts[i]
// (ss_ddpm_update's own expression), the transition t = ts[i] -> s = ts[i+1] is
//   order 1:  x' = c1 x0_i + c2 x,  (c1, c2) = ddim_coef(ac_t, ac_s, 0) = (-alpha_s (e^-h - 1), sigma_s / sigma_t): DDIM with eta = 0
//   order 2:  x' = b0 x0_i + b1 x0_{i-1} + c2 x,  r = (lambda_t - lambda_{ts[i-1]}) / h,  b0 = c1 (1 + 1/(2r)),  b1 = -c1 / (2r)
// Order 2 needs a previous x0 and a finite h: the first transition of a list and the last one (to x_0: h = inf) are first order, the last one
// through the fused DDPM epilogue exactly as DDIM's. Every other position is one plain evaluation (mel_eps) and one update launch.
// ---------------------------------------------------------------------------------------------
namespace {
// x0 as ss_ddpm_update forms it, then x' = fma(b1, x0_prev, fma(b0, x0, c2 * x)) (second) or fma(b0, x0, c2 * x)
__device__ __forceinline__ float dpmpp_update(float x, float eps, float x0_prev, float recip, float recipm1, float b0, float b1, float c2, bool second,
                                              float& x0_out) {
#pragma clang fp contract(off)
  const float a = recip * x, b = recipm1 * eps;
  const float x0 = fminf(fmaxf(a - b, -1.0f), 1.0f);
  const float c2x = c2 * x;
  float xn = __builtin_fmaf(b0, x0, c2x);
  if (second) xn = __builtin_fmaf(b1, x0_prev, xn);
  x0_out = x0;
  return xn;
}

// One thread per float4 of [B][T][M] (M a multiple of 4: a float4 never straddles a row); the grid covers all n4 of them. x and x0 (the history,
// read as x0_prev when `second`) are updated in place; rows t >= lens[b] of both are written as 0.
__global__ __launch_bounds__(256) void dpmpp_update_kernel(float4* __restrict__ x, const float4* __restrict__ eps, float4* __restrict__ x0h,
                                                           const int32_t* __restrict__ lens, int64_t n4, int T, int M4, float recip, float recipm1,
                                                           float b0, float b1, float c2, int second) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const int64_t row = i / M4;
  const int b = (int)(row / T), t = (int)(row % T);
  if (lens && t >= lens[b]) {
    x[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    x0h[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const float4 xv = x[i], ev = eps[i];
  const float4 pv = second ? x0h[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 xn, x0;
  xn.x = dpmpp_update(xv.x, ev.x, pv.x, recip, recipm1, b0, b1, c2, second != 0, x0.x);
  xn.y = dpmpp_update(xv.y, ev.y, pv.y, recip, recipm1, b0, b1, c2, second != 0, x0.y);
  xn.z = dpmpp_update(xv.z, ev.z, pv.z, recip, recipm1, b0, b1, c2, second != 0, x0.z);
  xn.w = dpmpp_update(xv.w, ev.w, pv.w, recip, recipm1, b0, b1, c2, second != 0, x0.w);
  x[i] = xn;
  x0h[i] = x0;
}

inline double half_logsnr(double ac) { return 0.5 * log(ac / (1.0 - ac)); }
}  // namespace

extern "C" int ss_meldiff_sample_dpmpp(const ss_wavenet* net, float* x, const float* cond, const int32_t* lens, int B, int T, const int32_t* ts,
                                       int n_ts, int i_lo, int i_hi, const double* alphas_cumprod, int order, float* hist, int do_precompute,
                                       void* ws, int64_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SS_CHECK_ARG(net && x && cond && ws && ts && alphas_cumprod && hist, "ss_meldiff_sample_dpmpp: null pointer");
  SS_CHECK_ARG(n_ts >= 1, "ss_meldiff_sample_dpmpp: n_ts=%d must be positive", n_ts);
  for (int i = 0; i < n_ts; ++i)
    SS_CHECK_ARG(ts[i] >= 0 && ts[i] < net->steps && (i == 0 || ts[i] < ts[i - 1]),
                 "ss_meldiff_sample_dpmpp: ts must be strictly decreasing in [0, steps=%d) (ts[%d]=%d)", net->steps, i, ts[i]);
  SS_CHECK_ARG(0 <= i_lo && i_lo <= i_hi && i_hi <= n_ts, "ss_meldiff_sample_dpmpp: bad position range [%d, %d) of %d", i_lo, i_hi, n_ts);
  SS_CHECK_ARG(order == 1 || order == 2, "ss_meldiff_sample_dpmpp: order=%d must be 1 or 2", order);
  SS_CHECK_ARG(net->in_dim > 0 && net->in_dim % 4 == 0, "ss_meldiff_sample_dpmpp: in_dim=%d must be a multiple of 4 (one float4 per thread)", net->in_dim);
  SS_CHECK_ARG(((uintptr_t)x | (uintptr_t)hist) % 16 == 0, "ss_meldiff_sample_dpmpp: x and hist must be 16-byte aligned");
  SamplerCtx s;
  SS_PROPAGATE(open_sampler("ss_meldiff_sample_dpmpp", net, B, T, cond, lens, ws, ws_bytes, 1, false, do_precompute != 0, stream, s));
  const int M = net->in_dim;
  const int64_t n = (int64_t)B * T * M, n4 = n / 4;
  float* eps = hist;        // the evaluation's output
  float* x0h = hist + n;    // x0 of the previous position
  const int64_t blocks = (n4 + 255) / 256;
  SS_CHECK_ARG(blocks <= 0x7fffffff, "ss_meldiff_sample_dpmpp: B*T*in_dim=%lld is beyond one grid", (long long)n);
  for (int i = i_lo; i < i_hi; ++i) {
    const int t = ts[i];
    const bool last = i + 1 == n_ts;   // the list's last entry, wherever the call is cut
    const DdimCoef k = ddim_coef(alphas_cumprod[t], last ? 1.0 : alphas_cumprod[ts[i + 1]], 0.0);
    if (last) {   // to x_0: first order, the fused epilogue (DDIM's last transition, launch for launch)
      SS_PROPAGATE(mel_step(net, s.sf, x, lens, B, T, s.w, t, i, net->sqrt_recip_ac[t], net->sqrt_recipm1_ac[t], (float)k.c1, (float)k.c2, 0.0f, nullptr, 0, nullptr,
                            (uint32_t)t, stream));
      continue;
    }
    double b0 = k.c1, b1 = 0.0;
    const bool second = order == 2 && i > 0;
    if (second) {
      const double lam_t = half_logsnr(alphas_cumprod[t]);
      const double r = (lam_t - half_logsnr(alphas_cumprod[ts[i - 1]])) / (half_logsnr(alphas_cumprod[ts[i + 1]]) - lam_t);
      b0 = k.c1 * (1.0 + 1.0 / (2.0 * r));
      b1 = -k.c1 / (2.0 * r);
    }
    SS_PROPAGATE(mel_eps(net, s.sf, x, eps, lens, B, T, s.w, t, i, stream));
    hipLaunchKernelGGL(dpmpp_update_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, reinterpret_cast<float4*>(x), reinterpret_cast<const float4*>(eps),
                       reinterpret_cast<float4*>(x0h), lens, n4, T, M / 4, net->sqrt_recip_ac[t], net->sqrt_recipm1_ac[t], (float)b0, (float)b1, (float)k.c2,
                       second ? 1 : 0);
    SS_CHECK_LAUNCH("dpmpp_update_kernel");
  }
  return SS_OK;
}

// ---------------------------------------------------------------------------------------------
// PLMS / "pndm_speedup" sampler of the reference (shallow_diffusion_tts.py:165-197 p_sample_plms, loop :254-260):
//   x_prev = x + (a_prev - a_t) * (kx * x - ke * eps'),  eps' = linear multistep combination of the eps history.
// The reference runs it for one utterance at a time (its `max(t - interval, 0)` on a tensor only works for B = 1).
// ---------------------------------------------------------------------------------------------
namespace {
__global__ void plms_update_kernel(const float* __restrict__ x, float* __restrict__ x_out, const float* __restrict__ e0,
                                   const float* __restrict__ e1, const float* __restrict__ e2, const float* __restrict__ e3,
                                   int order, float d, float kx, float ke, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float n0 = e0[i];
    float prime;
    switch (order) {  // same operation order as the reference expressions (:186-193)
      case 0: prime = n0; break;
      case 1: prime = (n0 + e1[i]) / 2.0f; break;
      case 2: prime = (3.0f * n0 - e1[i]) / 2.0f; break;
      case 3: prime = (23.0f * n0 - 16.0f * e1[i] + 5.0f * e2[i]) / 12.0f; break;
      default: prime = (55.0f * n0 - 59.0f * e1[i] + 37.0f * e2[i] - 9.0f * e3[i]) / 24.0f; break;
    }
    const float xv = x[i];
    x_out[i] = xv + d * (kx * xv - ke * prime);
  }
}
}  // namespace

extern "C" int ss_meldiff_sample_plms(const ss_wavenet* net, float* x, const float* cond, const int32_t* lens, int B, int T,
                                      int step_hi, int interval, const float* alphas_cumprod, int do_precompute, float* hist,
                                      void* ws, int64_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SS_CHECK_ARG(net && x && cond && ws && hist && alphas_cumprod, "ss_meldiff_sample_plms: null pointer");
  SS_CHECK_ARG(step_hi >= 1 && step_hi <= net->steps, "ss_meldiff_sample_plms: step_hi=%d must be in [1, steps]", step_hi);
  SS_CHECK_ARG(interval >= 1 && interval < step_hi, "ss_meldiff_sample_plms: interval=%d must be in [1, step_hi)", interval);
  SamplerCtx s;
  SS_PROPAGATE(open_sampler("ss_meldiff_sample_plms", net, B, T, cond, lens, ws, ws_bytes, 1, false, do_precompute != 0, stream, s));
  const StackForm& sf = s.sf;
  const WsLayout& w = s.w;
  const int64_t n = (int64_t)B * T * net->in_dim;
  float* slot[5];
  for (int i = 0; i < 5; ++i) slot[i] = hist + i * n;  // ring of eps(x_t, t): the current one + the last 4
  float* x_pred = hist + 5 * n;
  const int blocks = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
  int n_hist = 0, cur = 0, eval = 0;   // evaluations counted as they come (the first step evaluates twice)
  const int t_first = (step_hi - 1) / interval * interval;  // reversed(range(0, K_step, interval)), shallow_diffusion_tts.py:254-260
  for (int t = t_first; t >= 0; t -= interval) {
    const int tp = t - interval > 0 ? t - interval : 0;
    const float a_t = alphas_cumprod[t], a_p = alphas_cumprod[tp];
    const float a_t_sq = sqrtf(a_t), a_p_sq = sqrtf(a_p);
    const float d = a_p - a_t;
    const float kx = 1.0f / (a_t_sq * (a_t_sq + a_p_sq));
    const float ke = 1.0f / (a_t_sq * (sqrtf((1.0f - a_p) * a_t) + sqrtf((1.0f - a_t) * a_p)));
    float* e0 = slot[cur];
    SS_PROPAGATE(mel_eps(net, sf, x, e0, lens, B, T, w, t, eval++, stream));
    auto h = [&](int back) { return slot[(cur + 5 - back) % 5]; };
    if (n_hist == 0) {
      hipLaunchKernelGGL(plms_update_kernel, dim3(blocks), dim3(256), 0, stream, x, x_pred, e0, e0, e0, e0, 0, d, kx, ke, n);
      float* e_prev = slot[(cur + 1) % 5];  // scratch: overwritten by the next step's eps
      SS_PROPAGATE(mel_eps(net, sf, x_pred, e_prev, lens, B, T, w, tp, eval++, stream));
      hipLaunchKernelGGL(plms_update_kernel, dim3(blocks), dim3(256), 0, stream, x, x, e0, e_prev, e0, e0, 1, d, kx, ke, n);
    } else {
      const int order = n_hist == 1 ? 2 : n_hist == 2 ? 3 : 4;
      hipLaunchKernelGGL(plms_update_kernel, dim3(blocks), dim3(256), 0, stream, x, x, e0, h(1), h(2), h(3), order, d, kx, ke, n);
    }
    SS_CHECK_LAUNCH("ss_meldiff_sample_plms");
    if (n_hist < 4) ++n_hist;
    cur = (cur + 1) % 5;
  }
  return SS_OK;
}

extern "C" int ss_mel_qsample(const float* coarse_mel, const float* spec_min, const float* spec_max, float sqrt_ac,
                              float sqrt_1mac, const float* noise, uint64_t seed, const uint64_t* seed_dev, float* x, int B,
                              int T, int M, void* stream) {
  SS_CHECK_ARG(coarse_mel && spec_min && spec_max && x, "ss_mel_qsample: null pointer");
  hipLaunchKernelGGL(mel_qsample_kernel, dim3(grid_for((int64_t)B * T * M)), dim3(256), 0, (hipStream_t)stream, coarse_mel,
                     spec_min, spec_max, sqrt_ac, sqrt_1mac, noise, seed, seed_dev, x, (int64_t)B * T, T, M);
  SS_CHECK_LAUNCH("ss_mel_qsample");
  return SS_OK;
}

extern "C" int ss_mel_denorm(const float* x, const float* spec_min, const float* spec_max, float* mel, int B, int T, int M,
                             const int32_t* lens, int32_t* nonfinite, void* stream) {
  SS_CHECK_ARG(x && spec_min && spec_max && mel, "ss_mel_denorm: null pointer");
  hipLaunchKernelGGL(mel_denorm_kernel, dim3(grid_for((int64_t)B * T * M)), dim3(256), 0, (hipStream_t)stream, x, spec_min,
                     spec_max, mel, B, T, M, lens, nonfinite);
  SS_CHECK_LAUNCH("ss_mel_denorm");
  return SS_OK;
}
