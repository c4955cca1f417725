// The residual stack of the two denoisers (DiffNet / DDiffNet), library-internal: the form it takes for one (net, B, T), its workspace, the
// launches (wavenet_stack.hip), and what the samplers' tail kernels share (f0_sampler.hip, mel_sampler.hip).
#pragma once
#include "common.h"
#include "../../include/stylesinger_hip.h"

namespace ss_stack {

constexpr int MTR = 2;   // frames per workgroup of mel_tail_kernel

// The form the residual stack takes for one (net, B, T) under the tuning knobs. resolve_form() fills it ONCE per sampler call and is the only
// code that reads the mode fields, the optional weight pointers and the knobs; ws_layout() adds up the buffers of the form, the stack
// functions launch it.
enum StackKind {
  STACK_FP32,     // fp32 activations in HBM on the fp32-MFMA kernels (direct / F(2,3) / F(4,3) gates; "bf16" without the 16-bit packs rounds in-kernel; "bf16x3")
  STACK_PAIR16,   // 16-bit activations in HBM: a gate and a residual-projection launch per layer on ss_gemm_bf16
  STACK_FUSED16,  // fp16 terms, ONE ss_layer512 launch per layer (gate + residual projection, G kept in LDS)
};
enum GateEntry { GATE_CONV, GATE_WINO23, GATE_WINO43, GATE_WINO43_16, GATE_WINO43_16W, GATE_WINO43_16X };
enum ProjEntry { PROJ_CONV, PROJ_RES16, PROJ_RES16W };
enum SkipEntry { SKIP_CONV, SKIP_STORE16, SKIP_SPLITK, SKIP_X3 };
struct LayerForm {
  int d;               // dilation
  GateEntry gate;      // STACK_FP32: the gate's entry point ...
  int mt;              // ... its row tiling (the 16x16x4 entry points; 0 = picked per launch) ...
  int64_t e16_floats;  // ... and, > 0, GATE_WINO43_16W reads its conditioner addend from a slab of this many floats laid out for exactly that tiling
  ProjEntry proj;      // STACK_FP32: the output projection's entry point
  bool q4_gate;        // STACK_PAIR16, "fp16q4": the gate tries ss_gemm_bf16_gate128q first
};
struct StackForm {
  StackKind kind;
  int conv_bf16;     // ss_conv_gemm_args.mfma_bf16 of the STACK_FP32 launches
  int outer_bf16;    // ... of the conditioner and skip projections: exact fp32 in the split modes (a fixed rounding error of E would enter every step)
  bool cond16;       // the conditioner is rounded once to bf16 and E comes from ss_gemm_bf16
  bool skip_folded;  // the K = L*C skip GEMM + ReLU is the stack's output (its weights carry skip_projection / sqrt(L)): no skip_projection launch
  bool mel_tail;     // small launches: the mel sampler runs output projection + DDPM update + next input projection as one launch (mel_tail_kernel)
  // STACK_FP32
  bool defer;        // deferred skip: the output projections run their residual half only, the skip sum is one GEMM at the end of the stack
  SkipEntry skip;    // that GEMM's entry point, row tile 16 * mt16 (0 = picked per launch) and K slices (1 = do not split)
  int mt16, ksplit;
  bool partials_ok;  // SKIP_SPLITK may leave its slices to the caller's tail kernel (ss_gemm16_store_partials) instead of reducing them
  // 16-bit kinds. split (ss_gemm_bf16_args.split): 0 = bf16 operands; 1 = "bf16x2", every operand a (hi, mid) bf16 pair, pairs interleaved by 32
  // channels (one 128-byte line = 32 channels of both planes; rows of Yh / GAh / the weights are twice as long), the matrix cores run
  // hi*hi + hi*mid + mid*hi; 2 = "fp16x2", the same layouts with fp16 terms, weights-only split (two products), accumulators scaled by
  // net->mfma_out_scale
  int split, planes;   // planes per 16-bit row
  int gplanes;         // ... per row of GAh: 1 when g_compact
  bool g_compact;      // STACK_FUSED16 whose skip GEMM runs on the many-round kernel: GAh rows hold the L*C hi terms only (no dead second plane)
  bool one_product;    // "fp16sd": one weight term
  bool skip_w_compact; // ... and the skip GEMM reads the one-term sets without their zero plane (w_skipall_c: L2-resident)
  bool q4_skip;        // "fp16q4": the skip GEMM tries ss_gemm_bf16_tile256q first
  // "fp16sd": network evaluation j of a sampling loop (0 for its first one, in an order that does not depend on how a loop is cut into calls)
  // reads weight set j % n_wsets (set * ws_* stride on every 16-bit weight pointer) and addend set j % n_esets (0 = one fp32 addend slab).
  // Launch parameters only: a captured hipGraph replays the same sequence.
  int n_wsets, n_esets;
  LayerForm layer[SS_MAX_LAYERS];
};

struct WsLayout {
  float* E;   // [B*T][L*2C]
  float* X;   // [B*T][C]
  float* G;   // [B*T][C]
  float* S;   // [B*T][C]
  float* O;   // [B*T][4]   (f0 net output)
  float* GA;  // [B*T][L*C] gate outputs of ALL layers (deferred-skip mode only, else null)
  float* E16[SS_MAX_LAYERS];  // per layer: the conditioner addend in the 16x16x4 gate kernel's fetch order (null: the layer reads E)
  float* KP;  // [ksplit][B*T][C] partial sums of the split-K skip GEMM (small launches only, else null)
  // 16-bit kinds: the hidden activations travel as 16-bit rows
  uint16_t* Yh;     // [B*T][C]        x + dstep of the next layer (the dilated conv's operand)
  uint16_t* GAh;    // [B*T][L*C]      gate outputs of all layers
  uint16_t* condh;  // [B*T][cond_dim] conditioner
  // STACK_FUSED16: the stream as hi rows (double buffered) + pairs in accumulator order, and every layer's addend slab in the kernel's accumulator order
  uint16_t* H512[2];  // ss_layer512_h_elems: slot-major tiles
  void* P512;         // ss_layer512_stream_bytes
  float* E512;        // [L][ss_layer512_addend_floats]
  int64_t e512_layer; // floats per layer
  uint16_t* E512h;    // StackForm.n_esets > 0: [set][L][ss_layer512_addend_halfs] instead of E512
  int64_t e512h_layer, e512h_set;
  int64_t bytes;
};

StackForm resolve_form(const ss_wavenet* net, int B, int T);
WsLayout ws_layout(const ss_wavenet* net, const StackForm& f, int B, int T, void* base);
// E = cond . Wc^T + (bc + b_dil)  for all layers at once
int precompute_cond(const ss_wavenet* net, const StackForm& sf, const float* cond, const int32_t* lens, int B, int T, const WsLayout& w, hipStream_t stream);
// The L residual layers + skip projection; X in/out, leaves relu(skip_projection) in G. `step` = network time, `eval` = index of this network
// evaluation in its sampling loop (StackForm.n_wsets).
// leave_partials: the caller's next kernel (f0_tail_kernel / mel_tail_kernel) adds the split-K slices of the skip GEMM itself whenever
// sf.partials_ok: the reduction launch is then left out
int run_residual_stack(const ss_wavenet* net, const StackForm& sf, int step, int eval, const int32_t* lens, int B, int T, const WsLayout& w, hipStream_t stream,
                       bool leave_partials = false);

// What every sampler entry point (`who`) opens with, all of it before its first launch: the net's depth and width (C a multiple of c_multiple:
// 32 for the mel and ProDiff samplers, 64 for the f0 pair, 1 = not asked for DDIM and PLMS), the group rule (pairs_ok: the f0 entries take two
// nets over an even item count; every other entry takes one net), the stack's form, its workspace and that ws holds it, and, if asked, E.
struct SamplerCtx { StackForm sf; WsLayout w; };
int open_sampler(const char* who, const ss_wavenet* net, int B, int T, const float* cond, const int32_t* lens, void* ws, int64_t ws_bytes, int c_multiple,
                 bool pairs_ok, bool do_precompute, hipStream_t stream, SamplerCtx& out);

// The DDIM family's update coefficients of the transition ac_t -> ac_prev (cumprod alpha; 1 for the transition to x_0), Song et al. 2021 eq. 12 / 16:
//   x_prev = c1 x0 + c2 x + sigma z. Both strided samplers (ss_meldiff_sample_ddim, ss_f0diff_sample_strided) take them from here, in double.
struct DdimCoef { double c1, c2, sigma; };
inline DdimCoef ddim_coef(double ac_t, double ac_p, double eta) {
  const double sig = eta * sqrt((1.0 - ac_p) / (1.0 - ac_t)) * sqrt(fmax(0.0, 1.0 - ac_t / ac_p));
  const double c2 = sqrt(fmax(0.0, 1.0 - ac_p - sig * sig) / (1.0 - ac_t));
  const double c1 = sqrt(ac_p) - c2 * sqrt(ac_t);
  return {c1, c2, sig};
}

// where a tail kernel reads the stack output g = relu(skip GEMM) from: the reduced tensor G, or the split-K slices P[s][row][C] (+ bias, ReLU,
// row mask - the arithmetic and order of splitk_reduce_kernel)
struct SkipSrc {
  const float* G;
  const float* P;
  const float* bias;
  int ksplit;
  int64_t per;   // floats per slice = B*T*C
};
__device__ __forceinline__ float4 skip_load4(const SkipSrc& s, const float* bias, int64_t row, int C, int k, bool masked) {
  if (s.ksplit <= 1) return *reinterpret_cast<const float4*>(s.G + row * C + k);
  float4 v = *reinterpret_cast<const float4*>(s.P + row * C + k);
  for (int q = 1; q < s.ksplit; ++q) {
    const float4 u = *reinterpret_cast<const float4*>(s.P + q * s.per + row * C + k);
    v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
  }
  if (bias) {
    v.x += bias[k]; v.y += bias[k + 1]; v.z += bias[k + 2]; v.w += bias[k + 3];
  }
  v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
  if (masked) v = make_float4(0.f, 0.f, 0.f, 0.f);
  return v;
}
// the stack's output as a tail kernel reads it after run_residual_stack(..., leave_partials = true)
inline SkipSrc skip_src(const ss_wavenet* net, const StackForm& sf, const WsLayout& w, int B, int T) {
  return {w.G, w.KP, sf.partials_ok ? net->b_skipall : nullptr, sf.partials_ok ? sf.ksplit : 1, (int64_t)B * T * net->C};
}

}  // namespace ss_stack
