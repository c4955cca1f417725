// Diffusion samplers: the three reverse loops of the hot path, as host-side launch sequences over
// the fp32-MFMA conv kernel plus small fused sampler-update kernels.
//
//   mel : DiffusionDecoder.forward (modules/diff/shallow_diffusion_tts.py:285-307) with DiffNet (modules/diff/net.py:81-130)
//   f0  : GaussianMultinomialDiffusion.sample (modules/diff/gaussian_multinomial_diffusion.py:922-942) with DDiffNet (net.py:215-266)
//
// Restructuring vs the reference (same arithmetic, fewer flops / launches):
//   * conditioner_projection(cond) of every layer is step-invariant -> computed ONCE per utterance
//     batch as a single [B*T, 256] x [256, L*2C] GEMM ("E"), and the dilated-conv bias is folded into it;
//   * diffusion_projection_l(mlp(sinemb(t))) depends on weights only -> a [steps][L][C] table built at
//     load time and applied as a per-channel bias in the A-operand prologue of the dilated conv;
//   * gate (sigmoid*tanh), residual/sqrt(2), skip accumulation and the DDPM posterior step are GEMM epilogues.
// Nothing here allocates or synchronises: the whole loop is hipGraph-capturable.
#include "common.h"
#include <stdlib.h>
#include <cmath>
#include <vector>
#include "../../include/stylesinger_hip.h"

namespace {

inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
inline int round_up32(int x) { return (x + 31) / 32 * 32; }
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

StackForm resolve_form(const ss_wavenet* net, int B, int T) {
  StackForm f;
  memset(&f, 0, sizeof(f));
  const SsTuning& knob = g_ss_tuning;
  const int C = net->C, L = net->L, nl = L < SS_MAX_LAYERS ? L : SS_MAX_LAYERS;
  f.split = net->mfma_split == 0 ? 0 : net->mfma_split == 2 ? 2 : 1;
  f.planes = f.split ? 2 : 1;
  const bool h16 = net->mfma_bf16 && net->w_dil_h[0] && net->w_skipall_h && (net->w_cond_h || f.split);
  f.kind = h16 ? STACK_PAIR16 : STACK_FP32;
  f.conv_bf16 = net->mfma_bf16;
  f.outer_bf16 = f.split ? 0 : net->mfma_bf16;
  f.cond16 = h16 && !f.split;
  f.defer = !h16 && net->w_skipall;
  f.skip_folded = net->skipall_folded && (h16 || f.defer);
  f.mel_tail = knob.mel_tail != 0 && !net->mfma_bf16 && (int64_t)B * T <= 8L * ss_n_cu() && (C % 4) == 0 && (net->in_dim % 4) == 0 &&
               (size_t)(MTR * C + MTR * round_up32(net->in_dim)) * 4 <= 48 * 1024;
  f.one_product = net->mfma_products == 1;
  f.n_wsets = net->n_wsets > 1 ? net->n_wsets : 1;
  f.q4_skip = f.split == 2 && net->w_skipall_q && net->q_scale_z > 0.f;
  // the fp16x2 stack as ONE ss_layer512 launch per layer (knob "layer512"): the net carries the fragment-order packs of every layer, one weight
  // group, C = 256, dilations <= 8, and the launch fills the chip (ss_layer512_ok). Not "fp16q4": its gate runs the second product on the fp4
  // instruction (gate128q), two launches per layer
  if (h16 && knob.layer512 && f.split == 2 && net->n_groups <= 1 && C == 256 && !(net->w_dil_q[0] && net->q_scale_gate > 0.f)) {
    bool packs = true;
    for (int l = 0; l < nl; ++l) packs = packs && net->w_dil_f[l] && (l + 1 == L || net->w_out_f[l]);
    const int dmax = 1 << ((L < net->dil_cycle ? L : net->dil_cycle) - 1);
    if (packs && ss_layer512_ok(B, T, C, dmax, L * C * 2)) f.kind = STACK_FUSED16;
  }
  if (f.kind == STACK_FUSED16) {
    // the skip GEMM's many-round kernel reads a compact operand (ss_gemm_bf16_args.a_compact). Its size rule, >= 2 rounds of 256-row tiles, belongs
    // to gemm_bf16_tile256.hip; it is restated here because the layout of GAh is fixed before any launch
    f.g_compact = knob.gate256 != 0 && (long)ss_cdiv(T, 256) * B >= 2L * ss_n_cu() && ((L * C) % 64) == 0 && C <= 256;
    f.skip_w_compact = f.g_compact && f.one_product && net->w_skipall_c && net->n_groups <= 1;
    if (f.one_product && net->n_esets > 0) f.n_esets = net->n_esets;   // the addend as fp16 sets (half the bytes per launch; ss_layer512_tile_addend_f16)
  }
  f.gplanes = f.g_compact ? 1 : f.planes;
  f.ksplit = 1;
  if (f.defer) {
    const bool x3 = net->mfma_x3 && net->w_skipall_x3;   // opt-in bf16x3 mode: split operands on the bf16 matrix cores (gemm16x.hip)
    if (!net->mfma_bf16 && (C & 3) == 0) f.ksplit = ss_gemm16_ksplit_pick(B, T, C, L * C);   // one short utterance: split K over the idle CUs
    // long-K launch: when 64-row tiles also fit one round at three workgroups per CU they beat the 96-row pick (mel at C2: 240.7 vs 250.7 us)
    f.mt16 = (long)((T + 63) / 64) * B * ((C + 63) / 64) <= 3L * ss_n_cu() && !x3 ? 4 : 0;
    // fp32 operands: 16x16x4 tiles, both operands by LDS-DMA (gemm16.hip)
    f.skip = net->mfma_bf16 ? SKIP_CONV : f.skip_folded && x3 ? SKIP_X3 : f.ksplit > 1 ? SKIP_SPLITK : SKIP_STORE16;
    f.partials_ok = f.skip == SKIP_SPLITK && f.skip_folded;
  }
  const int g16 = knob.gate16;  // 0: 32x32x2 tiles; 1: per-launch pick; 2 / 3: 16x16x4 tiles of 16*MT quads
  for (int l = 0; l < nl; ++l) {
    LayerForm& y = f.layer[l];
    y.d = 1 << (l % net->dil_cycle);
    if (h16) {   // every other launch of "fp16q4" is fp16x2's
      y.q4_gate = f.split == 2 && net->w_dil_q[l] && net->q_scale_gate > 0.f;
      continue;
    }
    // deferred skip at C = 192 | 256: 16x16x4 tiles, balanced single round (gemm16.hip), weights in the kernel's fetch order when the net has them
    if (f.defer && !net->mfma_bf16 && (C == 192 || C == 256)) y.proj = net->w_out16[l] ? PROJ_RES16W : PROJ_RES16;
    if (!net->w_dil_wino[l] || net->mfma_bf16) continue;   // GATE_CONV
    if (net->wino_m != 4) y.gate = GATE_WINO23;            // pairs of frames (t, t+d) from 4 products instead of 6
    else if (net->mfma_x3 && net->w_dil_x3[l]) y.gate = GATE_WINO43_16X;   // opt-in "bf16x3" mode: split operands on the bf16 matrix cores
    else if (g16 == 0) y.gate = GATE_WINO43;
    else {
      y.gate = net->w_dil_wino16[l] ? GATE_WINO43_16W : GATE_WINO43_16;
      y.mt = g16 == 1 ? 0 : g16;
      if (!net->w_dil_wino16[l] || net->mfma_x3) continue;
      // the layer's slab of E is re-laid once per forward in the kernel's fetch order (ss_gate16_tile_addend), so that a wave's addend fetch is
      // 1 KB contiguous per instruction instead of 8 lines x 32 B; for that the tiling is fixed here
      int mt = g16 == 1 ? ss_wino43_gate16_pick(B, T, 2 * C, y.d) : g16;
      if (mt == 1 && !(knob.gate16_ks != 0 && C >= 64)) mt = 2;   // wino43_gate16.hip's rule, as ss_wino43_gate16 resolves it: MT = 1 is K-staged only
      const int64_t fl = mt > 0 ? ss_gate16_tiled_floats(B, T, 2 * C, y.d, mt) : -1;
      if (fl <= 0 || fl * 4 >= (1ll << 31)) continue;
      y.mt = mt;
      y.e16_floats = fl;
    }
  }
  return f;
}

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

WsLayout ws_layout(const ss_wavenet* net, const StackForm& f, int B, int T, void* base) {
  WsLayout w;
  memset(&w, 0, sizeof(w));
  const int64_t rows = (int64_t)B * T;
  int64_t off = 0;
  char* p = (char*)base;
  auto take = [&](int64_t floats) {
    float* r = (float*)(p + off);
    off = align_up(off + floats * 4, 256);
    return r;
  };
  w.E = take(rows * net->L * 2 * net->C);
  w.X = take(rows * net->C);
  w.G = take(rows * net->C);
  w.S = take(rows * net->C);
  w.O = take(rows * 4);
  if (f.defer) w.GA = take(rows * net->L * net->C);
  for (int l = 0; l < net->L && l < SS_MAX_LAYERS; ++l)
    if (f.layer[l].e16_floats) w.E16[l] = take(f.layer[l].e16_floats);
  if (f.ksplit > 1) w.KP = take((int64_t)f.ksplit * rows * net->C);
  if (f.kind != STACK_FP32) {
    w.Yh = (uint16_t*)take((rows * net->C * f.planes + 1) / 2);
    w.GAh = (uint16_t*)take((rows * net->L * net->C * f.gplanes + 1) / 2);
    if (f.cond16) w.condh = (uint16_t*)take((rows * net->cond_dim + 1) / 2);
  }
  if (f.kind == STACK_FUSED16) {
    w.H512[0] = (uint16_t*)take((ss_layer512_h_elems(B, T) + 1) / 2);
    w.H512[1] = (uint16_t*)take((ss_layer512_h_elems(B, T) + 1) / 2);
    w.P512 = take(ss_layer512_stream_bytes(B, T) / 4);
    if (f.n_esets) {
      w.e512h_layer = ss_layer512_addend_halfs(B, T);
      w.e512h_set = w.e512h_layer * net->L;
      w.E512h = (uint16_t*)take((w.e512h_set * f.n_esets + 1) / 2);
    } else {
      w.e512_layer = ss_layer512_addend_floats(B, T);
      w.E512 = take(w.e512_layer * net->L);
    }
  }
  w.bytes = off;
  return w;
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
// the A operand / the output of a launch (either argument struct) as [B][T][ld] rows
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

// E = cond . Wc^T + (bc + b_dil)  for all layers at once
int precompute_cond(const ss_wavenet* net, const StackForm& sf, const float* cond, const int32_t* lens, int B, int T, const WsLayout& w, hipStream_t stream) {
  const int NE = net->L * 2 * net->C;
  if (sf.cond16) {  // cond rounded once to bf16, then E = cond . Wc^T + (bc + b_dil) on the bf16 kernel (fp32 out)
    SS_PROPAGATE(ss_to_bf16(cond, nullptr, w.condh, B, T, net->cond_dim, net->cond_dim, net->cond_dim, nullptr, 0, 0, stream));
    ss_gemm_bf16_args h = base_args_h(net, B, T, lens);
    set_a(h, w.condh, net->cond_dim, T);
    h.K = net->cond_dim;
    h.W = net->w_cond_h;
    h.w_group_stride = net->gs_w_cond_h;
    h.N = NE;
    h.Np = NE;
    h.epi = SS_HEPI_STORE;
    h.bias = net->b_cond;
    h.bias_group_stride = net->gs_b_cond;
    set_c(h, w.E, NE, T);
    h.mask_rows = 0;
    return ss_gemm_bf16(&h, stream);
  }
  ss_conv_gemm_args a = base_args(B, T, lens);
  set_a(a, cond, net->cond_dim, T);
  a.Cin = net->cond_dim;
  a.W = net->w_cond;
  a.N = NE;
  a.Np = NE;
  a.Kp = round_up32(net->cond_dim);
  a.epi = SS_EPI_STORE;
  a.bias = net->b_cond;
  set_c(a, w.E, NE, T);
  a.mask_rows = 0;
  a.mfma_bf16 = sf.outer_bf16;
  set_groups(a, net, B, net->gs_w_cond, net->gs_b_cond);
  SS_PROPAGATE(ss_conv_gemm(&a, stream));
  for (int l = 0; l < net->L; ++l) {   // the layer's addend columns again, in the order its kernel fetches them
    const float* El = w.E + (int64_t)l * 2 * net->C;
    if (w.E512)   // ss_layer512's accumulator order
      SS_PROPAGATE(ss_layer512_tile_addend(El, NE, (int64_t)T * NE, w.E512 + (int64_t)l * w.e512_layer, B, T, stream));
    if (w.E512h)  // ... as n_esets fp16 sigma-delta sets (fp16sd)
      SS_PROPAGATE(ss_layer512_tile_addend_f16(El, NE, (int64_t)T * NE, w.E512h + (int64_t)l * w.e512h_layer, sf.n_esets, w.e512h_set, B, T, stream));
    if (w.E16[l])
      SS_PROPAGATE(ss_gate16_tile_addend(El, NE, (int64_t)T * NE, w.E16[l], B, T, 2 * net->C, sf.layer[l].d, sf.layer[l].mt, stream));
  }
  return SS_OK;
}

// The L residual layers + skip projection; X in/out, leaves relu(skip_projection) in G. `step` = network time, `eval` = index of this network
// evaluation in its sampling loop (StackForm.n_wsets). One function per StackKind:
//
// STACK_FP32. Deferred-skip mode (net->w_skipall set): the per-layer output projection only runs its residual half (N = C, no skip
// read-modify-write), every layer's gate output is kept ([rows][L*C]) and the skip sum of all layers is ONE GEMM with
// K = L*C at the end of the stack - same products, summed in one accumulator chain instead of layer by layer.
int skip_gemm_f32(const ss_wavenet* net, const StackForm& sf, const int32_t* lens, int B, int T, const WsLayout& w, hipStream_t stream, bool leave_partials) {
  const int C = net->C, L = net->L;
  // S = sum_l skip_l = [g_0 | g_1 | ... | g_{L-1}] . [W_skip_0 ; ... ; W_skip_{L-1}]^T + sum_l b_skip_l
  ss_conv_gemm_args k = base_args(B, T, lens);
  set_a(k, w.GA, L * C, T);
  k.Cin = L * C;
  k.W = net->w_skipall;
  k.N = C;
  k.Np = round_up32(C);
  k.Kp = L * C;
  k.epi = SS_EPI_STORE;
  k.bias = net->b_skipall;
  set_c(k, sf.skip_folded ? w.G : w.S, C, T);
  if (sf.skip_folded) k.act = SS_ACT_RELU;
  k.tile = SS_TILE_64x64;
  k.mfma_bf16 = sf.conv_bf16;
  set_groups(k, net, B, net->gs_w_skipall, net->gs_b_skipall);
  switch (sf.skip) {
    case SKIP_X3:
      k.w_group_stride = net->gs_w_skipall_x3;
      return ss_gemm16x_store(&k, net->w_skipall_x3, sf.mt16, stream);
    case SKIP_SPLITK:
      return leave_partials && sf.partials_ok ? ss_gemm16_store_partials(&k, 4, sf.ksplit, w.KP, stream) : ss_gemm16_store_splitk(&k, 4, sf.ksplit, w.KP, stream);
    case SKIP_STORE16: return ss_gemm16_store(&k, sf.mt16, stream);
    default: return ss_conv_gemm(&k, stream);
  }
}

int run_stack_f32(const ss_wavenet* net, const StackForm& sf, int step, const int32_t* lens, int B, int T, const WsLayout& w, hipStream_t stream, bool leave_partials) {
  const int C = net->C, L = net->L;
  const int NE = L * 2 * C;
  const int ldg = sf.defer ? L * C : C;
  for (int l = 0; l < L; ++l) {
    const LayerForm& y = sf.layer[l];
    // y = dilated_conv(x + dstep) + cond_proj ; g = sigmoid(y[:C]) * tanh(y[C:])   (net.py:66-73)
    ss_conv_gemm_args a = base_args(B, T, lens);
    set_a(a, w.X, C, T);
    a.Cin = C;
    set_taps3(a, y.d);
    a.a_bias = net->dstep + ((int64_t)step * L + l) * C;
    a.W = net->w_dil[l];
    a.N = C;
    a.Np = 2 * C;
    a.Kp = round_up32(C);
    a.epi = SS_EPI_GATE;
    a.E = w.E + (int64_t)l * 2 * C;
    a.lde = NE;
    a.e_batch_stride = (int64_t)T * NE;
    float* Gl = sf.defer ? w.GA + (int64_t)l * C : w.G;
    set_c(a, Gl, ldg, T);
    a.mfma_bf16 = sf.conv_bf16;
    set_groups(a, net, B, net->gs_w_dil, 0, net->gs_dstep);
    if (y.gate != GATE_CONV) {
      a.W = net->w_dil_wino[l];
      a.w_group_stride = net->gs_w_dil_wino;
    }
    switch (y.gate) {
      case GATE_CONV: SS_PROPAGATE(ss_conv_gemm(&a, stream)); break;
      case GATE_WINO23: SS_PROPAGATE(ss_wino_gate(&a, y.d, stream)); break;
      case GATE_WINO43: SS_PROPAGATE(ss_wino43_gate(&a, y.d, stream)); break;
      case GATE_WINO43_16: SS_PROPAGATE(ss_wino43_gate16(&a, y.d, y.mt, stream)); break;
      case GATE_WINO43_16W:
        if (y.e16_floats) {   // addend in fetch order, laid out for exactly this tiling
          a.E = w.E16[l];
          a.e_tiled = 1;
        }
        SS_PROPAGATE(ss_wino43_gate16w(&a, net->w_dil_wino16[l], y.d, y.mt, stream));
        break;
      case GATE_WINO43_16X:
        a.w_group_stride = net->gs_w_dil_x3;
        SS_PROPAGATE(ss_wino43_gate16x(&a, net->w_dil_x3[l], y.d, 0, stream));
        break;
    }
    // y = output_projection(g) ; x = (x + y[:C]) / sqrt(2) ; skip += y[C:]   (net.py:75-77)
    // deferred-skip form: this launch only produces the residual stream, and the LAST layer's stream is never read (net.py:120-127)
    if (sf.defer && l + 1 == L) break;
    ss_conv_gemm_args o = base_args(B, T, lens);
    set_a(o, Gl, ldg, T);
    o.Cin = C;
    o.W = net->w_out[l];
    o.N = sf.defer ? C : 2 * C;  // deferred skip: only the residual half (the first C packed rows) runs per layer
    if (sf.defer) o.tile = SS_TILE_64x64;
    o.Np = 2 * C;
    o.Kp = round_up32(C);
    o.epi = SS_EPI_RESSKIP;
    o.bias = net->b_out[l];
    o.Nh = C;
    o.R = w.X;
    o.ldr = C;
    o.r_batch_stride = (int64_t)T * C;
    set_c(o, w.X, C, T);
    o.post_scale = 0.70710678118654752440f;  // 1/sqrt(2.0)
    o.C2 = w.S;
    o.ldc2 = C;
    o.c2_batch_stride = (int64_t)T * C;
    o.accumulate = sf.defer ? 0 : l > 0;
    o.mfma_bf16 = sf.conv_bf16;
    set_groups(o, net, B, net->gs_w_out, net->gs_b_out);
    if (y.proj == PROJ_RES16W) {
      o.w_group_stride = net->gs_w_out16;
      SS_PROPAGATE(ss_gemm16_resw(&o, net->w_out16[l], 0, stream));
    } else {
      SS_PROPAGATE(y.proj == PROJ_RES16 ? ss_gemm16_res(&o, 0, stream) : ss_conv_gemm(&o, stream));
    }
  }
  return sf.defer ? skip_gemm_f32(net, sf, lens, B, T, w, stream, leave_partials) : SS_OK;
}

// The 16-bit kinds: per layer gate (stream -> GAh[l]) and residual projection (GAh[l] -> stream + dstep_{l+1}), then the K = L*C skip GEMM -> S (fp32).
// Same operand roundings as oracle/restatement.py with set_matmul_rounding("bf16") - each operand is rounded once, where it is produced.
inline int64_t wset_off(const StackForm& sf, int eval, int64_t stride) { return (int64_t)(eval % sf.n_wsets) * stride; }
// "fp16q4" (try_q4): the launch with its second product on the fp4 instruction (weight pack Wq, A-operand scale q_scale) when that kernel's own
// _ok rule takes it. The rule reads the filled argument struct, so it is asked here, per launch, and not in resolve_form()
int launch_h(const ss_gemm_bf16_args& a, bool try_q4, const uint16_t* Wq, int64_t gs_wq, float q_scale, int (*q_ok)(const ss_gemm_bf16_args*),
             int (*q_run)(const ss_gemm_bf16_args*, void*), hipStream_t stream) {
  if (try_q4) {
    ss_gemm_bf16_args q = a;
    q.split = 3;
    q.W = Wq;
    q.w_group_stride = gs_wq;
    q.q_scale = q_scale;
    if (q_ok(&q)) return q_run(&q, stream);
  }
  return ss_gemm_bf16(&a, stream);
}

int skip_gemm_h(const ss_wavenet* net, const StackForm& sf, int eval, const int32_t* lens, int B, int T, const WsLayout& w, hipStream_t stream) {
  const int C = net->C, L = net->L;
  ss_gemm_bf16_args k = base_args_h(net, B, T, lens);
  set_a(k, w.GAh, L * C * sf.gplanes, T);
  k.a_compact = sf.g_compact ? 1 : 0;
  k.split = sf.split;
  k.out_scale = net->mfma_out_scale;
  k.K = L * C;
  if (sf.skip_w_compact) {
    k.W = net->w_skipall_c + wset_off(sf, eval, net->ws_w_skipall_c);
    k.one_product = 2;
  } else {
    k.W = net->w_skipall_h + wset_off(sf, eval, net->ws_w_skipall_h);
    k.one_product = sf.one_product ? 1 : 0;
  }
  k.w_group_stride = net->gs_w_skipall_h;
  k.N = C;
  k.Np = round_up32(C);
  k.epi = SS_HEPI_STORE;
  k.bias = net->b_skipall;
  k.bias_group_stride = net->gs_b_skipall;
  set_c(k, sf.skip_folded ? w.G : w.S, C, T);
  if (sf.skip_folded) k.act = SS_ACT_RELU;
  return launch_h(k, sf.q4_skip, net->w_skipall_q, net->gs_w_skipall_q, net->q_scale_z, ss_gemm_bf16_tile256q_ok, ss_gemm_bf16_tile256q, stream);
}

// STACK_PAIR16: Yh = 16-bit (x + dstep_0) on entry; the residual projection updates X (fp32, bf16 mode only) and writes Yh for the next layer
int run_stack_pair16(const ss_wavenet* net, const StackForm& sf, int step, int eval, const int32_t* lens, int B, int T, const WsLayout& w, hipStream_t stream) {
  const int C = net->C, L = net->L, pl = sf.planes;
  const int NE = L * 2 * C;
  const float* dstep0 = net->dstep + (int64_t)step * L * C;
  const int gsz = net->n_groups > 1 ? B / net->n_groups : 0;
  if (sf.split == 2) SS_PROPAGATE(ss_split_f16(w.X, dstep0, 1.0f, w.Yh, B, T, C, C, 2 * C, lens, gsz, net->gs_dstep, stream));
  else if (sf.split) SS_PROPAGATE(ss_split_bf16(w.X, dstep0, w.Yh, B, T, C, C, 2 * C, lens, gsz, net->gs_dstep, stream));
  else SS_PROPAGATE(ss_to_bf16(w.X, dstep0, w.Yh, B, T, C, C, C, lens, gsz, net->gs_dstep, stream));
  for (int l = 0; l < L; ++l) {
    ss_gemm_bf16_args g = base_args_h(net, B, T, lens);
    set_a(g, w.Yh, C * pl, T);
    g.split = sf.split;
    g.out_scale = net->mfma_out_scale;
    g.K = C;
    set_taps3(g, sf.layer[l].d);
    g.W = net->w_dil_h[l] + wset_off(sf, eval, net->ws_w_dil_h);
    g.w_group_stride = net->gs_w_dil_h;
    g.N = C;
    g.Np = 2 * C;
    g.epi = SS_HEPI_GATE;
    g.E = w.E + (int64_t)l * 2 * C;
    g.lde = NE;
    g.e_batch_stride = (int64_t)T * NE;
    set_c(g, w.GAh + (int64_t)l * C * pl, L * C * pl, T);
    SS_PROPAGATE(launch_h(g, sf.layer[l].q4_gate, net->w_dil_q[l], net->gs_w_dil_q, net->q_scale_gate, ss_gemm_bf16_gate128q_ok, ss_gemm_bf16_gate128q, stream));
    // the residual stream of the LAST layer is never read (only the skip sum leaves the stack, net.py:120-127): no projection for it
    if (l + 1 == L) break;
    ss_gemm_bf16_args o = base_args_h(net, B, T, lens);
    set_a(o, w.GAh + (int64_t)l * C * pl, L * C * pl, T);
    o.split = sf.split;
    o.out_scale = net->mfma_out_scale;
    o.K = C;
    o.W = net->w_out_h[l] + wset_off(sf, eval, net->ws_w_out_h);
    o.w_group_stride = net->gs_w_out_h;
    o.N = C;
    o.Np = C;  // the residual half = the first C packed rows
    o.epi = SS_HEPI_RESX;
    o.bias = net->b_out[l];
    o.bias_group_stride = net->gs_b_out;
    o.post_scale = 0.70710678118654752440f;
    o.next_bias = net->dstep + ((int64_t)step * L + l + 1) * C;
    o.next_bias_group_stride = net->gs_dstep;
    o.Y = w.Yh;
    o.ldy = C * pl;
    o.y_batch_stride = (int64_t)T * C * pl;
    if (sf.split) {   // split mode: the stream lives only as the pair Yh = x + dstep_l (16 significant bits; measured harmless, oracle/bf16x2_numerics.py)
      o.cur_bias = net->dstep + ((int64_t)step * L + l) * C;
      o.cur_bias_group_stride = net->gs_dstep;
    } else {
      o.X = w.X;
      o.ldx = C;
      o.x_batch_stride = (int64_t)T * C;
    }
    SS_PROPAGATE(ss_gemm_bf16(&o, stream));
  }
  return skip_gemm_h(net, sf, eval, lens, B, T, w, stream);
}

// STACK_FUSED16: gate + residual projection of layer l in one launch, G kept in LDS; the stream alternates between the two H512 buffers
int run_stack_fused16(const ss_wavenet* net, const StackForm& sf, int step, int eval, const int32_t* lens, int B, int T, const WsLayout& w, hipStream_t stream) {
  const int C = net->C, L = net->L;
  SS_PROPAGATE(ss_layer512_entry(w.X, C, (int64_t)T * C, net->dstep + (int64_t)step * L * C, lens, w.H512[0], w.P512, B, T, stream));
  for (int l = 0; l < L; ++l) {
    ss_layer512_args f;
    memset(&f, 0, sizeof(f));
    f.Hin = w.H512[l & 1];
    f.d = sf.layer[l].d;
    f.lens = lens;
    f.B = B;
    f.T = T;
    f.Wg = net->w_dil_f[l] + wset_off(sf, eval, net->ws_w_dil_f);
    f.n_products = sf.one_product ? 1 : 2;
    if (sf.n_esets) {   // evaluation j reads addend set j % n_esets
      f.E512 = reinterpret_cast<const float*>(w.E512h + (int64_t)(eval % sf.n_esets) * w.e512h_set + (int64_t)l * w.e512h_layer);
      f.e_f16 = 1;
    } else {
      f.E512 = w.E512 + (int64_t)l * w.e512_layer;
    }
    f.G = w.GAh + (int64_t)l * C * sf.gplanes;
    f.g_batch_stride = (int64_t)T * L * C * sf.gplanes;
    f.ldg = L * C * sf.gplanes;
    f.g_compact = sf.g_compact ? 1 : 0;
    f.mask_rows = 1;
    f.out_scale = net->mfma_out_scale;
    f.post_scale = 0.70710678118654752440f;
    if (l + 1 < L) {   // the residual stream of the last layer is never read (net.py:120-127)
      f.Hout = w.H512[(l & 1) ^ 1];
      f.P = w.P512;
      f.Wr = net->w_out_f[l] + wset_off(sf, eval, net->ws_w_out_f);
      f.bias_r = net->b_out[l];
      f.next_bias = net->dstep + ((int64_t)step * L + l + 1) * C;
      f.cur_bias = net->dstep + ((int64_t)step * L + l) * C;
    }
    SS_PROPAGATE(ss_layer512(&f, stream));
  }
  return skip_gemm_h(net, sf, eval, lens, B, T, w, stream);
}

// leave_partials: the caller's next kernel (f0_tail_kernel / mel_tail_kernel) adds the split-K slices of the skip GEMM itself whenever
// sf.partials_ok: the reduction launch is then left out
int run_residual_stack(const ss_wavenet* net, const StackForm& sf, int step, int eval, const int32_t* lens, int B, int T, const WsLayout& w, hipStream_t stream,
                       bool leave_partials = false) {
  switch (sf.kind) {
    case STACK_FP32: SS_PROPAGATE(run_stack_f32(net, sf, step, lens, B, T, w, stream, leave_partials)); break;
    case STACK_PAIR16: SS_PROPAGATE(run_stack_pair16(net, sf, step, eval, lens, B, T, w, stream)); break;
    case STACK_FUSED16: SS_PROPAGATE(run_stack_fused16(net, sf, step, eval, lens, B, T, w, stream)); break;
  }
  if (sf.skip_folded) return SS_OK;
  // x = relu(skip_projection(sum(skip) / sqrt(L)))   (net.py:124-127)
  const int C = net->C;
  ss_conv_gemm_args s = base_args(B, T, lens);
  set_a(s, w.S, C, T);
  s.Cin = C;
  s.a_scale = 1.0f / sqrtf((float)net->L);
  s.W = net->w_skip;
  s.N = C;
  s.Np = round_up32(C);
  s.Kp = round_up32(C);
  s.epi = SS_EPI_STORE;
  s.bias = net->b_skip;
  s.act = SS_ACT_RELU;
  set_c(s, w.G, C, T);
  s.mfma_bf16 = sf.outer_bf16;
  set_groups(s, net, B, net->gs_w_skip, net->gs_b_skip);
  return ss_conv_gemm(&s, stream);
}

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

inline int grid_for(int64_t n) {
  int64_t g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

}  // namespace

extern "C" int64_t ss_wavenet_workspace_bytes(const ss_wavenet* net, int B, int T) {
  if (!net || B <= 0 || T <= 0) return -1;
  return ws_layout(net, resolve_form(net, B, T), B, T, nullptr).bytes;
}

// x_in -> w.X = relu(input_projection(x_in))  (net.py:114-116)
static int mel_input_proj(const ss_wavenet* net, const float* x_in, const int32_t* lens, int B, int T, const WsLayout& w, hipStream_t stream) {
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
static int mel_net_body(const ss_wavenet* net, const StackForm& sf, const float* x_in, float* out, const int32_t* lens, int B, int T, const WsLayout& w,
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
static int mel_eps(const ss_wavenet* net, const StackForm& sf, const float* x_in, float* eps_out, const int32_t* lens, int B, int T, const WsLayout& w,
                   int t, int eval, hipStream_t stream) {
  ss_conv_gemm_args f;
  SS_PROPAGATE(mel_net_body(net, sf, x_in, eps_out, lens, B, T, w, t, eval, stream, f));
  f.epi = SS_EPI_STORE;
  f.mask_rows = 0;
  return ss_conv_gemm(&f, stream);
}

// One reverse step of the mel net at network time `t` with explicit update coefficients
//   x0 = clamp(recip*x - recipm1*eps, -1, 1) ; x <- c1*x0 + c2*x + sigma*z
static int mel_step(const ss_wavenet* net, const StackForm& sf, float* x, const int32_t* lens, int B, int T, const WsLayout& w, int t, int eval,
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

extern "C" int ss_meldiff_sample(const ss_wavenet* net, float* x, const float* cond, const int32_t* lens, int B, int T,
                                 const float* noise, uint64_t seed, const uint64_t* seed_dev, int step_lo, int step_hi,
                                 int do_precompute, void* ws, int64_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SS_CHECK_ARG(net && x && cond && ws, "ss_meldiff_sample: null pointer");
  SS_CHECK_ARG(net->L > 0 && net->L <= SS_MAX_LAYERS && (net->C % 32) == 0, "ss_meldiff_sample: bad net C=%d L=%d", net->C, net->L);
  SS_CHECK_ARG(0 <= step_lo && step_lo <= step_hi && step_hi <= net->steps, "ss_meldiff_sample: bad step range");
  SS_CHECK_ARG(net->n_groups <= 1, "ss_meldiff_sample: grouped nets are only supported by the f0 sampler");
  const StackForm sf = resolve_form(net, B, T);
  const WsLayout w = ws_layout(net, sf, B, T, ws);
  SS_CHECK_ARG(ws_bytes >= w.bytes, "ss_meldiff_sample: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)w.bytes);
  const int M = net->in_dim, C = net->C;
  if (do_precompute) SS_PROPAGATE(precompute_cond(net, sf, cond, lens, B, T, w, stream));
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
    const SkipSrc src = {w.G, w.KP, sf.partials_ok ? net->b_skipall : nullptr, sf.partials_ok ? sf.ksplit : 1, (int64_t)B * T * C};
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
  SS_CHECK_ARG(net->n_groups <= 1 && net->L > 0 && net->L <= SS_MAX_LAYERS && (net->C % 32) == 0, "ss_prodiff_sample: bad net");
  SS_CHECK_ARG(n_steps >= 1 && n_steps <= net->steps, "ss_prodiff_sample: n_steps=%d outside [1, %d]", n_steps, net->steps);
  const StackForm sf = resolve_form(net, B, T);
  const WsLayout w = ws_layout(net, sf, B, T, ws);
  SS_CHECK_ARG(ws_bytes >= w.bytes, "ss_prodiff_sample: workspace too small");
  const int M = net->in_dim;
  if (do_precompute) SS_PROPAGATE(precompute_cond(net, sf, cond, lens, B, T, w, stream));
  for (int t = n_steps - 1; t >= 0; --t) {
    SS_PROPAGATE(mel_step(net, sf, x, lens, B, T, w, t, n_steps - 1 - t, 0.0f, 0.0f, c1[t], c2[t], t > 0 ? sigma[t] : 0.0f,
                          noise ? noise + (int64_t)t * B * T * M : nullptr, seed, seed_dev, (uint32_t)t, stream, 1));
  }
  return SS_OK;
}

// Strided sampler (DDIM family, Song et al. 2021 eq. 12 / 16) over the SAME denoiser: visits network times ts[0] > ts[1] > ... and jumps
// x_{ts[i]} -> x_{ts[i+1]} (-> x_0 after the last).  With x0 = clamp(...), eps' = (x - sqrt(ac_t) x0)/sqrt(1-ac_t) and
//   sigma = eta * sqrt((1-ac_prev)/(1-ac_t)) * sqrt(1 - ac_t/ac_prev):
//   x_prev = sqrt(ac_prev) x0 + sqrt(1-ac_prev-sigma^2) eps' + sigma z = c1 x0 + c2 x + sigma z,
//   c2 = sqrt((1-ac_prev-sigma^2)/(1-ac_t)), c1 = sqrt(ac_prev) - c2 sqrt(ac_t)
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
  SS_CHECK_ARG(net->n_groups <= 1 && net->L > 0 && net->L <= SS_MAX_LAYERS, "ss_meldiff_sample_ddim: bad net");
  SS_CHECK_ARG(eta >= 0.0f && eta <= 1.0f, "ss_meldiff_sample_ddim: eta=%g outside [0, 1]", (double)eta);
  const StackForm sf = resolve_form(net, B, T);
  const WsLayout w = ws_layout(net, sf, B, T, ws);
  SS_CHECK_ARG(ws_bytes >= w.bytes, "ss_meldiff_sample_ddim: workspace too small");
  for (int i = 0; i < n_ts; ++i)
    SS_CHECK_ARG(ts[i] >= 0 && ts[i] < net->steps && (i == 0 || ts[i] < ts[i - 1]), "ss_meldiff_sample_ddim: ts must be strictly decreasing in [0,steps)");
  const int M = net->in_dim;
  if (do_precompute) SS_PROPAGATE(precompute_cond(net, sf, cond, lens, B, T, w, stream));
  for (int i = 0; i < n_ts; ++i) {
    const int t = ts[i];
    const double ac_t = alphas_cumprod[t];
    const double ac_p = (i + 1 < n_ts) ? alphas_cumprod[ts[i + 1]] : 1.0;
    const double sig = (double)eta * sqrt((1.0 - ac_p) / (1.0 - ac_t)) * sqrt(fmax(0.0, 1.0 - ac_t / ac_p));
    const double c2 = sqrt(fmax(0.0, 1.0 - ac_p - sig * sig) / (1.0 - ac_t));
    const double c1 = sqrt(ac_p) - c2 * sqrt(ac_t);
    const bool draw = eta > 0.0f;  // like p_sample, a stochastic run draws at every step (sigma = 0 on the last)
    SS_PROPAGATE(mel_step(net, sf, x, lens, B, T, w, t, i, net->sqrt_recip_ac[t], net->sqrt_recipm1_ac[t], (float)c1, (float)c2, (float)sig,
                          (draw && noise) ? noise + (int64_t)t * B * T * M : nullptr, seed, draw ? seed_dev : nullptr, (uint32_t)t, stream));
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
  SS_CHECK_ARG(net->n_groups <= 1 && net->L > 0 && net->L <= SS_MAX_LAYERS, "ss_meldiff_sample_plms: bad net");
  SS_CHECK_ARG(step_hi >= 1 && step_hi <= net->steps, "ss_meldiff_sample_plms: step_hi=%d must be in [1, steps]", step_hi);
  SS_CHECK_ARG(interval >= 1 && interval < step_hi, "ss_meldiff_sample_plms: interval=%d must be in [1, step_hi)", interval);
  const StackForm sf = resolve_form(net, B, T);
  const WsLayout w = ws_layout(net, sf, B, T, ws);
  SS_CHECK_ARG(ws_bytes >= w.bytes, "ss_meldiff_sample_plms: workspace too small");
  const int64_t n = (int64_t)B * T * net->in_dim;
  float* slot[5];
  for (int i = 0; i < 5; ++i) slot[i] = hist + i * n;  // ring of eps(x_t, t): the current one + the last 4
  float* x_pred = hist + 5 * n;
  if (do_precompute) SS_PROPAGATE(precompute_cond(net, sf, cond, lens, B, T, w, stream));
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

// the input row of a call's first evaluation; every later one is written by the previous step's tail kernel
static int f0_first_input(const ss_wavenet* net, const float* f0, const int32_t* uv, const int32_t* lens, int B, int T, const WsLayout& w, hipStream_t stream) {
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
static int f0_step(const ss_wavenet* net, const StackForm& sf, float* f0, int32_t* uv, const float* lo, const float* hi, const int32_t* lens, int B, int T,
                   const WsLayout& w, int t, int eval, bool final_step, const F0StepCoef& k, const float* noise_t, const float* gumbel_t, uint64_t seed,
                   const uint64_t* seed_dev, bool write_x, hipStream_t stream) {
  const int C = net->C;
  const int64_t n = (int64_t)B * T;
  const int gsz = net->n_groups > 1 ? B / net->n_groups : 0;
  SS_PROPAGATE(run_residual_stack(net, sf, t, eval, lens, B, T, w, stream, true));
  // partials_ok: the skip GEMM left its split-K slices in w.KP and the tail kernel adds them
  const SkipSrc src = {w.G, w.KP, sf.partials_ok ? net->b_skipall : nullptr, sf.partials_ok ? sf.ksplit : 1, n * C};
  // output projection (C -> 3) + joint sampler update + the next evaluation's input row, one launch (f0_tail_kernel)
  hipLaunchKernelGGL(f0_tail_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, stream, src, net->gs_b_skipall, net->w_final, net->b_final, f0, uv, lo, hi,
                     noise_t, gumbel_t, seed, seed_dev, t, final_step ? 1 : 0, B, T, C, k, net->w_in, net->b_in, net->uv_embed, write_x ? w.X : nullptr, lens,
                     gsz, net->gs_w_final, net->gs_b_final, net->gs_w_in, net->gs_b_in, net->gs_uv_embed);
  SS_CHECK_LAUNCH("f0_tail_kernel");
  return SS_OK;
}

extern "C" int ss_f0diff_sample(const ss_wavenet* net, float* f0, int32_t* uv, const float* cond, const float* lo,
                                const float* hi, const int32_t* lens, int B, int T, const float* noise,
                                const float* gumbel_u, uint64_t seed, const uint64_t* seed_dev, int step_lo, int step_hi,
                                int do_precompute, void* ws, int64_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SS_CHECK_ARG(net && f0 && uv && cond && lo && hi && ws, "ss_f0diff_sample: null pointer");
  SS_CHECK_ARG(net->L > 0 && net->L <= SS_MAX_LAYERS && (net->C % 64) == 0, "ss_f0diff_sample: bad net C=%d L=%d", net->C, net->L);
  SS_CHECK_ARG(0 <= step_lo && step_lo <= step_hi && step_hi <= net->steps, "ss_f0diff_sample: bad step range");
  SS_CHECK_ARG(net->out_dim == 3 && net->in_dim == 1, "ss_f0diff_sample: net must be the 1->3 DDiffNet");
  SS_CHECK_ARG(net->n_groups <= 1 || (net->n_groups == 2 && B % 2 == 0), "ss_f0diff_sample: paired nets need an even item count");
  const StackForm sf = resolve_form(net, B, T);
  const WsLayout w = ws_layout(net, sf, B, T, ws);
  SS_CHECK_ARG(ws_bytes >= w.bytes, "ss_f0diff_sample: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)w.bytes);
  const int64_t n = (int64_t)B * T;
  if (do_precompute) SS_PROPAGATE(precompute_cond(net, sf, cond, lens, B, T, w, stream));
  for (int t = step_hi - 1; t >= step_lo; --t) {
    if (t == step_hi - 1) SS_PROPAGATE(f0_first_input(net, f0, uv, lens, B, T, w, stream));
    const int tm1 = t > 0 ? t - 1 : 0;
    const F0StepCoef k = {net->sqrt_recip_ac[t], net->sqrt_recipm1_ac[t], net->post_c1[t], net->post_c2[t],
                          t > 0 ? expf(0.5f * net->post_logvar[t]) : 0.0f, net->log_alpha[t], net->log_1m_alpha[t],
                          net->log_cumprod_alpha[tm1], net->log_1m_cumprod_alpha[tm1]};
    SS_PROPAGATE(f0_step(net, sf, f0, uv, lo, hi, lens, B, T, w, t, net->steps - 1 - t, t == 0, k, noise ? noise + (int64_t)t * n : nullptr,
                         gumbel_u ? gumbel_u + (int64_t)t * n * 2 : nullptr, seed, seed_dev, t > step_lo, stream));
  }
  return SS_OK;
}

// ---------------------------------------------------------------------------------------------
// Strided joint f0 / uv sampler: network times ts[0] > ts[1] > ... ; the transition t -> s (s = the next entry; "final" = x_0 after the last,
// cumprod alpha = 1, Lambda = 0). With a_i = 1 - beta_i, ac = cumprod(a), Lambda = cumsum(log a), all in double:
//   Gaussian half (the DDIM family of ss_meldiff_sample_ddim, the dyn_clip clamp on x0 kept):
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
  const double sig = eta * sqrt((1.0 - ac_s) / (1.0 - ac_t)) * sqrt(fmax(0.0, 1.0 - ac_t / ac_s));
  const double c2 = sqrt(fmax(0.0, 1.0 - ac_s - sig * sig) / (1.0 - ac_t));
  const double c1 = sqrt(ac_s) - c2 * sqrt(ac_t);
  const double la = lam_t - lam_s;
  F0StepCoef k;
  k.recip = (float)sqrt(1.0 / ac_t);
  k.recipm1 = (float)sqrt(1.0 / ac_t - 1.0);
  k.c1 = (float)c1;
  k.c2 = (float)c2;
  k.sigma = (float)sig;
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
  SS_CHECK_ARG(net->L > 0 && net->L <= SS_MAX_LAYERS && (net->C % 64) == 0, "ss_f0diff_sample_strided: bad net C=%d L=%d", net->C, net->L);
  SS_CHECK_ARG(net->out_dim == 3 && net->in_dim == 1, "ss_f0diff_sample_strided: net must be the 1->3 DDiffNet");
  SS_CHECK_ARG(net->n_groups <= 1 || (net->n_groups == 2 && B % 2 == 0), "ss_f0diff_sample_strided: paired nets need an even item count");
  const StackForm sf = resolve_form(net, B, T);
  const WsLayout w = ws_layout(net, sf, B, T, ws);
  SS_CHECK_ARG(ws_bytes >= w.bytes, "ss_f0diff_sample_strided: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)w.bytes);
  const int64_t n = (int64_t)B * T;
  if (do_precompute) SS_PROPAGATE(precompute_cond(net, sf, cond, lens, B, T, w, stream));
  const bool draw = eta > 0.0f;   // eta = 0: sigma = 0 on every transition and the Gaussian tape is never read
  for (int i = i_lo; i < i_hi; ++i) {
    if (i == i_lo) SS_PROPAGATE(f0_first_input(net, f0, uv, lens, B, T, w, stream));
    const int t = ts[i];
    const bool final_step = i + 1 == n_ts;   // the list's last entry, wherever the call is cut
    const F0StepCoef k = f0_strided_coef(sc, t, final_step ? -1 : ts[i + 1], (double)eta);
    // evaluation i of the loop; tape rows and the Philox counter are those of network time t
    SS_PROPAGATE(f0_step(net, sf, f0, uv, lo, hi, lens, B, T, w, t, i, final_step, k, (draw && noise) ? noise + (int64_t)t * n : nullptr,
                         gumbel_u ? gumbel_u + (int64_t)t * n * 2 : nullptr, seed, seed_dev, i + 1 < i_hi, stream));
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
