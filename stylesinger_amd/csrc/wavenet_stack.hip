// The residual stack of the two denoisers, as host-side launch sequences over the fp32-MFMA conv kernel and the 16-bit GEMM kernels. The three
// reverse loops of the hot path (mel_sampler.hip, f0_sampler.hip) run it once per network evaluation.
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
#include "wavenet_stack.h"
#include "launch_args.h"

namespace ss_stack {

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
    // the skip GEMM's many-round kernel reads a compact operand (ss_gemm_bf16_args.a_compact). The layout of GAh is fixed before any launch, so
    // the kernel's size rule is asked of its owner here (ss_gemm_bf16_tile256_rounds_ok)
    f.g_compact = knob.gate256 != 0 && ss_gemm_bf16_tile256_rounds_ok(B, T) && ((L * C) % 64) == 0 && C <= 256;
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
      // 1 KB contiguous per instruction instead of 8 lines x 32 B; for that the tiling is fixed here: the one the launch itself would run
      const int mt = ss_wino43_gate16_mt(B, T, 2 * C, y.d, round_up32(C), y.mt);
      const int64_t fl = mt > 0 ? ss_gate16_tiled_floats(B, T, 2 * C, y.d, mt) : -1;
      if (fl <= 0 || fl * 4 >= (1ll << 31)) continue;
      y.mt = mt;
      y.e16_floats = fl;
    }
  }
  return f;
}

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

namespace {

// One function per StackKind:
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
    set_r(o, w.X, C, T);
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

}  // namespace

int run_residual_stack(const ss_wavenet* net, const StackForm& sf, int step, int eval, const int32_t* lens, int B, int T, const WsLayout& w, hipStream_t stream,
                       bool leave_partials) {
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

int open_sampler(const char* who, const ss_wavenet* net, int B, int T, const float* cond, const int32_t* lens, void* ws, int64_t ws_bytes, int c_multiple,
                 bool pairs_ok, bool do_precompute, hipStream_t stream, SamplerCtx& out) {
  SS_CHECK_ARG(net->L > 0 && net->L <= SS_MAX_LAYERS && (net->C % c_multiple) == 0, "%s: bad net C=%d L=%d", who, net->C, net->L);
  if (pairs_ok) SS_CHECK_ARG(net->n_groups <= 1 || (net->n_groups == 2 && B % 2 == 0), "%s: paired nets need an even item count", who);
  else SS_CHECK_ARG(net->n_groups <= 1, "%s: grouped nets are only supported by the f0 sampler", who);
  out.sf = resolve_form(net, B, T);
  out.w = ws_layout(net, out.sf, B, T, ws);
  SS_CHECK_ARG(ws_bytes >= out.w.bytes, "%s: workspace too small (%lld < %lld)", who, (long long)ws_bytes, (long long)out.w.bytes);
  if (do_precompute) SS_PROPAGATE(precompute_cond(net, out.sf, cond, lens, B, T, out.w, stream));
  return SS_OK;
}

}  // namespace ss_stack

extern "C" int64_t ss_wavenet_workspace_bytes(const ss_wavenet* net, int B, int T) {
  if (!net || B <= 0 || T <= 0) return -1;
  return ss_stack::ws_layout(net, ss_stack::resolve_form(net, B, T), B, T, nullptr).bytes;
}
