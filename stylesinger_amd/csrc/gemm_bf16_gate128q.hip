// The "fp16q4" gate (ss_gemm_bf16_args.split = 3): gate128_kernel (gemm_bf16_gate128.hip: 256 x 128 tiles, compact A image, two workgroups per
// CU) with the SECOND product of every 32-channel step - activation x weight-lo, a correction of relative size 2^-12 that needs two or three
// significant bits (oracle/second_product_numerics.py: 3.4e-5 / 4.2e-5 on the reference's goldens, bar 1e-4) - moved from the fp16 matrix
// instruction to the block-scaled fp4 one (v_mfma_scale_f32_32x32x64_f8f6f4: 3.7x the fp16 issue rate, tools/ubench/mfma_mx_layout.hip).
//   * Steps are paired in issue order (2 p, 2 p + 1). The instruction pairs lane (i, h) of A with lane (j, h) of B element by element, so its
//     K = 64 can be ANY 64 K indices: here the 2 x 2 k-steps of the pair. Lane (row, h) already holds exactly those 32 values of its row in the
//     four fp16 A fragments of the pair - it converts them in registers (v_cvt_scalef32_pk_fp4_f16, fixed power-of-two scale args.q_scale,
//     semantics measured by tools/ubench/cvt_fp4_probe.hip). NO fp4 copy of any activation exists in HBM or LDS.
//   * The weights' lo plane is packed once in that element order (gate128_layout.h, g128q; stylesinger_amd.lib.pack_gate_q4): 16 bytes per
//     lane half + one E8M0 scale byte, inside the second half of the weight line of the pair's odd step. Even steps fetch only their hi halves.
//   * Per pair 32 fp16 MFMAs + 8 block-scaled ones instead of 64: 0.63 of the matrix time at the measured issue rates.
// What it shares with gate128_kernel - descriptors, A / addend DMA roles, fragment addresses, the gate epilogue - is g128::tile / g128::gate_epilogue
// (gate128_layout.h); the fp4 register pieces it shares with tile256q_store_kernel are in gemm_lds_dma.h. Dispatched to by the denoiser stack
// (wavenet_stack.hip) for fp16q4 launches that pass ss_gemm_bf16_gate128q_ok.
#include "gate128_layout.h"
#include <type_traits>
#include <utility>

namespace {

using namespace ss_dev;

using namespace g128;
using g128q::CCS;   // K = 256 channels per tap = 8 chunks of 32

__global__ __launch_bounds__(256, 2) void gate128q_kernel(const ss_gemm_bf16_args a, int m_tiles_per_item, int m_tiles, int n_tiles, int d,
                                                          unsigned long long* clock_probe_out) {
  const clock_probe probe(clock_probe_out);
#include "gate128_prologue.h"
  // weight lines of EVEN steps carry nothing in their second half (slots 4-7): those lanes fetch nothing; odd steps carry the pair's fp4 lo
  // terms in slots 4, 5 and their scales in slot 6 (slot 7 unused)
  const int b_slot = b_dma_slot(wave, lane);
  const int b_dead_even = b_slot >= 4 ? (int)0x80000000 : 0, b_dead_odd = b_slot == 7 ? (int)0x80000000 : 0;
  auto piece_b = [&](char* buf, int S, int j) {   // the weight tile of step S
    glds16(rsrc_w, buf + (wave + 4 * j) * 1024, b_voff | ((S & 1) ? b_dead_odd : b_dead_even), g128q::step_line(S) * 128 + 32 * j * ldw * 2);
  };
  const int b_scale_off = b_frags.base + ((6 ^ b_swz(b_row)) << 4) + lh;   // byte lh of logical slot 6: this lane half's block scale (+ n * 32 * B_ROWB)

  f32x16 acc[4][2];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  // step S = 3 cc + tap (head and DMA piece list: gate_step). Per step the fp16 product a x hi only: k-step 0 (8 MFMAs) inside the step, k-step 1
  // (8) deferred past the next barrier as in gate128_kernel. Per PAIR of steps one block-scaled group (8 MFMAs) a_q x lo_q, issued after the
  // barrier that follows the odd step (deferred with that step's k-step 1: 16 deferred MFMAs after odd steps, 8 after even ones). The DMA pieces
  // of a step are issued one after each of its first MFMAs (deferred ones first, then k-step 0's).
  const float qs = a.q_scale;    // the activations' fixed fp4 scale: q = fp4(v / qs)
  const int sa = q4_e8m0(qs);
  bf16x8 p_ah[4], p_bh[2];
  unsigned aq[4][4];          // [m][register r]: the pair's 32 A values of this lane as fp4, r = 2 * (step parity) + k-step
  v8i bq[2];                  // [n]: the pair's 32 weight-lo values of this lane as fp4 (registers 0-3)
  int sb[2] = {127, 127};     // [n]: their block scale
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int i = 0; i < 8; ++i) bq[n][i] = 0;
  auto mfma_h = [&](int m, int n, const bf16x8 (&fa)[4], const bf16x8 (&fb)[2]) { acc[m][n] = ss_mfma_32x32x16<true>(fa[m], fb[n], acc[m][n]); };
  auto mfma_q = [&](int m, int n) { q4_mfma(acc[m][n], aq[m], bq[n], sa, sb[n]); };
  auto step = [&](auto stag) {
    constexpr int S = decltype(stag)::value;
    const gate_step<S, CCS> st(A0, B0, A1, B1);
    st.open();
    constexpr int TAP = st.TAP, NP = st.NP;
    constexpr bool ODD = (S & 1) != 0;
    bf16x8 ah0[4], bh0[2];
    a_frags[TAP](st.Ac, 0, ah0);
    b_frags(st.Bc, 0, bh0);
    __builtin_amdgcn_sched_barrier(0);
    auto piece = [&](int i) { st.piece(i, piece_b, piece_a, [&](int j) { piece_e(EQ0, 0, j); }); };
    // MFMA slots of this step before its second k-step's fragments are needed: the deferred ones of step S-1 (its k-step 1; after an odd step
    // also the pair's block-scaled group), then this step's k-step 0
    constexpr int ND = S == 0 ? 0 : (ODD ? 8 : 16);   // S odd -> step S-1 was even: 8 deferred; S even -> S-1 odd: 16
    static_assert(NP <= ND + 8, "more DMA pieces than MFMA slots to spread them over");
    if constexpr (S == 0) {
#pragma unroll
      for (int i = 0; i < NP; ++i) piece(i);
    }
    auto spread = [&](int i) {   // one DMA piece after each of the step's first NP MFMAs
      if (S > 0 && i < NP) {
        __builtin_amdgcn_sched_barrier(0);
        piece(i);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
#pragma unroll
    for (int i = 0; i < ND; ++i) {
      if (i < 8) mfma_h((i >> 1) & 3, i & 1, p_ah, p_bh);   // k-step 1 of step S-1
      else mfma_q(((i - 8) >> 1) & 3, (i - 8) & 1);          // the block-scaled group of the pair that ended with step S-1
      spread(i);
    }
    __builtin_amdgcn_sched_barrier(0);
    // this step's k-step 1 fragments (used after the next barrier) and, in odd steps, the pair's weight-lo terms + scales: in flight under k-step 0
    a_frags[TAP](st.Ac, 2, p_ah);
    b_frags(st.Bc, 2, p_bh);
    [[maybe_unused]] bf16x8 bqr[2];
    if constexpr (ODD) b_frags(st.Bc, 4, bqr);   // slot 4: this lane half's fp4 lo terms of the pair
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      mfma_h((k >> 1) & 3, k & 1, ah0, bh0);                 // k-step 0 of this step
      spread(ND + k);
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (ODD) q4_unpack<B_ROWB>(bqr, st.Bc + b_scale_off, bq, sb);
    __builtin_amdgcn_sched_barrier(0);
    // my own A values of this step as fp4: registers 2 * parity + ks of the pair's operand
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      aq[m][2 * (S & 1)] = q4_cvt8(ah0[m], qs);
      aq[m][2 * (S & 1) + 1] = q4_cvt8(p_ah[m], qs);
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (st.LAST) {   // nothing follows: the deferred work of the last (odd) step now
#pragma unroll
      for (int i = 0; i < 8; ++i) mfma_h((i >> 1) & 3, i & 1, p_ah, p_bh);
#pragma unroll
      for (int i = 0; i < 8; ++i) mfma_q((i >> 1) & 3, i & 1);
    }
  };
#pragma unroll
  for (int j = 0; j < 5; ++j) piece_a(A0, 0, j);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int j = 0; j < 4; ++j) piece_b(B0, 0, j);
  __builtin_amdgcn_sched_barrier(0);
  static_assert((CCS & 1) == 0, "the epilogue's LDS plan assumes the last step reads A1 / B1");
  unrolled_steps(step, std::make_integer_sequence<int, 3 * CCS>{});

#include "gate128_epilogue.h"
  probe.end(tid);
}

}  // namespace

// The launch contract (gate128_kernel's with split = 3 and the fp4 scale): nullptr, or the first rule the launch breaks; the launcher puts the
// kernel's name in front. ss_gemm_bf16_gate128q_ok
// asks it, so a launch that misses a rule falls back to the fp16x2 kernels instead of failing; ss_gemm_bf16_gate128q refuses with the same message.
static const char* gate128q_contract(const ss_gemm_bf16_args& a) {
  if (!(a.split == 3 && ss_out_scale_ok(a.out_scale))) return "fp16q4 operands only (split = 3, 0 < out_scale <= 1)";
  if (!ss_q_scale_ok(a.q_scale)) return "q_scale must be a power of two, 2^-21 .. 2^19";
  return g128_shared_contract(a);
}

// 1 if this GATE launch should run on the fp16q4 two-workgroups-per-CU kernel: the contract holds and there are enough rows that 256-row tiles
// fill the chip several times over (or the q4_force knob is set)
extern "C" int ss_gemm_bf16_gate128q_ok(const ss_gemm_bf16_args* a) {
  if (!a || gate128q_contract(*a)) return 0;
  const long tiles = (long)ss_cdiv(a->T, BM) * a->B * (a->Np / BN);
  return (g_ss_tuning.q4_force || tiles >= 8l * ss_n_cu()) ? 1 : 0;   // four rounds of two workgroups per CU
}

// ---- fp16q4 range guard: max |a| / (6 q_scale) over the hi plane of the A operand (rows < lens[b]) -> atomicMax on the float's bits
namespace {
__global__ void q4_guard_kernel(const uint16_t* __restrict__ A, int64_t a_batch_stride, int lda, int K, int T, const int32_t* __restrict__ lens, float inv_limit,
                                unsigned int* __restrict__ out, int64_t n) {
  float m = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {   // one 16-byte group of 8 channels each
    const int g = (int)(i % (K / 8));
    const int64_t r = i / (K / 8);
    const int b = (int)(r / T), t = (int)(r % T);
    if (lens && t >= lens[b]) continue;
    const uint4 v = *reinterpret_cast<const uint4*>(A + (int64_t)b * a_batch_stride + (int64_t)t * lda + (g >> 2) * 64 + (g & 3) * 8);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      m = fmaxf(m, fabsf(ss_t2f_packed<true>(w[k], 0)));
      m = fmaxf(m, fabsf(ss_t2f_packed<true>(w[k], 1)));
    }
  }
  m *= inv_limit;
  if (!(m == m)) m = INFINITY;   // a NaN operand counts as out of range
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(out, __float_as_uint(m));
}
}  // namespace

int ss_q4_guard_launch(const ss_gemm_bf16_args* a, int which, void* stream) {
  if (!g_ss_q4_guard) return SS_OK;
  const int64_t n = (int64_t)a->B * a->T * (a->K / 8);
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(q4_guard_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a->A, a->a_batch_stride, a->lda, a->K, a->T, a->lens, 1.0f / (6.0f * a->q_scale),
                     g_ss_q4_guard + which, n);
  SS_CHECK_LAUNCH("ss_q4_guard");
  return SS_OK;
}

extern "C" int ss_gemm_bf16_gate128q(const ss_gemm_bf16_args* args, void* stream) {
  SS_CHECK_ARG(args != nullptr, "ss_gemm_bf16_gate128q: null args");
  const ss_gemm_bf16_args& a = *args;
  const char* why = gate128q_contract(a);
  SS_CHECK_ARG(!why, "ss_gemm_bf16_gate128q: %s (q_scale = %g)", why, (double)a.q_scale);
  const int m_tiles_per_item = ss_cdiv(a.T, BM);
  const int m_tiles = m_tiles_per_item * a.B;
  const int n_tiles = a.Np / BN;
  const size_t lds = (size_t)80 * 1024;
  SS_PROPAGATE(ss_allow_lds("ss_gemm_bf16_gate128q", &gate128q_kernel, lds));
  SS_PROPAGATE(ss_q4_guard_launch(&a, 0, stream));
  hipLaunchKernelGGL(gate128q_kernel, dim3(ss_cdiv(m_tiles, 8) * 8 * n_tiles), dim3(256), lds, (hipStream_t)stream, a, m_tiles_per_item, m_tiles, n_tiles, a.tap_off[2],
                     g_ss_tuning.clock_probe);
  SS_CHECK_LAUNCH("ss_gemm_bf16_gate128q");
  return SS_OK;
}

extern "C" int ss_gate128q_kindex(int32_t* out, int n) {
  SS_CHECK_ARG(out != nullptr && n >= g128q::PAIRS * 2 * 32, "ss_gate128q_kindex: need room for %d entries", g128q::PAIRS * 2 * 32);
  for (int p = 0; p < g128q::PAIRS; ++p)
    for (int h = 0; h < 2; ++h)
      for (int e = 0; e < 32; ++e) out[(p * 2 + h) * 32 + e] = g128q::q_kindex(p, h, e, 256);
  return g128q::PAIRS * 2 * 32;
}
