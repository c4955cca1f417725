// The "fp16q4" long-K STORE GEMM (ss_gemm_bf16_args.split = 3, SS_HEPI_STORE: the K = L*C skip GEMM of the denoiser loops) for many-round
// launches: tile256s_kernel<STORE, true> (gemm_bf16_tile256.hip: 256 rows x all N <= 256 columns per workgroup, 8 waves, both operands by LDS-DMA)
// with the SECOND product of every 32-channel step - activation x weight-lo - on the block-scaled fp4 matrix instruction, exactly as
// gate128q_kernel does it (gemm_bf16_gate128q.hip): consecutive chunks (2 p, 2 p + 1) form a pair; a lane converts its own four fp16 A fragments
// of the pair to fp4 in registers (fixed power-of-two scale args.q_scale: the A operand here is the gate output z in (-1, 1), scale 2^-2 in the
// numerics study) and meets the pair's weight-lo terms, packed once in that lane order in the second half of the ODD chunk's weight line
// (stylesinger_amd.lib.pack_skip_q4, element order g128q-style: t128q::q_kindex). Per pair 32 fp16 MFMAs + 8 block-scaled ones instead of 64.
// The launch sits at the chip's power-limited matrix rate, so fewer matrix instructions are what makes it faster.
// The fp4 register pieces (q4_cvt8, q4_mfma, q4_unpack) and the STORE epilogue both kernels share are in gemm_lds_dma.h. Dispatched to by the denoiser
// stack (wavenet_stack.hip) for fp16q4 launches that pass ss_gemm_bf16_tile256q_ok.
#include "gemm_lds_dma.h"
#include "gate128_layout.h"
#include <type_traits>

namespace {

using namespace ss_dev;

constexpr int BM = 256, BN = 256;
constexpr int ROWB = 128;   // bytes per LDS row: A = 32 channels x (hi | unused plane), B = 32 channels hi | the pair's fp4 lo terms + scales

__global__ __launch_bounds__(512, 2) void tile256q_store_kernel(const ss_gemm_bf16_args a, int m_tiles_per_item, int m_tiles, int kchunks) {
  extern __shared__ __attribute__((aligned(16))) char smem_t256q[];   // 128 KB: [A0 32 K][B0 32 K][A1 32 K][B1 32 K]; epilogue: 2 x 64 KB staging
  char* const A0 = smem_t256q;
  char* const B0 = A0 + BM * ROWB;
  char* const A1 = B0 + BN * ROWB;
  char* const B1 = A1 + BM * ROWB;

  const int mt = blockIdx.x;
  if (mt >= m_tiles) return;
  const int b = mt / m_tiles_per_item;
  const int t0 = (mt % m_tiles_per_item) * BM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int l31 = lane & 31, lh = lane >> 5;
  const int len = ss_uniform_len(a.lens, b, a.T);
  const int grp_w = a.group_size > 0 ? b / a.group_size : 0;
  const int ldw = 2 * a.K;            // 16-bit terms per packed weight row (one 64-element line per 32-channel chunk)

  const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc(
      uniform_ptr(a.A + (int64_t)b * a.a_batch_stride), 0, __builtin_amdgcn_readfirstlane(len * a.lda * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(
      uniform_ptr(a.W + (int64_t)grp_w * a.w_group_stride), 0, __builtin_amdgcn_readfirstlane(a.Np * ldw * 2), 0x00020000);

  // DMA roles: tile256s_kernel's. 32 pieces of 8 rows x 128 B per operand and step; wave w issues pieces w, w + 8, w + 16, w + 24 of both. Lane i
  // of a piece lands at (row i >> 3, physical slot i & 7) and fetches logical slot (i & 7) ^ ((row >> 1) & 7). Dead lanes (nothing fetched, zeros
  // written): the A operand's second plane (slots 4-7) always; the weight line's slots 4-7 in EVEN chunks, slot 7 in odd ones
  const int r0 = 8 * wave + (lane >> 3);
  const int slot0 = (lane & 7) ^ ((r0 >> 1) & 7);
  const int a_voff = (((t0 + r0) * a.lda + slot0 * 8) * 2) | (slot0 >= 4 ? (int)0x80000000 : 0);   // rows >= len are out of range anyway
  const int b_voff = (r0 * ldw + slot0 * 8) * 2;                                                  // packed weight rows >= Np read zeros
  const int b_dead_even = slot0 >= 4 ? (int)0x80000000 : 0, b_dead_odd = slot0 == 7 ? (int)0x80000000 : 0;
  auto piece = [&](char* Ab, char* Bb, int c, int i) {     // i = 0..3: A pieces, 4..7: B pieces of chunk c
    const int j = i & 3;
    if (i < 4) glds16(rsrc_a, Ab + (wave + 8 * j) * 8 * ROWB, a_voff + 64 * j * a.lda * 2, c * ROWB);
    else glds16(rsrc_w, Bb + (wave + 8 * j) * 8 * ROWB, b_voff | ((c & 1) ? b_dead_odd : b_dead_even), c * ROWB + 64 * j * ldw * 2);
  };

  // fragment addresses: row = 128 wm + 32 m + l31 for A, 64 wn + 32 n + l31 for B; slot (2 ks) ^ swz = hi plane of k-step ks; B slot 4 ^ swz = this
  // lane half's 32 fp4 lo terms of the pair (odd chunks), byte lh of logical slot 6 = their E8M0 scale
  const frags<4, ROWB> a_frags{(128 * wm + l31) * ROWB, (((128 * wm + l31) >> 1) & 7) ^ lh};
  const int b_row = 64 * wn + l31;
  const frags<2, ROWB> b_frags{b_row * ROWB, ((b_row >> 1) & 7) ^ lh};
  const int b_scale_off = b_frags.base + ((6 ^ ((b_row >> 1) & 7)) << 4) + lh;

  f32x16 acc[4][2];
  clear_acc(acc);

  const float qs = a.q_scale;
  const int sa = q4_e8m0(qs);
  // deferred past the next barrier: k-step 1 of a step (fragments p_ah, p_bh) and, after odd steps, the pair's block-scaled group (aq, bq, sb);
  // all zero before the first step, so that the first step's deferred instructions add nothing
  bf16x8 p_ah[4], p_bh[2];
  unsigned aq[4][4];
  v8i bq[2];
  int sb[2] = {127, 127};
#pragma unroll
  for (int m = 0; m < 4; ++m) {
#pragma unroll
    for (int e = 0; e < 8; ++e) p_ah[m][e] = (__bf16)0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) aq[m][i] = 0u;
  }
#pragma unroll
  for (int n = 0; n < 2; ++n) {
#pragma unroll
    for (int e = 0; e < 8; ++e) p_bh[n][e] = (__bf16)0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) bq[n][i] = 0;
  }
  auto mfma_h = [&](int m, int n, const bf16x8 (&fa)[4], const bf16x8 (&fb)[2]) { acc[m][n] = ss_mfma_32x32x16<true>(fa[m], fb[n], acc[m][n]); };
  auto mfma_q = [&](int m, int n) { q4_mfma(acc[m][n], aq[m], bq[n], sa, sb[n]); };
  auto step = [&](auto par_tag, const char* Ac, const char* Bc, char* An, char* Bn, int c, bool more) {
    constexpr int PAR = decltype(par_tag)::value;   // chunk parity inside its pair
    wait_vmcnt<0>();                  // my pieces of chunk c have landed (nothing younger is in flight)
    __builtin_amdgcn_s_barrier();     // everyone's have; everyone finished reading chunk c-1's buffers
    bf16x8 ah0[4], bh0[2];
    a_frags(Ac, 0, ah0);
    b_frags(Bc, 0, bh0);
    __builtin_amdgcn_sched_barrier(0);
    // deferred by the previous step: its k-step 1 (8) and, when that step closed a pair (this one opens the next: PAR == 0), the pair's
    // block-scaled group (8); one DMA piece of the next chunk after each of the first 8
    constexpr int ND = PAR == 0 ? 16 : 8;
#pragma unroll
    for (int i = 0; i < ND; ++i) {
      if (i < 8) mfma_h((i >> 1) & 3, i & 1, p_ah, p_bh);
      else mfma_q(((i - 8) >> 1) & 3, (i - 8) & 1);
      if (i < 8) {
        __builtin_amdgcn_sched_barrier(0);
        if (more) piece(An, Bn, c + 1, i);   // wave-uniform branch
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    a_frags(Ac, 2, p_ah);
    b_frags(Bc, 2, p_bh);
    [[maybe_unused]] bf16x8 bqr[2];
    if constexpr (PAR == 1) b_frags(Bc, 4, bqr);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 8; ++k) mfma_h((k >> 1) & 3, k & 1, ah0, bh0);   // k-step 0 of this step
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (PAR == 1) q4_unpack<ROWB>(bqr, Bc + b_scale_off, bq, sb);
#pragma unroll
    for (int m = 0; m < 4; ++m) {   // my own A values of this step as fp4: registers 2 * PAR + ks of the pair's operand
      aq[m][2 * PAR] = q4_cvt8(ah0[m], qs);
      aq[m][2 * PAR + 1] = q4_cvt8(p_ah[m], qs);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;
#pragma unroll
  for (int i = 0; i < 8; ++i) piece(A0, B0, 0, i);
  __builtin_amdgcn_sched_barrier(0);
  for (int c = 0; c < kchunks; c += 2) {   // kchunks is even (checked by the launcher)
    step(P0{}, A0, B0, A1, B1, c, true);
    step(P1{}, A1, B1, A0, B0, c + 1, c + 2 < kchunks);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) mfma_h((i >> 1) & 3, i & 1, p_ah, p_bh);   // the last (odd) step's deferred work
#pragma unroll
  for (int i = 0; i < 8; ++i) mfma_q((i >> 1) & 3, i & 1);

  // ---- epilogue: the fp16 STORE form of tile256_store_epilogue (gemm_lds_dma.h), as tile256s_kernel<SS_HEPI_STORE, true>
  const int row_lim = a.mask_rows ? (len < a.T ? len : a.T) : a.T;
  const float* biasg = a.bias ? a.bias + (int64_t)grp_w * a.bias_group_stride : nullptr;
  __builtin_amdgcn_s_barrier();   // everyone is done reading the operand buffers
  const int st_wr = (32 * wm + 4 * lh) * (BN * 4) + (64 * wn + l31) * 4;   // + rr * BN * 4 (+ 128 for n = 1)
  constexpr bool W2 = true;
  char* const smem = smem_t256q;
#include "tile256_store_epilogue.h"
}

}  // namespace

// The launch contract (tile256s_kernel's STORE form with split = 3 and the fp4 scale): nullptr, or the first rule the launch breaks; the launcher
// puts the kernel's name in front. ss_gemm_bf16_tile256q_ok asks it; ss_gemm_bf16_tile256q refuses with the same message.
static const char* tile256q_contract(const ss_gemm_bf16_args& a) {
  if (!(a.A && a.W && a.C && a.split == 3 && a.ntaps == 1 && a.tap_off[0] == 0 && a.epi == SS_HEPI_STORE && ss_out_scale_ok(a.out_scale)))
    return "fp16q4 operands (split = 3, 0 < out_scale <= 1), one tap at offset 0, STORE";
  if (!ss_q_scale_ok(a.q_scale)) return "q_scale must be a power of two, 2^-21 .. 2^19";
  if (!(a.N > 0 && a.N <= BN && a.Np >= a.N && (a.K % 64) == 0 && a.lda >= 2 * a.K && (a.lda % 8) == 0))
    return "N <= 256, K % 64 == 0, lda % 8 == 0 and >= 2 K";
  if (!(ss_aligned16(a.A) && ss_aligned16(a.W) && (a.a_batch_stride & 7) == 0)) return "A/W must be 16-byte aligned";
  if (!(ss_fits_i31(a.T, a.lda, 2) && ss_fits_i31(a.Np, a.K, 4) && ss_fits_i31(a.T, a.ldc, 4))) return "item too large for 32-bit offsets";
  if (!((a.N % 4) == 0 && (a.ldc % 4) == 0 && (a.act == SS_ACT_NONE_ || a.act == SS_ACT_RELU_))) return "N % 4 == 0, ldc % 4 == 0, act none | relu";
  return nullptr;
}

// 1 if this STORE launch should run on the fp16q4 256-row kernel: the contract holds and there are at least two rounds of tiles (or q4_force)
extern "C" int ss_gemm_bf16_tile256q_ok(const ss_gemm_bf16_args* a) {
  if (!a || tile256q_contract(*a)) return 0;
  return (g_ss_tuning.q4_force || (long)ss_cdiv(a->T, BM) * a->B >= 2L * ss_n_cu()) ? 1 : 0;
}

extern "C" int ss_gemm_bf16_tile256q(const ss_gemm_bf16_args* args, void* stream) {
  SS_CHECK_ARG(args != nullptr, "ss_gemm_bf16_tile256q: null args");
  const ss_gemm_bf16_args& a = *args;
  const char* why = tile256q_contract(a);
  SS_CHECK_ARG(!why, "ss_gemm_bf16_tile256q: %s (q_scale = %g)", why, (double)a.q_scale);
  const int m_tiles_per_item = ss_cdiv(a.T, BM);
  const int m_tiles = m_tiles_per_item * a.B;
  const size_t lds = (size_t)128 * 1024;
  SS_PROPAGATE(ss_allow_lds("ss_gemm_bf16_tile256q", &tile256q_store_kernel, lds));
  SS_PROPAGATE(ss_q4_guard_launch(&a, 1, stream));
  hipLaunchKernelGGL(tile256q_store_kernel, dim3(m_tiles), dim3(512), lds, (hipStream_t)stream, a, m_tiles_per_item, m_tiles, a.K / 32);
  SS_CHECK_LAUNCH("ss_gemm_bf16_tile256q");
  return SS_OK;
}

// K index of element e of lane half h in chunk pair p of a 1-tap GEMM (the order lib.pack_skip_q4 packs the fp4 lo terms in)
extern "C" int ss_tile256q_kindex(int32_t* out, int n_pairs) {
  SS_CHECK_ARG(out != nullptr && n_pairs > 0, "ss_tile256q_kindex: bad args");
  for (int p = 0; p < n_pairs; ++p)
    for (int h = 0; h < 2; ++h)
      for (int e = 0; e < 32; ++e) out[(p * 2 + h) * 32 + e] = t128q_kindex(p, h, e);
  return n_pairs * 64;
}
