// The "fp16x2" gate (ss_gemm_bf16_args.split = 2, SS_HEPI_GATE: dilated conv + conditioner addend + sigmoid * tanh, modules/diff/net.py:66-73)
// for many-round launches with TWO workgroups per CU: 256 rows x 128 packed columns per workgroup, 4 waves, 80 KB of LDS.
//
// Why (gate256_kernel<8, 2>, profiles/r04_bench_c4_fp16x2_20steps_kernel_stats.csv): at the BASELINE config 4 shape that kernel spends 311 us
// on 270 k matrix-pipe cycles per SIMD (46 % busy). One 160 KB workgroup owns a CU: its eight waves leave every barrier in lockstep, and while
// it runs its epilogue (1024 VALU instructions per lane, a quarter of them transcendental, four addend quarters by DMA) or waits at a step
// barrier, the matrix pipes have nothing else to run. The fp16x2 mode frees the LDS that a second workgroup needs: the A operand's second plane
// is never read, so the A image is COMPACT here - 64 bytes per row (the hi plane of a 32-channel chunk), 20 KB per buffer instead of 40 -
// and half the columns halve the weight tile: operands 2 x (20 + 16) KB = 72 KB, epilogue view 2 x 32 KB addend quarters + 16 KB staging =
// 80 KB. A SIMD then holds one wave of each of two INDEPENDENT workgroups: one's MFMAs fill the other's epilogue and barrier waits.
// Everything else is the plan of gate256_kernel<8, 2>: the wave tile (128 x 64: 4 x 2 accumulators, 8 fragment reads per 16 MFMAs), 24 steps of 32
// channels x 2 k-steps x 2 products (hi x hi, hi x lo) with the second k-step's 16 MFMAs deferred past the next barrier and the DMA pieces
// issued between them, 5 A + 4 B (+ 8 addend) pieces per wave exactly as there - so the counted s_waitcnt of both loops carry over.
// All index math lives in gate128_layout.h and is checked on the host against a tagged LDS image (tools/layout_check_gate128.cpp). The same header
// holds what this kernel shares with gate128q_kernel (g128::tile, g128::gate_epilogue); the step head and its DMA piece list (gate_step), shared
// with gate256_kernel as well, are in gemm_lds_dma.h. This file keeps the weight pieces and the step.
// Arithmetic contract = gate256_kernel<8, 2>: results equal up to the K summation order (the same order, in fact: same steps, same tiles).
#include "gate128_layout.h"
#include <type_traits>
#include <utility>

namespace {

using namespace ss_dev;

using namespace g128;
constexpr int CCS = 8;   // K = 256 channels per tap = 8 chunks of 32

__global__ __launch_bounds__(256, 2) void gate128_kernel(const ss_gemm_bf16_args a, int m_tiles_per_item, int m_tiles, int n_tiles, int d,
                                                          unsigned long long* clock_probe_out) {
  const clock_probe probe(clock_probe_out);
#include "gate128_prologue.h"
  auto piece_b = [&](char* buf, int S, int j) {   // the weight tile of step S = 3 cc + tap
    glds16(rsrc_w, buf + (wave + 4 * j) * 1024, b_voff, ((S % 3) * CCS + S / 3) * 128 + 32 * j * ldw * 2);
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  // step S = 3 cc + tap (gate256_kernel's step_w2): at its top my pieces of this step's operands have landed (counted vmcnt: the A chunk of
  // cc + 1 is issued in the tap-1 step AFTER that step's weight pieces, so at the top of the tap-2 step its 5 pieces may still fly); barrier;
  // first fragment reads; the 16 MFMAs step S-1 deferred (hi x lo, hi x hi of its second k-step) with this step's DMA pieces between them;
  // then hi x hi and hi x lo of the first k-step, the second k-step's fragments are read and its MFMAs left for after the next barrier.
  bf16x8 p_ah[4], p_bh[2], p_bm[2];
  auto step = [&](auto stag) {
    const gate_step<decltype(stag)::value, CCS> st(A0, B0, A1, B1);
    st.open();
    constexpr int TAP = st.TAP;
    const char* const Ac = st.Ac;
    const char* const Bc = st.Bc;
    bf16x8 ah0[4], bh0[2];
    a_frags[TAP](Ac, 0, ah0);
    b_frags(Bc, 0, bh0);
    __builtin_amdgcn_sched_barrier(0);
    st.template deferred<true>(acc, p_ah, p_bm, p_bh, [&](int i) { st.piece(i, piece_b, piece_a, [&](int j) { piece_e(EQ0, 0, j); }); });
    __builtin_amdgcn_sched_barrier(0);
    bf16x8 bm0[2];
    b_frags(Bc, 4, bm0);
    __builtin_amdgcn_sched_barrier(0);
    mfma8<true>(acc, ah0, bh0);            // k-step 0: hi x hi
    __builtin_amdgcn_sched_barrier(0);
    a_frags[TAP](Ac, 2, p_ah);
    b_frags(Bc, 2, p_bh);
    __builtin_amdgcn_sched_barrier(0);
    mfma8<true>(acc, ah0, bm0);            // k-step 0: hi x lo
    __builtin_amdgcn_sched_barrier(0);
    b_frags(Bc, 6, p_bm);            // k-step 1's two groups run after the next barrier
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (st.LAST) {
      mfma8<true>(acc, p_ah, p_bm);
      mfma8<true>(acc, p_ah, p_bh);
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

// The launch contract: nullptr, or the first rule the launch breaks (the launcher puts the kernel's name in front). ss_gemm_bf16_gate128_ok asks it, so a launch that misses a rule falls
// back to the other kernels instead of failing; ss_gemm_bf16_gate128 refuses with the same message.
static const char* gate128_contract(const ss_gemm_bf16_args& a) {
  if (!(a.split == 2 && ss_out_scale_ok(a.out_scale))) return "fp16x2 operands only (split = 2, 0 < out_scale <= 1)";
  return g128_shared_contract(a);
}

// 1 if ss_gemm_bf16 should hand this GATE launch to the two-workgroups-per-CU kernel: the contract holds and there are enough rows that
// 256-row tiles fill the chip several times over
extern "C" int ss_gemm_bf16_gate128_ok(const ss_gemm_bf16_args* a) {
  if (!a || gate128_contract(*a)) return 0;
  const long tiles = (long)ss_cdiv(a->T, BM) * a->B * (a->Np / BN);
  return tiles >= 8l * ss_n_cu() ? 1 : 0;   // four rounds of two workgroups per CU (2048 tiles on the 256 CUs of an MI355X)
}

extern "C" int ss_gemm_bf16_gate128(const ss_gemm_bf16_args* args, void* stream) {
  SS_CHECK_ARG(args != nullptr, "ss_gemm_bf16_gate128: null args");
  const ss_gemm_bf16_args& a = *args;
  const char* why = gate128_contract(a);
  SS_CHECK_ARG(!why, "ss_gemm_bf16_gate128: %s", why);
  const int m_tiles_per_item = ss_cdiv(a.T, BM);
  const int m_tiles = m_tiles_per_item * a.B;
  const int n_tiles = a.Np / BN;
  return ss_launch_lds("ss_gemm_bf16_gate128", &gate128_kernel, ss_cdiv(m_tiles, 8) * 8 * n_tiles, 256, (size_t)80 * 1024, stream, a, m_tiles_per_item, m_tiles, n_tiles,
                       a.tap_off[2], g_ss_tuning.clock_probe);
}
