// Device code shared by the many-round 16-bit LDS-DMA GEMM kernels: gate256_kernel (gemm_bf16_gate256.hip), gate128_kernel / gate128q_kernel
// (gemm_bf16_gate128.hip / gemm_bf16_gate128q.hip), tile256s_kernel (gemm_bf16_tile256.hip) and tile256q_store_kernel (gemm_bf16_tile256q.hip).
// All five keep a wave tile of 128 x 64 = 4 x 2 accumulators of 32x32 and feed it from swizzled LDS images whose fragments sit 32 rows apart, so
// the fragment reads, the 8-MFMA product group, the step bookkeeping of the 3-tap gates, the gate activation and the fp16q4 register pieces are
// written once, here. Like device_prims.h: everything is __forceinline__ and lives in namespace ss_dev; accumulators, fragments and LDS pointers
// are taken by reference - nothing here copies a register array or indexes one at run time.
// Only what leaves every kernel instruction for instruction as it was (vector opcode counts, registers, schedule) lives here as functions. What
// does not - any function or struct around the XCD-aware tile walk, the gate128 prologue / epilogue or the STORE epilogue makes the compiler
// select other vector address arithmetic - is either shared as kernel TEXT (gate128_prologue.h, gate128_epilogue.h, tile256_store_epilogue.h,
// #included inside the kernel bodies) or, for the five-line tile walk, left in its three kernels. For the same reason gate128 / gate128q clear
// their accumulators themselves (clear_acc costs gate128 a v_readfirstlane), and gate256's dma_b keeps its own DMA line.
// The clock probe below serves gate128 / gate128q only; the Winograd gate files and layer512.hip keep their own copies (another family).
#pragma once
#include "common.h"
#include "device_prims.h"
#include "../../include/stylesinger_hip.h"
#include "pair16.h"

namespace ss_dev {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));

// ss_set_clock_probe: workgroup 0 reports the shader cycles and 100 MHz ticks its first wave lived (-> the clock the launch sustained)
struct clock_probe {
  unsigned long long* const out;
  const bool probing;
  unsigned long long c0 = 0, r0 = 0;
  __device__ __forceinline__ explicit clock_probe(unsigned long long* p) : out(p), probing(p != nullptr && blockIdx.x == 0) {
    if (probing) {
      c0 = __builtin_readcyclecounter();
      r0 = __builtin_amdgcn_s_memrealtime();
    }
  }
  __device__ __forceinline__ void end(int tid) const {
    if (probing && tid == 0) {
      atomicAdd(out, (unsigned long long)__builtin_readcyclecounter() - c0);
      atomicAdd(out + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime() - r0);
    }
  }
};

// N fragments 32 rows apart (rows of ROWB bytes) at one slot: byte_off = row base + (physical slot << 4)
template <int N, int ROWB>
__device__ __forceinline__ void read_frags(const char* buf, int byte_off, bf16x8 (&f)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) f[i] = *reinterpret_cast<const bf16x8*>(buf + byte_off + i * 32 * ROWB);
}
// ... as one lane addresses them in a swizzled image: `base` = byte of its first row, logical 16-byte slot s sits at physical slot s ^ swz
// (the lane half lh is folded into swz; 32 more rows leave the swizzle unchanged): one XOR per read
template <int N, int ROWB>
struct frags {
  int base, swz;
  __device__ __forceinline__ void operator()(const char* buf, int slot, bf16x8 (&f)[N]) const { read_frags<N, ROWB>(buf, base + ((slot ^ swz) << 4), f); }
};

// one product group of the wave tile: 4 x 2 MFMAs of 32x32x16
template <bool F16>
__device__ __forceinline__ void mfma8(f32x16 (&acc)[4][2], const bf16x8 (&fa)[4], const bf16x8 (&fb)[2]) {
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[m][n] = ss_mfma_32x32x16<F16>(fa[m], fb[n], acc[m][n]);
}

__device__ __forceinline__ void clear_acc(f32x16 (&acc)[4][2]) {
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;
}

// Step S = 3 cc + tap of the 3-tap gate kernels (CCS channel chunks per tap; weight tiles alternate B0 / B1 every step, A chunks A0 / A1 every
// channel chunk). open() opens the step: my pieces of this step's operands have landed - counted vmcnt: the A chunk of cc + 1 is issued
// in the tap-1 step AFTER that step's weight pieces, so at the top of the tap-2 step its 5 pieces may still fly - then the barrier (everyone's
// pieces landed, everyone finished reading step S - 1).
// DMA pieces the step issues, in this order (the vmcnt counts rely on it): the weight tile of step S + 1, at tap 1 the A chunk cc + 1, in the
// last step the first addend quarter (into A0 / B0, which that step does not read). No DMA is ever issued past the last step: the epilogue's
// addend quarters reuse this memory and must not race with zero fills.
template <int S, int CCS>
struct gate_step {
  static constexpr int CC = S / 3, TAP = S % 3;
  static constexpr bool LAST = S + 1 >= 3 * CCS, A_NEXT = TAP == 1 && CC + 1 < CCS;
  static constexpr int NB = LAST ? 0 : 4, NA = A_NEXT ? 5 : 0, NE = LAST ? 8 : 0, NP = NB + NA + NE;
  const char* const Ac;
  const char* const Bc;
  char* const An;
  char* const Bn;
  __device__ __forceinline__ gate_step(char* A0, char* B0, char* A1, char* B1)
      : Ac((CC & 1) ? A1 : A0), Bc((S & 1) ? B1 : B0), An((CC & 1) ? A0 : A1), Bn((S & 1) ? B0 : B1) {}
  __device__ __forceinline__ void open() const {
    if constexpr (TAP == 2 && CC + 1 < CCS) wait_vmcnt<5>();
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
  }
  // piece i < NP: piece_b(buffer, step, j), piece_a(buffer, chunk, j), piece_e(j)
  template <class PB, class PA, class PE>
  __device__ __forceinline__ void piece(int i, PB&& piece_b, PA&& piece_a, PE&& piece_e) const {
    if (i < NB) piece_b(Bn, S + 1, i);
    else if (i < NB + NA) piece_a(An, CC + 1, i - NB);
    else piece_e(i - NB - NA);
  }
  // the two product groups step S - 1 deferred past this step's barrier (p_ah x p_bm, then p_ah x p_bh), one DMA piece after every MFMA until
  // the pieces are out: the matrix pipe has work while every wave of the workgroup is issuing DMA / waiting on LDS. The first step defers nothing.
  template <bool F16, class P>
  __device__ __forceinline__ void deferred(f32x16 (&acc)[4][2], const bf16x8 (&p_ah)[4], const bf16x8 (&p_bm)[2], const bf16x8 (&p_bh)[2], P&& piece_i) const {
    static_assert(NP <= 16, "more DMA pieces than deferred MFMAs");
    if constexpr (S > 0) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int m = (i >> 1) & 3, n = i & 1;
        acc[m][n] = ss_mfma_32x32x16<F16>(p_ah[m], i < 8 ? p_bm[n] : p_bh[n], acc[m][n]);
        if (i < NP) {
          __builtin_amdgcn_sched_barrier(0);
          piece_i(i);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < NP; ++i) piece_i(i);
    }
  }
};

// The gate nonlinearity sigmoid(x_s) * tanh(x_t) on the hardware exp2 / rcp units: act(x) = sc * rcp(1 + exp2(x * mul)) + sh is the sigmoid
// with (-log2 e, 1, 0) and tanh with (-2 log2 e, 2, -1). gate_mode 0 = the first operand is the sigmoid's, else the second.
struct gate_act {
  float m0, s0, h0, m1, s1, h1;
  __device__ __forceinline__ explicit gate_act(int gate_mode) {
    const bool sig_first = gate_mode == 0;
    const float L2E = 1.44269504088896340736f;
    m0 = (sig_first ? -1.0f : -2.0f) * L2E, s0 = sig_first ? 1.0f : 2.0f, h0 = sig_first ? 0.0f : -1.0f;
    m1 = (sig_first ? -2.0f : -1.0f) * L2E, s1 = sig_first ? 2.0f : 1.0f, h1 = sig_first ? -1.0f : 0.0f;
  }
  static __device__ __forceinline__ float act(float x, float mul, float sc, float sh) {
    return fmaf(__builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * mul)), sc, sh);
  }
  __device__ __forceinline__ float operator()(float x0, float x1) const { return act(x0, m0, s0, h0) * act(x1, m1, s1, h1); }
};

// ---- fp16q4 (ss_gemm_bf16_args.split = 3): the second product of a PAIR of 32-channel steps on the block-scaled fp4 matrix instruction.
// 8 fp16 -> 8 fp4 at the fixed power-of-two scale qs: element t in nibble t & 1 of byte t >> 1 (tools/ubench/cvt_fp4_probe.hip)
__device__ __forceinline__ unsigned q4_cvt8(const bf16x8& f, float qs) {
  const ss_f16x8 v = __builtin_bit_cast(ss_f16x8, f);
  unsigned r = 0;
  r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(r, h2{v[0], v[1]}, qs, 0);
  r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(r, h2{v[2], v[3]}, qs, 1);
  r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(r, h2{v[4], v[5]}, qs, 2);
  r = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(r, h2{v[6], v[7]}, qs, 3);
  return r;
}
// qs as the instruction's E8M0 scale byte: qs is a power of two, its biased exponent IS 127 + log2(qs)
__device__ __forceinline__ int q4_e8m0(float qs) { return (int)((__builtin_bit_cast(unsigned, qs) >> 23) & 0xffu); }
// acc += aq (this lane's 32 A values of the pair, registers 2 * (step parity) + k-step) x bq (its 32 weight-lo values, registers 0-3)
__device__ __forceinline__ void q4_mfma(f32x16& acc, const unsigned (&aq)[4], const v8i& bq, int sa, int sb) {
  v8i av;
#pragma unroll
  for (int i = 0; i < 4; ++i) av[i] = (int)aq[i];
#pragma unroll
  for (int i = 4; i < 8; ++i) av[i] = 0;
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bq, acc, 4, 4, 0, sa, 0, sb);
}
// the pair's weight-lo fragments as read from the odd step's weight line (logical slot 4 + lh) -> operand registers, and their block scales
// (byte lh of logical slot 6 of the same line: scale_at + n * 32 * ROWB)
template <int ROWB>
__device__ __forceinline__ void q4_unpack(const bf16x8 (&bqr)[2], const char* scale_at, v8i (&bq)[2], int (&sb)[2]) {
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const u32x4 w = __builtin_bit_cast(u32x4, bqr[n]);
#pragma unroll
    for (int i = 0; i < 4; ++i) bq[n][i] = (int)w[i];
    sb[n] = *reinterpret_cast<const uint8_t*>(scale_at + n * 32 * ROWB);
  }
}

}  // namespace ss_dev
