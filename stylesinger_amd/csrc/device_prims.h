// Device primitives shared by the kernel sources (gfx950): vector typedefs, buffer-descriptor and LDS-DMA helpers, the LDS slot
// swizzles, the quad -> frame map and the float4 / float2 arithmetic of the Winograd F(4,3) kernels, and the bf16 conversions.
// Everything is __forceinline__ and lives in namespace ss_dev; a source opens it inside its own anonymous namespace
// (using namespace ss_dev;). Per-kernel tile constants (BK, BN, ROWB, HALO, ...) stay with their kernels.
#pragma once
#include "common.h"
#include <type_traits>
#include <utility>

namespace ss_dev {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// A pointer for __builtin_amdgcn_make_buffer_rsrc: both halves go through readfirstlane so that hipcc can PROVE the descriptor
// wave-uniform; otherwise every buffer op is wrapped in a waterfall loop (cdna_hip_programming.md T20). The builtin takes a pointer
// to non-const, so constness is dropped here.
template <class T>
__device__ __forceinline__ std::remove_const_t<T>* uniform_ptr(T* p) {
  const uint64_t v = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return reinterpret_cast<std::remove_const_t<T>*>(((uint64_t)hi << 32) | lo);
}

// s_waitcnt vmcnt(N), other counters untouched (gfx9 encoding: vmcnt = imm[3:0] | imm[15:14] << 4, expcnt imm[6:4], lgkmcnt imm[11:8])
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}

// Wave-wide reductions (64 lanes, xor butterfly: every lane ends with the result, and the order of the additions is fixed)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// Wave-wide scans. Inclusive max scan (lane l ends with the maximum over lanes 0 .. l) and its mirror, the suffix minimum (lanes l .. 63).
__device__ __forceinline__ int wave_scan_max(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int n = __shfl_up(v, o);
    if (lane >= o) v = max(v, n);
  }
  return v;
}
__device__ __forceinline__ int wave_scan_min_down(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int n = __shfl_down(v, o);
    if (lane + o < 64) v = min(v, n);
  }
  return v;
}
// Exclusive count of a predicate: the lanes below this one for which it holds; total = the wave's count (one ballot, no shuffles).
// Every lane of the wave must call it.
__device__ __forceinline__ int wave_rank(bool p, int lane, int& total) {
  const unsigned long long mask = __ballot(p);
  total = __popcll(mask);
  return __popcll(mask & ((1ull << lane) - 1ull));
}

// LDS-DMA of 64 x 16 bytes: lane i's 16 bytes land at lds_dst + 16 i (wave-uniform destination, per-lane source offset).
// (A __device__ helper on purpose: with the builtin written directly inside the templated __global__ body, the host pass of hipcc
//  (ROCm 7.2) silently drops the kernel's launch stub and the library no longer links.)
template <int AUX = 0>   // cache-policy bits (0 in the product; 16 = sc1: reads past this CU's L1, for operands another workgroup published write-through)
__device__ __forceinline__ void glds16(__amdgpu_buffer_rsrc_t rsrc, void* lds_dst, int voffset, int soffset) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds_dst, 16, voffset, soffset, 0, AUX);
}

// f(integral_constant<int, 0>{}), f(integral_constant<int, 1>{}), ...: a K loop whose step index is a compile-time constant
template <class F, int... I>
__device__ __forceinline__ void unrolled_steps(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}

// LDS image of a staged fp32 operand tile: row r holds 32 consecutive K values = 8 slots of 16 B. Slot s of row r lives
// at physical slot s ^ ((r >> 1) & 7). With 128-B rows the 64 banks (256 B) hold two rows, so a ds_read_b128 lane
// group (rows {0-3,12-15,20-27} of one 16-B column, MI355X_MICROARCH.md §LDS) conflicts iff two rows agree in
// parity and in (r>>1)&7, i.e. are congruent mod 16 - none are. ds_write_b128 (8 contiguous lanes = the 8 slots of
// one row) is conflict-free too. Dropping the +4 padding cuts a 64x128 tile to 48 KiB -> 3 blocks per CU.
// Returns the float index of the slot.
__device__ __forceinline__ int lds_slot(int row, int slot) { return row * 32 + ((slot ^ ((row >> 1) & 7)) << 2); }

// 16-byte slot swizzle of a [rows][32] fp32 tile read by the 16x16 MFMA kernels. Reads: lane (r = l & 15, kg = l >> 4) takes slots
// 2kg, 2kg+1 of row r; with the ds_read_b128 lane groups of gfx950 ({0-3,12-15,20-27}, ...) this map is conflict-free (simulated,
// tools/lds_sim.py; SQ_LDS_BANK_CONFLICT = 0).
__device__ __forceinline__ int swz16(int row) { return ((row >> 1) & 7) ^ ((((row >> 2) ^ (row >> 3)) & 1) << 1); }

// 64-byte LDS rows (32 bf16) of the bf16x3 kernels: 16-byte slot s of row r lives at r * 64 + ((s ^ swz64(r)) << 4), conflict-free for
// the same lane groups (per residue of r mod 4 the four lanes of a group hit slots 0, 1, 2, 3).
__device__ __forceinline__ int swz64(int row) { return (row & 8) ? 3 : 0; }

// Winograd F(4,3) at dilation d (a power of two): quads are formed inside groups of 4 d frames, quad q covers the frames t, t + d,
// t + 2d, t + 3d with t = wino43_frame(q, d). For q = 0 mod 4 and r < 4: frame of quad q + r = frame of q + wino43_frame(r, d).
__device__ __forceinline__ int wino43_frame(int q, int d) { return q + 3 * (q & ~(d - 1)); }

// elementwise helpers on float4 / float2 (the two staging slot widths of the F(4,3) input transform)
__device__ __forceinline__ float4 vfma(float c, const float4& r, const float4& v) {
  return make_float4(fmaf(c, r.x, v.x), fmaf(c, r.y, v.y), fmaf(c, r.z, v.z), fmaf(c, r.w, v.w));
}
__device__ __forceinline__ float2 vfma(float c, const float2& r, const float2& v) { return make_float2(fmaf(c, r.x, v.x), fmaf(c, r.y, v.y)); }
__device__ __forceinline__ float4 vadd(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float2 vadd(const float2& a, const float2& b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float4 vsub(const float4& a, const float4& b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float2 vsub(const float2& a, const float2& b) { return make_float2(a.x - b.x, a.y - b.y); }

// float <-> bf16 bits: round to nearest even (v_cvt_pk_bf16_f32), like torch's .bfloat16()
__device__ __forceinline__ uint16_t f2bf(float x) { return __builtin_bit_cast(uint16_t, (__bf16)x); }
__device__ __forceinline__ float bf2f(uint16_t h) { return __builtin_bit_cast(float, (uint32_t)h << 16); }

// two fp32 values -> their three bf16 terms (x = hi + mid + lo, round-to-nearest each), packed pairwise (low half = first value)
__device__ __forceinline__ void split3(float x, float y, uint32_t& hi, uint32_t& mid, uint32_t& lo) {
  auto pk = [](float p, float q) {
    const f32x2 v = {p, q};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
  };
  hi = pk(x, y);
  const float rx = x - __builtin_bit_cast(float, hi << 16), ry = y - __builtin_bit_cast(float, hi & 0xffff0000u);
  mid = pk(rx, ry);
  lo = pk(rx - __builtin_bit_cast(float, mid << 16), ry - __builtin_bit_cast(float, mid & 0xffff0000u));
}

}  // namespace ss_dev
