// Grouped Winograd F(4,4) form of the HiFi-GAN ResBlock convs with k = 7 / 11 taps (hifigan.py ResBlock1; dilation 1 / 3 / 5, C -> C
// channels, leaky-relu in front, bias + residual behind), exact-fp32 MFMA. The sibling of wino43_conv.hip, which keeps k = 3, the
// rectangular convs and the GELU epilogue.
//
// A k-tap conv is split into G = ceil(k / 4) groups of four taps (the last group zero padded at its end). Group g reads the frames
// t + s_g + i d (s_g = (4 g - (k - 1) / 2) d, i = 0..6) of a quad of output frames (t, t + d, t + 2d, t + 3d) and contributes seven
// products m_j += c_j(g) . G_j(g) of the F(4,4) transforms on the points {0, 1, -1, 2, -2, 1/2, inf}; the seven accumulators run over all
// groups and all input channels, ONE output transform at the end, all of its factors powers of two:
//   z[t]    = m0 + m1 + m2 + m3 + m4 + m5           z[t+d]  = (m1 - m2) + 2 (m3 - m4) + m5 / 2
//   z[t+2d] = (m1 + m2) + 4 (m3 + m4) + m5 / 4      z[t+3d] = (m1 - m2) + 8 (m3 - m4) + m5 / 8 + m6
// 7 G matrix products per 4 output frames: k = 7: 14 (F(4,3) groups: 18), k = 11: 21 (24); k = 3 would be 7 against 6 and k = 5, 9 gain
// nothing either, which is the rule of ss_wino44_conv_ok. Weights: lib.wino44_group_weight (the 7 x 4 filter matrix in float64, rounded
// once) + ss_pack_conv_weight, i.e. packed rows of 7 G components of Kp floats.
//
// Input transform of a quad's seven raw rows r0..r6 (rows of B^T are the polynomials prod_{l != j} (x - p_l); 24 VALU per element):
//   Pv = 2 r1 - 4 r2 - r3 / 2 + r4    Pu = 2 r2 - 4 r3 - r4 / 2 + r5    c1 = Pu + Pv      c2 = Pu - Pv
//   Qv = r1 / 2 - r2 - r3 / 2 + r4    Qu = r2 / 2 - r3 - r4 / 2 + r5    c3 = Qu + 2 Qv    c4 = Qu - 2 Qv
//   c5 = 4 r1 - 5 r3 + r5    F0 = 4 r0 - 5 r2 + r4    E2 = 4 r2 - 5 r4 + r6    c0 = c5 - F0 / 2    c6 = E2 - c5 / 2
// Components are consumed in the order c5, c6, c0, c1, c2, c3, c4: c5, F0 and E2 are formed with the first build, after which r0 and r6 are
// dead, and all rows are dead after the sixth build (c3), so at most 64 row / term registers are live per thread of the 64-column tile
// (the order c1..c4 first, with the rows fetched three components ahead, spilled). The rows r1..r5 of the next step are fetched two
// components ahead, r0 and r6 one component ahead.
//
// Tile, staging, zero padding and epilogue are those of wino43_conv.hip: 64 quads (256 frames) x 64 output channels (x 32 where C is no
// multiple of 64: the C = 32 stage), 4 (2) waves x 7 accumulators of 32 x 32, K loop over (group, 32-channel chunk), one LDS tile +
// barrier per component; moving to the next tap group adds 4 d rows to the row offsets. A step has seven positions, so the LDS double
// buffer changes parity from step to step: the K loop is unrolled over step pairs (the 32-column tile also takes an odd step count).
// Every group still fetches and transforms its own rows. Group g + 1 of quad q reads the frames group g reads for quad q + d, so the
// transformed input could be built once per conv and K chunk for 64 + (G - 1) d rows, but that needs the raw frames (or all seven
// components of up to 74 rows) in LDS; the measured launch times follow the product count (0.78 - 0.84 of the F(4,3) time for
// 14 / 18 of the products at C >= 64), i.e. the transform is hidden behind the matrix pipe, and it is not done here.
// Zero-padding rule, the one of conv_gemm_kernel.h: the A operand of item b is a buffer of lens[b] * lda floats (lens[b] clamped to
// [0, T]; T without lens), so every tap that lands on a row < 0 or >= lens[b] reads 0 - with mask_rows = 0 too; mask_rows only decides
// whether OUTPUT rows >= lens[b] are written as 0 or as the conv of that zero-extended input. Rows >= T are never written.
#include "common.h"
#include "device_prims.h"
#include "../../include/stylesinger_hip.h"
#include <type_traits>

namespace {

using namespace ss_dev;

constexpr int BK = 32;
constexpr int LD = BK;
constexpr int BQ = 64;   // quads per tile (= 256 output frames)
constexpr int NC = 7;    // components of F(4,4)
constexpr int NR = 7;    // raw rows of a quad

template <int D>
__device__ __forceinline__ int frame_of_quad(int q) {
  if constexpr (D == 1) return 4 * q;
  else return (q / D) * (4 * D) + (q % D);
}

// BN = column-tile width, as in wino43_conv.hip. 64: four waves as 2 x 2 wave tiles of 32 quads x 32 columns (256 threads, two staging
// passes per operand, two workgroups per CU). 32: two waves stacked over the 64 quads, one column block (128 threads, four staging passes
// for the quad rows, two for the weights; one wave per SIMD with the accumulators in AGPRs).
template <int D, bool LRELU, int BN>
__global__ __launch_bounds__(BN * 4, BN == 64 ? 2 : 1) void wino44_conv_kernel(const ss_conv_gemm_args a, int q_tiles_per_item, int q_tiles,
                                                                               int n_tiles, int groups, int lo_rows) {
  static_assert(BN == 64 || BN == 32, "column tile of 64 or 32");
  constexpr int NT = BN * 4;        // threads
  constexpr int RP = NT / 8;        // tile rows staged per pass (8 threads x float4 cover a 32-wide K chunk)
  constexpr int AP = BQ / RP;       // staging passes over the quad rows
  constexpr int BP = BN / RP;       // staging passes over the weight rows
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                  // [2][BQ][LD]
  float* Bs = smem + 2 * BQ * LD;    // [2][BN][LD]

  // 8 consecutive workgroups share a column tile and walk 8 row tiles: the weight slice stays hot in the XCD's L2
  const int id = blockIdx.x;
  const int grp = id / (8 * n_tiles);
  const int rem = id % (8 * n_tiles);
  const int qt = grp * 8 + (rem & 7);
  const int nt = rem >> 3;
  if (qt >= q_tiles) return;
  const int b = __builtin_amdgcn_readfirstlane(qt / q_tiles_per_item);
  const int q0 = __builtin_amdgcn_readfirstlane((qt % q_tiles_per_item) * BQ);
  const int n0 = nt * BN;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = BN == 64 ? wave >> 1 : wave, wn = BN == 64 ? wave & 1 : 0;
  const int l31 = lane & 31, lh = lane >> 5;

  const int len = ss_uniform_len(a.lens, b, a.T);
  const int kchunks = a.Kp / BK;
  const int ldw = groups * NC * a.Kp;

  const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc(
      uniform_ptr(a.A + (int64_t)b * a.a_batch_stride), 0, __builtin_amdgcn_readfirstlane(len * a.lda * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_w =
      __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(a.W), 0, __builtin_amdgcn_readfirstlane(a.Np * ldw * 4), 0x00020000);

  const int st_c4 = tid & 7;
  const int st_row = tid >> 3;  // 0..RP-1; AP passes cover the 64 quad rows, BP passes the BN weight rows
  // roff[i] = byte offset of raw row 0 of quad row i for the CURRENT tap group: frame t - lo (+ 4 d per group); raw row r is r d frames
  // further. A negative offset is >= 2^31 as the unsigned offset the buffer check sees -> out of range -> 0, like every frame >= len.
  int roff[AP];
#pragma unroll
  for (int i = 0; i < AP; ++i) roff[i] = ((frame_of_quad<D>(q0 + st_row + i * RP) - lo_rows) * a.lda + st_c4 * 4) * 4;
  const int row_step = D * a.lda * 4;
  const int group_step = 4 * row_step;
  int w_voff[BP];
#pragma unroll
  for (int i = 0; i < BP; ++i) w_voff[i] = ((n0 + st_row + i * RP) * ldw + st_c4 * 4) * 4;

  using Yes = std::true_type;
  using No = std::false_type;
  u32x4 rr[AP][NR], rb[BP];
  auto load_rows = [&](int ci0b, auto ends) {  // ci0b = byte offset of the K chunk inside a row (wave-uniform -> SGPR soffset); rows 1..5 or 0, 6
    ci0b = __builtin_amdgcn_readfirstlane(ci0b);
#pragma unroll
    for (int i = 0; i < AP; ++i)
#pragma unroll
      for (int r = 0; r < NR; ++r)
        if ((r == 0 || r == NR - 1) == decltype(ends)::value) rr[i][r] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, roff[i] + r * row_step, ci0b, 0);
  };
  auto load_b = [&](int cb) {  // cb = byte offset of the weight chunk inside a packed row (wave-uniform)
    cb = __builtin_amdgcn_readfirstlane(cb);
#pragma unroll
    for (int i = 0; i < BP; ++i) rb[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, w_voff[i], cb, 0);
  };
  const float slope = a.a_lrelu;
  auto act_rows = [&]() {
    if constexpr (LRELU) {
#pragma unroll
      for (int i = 0; i < AP; ++i)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const f32x4 v = __builtin_bit_cast(f32x4, rr[i][r]);
          const f32x4 sv = v * slope;   // two v_pk_mul_f32
          f32x4 o;
          o.x = ss_lrelu_max(v.x, sv.x);
          o.y = ss_lrelu_max(v.y, sv.y);
          o.z = ss_lrelu_max(v.z, sv.z);
          o.w = ss_lrelu_max(v.w, sv.w);
          rr[i][r] = __builtin_bit_cast(u32x4, o);
        }
    }
  };
  int a_wr[AP];
#pragma unroll
  for (int i = 0; i < AP; ++i) a_wr[i] = lds_slot(st_row + i * RP, st_c4);
  // position p builds component ORD[p] (c5, c6, c0, c1, c2, c3, c4) from the raw rows / the kept terms of the header comment
  float4 tU[AP], tV[AP], tW[AP];
  auto store_a = [&](float* Ad, auto ptag) {
    constexpr int P = decltype(ptag)::value;
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      auto R = [&](int q) { return __builtin_bit_cast(float4, rr[i][q]); };
      float4 v;
      if constexpr (P == 0) {   // the only read of r0 and r6
        tU[i] = vfma(4.f, R(1), vfma(-5.f, R(3), R(5)));
        tV[i] = vfma(4.f, R(0), vfma(-5.f, R(2), R(4)));
        tW[i] = vfma(4.f, R(2), vfma(-5.f, R(4), R(6)));
        v = tU[i];
      } else if constexpr (P == 1) {
        v = vfma(-0.5f, tU[i], tW[i]);
      } else if constexpr (P == 2) {
        v = vfma(-0.5f, tV[i], tU[i]);
      } else if constexpr (P == 3) {
        tV[i] = vfma(2.f, R(1), vfma(-4.f, R(2), vfma(-0.5f, R(3), R(4))));
        tU[i] = vfma(2.f, R(2), vfma(-4.f, R(3), vfma(-0.5f, R(4), R(5))));
        v = vadd(tU[i], tV[i]);
      } else if constexpr (P == 4) {
        v = vsub(tU[i], tV[i]);
      } else if constexpr (P == 5) {   // the last read of the raw rows
        tV[i] = vfma(0.5f, R(1), vfma(-0.5f, R(3), vsub(R(4), R(2))));
        tU[i] = vfma(0.5f, R(2), vfma(-0.5f, R(4), vsub(R(5), R(3))));
        v = vfma(2.f, tV[i], tU[i]);
      } else {
        v = vfma(-2.f, tV[i], tU[i]);
      }
      *reinterpret_cast<float4*>(Ad + a_wr[i]) = v;
    }
  };
  auto store_b = [&](float* Bd) {
#pragma unroll
    for (int i = 0; i < BP; ++i)
      *reinterpret_cast<float4*>(Bd + lds_slot(st_row + i * RP, st_c4)) = __builtin_bit_cast(float4, rb[i]);
  };

  f32x16 acc[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  constexpr int ORD[NC] = {5, 6, 0, 1, 2, 3, 4};
  const int kb = a.Kp * 4;   // bytes of one component in a packed weight row
  const int cs = BK * 4;     // bytes of one K chunk
  // step (g, k) = one tap group x one 32-channel chunk; position p of it uses the weights at (g * 7 + ORD[p]) * kb + k * cs
  const int steps = groups * kchunks;

  const int swz = (l31 >> 1) & 7;
  const int a_row = (wm * 32 + l31) * LD;
  const int b_row = (wn * 32 + l31) * LD;
  auto read_frags = [&](const float* Ac, const float* Bc, int q, float4& af, float4& bf) {
    const int so = ((2 * q + lh) ^ swz) << 2;
    af = *reinterpret_cast<const float4*>(Ac + a_row + so);
    bf = *reinterpret_cast<const float4*>(Bc + b_row + so);
  };
  auto mfma4 = [&](f32x16& c, const float4& af, const float4& bf) {
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, bf.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, bf.y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, bf.z, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, bf.w, c, 0, 0, 0);
  };
  // position P of a step of parity E: MFMAs from LDS buffer (E + P) & 1 into acc[ORD[P]]; in their shadow the component of position P+1
  // (or position 0 of the next step) is built and stored with the weight registers, then the weights two positions ahead are fetched into
  // the same registers and - at position 4, the raw rows being dead, rows 1..5, at position 5 rows 0 and 6 - the raw rows of the next step.
  //   wb  = weight byte offset of the position two ahead;  rows_cb = K-chunk byte offset of the next step's rows
  auto chunk = [&](auto etag, auto ptag, auto stage_tag, auto fetch_b_tag, auto fetch_rows_tag, int wb, int rows_cb, bool new_group) {
    constexpr int P = decltype(ptag)::value;
    constexpr int CUR = (decltype(etag)::value + P) & 1;
    constexpr int PN = (P + 1) % NC;
    const float* Ac = As + CUR * BQ * LD;
    const float* Bc = Bs + CUR * BN * LD;
    float4 af0, af1, bf0, bf1;
    read_frags(Ac, Bc, 0, af0, bf0);
    read_frags(Ac, Bc, 1, af1, bf1);
    __builtin_amdgcn_sched_barrier(0);
    mfma4(acc[ORD[P]], af0, bf0);
    read_frags(Ac, Bc, 2, af0, bf0);
    __builtin_amdgcn_sched_barrier(0);
    mfma4(acc[ORD[P]], af1, bf1);
    read_frags(Ac, Bc, 3, af1, bf1);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (decltype(stage_tag)::value) {
      if constexpr (PN == 0) act_rows();   // first use of the next step's raw rows
      store_a(As + (CUR ^ 1) * BQ * LD, std::integral_constant<int, PN>{});
      store_b(Bs + (CUR ^ 1) * BN * LD);
    }
    __builtin_amdgcn_sched_barrier(0);  // stores first, then the fetches into the SAME registers
    if constexpr (decltype(fetch_b_tag)::value) load_b(wb);
    if constexpr (decltype(fetch_rows_tag)::value) {
      if constexpr (P == 4) {
        if (new_group) {   // wave-uniform: the next step starts the next tap group, 4 d frames further
#pragma unroll
          for (int i = 0; i < AP; ++i) roff[i] += group_step;
        }
        load_rows(rows_cb, No{});
      } else {
        load_rows(rows_cb, Yes{});
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    mfma4(acc[ORD[P]], af0, bf0);
    mfma4(acc[ORD[P]], af1, bf1);
    __syncthreads();
  };
  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;
  using P2 = std::integral_constant<int, 2>;
  using P3 = std::integral_constant<int, 3>;
  using P4 = std::integral_constant<int, 4>;
  using P5 = std::integral_constant<int, 5>;
  using P6 = std::integral_constant<int, 6>;

  int g = 0, k = 0;   // current step
  // one step that has a successor: all seven positions stage and fetch
  auto step = [&](auto etag) {
    const bool wrap = k + 1 == kchunks;
    const int gn = wrap ? g + 1 : g, kn = wrap ? 0 : k + 1;   // next step
    const int wcur = g * NC * kb + k * cs, wnext = gn * NC * kb + kn * cs;
    chunk(etag, P0{}, Yes{}, Yes{}, No{}, wcur + ORD[2] * kb, 0, false);
    chunk(etag, P1{}, Yes{}, Yes{}, No{}, wcur + ORD[3] * kb, 0, false);
    chunk(etag, P2{}, Yes{}, Yes{}, No{}, wcur + ORD[4] * kb, 0, false);
    chunk(etag, P3{}, Yes{}, Yes{}, No{}, wcur + ORD[5] * kb, 0, false);
    chunk(etag, P4{}, Yes{}, Yes{}, Yes{}, wcur + ORD[6] * kb, kn * cs, wrap);
    chunk(etag, P5{}, Yes{}, Yes{}, Yes{}, wnext + ORD[0] * kb, kn * cs, false);
    chunk(etag, P6{}, Yes{}, Yes{}, No{}, wnext + ORD[1] * kb, 0, false);
    g = gn;
    k = kn;
  };
  using E0 = std::integral_constant<int, 0>;
  using E1 = std::integral_constant<int, 1>;

  load_rows(0, No{});
  load_rows(0, Yes{});
  load_b(ORD[0] * kb);
  act_rows();
  store_a(As, P0{});
  store_b(Bs);
  load_b(ORD[1] * kb);   // weights of position 1: in flight across the barrier
  __syncthreads();

  // the last step: nothing left to fetch
  auto last_step = [&](auto etag) {
    const int wcur = g * NC * kb + k * cs;
    chunk(etag, P0{}, Yes{}, Yes{}, No{}, wcur + ORD[2] * kb, 0, false);
    chunk(etag, P1{}, Yes{}, Yes{}, No{}, wcur + ORD[3] * kb, 0, false);
    chunk(etag, P2{}, Yes{}, Yes{}, No{}, wcur + ORD[4] * kb, 0, false);
    chunk(etag, P3{}, Yes{}, Yes{}, No{}, wcur + ORD[5] * kb, 0, false);
    chunk(etag, P4{}, Yes{}, Yes{}, No{}, wcur + ORD[6] * kb, 0, false);
    chunk(etag, P5{}, Yes{}, No{}, No{}, 0, 0, false);
    chunk(etag, P6{}, No{}, No{}, No{}, 0, 0, false);
  };
  if constexpr (BN == 64) {   // Kp % 64 == 0: an even number of steps
    for (int s = 0; s + 2 < steps; s += 2) {
      step(E0{});
      step(E1{});
    }
    step(E0{});
    last_step(E1{});
  } else {
    int left = steps;
    for (; left > 2; left -= 2) {
      step(E0{});
      step(E1{});
    }
    if (left == 2) {
      step(E0{});
      last_step(E1{});
    } else {
      last_step(E0{});
    }
  }

  // ---- epilogue: output transform, then the STORE epilogue of ss_conv_gemm: v = act((z + bias) * pre_scale); v = (v + R) * post_scale
  // (+ C when accumulating); rows >= len are written as 0 (mask_rows), rows >= T dropped by the buffer range check.
  // accumulator row r of this lane -> quad (r & 3) + 8 (r >> 2) + 4 lh of the wave's 32 quads; column n0 + 32 wn + l31
  const int col = n0 + wn * 32 + l31;
  const bool col_ok = col < a.N;
  const int oob = col_ok ? 0 : (int)0x80000000;
  const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(
      uniform_ptr(a.C + (int64_t)b * a.c_batch_stride), 0, __builtin_amdgcn_readfirstlane((int)((int64_t)a.T * a.ldc * 4)), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_r = __builtin_amdgcn_make_buffer_rsrc(
      uniform_ptr(a.R ? const_cast<float*>(a.R) + (int64_t)b * a.r_batch_stride : a.C), 0,
      __builtin_amdgcn_readfirstlane(a.R ? (int)((int64_t)a.T * a.ldr * 4) : 0), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_p = __builtin_amdgcn_make_buffer_rsrc(   // previous value of C (accumulate), else an empty range -> 0
      uniform_ptr(a.C + (int64_t)b * a.c_batch_stride), 0, __builtin_amdgcn_readfirstlane(a.accumulate ? (int)((int64_t)a.T * a.ldc * 4) : 0),
      0x00020000);
  const float bs = (a.bias && col_ok) ? a.bias[col] : 0.f;
  const int row_lim = a.mask_rows ? (len < a.T ? len : a.T) : a.T;
  const int ldc4 = a.ldc * 4, ldr4 = a.ldr * 4;
  const int qbase = q0 + wm * 32 + 4 * lh;
  const bool lrelu_out = a.act == SS_ACT_LRELU_;
#pragma unroll
  for (int rb4 = 0; rb4 < 4; ++rb4) {   // four quads (16 output frames) at a time: all loads first, then compute + store
    float rv[4][4], pv[4][4];
    int tq[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      tq[e] = frame_of_quad<D>(qbase + e + 8 * rb4);
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const int t = tq[e] + o * D;
        rv[e][o] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc_r, t * ldr4 + (col * 4 + oob), 0, 0));
        pv[e][o] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc_p, t * ldc4 + (col * 4 + oob), 0, 0));
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = e + 4 * rb4;
      const float s12 = acc[1][r] + acc[2][r], d12 = acc[1][r] - acc[2][r];
      const float s34 = acc[3][r] + acc[4][r], d34 = acc[3][r] - acc[4][r];
      const float m5 = acc[5][r];
      float z[4];
      z[0] = (acc[0][r] + s12) + (s34 + m5);
      z[1] = fmaf(0.5f, m5, fmaf(2.0f, d34, d12));
      z[2] = fmaf(0.25f, m5, fmaf(4.0f, s34, s12));
      z[3] = fmaf(0.125f, m5, fmaf(8.0f, d34, d12)) + acc[6][r];
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const int t = tq[e] + o * D;
        float v = (z[o] + bs) * a.pre_scale;
        if (lrelu_out) v = ss_lrelu(v, a.act_slope);
        v = (v + rv[e][o]) * a.post_scale + pv[e][o];
        if (t >= row_lim) v = 0.f;
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsrc_c, t * ldc4 + (col * 4 + oob), 0, 0);
      }
    }
  }
}

template <int D, int BN>
void launch_conv(const ss_conv_gemm_args& a, int k, hipStream_t stream) {
  const int quads_per_item = ss_cdiv(a.T, 4 * D) * D;
  const int q_tiles_per_item = ss_cdiv(quads_per_item, BQ);
  const int q_tiles = q_tiles_per_item * a.B;
  const int n_tiles = a.Np / BN;
  const int grid = ss_cdiv(q_tiles, 8) * 8 * n_tiles;
  const size_t lds = (size_t)2 * (BQ + BN) * LD * sizeof(float);   // 32 KB (BN = 64) / 24 KB (BN = 32)
  const int groups = (k + 3) / 4, lo = (k - 1) / 2 * D;
  auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(BN * 4), lds, stream, a, q_tiles_per_item, q_tiles, n_tiles, groups, lo); };
  if (a.a_lrelu != 1.0f) go(wino44_conv_kernel<D, true, BN>);
  else go(wino44_conv_kernel<D, false, BN>);
}

template <int D>
void launch_conv(const ss_conv_gemm_args& a, int k, hipStream_t stream) {
  if (a.Np % 64 == 0) launch_conv<D, 64>(a, k, stream);
  else launch_conv<D, 32>(a, k, stream);
}

}  // namespace

// Which square convs run as F(4,4) groups. k: only where 7 ceil(k/4) < 6 ceil(k/3), i.e. 7 and 11 (k = 3, 5, 9 execute no fewer products
// than the F(4,3) groups). C: multiples of 32; multiples of 64 run the 64-column tile, the others - the C = 32 stage - the 32-column tile.
// The C = 32 stage IS in the rule: measured at its C2 shape (8 x 384 000 rows) the 32-column tile takes 0.90 - 0.91 (k = 7) and
// 0.97 - 0.98 (k = 11) of the time of ss_wino43_conv's; that stage is close to its memory limit and gains less than the
// 0.77 - 0.84 (k = 7) and 0.88 - 0.92 (k = 11) of the 64-column tile, but no shape lost.
extern "C" int ss_wino44_conv_ok(int C, int k, int dilation) {
  const bool fewer = k >= 1 && k <= 11 && (k & 1) && ((k + 3) / 4) * 7 < ((k + 2) / 3) * 6;
  return fewer && C > 0 && C % 32 == 0 && (dilation == 1 || dilation == 3 || dilation == 5) ? 1 : 0;
}

extern "C" int ss_wino44_conv(const ss_conv_gemm_args* args, int k, int dilation, void* stream) {
  SS_CHECK_ARG(args != nullptr, "ss_wino44_conv: null args");
  const ss_conv_gemm_args& a = *args;
  SS_CHECK_ARG(a.A && a.W && a.C, "ss_wino44_conv: null A/W/C");
  SS_CHECK_ARG(a.Cin == a.N && ss_wino44_conv_ok(a.Cin, k, dilation), "ss_wino44_conv: Cin=%d == N=%d (multiple of 32), k=%d (7|11), dilation=%d (1|3|5)",
               a.Cin, a.N, k, dilation);
  SS_CHECK_ARG(a.Kp == a.Cin && a.Np == a.N && (a.lda & 3) == 0 && a.lda >= a.Cin, "ss_wino44_conv: Kp == Cin, Np == N, lda a multiple of 4");
  SS_CHECK_ARG(a.epi == SS_EPI_STORE && (a.act == SS_ACT_NONE_ || a.act == SS_ACT_LRELU_) && !a.a_bias && a.a_scale == 1.0f && !a.mfma_bf16 &&
                   a.group_size == 0,
               "ss_wino44_conv: STORE epilogue, act none|lrelu, no input bias/scale, fp32, one weight set");
  SS_CHECK_ARG(a.a_lrelu > 0.0f && a.a_lrelu <= 1.0f, "ss_wino44_conv: input leaky-relu slope %g must be in (0, 1]", (double)a.a_lrelu);
  SS_CHECK_ARG(((int64_t)a.T + 1024) * a.lda * 4 < (1ll << 31) && (int64_t)a.T * a.ldc * 4 < (1ll << 31) &&
                   (!a.R || (int64_t)a.T * a.ldr * 4 < (1ll << 31)) && (int64_t)a.Np * ((k + 3) / 4) * NC * a.Kp * 4 < (1ll << 31),
               "ss_wino44_conv: item too large for 32-bit offsets");
  if (dilation == 1) launch_conv<1>(a, k, (hipStream_t)stream);
  else if (dilation == 3) launch_conv<3>(a, k, (hipStream_t)stream);
  else launch_conv<5>(a, k, (hipStream_t)stream);
  SS_CHECK_LAUNCH("ss_wino44_conv");
  return SS_OK;
}
