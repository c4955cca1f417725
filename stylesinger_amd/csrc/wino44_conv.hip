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
// Components are consumed in the order c5, c6, c0, c1, c2, c3, c4 and built in three sets, each written to LDS at once: {c5, c6, c0}
// (the only read of r0 and r6), {c1, c2}, {c3, c4} (the last read of the rows). No term is kept in registers between components, so a
// thread holds the raw rows alone: 7 x 4 floats per 16-byte pass.
//
// Tile, zero padding and epilogue are those of wino43_conv.hip: 64 quads (256 frames) x 64 output channels (x 32 where C is no multiple
// of 64: the C = 32 stage), 4 (2) waves x 7 accumulators of 32 x 32.
//
// One transformed tile serves all tap groups. frame_of_quad(q + g d) = frame_of_quad(q) + 4 d g, so group g of quad q reads exactly the
// frames group 0 reads for quad q + g d and V(group g, quad q) = V(group 0, quad q + g d) bit for bit. The K loop therefore runs
// K chunk (outer) -> component -> tap group (inner): per K chunk and component ONE A tile of 64 + (G - 1) d quad rows (the 64 quads of
// the workgroup + a halo of at most 10) is built with the group-0 row offsets, and group g reads its fragments from the tile rows g d
// further (the slot swizzle follows the row actually read) and multiplies by the weights of (group g, component), staged per
// sub-position and double buffered as before. A K chunk has 7 G sub-positions, one barrier each. The A tiles are four LDS tiles with a
// fixed component -> tile map (SLOT), so a set of components can be written while another component is read; 40 KB + the B double buffer
// = 56 KB (64 columns: two workgroups per CU) / 48 KB. Against one tile per (group, component): the row fetches, the input leaky-relu,
// the transform and the A stores happen once per K chunk, not G times, for (G - 1) d / 64 more rows. Counted in the ISA between the first
// and the last MFMA (d = 3; before -> after): VALU per 32x32x2 MFMA 2.38 -> 0.92 (k = 7) / 0.85 (k = 11) with the input leaky-relu and
// 1.69 -> 0.73 / 0.56 without on the 64-column tile, 4.34 -> 1.54 / 1.69 and 3.39 -> 1.17 / 1.16 on the 32-column tile (v_accvgpr moves:
// about 1 -> 0 / 0.13 - 0.25 per MFMA); buffer loads per 16 MFMAs 12 -> 3.4 / 3.0 (64 columns), 4.4 / 3.7 (32 columns); 236 - 248 VGPRs,
// no AGPRs, no scratch, two waves per SIMD on the 64-column tile; no scratch and one wave per SIMD on the 32-column tile.
// Measured per launch at the C2 shapes (8 items, d = 3, input leaky-relu; DESIGN.md 3.5, profiles/r09_wino_shared_resblock_kernel_times.json):
// 0.88 - 0.93 of the time of the loop that built a tile per group, at every C and both k (33.7 -> 29.4 ms for the 48 launches of a
// pass). The earlier reading "the launch times follow the product count, so the transform is hidden" did not hold: the fetches and
// barriers scaled with the product count too. The halo reads only frames the tile-per-group loop read as well, through the same per-item
// buffer range, so the 32-bit offset guard of ss_wino44_conv is unchanged (tests/test_wino_shared_tile_cpu.py).
//
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
constexpr int AR = 80;   // rows of an A tile in LDS: the 64 quads + the halo of (G - 1) d <= 10 quads the later tap groups read
constexpr int NA = 4;    // A tiles in LDS
// Position p of a K chunk (component ORD[p]) lives in A tile SLOT[p]. Positions 0..2 are written while position 6 of the chunk before is
// read (tile 3), positions 3, 4 while position 2 is read (tiles 0, 1 are done), positions 5, 6 while position 4 is read (tiles 2 and 3
// are done): no tile is written while it is read or before it has been read, and the assignment is the same in every chunk.
constexpr int SLOT[7] = {0, 1, 2, 0, 1, 2, 3};

// The value stays in its register, but the compiler may not carry anything derived from it across this point: the offsets of the raw rows
// of a pass (row r = row 0 + r d lda, one VALU each, once per K chunk) are formed where they are used, not hoisted out of the K loop
// into 7 registers per pass that the row staging needs. (The fragment addresses ARE hoisted: forming them per sub-position cost 0.75
// VALU per MFMA and measured 3 - 5 % slower.)
__device__ __forceinline__ int formed_here(int x) {
  asm volatile("" : "+v"(x));
  return x;
}

template <int D>
__device__ __forceinline__ int frame_of_quad(int q) {
  if constexpr (D == 1) return 4 * q;
  else return (q / D) * (4 * D) + (q % D);
}

// BN = column-tile width, as in wino43_conv.hip. 64: four waves as 2 x 2 wave tiles of 32 quads x 32 columns (256 threads, two workgroups
// per CU); the quad rows are staged in two passes of 16-byte slots (8 threads per row) and the halo rows in one pass of 8-byte half slots
// (16 rows x 16 threads). 32: two waves stacked over the 64 quads, one column block (128 threads, one wave per SIMD with the accumulators in
// AGPRs); four passes of 16 rows for the quad rows and a fifth for the halo. G = tap groups (2: k = 7, 3: k = 11).
template <int D, bool LRELU, int BN, int G>
__global__ __launch_bounds__(BN * 4, BN == 64 ? 2 : 1) void wino44_conv_kernel(const ss_conv_gemm_args a, int q_tiles_per_item, int q_tiles,
                                                                               int n_tiles, int lo_rows) {
  static_assert(BN == 64 || BN == 32, "column tile of 64 or 32");
  static_assert(G == 2 || G == 3, "two or three tap groups");
  constexpr int NT = BN * 4;        // threads
  constexpr int RP = NT / 8;        // tile rows staged per pass (8 threads x float4 cover a 32-wide K chunk)
  constexpr int MP = BQ / RP;       // staging passes over the 64 quad rows
  constexpr int BP = BN / RP;       // staging passes over the weight rows
  constexpr int H = (G - 1) * D;    // halo rows: group g reads the tile rows g D further
  constexpr bool HALF = BN == 64;   // halo staged in 8-byte half slots (16 rows x 16 threads) / as one more 16-byte pass (BN = 32: 16 rows)
  constexpr int AP = HALF ? MP : MP + 1;   // 16-byte passes
  static_assert(H <= 16 && BQ + 16 <= AR, "halo rows fit one pass and the tile");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                  // [NA][AR][LD]
  float* Bs = smem + NA * AR * LD;   // [2][BN][LD]

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
  const int ldw = G * NC * a.Kp;

  const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc(
      uniform_ptr(a.A + (int64_t)b * a.a_batch_stride), 0, __builtin_amdgcn_readfirstlane(len * a.lda * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_w =
      __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(a.W), 0, __builtin_amdgcn_readfirstlane(a.Np * ldw * 4), 0x00020000);

  const int st_c4 = tid & 7;
  const int st_row = tid >> 3;  // 0..RP-1; MP passes cover the 64 quad rows, BP passes the BN weight rows
  // roff[i] = byte offset of raw row 0 of tile row i, i.e. of quad q0 + i for tap group 0: frame t - lo; raw row r is r d frames further.
  // A negative offset is >= 2^31 as the unsigned offset the buffer check sees -> out of range -> 0, like every frame >= len. Tile rows
  // >= 64 + H are read by no group: their offset is 2^31, nothing is fetched for them.
  constexpr int NOROW = (int)0x80000000;
  int roff[AP];
#pragma unroll
  for (int i = 0; i < AP; ++i) {
    const int row = st_row + i * RP;
    roff[i] = row < BQ + H ? ((frame_of_quad<D>(q0 + row) - lo_rows) * a.lda + st_c4 * 4) * 4 : NOROW;
  }
  const int h_row = BQ + (tid >> 4), h_c2 = tid & 15;   // the half-slot pass: tile row and 8-byte column of this thread
  const int hoff = h_row < BQ + H ? ((frame_of_quad<D>(q0 + h_row) - lo_rows) * a.lda + h_c2 * 2) * 4 : NOROW;
  const int row_step = D * a.lda * 4;
  int w_voff[BP];
#pragma unroll
  for (int i = 0; i < BP; ++i) w_voff[i] = ((n0 + st_row + i * RP) * ldw + st_c4 * 4) * 4;

  using Yes = std::true_type;
  using No = std::false_type;
  u32x4 rr[AP][NR], rb[BP];
  u32x2 rh[NR];
  // rows 1..5 (ends = No) or 0, 6 (ends = Yes) of 16-byte pass i / of the half-slot pass; cb = byte offset of the K chunk inside a row
  // (wave-uniform -> SGPR soffset)
  auto load_rows = [&](int i, int cb, auto ends) {
    const int o = formed_here(roff[i]);
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if ((r == 0 || r == NR - 1) == decltype(ends)::value) rr[i][r] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, o + r * row_step, cb, 0);
  };
  auto load_half = [&](int cb, auto ends) {
    const int o = formed_here(hoff);
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if ((r == 0 || r == NR - 1) == decltype(ends)::value) rh[r] = __builtin_amdgcn_raw_buffer_load_b64(rsrc_a, o + r * row_step, cb, 0);
  };
  auto load_b = [&](int cb) {  // cb = byte offset of the weight chunk inside a packed row (wave-uniform)
#pragma unroll
    for (int i = 0; i < BP; ++i) rb[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, w_voff[i], cb, 0);
  };
  const float slope = a.a_lrelu;
  auto act_rows = [&](int i) {
    if constexpr (LRELU) {
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
  auto act_half = [&]() {
    if constexpr (LRELU) {
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const f32x2 v = __builtin_bit_cast(f32x2, rh[r]);
        const f32x2 sv = v * slope;
        f32x2 o;
        o.x = ss_lrelu_max(v.x, sv.x);
        o.y = ss_lrelu_max(v.y, sv.y);
        rh[r] = __builtin_bit_cast(u32x2, o);
      }
    }
  };
  int a_wr[AP];
#pragma unroll
  for (int i = 0; i < AP; ++i) a_wr[i] = lds_slot(st_row + i * RP, st_c4);
  const int h_wr = lds_slot(h_row, h_c2 >> 1) + 2 * (h_c2 & 1);
  // The components are built in three sets, each written at once into LDS buffers of its own (SLOT), so no term is kept in registers
  // between positions: set 0 = c5, c6, c0 (the only read of r0 and r6), set 1 = c1, c2, set 2 = c3, c4 (the last read of the raw rows).
  // The same operations on a 16-byte slot (float4) and on a half slot (float2). Ad = buffer 0, w = this thread's slot in a buffer.
  auto build = [&](auto settag, auto R, float* Ad, int w) {
    constexpr int SET = decltype(settag)::value;
    using V = decltype(R(0));
    auto put = [&](int pos, const V& v) { *reinterpret_cast<V*>(Ad + SLOT[pos] * AR * LD + w) = v; };
    if constexpr (SET == 0) {
      const V c5 = vfma(4.f, R(1), vfma(-5.f, R(3), R(5)));
      const V F0 = vfma(4.f, R(0), vfma(-5.f, R(2), R(4)));
      const V E2 = vfma(4.f, R(2), vfma(-5.f, R(4), R(6)));
      put(0, c5);
      put(1, vfma(-0.5f, c5, E2));
      put(2, vfma(-0.5f, F0, c5));
    } else if constexpr (SET == 1) {
      const V Pv = vfma(2.f, R(1), vfma(-4.f, R(2), vfma(-0.5f, R(3), R(4))));
      const V Pu = vfma(2.f, R(2), vfma(-4.f, R(3), vfma(-0.5f, R(4), R(5))));
      put(3, vadd(Pu, Pv));
      put(4, vsub(Pu, Pv));
    } else {
      const V Qv = vfma(0.5f, R(1), vfma(-0.5f, R(3), vsub(R(4), R(2))));
      const V Qu = vfma(0.5f, R(2), vfma(-0.5f, R(4), vsub(R(5), R(3))));
      put(5, vfma(2.f, Qv, Qu));
      put(6, vfma(-2.f, Qv, Qu));
    }
  };
  auto store_a = [&](int i, auto settag) {
    build(settag, [&](int q) { return __builtin_bit_cast(float4, rr[i][q]); }, As, a_wr[i]);
  };
  auto store_half = [&](auto settag) {
    build(settag, [&](int q) { return __builtin_bit_cast(float2, rh[q]); }, As, h_wr);
  };
  auto store_b = [&](float* Bd) {
#pragma unroll
    for (int i = 0; i < BP; ++i)
      *reinterpret_cast<float4*>(Bd + lds_slot(st_row + i * RP, st_c4)) = __builtin_bit_cast(float4, rb[i]);
  };
  // the A work of one component is spread over the G sub-positions that run while it is built: the first half of the quad-row passes
  // with group 0, the second half with group 1, the halo with the last group. Raw rows: rows 1..5 of a pass are fetched behind the build
  // of the last set (P = 4), their last read; rows 0 and 6, which only the first set reads, one sub-position before that build.
  constexpr int HALO_G = G - 1;
  auto pass_group = [](int i) constexpr { return i >= MP ? HALO_G : i / (MP / 2); };
  auto fetch_mid_at = [](int pg) constexpr { return 4 * G + pg; };
  auto fetch_ends_at = [](int pg) constexpr { return 6 * G + pg - 1; };

  f32x16 acc[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  constexpr int ORD[NC] = {5, 6, 0, 1, 2, 3, 4};
  const int kb = a.Kp * 4;   // bytes of one component in a packed weight row
  const int cs = BK * 4;     // bytes of one K chunk
  // sub-position (k, p, g) = one 32-channel chunk x one component x one tap group; it uses the weights at (g * 7 + ORD[p]) * kb + k * cs
  constexpr int NS = NC * G;   // sub-positions of a K chunk

  // LDS byte offset of slot lh of this lane's fragment row: the A row of group g is g D rows further, and the slot swizzle follows the row
  // actually read; slot 2 q + lh = slot lh ^ 2 q, and rows start on 128 bytes, so ^ 32 q moves by 2 q slots inside the row
  auto slot0 = [&](int row) { return (row * LD + ((lh ^ ((row >> 1) & 7)) << 2)) * 4; };
  int a_s0[G];
#pragma unroll
  for (int g = 0; g < G; ++g) a_s0[g] = slot0(wm * 32 + l31 + g * D);
  const int b_s0 = slot0(wn * 32 + l31);
  auto mfma4 = [&](f32x16& c, const float4& af, const float4& bf) {
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, bf.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, bf.y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, bf.z, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, bf.w, c, 0, 0, 0);
  };
  // Sub-position S = P G + GI of K chunk k (parity E): MFMAs from A tile SLOT[P], rows shifted by GI D, and B buffer (E G + S) & 1
  // into acc[ORD[P]]. In their shadow, at P = 2, 4 and 6, this group's share of the passes builds a set of components (at P = 6 the first
  // set of chunk k + 1), and the weight registers (sub-position S + 1) go to the other B buffer; then the weights of S + 2 are
  // fetched into the same registers and, from P = 4 on, raw rows of chunk k + 1 (fetch_mid_at, fetch_ends_at). more = there is a
  // chunk k + 1 (wave-uniform): the last chunk fetches nothing and builds nothing past its position 6.
  auto sub = [&](auto etag, auto stag, int k, bool more) {
    constexpr int E = decltype(etag)::value, S = decltype(stag)::value;
    constexpr int P = S / G, GI = S % G;
    constexpr int BCUR = (E * G + S) & 1;
    constexpr int SET = P == 6 ? 0 : P == 2 ? 1 : P == 4 ? 2 : -1;   // the set of components built in the shadow of this position
    const float* Ac = As + SLOT[P] * AR * LD;
    const float* Bc = Bs + BCUR * BN * LD;
    const int a_s = a_s0[GI], b_s = b_s0;
    auto read_frags = [&](int q, float4& af, float4& bf) {
      af = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(Ac) + (a_s ^ (32 * q)));
      bf = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(Bc) + (b_s ^ (32 * q)));
    };
    float4 af0, af1, bf0, bf1;
    read_frags(0, af0, bf0);
    read_frags(1, af1, bf1);
    __builtin_amdgcn_sched_barrier(0);
    mfma4(acc[ORD[P]], af0, bf0);
    read_frags(2, af0, bf0);
    __builtin_amdgcn_sched_barrier(0);
    mfma4(acc[ORD[P]], af1, bf1);
    read_frags(3, af1, bf1);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (SET >= 0) {
      if (SET != 0 || more) {
        using Set = std::integral_constant<int, SET>;
#pragma unroll
        for (int i = 0; i < AP; ++i)
          if (pass_group(i) == GI) {
            if constexpr (SET == 0) act_rows(i);   // first use of the next chunk's raw rows
            store_a(i, Set{});
          }
        if constexpr (HALF && HALO_G == GI) {
          if constexpr (SET == 0) act_half();
          store_half(Set{});
        }
      }
    }
    if (S + 1 < NS || more) store_b(Bs + (BCUR ^ 1) * BN * LD);
    __builtin_amdgcn_sched_barrier(0);  // stores first, then the fetches into the SAME registers
    {
      constexpr int S2 = (S + 2) % NS;
      constexpr int wo = (S2 % G) * NC + ORD[S2 / G];
      if constexpr (S + 2 < NS) load_b(__builtin_amdgcn_readfirstlane(wo * kb + k * cs));
      else if (more) load_b(__builtin_amdgcn_readfirstlane(wo * kb + (k + 1) * cs));
    }
    if constexpr (P >= 4) {
      if (more) {
        const int cb = __builtin_amdgcn_readfirstlane((k + 1) * cs);
#pragma unroll
        for (int i = 0; i < AP; ++i) {
          if (fetch_mid_at(pass_group(i)) == S) load_rows(i, cb, No{});
          if (fetch_ends_at(pass_group(i)) == S) load_rows(i, cb, Yes{});
        }
        if constexpr (HALF && fetch_mid_at(HALO_G) == S) load_half(cb, No{});
        if constexpr (HALF && fetch_ends_at(HALO_G) == S) load_half(cb, Yes{});
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    mfma4(acc[ORD[P]], af0, bf0);
    mfma4(acc[ORD[P]], af1, bf1);
    __syncthreads();
  };
  using Set0 = std::integral_constant<int, 0>;
  using E0 = std::integral_constant<int, 0>;
  using E1 = std::integral_constant<int, 1>;

#pragma unroll
  for (int i = 0; i < AP; ++i) {
    load_rows(i, 0, No{});
    load_rows(i, 0, Yes{});
  }
  if constexpr (HALF) {
    load_half(0, No{});
    load_half(0, Yes{});
  }
  load_b(ORD[0] * kb);
#pragma unroll
  for (int i = 0; i < AP; ++i) {
    act_rows(i);
    store_a(i, Set0{});
  }
  if constexpr (HALF) {
    act_half();
    store_half(Set0{});
  }
  store_b(Bs);
  load_b(__builtin_amdgcn_readfirstlane((NC + ORD[0]) * kb));   // weights of sub-position 1 (group 1 of component c5): in flight across the barrier
  __syncthreads();

  // a K chunk has 7 G sub-positions: with G = 3 the B double buffer changes parity from chunk to chunk and the loop is unrolled over
  // chunk pairs
  auto chunk = [&](auto etag, int k, bool more) {
    unrolled_steps([&](auto stag) { sub(etag, stag, k, more); }, std::make_integer_sequence<int, NS>{});
  };
  if constexpr (G == 2) {
    for (int k = 0; k < kchunks; ++k) chunk(E0{}, k, k + 1 < kchunks);
  } else {
    for (int k = 0; k < kchunks; k += 2) {
      chunk(E0{}, k, k + 1 < kchunks);
      if (BN == 64 || k + 1 < kchunks) chunk(E1{}, k + 1, k + 2 < kchunks);   // Kp % 64 == 0: an even number of chunks
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

template <int D, int BN, int G>
void launch_conv(const ss_conv_gemm_args& a, hipStream_t stream) {
  const int quads_per_item = ss_cdiv(a.T, 4 * D) * D;
  const int q_tiles_per_item = ss_cdiv(quads_per_item, BQ);
  const int q_tiles = q_tiles_per_item * a.B;
  const int n_tiles = a.Np / BN;
  const int grid = ss_cdiv(q_tiles, 8) * 8 * n_tiles;
  const size_t lds = (size_t)(NA * AR + 2 * BN) * LD * sizeof(float);   // 56 KB (BN = 64: two workgroups per CU) / 48 KB (BN = 32)
  const int lo = (4 * G - 2) / 2 * D;   // (k - 1) / 2 frames in front of the output frame: k = 4 G - 1
  auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(BN * 4), lds, stream, a, q_tiles_per_item, q_tiles, n_tiles, lo); };
  if (a.a_lrelu != 1.0f) go(wino44_conv_kernel<D, true, BN, G>);
  else go(wino44_conv_kernel<D, false, BN, G>);
}

template <int D>
void launch_conv(const ss_conv_gemm_args& a, int k, hipStream_t stream) {
  const bool wide = a.Np % 64 == 0;
  if (k == 7) wide ? launch_conv<D, 64, 2>(a, stream) : launch_conv<D, 32, 2>(a, stream);
  else wide ? launch_conv<D, 64, 3>(a, stream) : launch_conv<D, 32, 3>(a, stream);
}

}  // namespace

// Which square convs run as F(4,4) groups. k: only where 7 ceil(k/4) < 6 ceil(k/3), i.e. 7 and 11 (k = 3, 5, 9 execute no fewer products
// than the F(4,3) groups). C: multiples of 32; multiples of 64 run the 64-column tile, the others - the C = 32 stage - the 32-column tile.
// The C = 32 stage IS in the rule: measured at its C2 shape (8 x 384 000 rows) the 32-column tile takes 0.90 - 0.91 (k = 7) and
// 0.97 - 0.98 (k = 11) of the time of ss_wino43_conv's; that stage is close to its memory limit and gains less than the
// 0.77 - 0.84 (k = 7) and 0.88 - 0.92 (k = 11) of the 64-column tile, but no shape lost. (Measured with one transformed tile per tap
// group; sharing the tile between the groups took a further 0.86 - 0.92 at every stage, the C = 32 stage included.)
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
