// Kernel text shared by gate128_kernel (gemm_bf16_gate128.hip) and gate128q_kernel (gemm_bf16_gate128q.hip), #included INSIDE each kernel body
// right after its clock probe: the LDS plan, the XCD-aware tile walk, the lane roles, the operand descriptors, the A / addend DMA pieces, the
// weight pieces' per-lane offset and the fragment addresses. Each kernel then adds its own weight pieces (piece_b), its step and, in gate128q,
// the fp4 registers; gate128_epilogue.h closes it.
// A text fragment and not a struct or a function on purpose: either form changes the compiled kernels (vector address arithmetic is selected
// differently once the code lives in a function of its own, as DESIGN.md section 3 records for the Winograd tile code), and these kernels must
// stay instruction for instruction what was measured. Expects in scope: a, m_tiles_per_item, m_tiles, n_tiles, d; namespaces ss_dev and g128.
  extern __shared__ __attribute__((aligned(16))) char smem_g128x[];   // 80 KB: two workgroups per CU
  // [A0 20 K][B0 16 K][A1 20 K][B1 16 K]: the operands of the LAST step live in A1 / B1, so the first 36 KB are free while it runs
  char* const A0 = smem_g128x;
  char* const B0 = A0 + AROWS * A_ROWB;
  char* const A1 = B0 + BN * B_ROWB;
  char* const B1 = A1 + AROWS * A_ROWB;
  // epilogue view: two 32-KB addend quarters and a 16-KB output staging tile
  char* const EQ0 = smem_g128x;
  char* const EQ1 = smem_g128x + 32 * 1024;
  char* const OUT = smem_g128x + 64 * 1024;

  // consecutive workgroups walk row tiles of the SAME column tile (ids = mod 8 -> one XCD): the weight slice stays in that XCD's L2
  const int id = blockIdx.x;
  const int grp = id / (8 * n_tiles);
  const int rem = id % (8 * n_tiles);
  const int mt = grp * 8 + (rem & 7);
  const int nt = rem >> 3;
  if (mt >= m_tiles) return;
  const int b = mt / m_tiles_per_item;
  const int t0 = (mt % m_tiles_per_item) * BM;
  const int n0 = nt * BN;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, lh = lane >> 5;
  const int len = ss_uniform_len(a.lens, b, a.T);
  const int grp_w = a.group_size > 0 ? b / a.group_size : 0;
  const int ldw = 3 * a.K * 2;   // 16-bit terms per packed weight row: 3 taps, both planes

  const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc(
      uniform_ptr(a.A + (int64_t)b * a.a_batch_stride), 0, __builtin_amdgcn_readfirstlane(len * a.lda * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(
      uniform_ptr(a.W + (int64_t)grp_w * a.w_group_stride), 0, __builtin_amdgcn_readfirstlane(a.Np * ldw * 2), 0x00020000);

  // ---- DMA roles (gate128_layout.h). A: wave w issues pieces w + 4 j (j < 5): piece w + 4 j starts 64 j rows after piece w and the swizzle
  // (row >> 2) & 3 does not depend on j: ONE per-lane offset. Only the hi plane (first 64 bytes of a chunk's 128-byte line) is fetched.
  // Rows before the item (negative offset = >= 2^31 unsigned) and rows >= len are out of range: the DMA writes zeros (the conv's padding).
  const int a_voff = ((t0 - HALO + a_dma_row(wave, lane)) * a.lda + a_dma_slot(wave, lane) * 8) * 2;
  const int a_tail_dead = wave < 1 ? 0 : (int)0x80000000;   // piece w + 16 = LDS rows 256 + 16 w ..: only rows < BM + 2 HALO = 272 are ever read
  auto piece_a = [&](char* buf, int cc, int j) {
    // the row offset of piece j goes into the VGPR offset (one add): for rows before the item the per-lane offset is negative and the
    // hardware adds the SGPR offset without wrapping - a positive SGPR part would leave valid rows of later pieces out of range
    glds16(rsrc_a, buf + (wave + 4 * j) * 1024, (a_voff + 64 * j * a.lda * 2) | (j == 4 ? a_tail_dead : 0), cc * 128);
  };
  const int b_voff = ((n0 + b_dma_row(wave, lane)) * ldw + b_dma_slot(wave, lane) * 8) * 2;   // weight pieces: wave w issues w + 4 j (j < 4), 32 j rows further, same swizzle

  // ---- fragment addresses: (row base, swizzle ^ lh) per tap, one XOR per read; 32 m more rows leave the swizzle unchanged
  frags<4, A_ROWB> a_frags[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int row = a_frag_row(wm, 0, l31, (j - 1) * d);
    a_frags[j] = {row * A_ROWB, a_swz(row) ^ lh};
  }
  const int b_row = b_frag_row(wn, 0, l31);
  const frags<2, B_ROWB> b_frags{b_row * B_ROWB, b_swz(b_row) ^ lh};

  // conditioner addend: fp32 [rows][lde]; the tile's 128 packed columns are 512 B contiguous per row -> two rows per DMA instruction
  const float* Eb = a.E ? a.E + (int64_t)b * a.e_batch_stride : nullptr;
  const __amdgpu_buffer_rsrc_t rsrc_e = __builtin_amdgcn_make_buffer_rsrc(
      uniform_ptr(Eb ? (const void*)Eb : (const void*)a.W), 0, __builtin_amdgcn_readfirstlane(Eb ? (int)((int64_t)a.T * a.lde * 4) : 0), 0x00020000);
  // piece w + 4 j of quarter q: tile rows e_dma_tile_row(w + 4 j, lane, q) = [2 w + (lane >> 5)] + 32 q + (j < 4 ? 8 j : 128 + 8 (j - 4))
  const int e_voff = ((t0 + 2 * wave + (lane >> 5)) * a.lde + n0) * 4 + e_dma_col_byte(lane);
  auto piece_e = [&](char* buf, int q, int j) {
    glds16(rsrc_e, buf + (wave + 4 * j) * 1024, e_voff, (q * 32 + (j < 4 ? 8 * j : 128 + 8 * (j - 4))) * a.lde * 4);
  };
  auto dma_e = [&](char* buf, int q) {
#pragma unroll
    for (int j = 0; j < 8; ++j) piece_e(buf, q, j);
  };
