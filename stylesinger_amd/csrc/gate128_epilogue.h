// The gate epilogue of gate128_kernel and gate128q_kernel, #included INSIDE each kernel body after its K loop (see gate128_prologue.h for why
// this is a text fragment). Expects what gate128_prologue.h declares, and acc.
  // ---- epilogue (gate256_kernel's plan with this tile's constants): the fp32 addend tile (256 rows x 512 B) arrives by LDS-DMA in four quarters of
  // 64 rows, double buffered (quarter 0 was issued inside the last MFMA step into the 36 KB that step no longer uses); the fp16 gate outputs of
  // a quarter are staged in LDS and leave as 16-byte stores (the hi halves of the pair layout's 128-byte groups only).
  // Pass q handles accumulator block m = q of every wave: tile rows 128 wm + 32 q + (0..31), LDS row k = 32 wm + (0..31).
  const float* biasg = a.bias ? a.bias + (int64_t)grp_w * a.bias_group_stride : nullptr;
  const int pcl = 64 * wn + l31;                 // packed column inside the tile (first operand; the second sits 32 further)
  const int ocl = 32 * wn + l31;                 // output channel inside the tile
  const bool ch_ok = (n0 >> 1) + ocl < a.N;
  const float b0 = (biasg && ch_ok) ? biasg[n0 + pcl] : 0.f, b1 = (biasg && ch_ok) ? biasg[n0 + pcl + 32] : 0.f;
  const gate_act gate(a.gate_mode);
  const int row_lim = a.mask_rows ? (len < a.T ? len : a.T) : a.T;
  const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(
      uniform_ptr((uint16_t*)a.C + (int64_t)b * a.c_batch_stride), 0, __builtin_amdgcn_readfirstlane((int)((int64_t)a.T * a.ldc * 2)), 0x00020000);
  __builtin_amdgcn_s_barrier();   // everyone is done with A1 / B1: the second quarter and the staging tile may overwrite them
  dma_e(EQ1, 1);
  const int e_rd = e_read_lds(wm, wn, l31, lh, 0, 0);        // + rr * E_ROWB (+ 128 for the second operand)
  const int o_wr = out_write_lds(wm, wn, l31, lh, 0);        // + rr * OUT_ROWB
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const char* Eq = (q & 1) ? EQ1 : EQ0;
    // my pieces of quarter q have landed; younger operations that may still fly, in issue order
    //   E0 | E1 | pass 0: E2, NST stores | pass 1: E3, NST stores | pass 2: NST stores | pass 3: NST stores
    constexpr int NST = 4;   // stores per thread and pass
    if (q == 0) wait_vmcnt<8>();
    else if (q == 1) wait_vmcnt<8 + NST>();
    else if (q == 2) wait_vmcnt<8 + 2 * NST>();
    else wait_vmcnt<2 * NST>();
    __builtin_amdgcn_s_barrier();  // everyone's pieces landed; everyone finished reading the staging tile of quarter q-1
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rr = acc_rr(r);
      const float e0 = *reinterpret_cast<const float*>(Eq + e_rd + rr * E_ROWB);
      const float e1 = *reinterpret_cast<const float*>(Eq + e_rd + rr * E_ROWB + 128);
      float g = gate(fmaf(acc[q][0][r], a.out_scale, b0 + e0), fmaf(acc[q][1][r], a.out_scale, b1 + e1));
      if (t0 + 128 * wm + 32 * q + 4 * lh + rr >= row_lim) g = 0.f;
      *reinterpret_cast<uint16_t*>(OUT + o_wr + rr * OUT_ROWB) = ss_f2t<true>(g);   // the second plane of the output rows is not written
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): my staging writes are done
    __builtin_amdgcn_s_barrier();         // the staging tile is complete; everyone finished reading addend quarter q
    if (q + 2 < 4) dma_e((q & 1) ? EQ1 : EQ0, q + 2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {   // 64 rows x 256 B = 1024 pieces of 16 B, four per thread
      const int p = tid + 256 * j;
      const int c16 = out_store_c16(p);
      const int grow = t0 + out_store_tile_row(p, q);
      const uint4 v = *reinterpret_cast<const uint4*>(OUT + p * 16);
      const bool ok = (n0 >> 1) + 32 * (c16 >> 3) < a.N && !(c16 & 4);   // N is a multiple of 32 (checked by the launcher); hi halves only
      const int off = ok ? grow * a.ldc * 2 + n0 * 2 + c16 * 16 : (int)0x80000000;   // logical channel n0/2 sits at physical element n0
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), rsrc_c, off, 0, 0);   // rows >= T dropped
    }
  }
