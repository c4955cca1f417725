// The STORE epilogue of the 256-row x 256-column 8-wave kernels tile256s_kernel<SS_HEPI_STORE, ..> (gemm_bf16_tile256.hip) and
// tile256q_store_kernel (gemm_bf16_tile256q.hip), #included INSIDE each kernel body after the barrier that ends the K loop: four passes of 64 rows
// (accumulator block m = q of every wave), staged as fp32 [64][256] in alternating 64-KB halves of the operand memory, then stored row-contiguously
// as 16-byte vectors. A text fragment and not a function on purpose: as a function it changes the vector address arithmetic the compiler selects,
// and these kernels must stay instruction for instruction what was measured (gate128_prologue.h). Expects in scope: a, acc, smem (the LDS block),
// st_wr, b, t0, tid, row_lim, biasg, BN and the constant W2 (fp16 terms: the accumulators are scaled by args.out_scale here).
  float* Cb = (float*)a.C + (int64_t)b * a.c_batch_stride;
  const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(Cb), 0, __builtin_amdgcn_readfirstlane((int)((int64_t)a.T * a.ldc * 4)), 0x00020000);
  const int c4 = (tid & 63) * 4;                 // this thread's 4 columns in every row it handles
  const int dead = c4 < a.N ? 0 : (int)0x80000000;   // N is a multiple of 4
  float bs[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) bs[e] = (biasg && !dead) ? biasg[c4 + e] : 0.f;
  const bool relu = a.act == SS_ACT_RELU;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    char* St = smem + (q & 1) * 64 * 1024;
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) *reinterpret_cast<float*>(St + st_wr + ((r & 3) + 8 * (r >> 2)) * (BN * 4) + n * 128) = acc[q][n][r];
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): my staging writes are done
    __builtin_amdgcn_s_barrier();         // the staging tile of pass q is complete (pass q-1's tile, the other half, is being read at most)
#pragma unroll
    for (int j = 0; j < 8; ++j) {         // 64 rows x 64 float4 = 4096 pieces, eight per thread: piece p = (row p >> 6, columns 4 (p & 63))
      const int k = (tid >> 6) + 8 * j;   // staging row of piece tid + 512 j
      const int grow = t0 + 128 * (k >> 5) + 32 * q + (k & 31);
      float4 v = *reinterpret_cast<const float4*>(St + k * (BN * 4) + c4 * 4);
      if constexpr (W2) v = make_float4(fmaf(v.x, a.out_scale, bs[0]), fmaf(v.y, a.out_scale, bs[1]), fmaf(v.z, a.out_scale, bs[2]), fmaf(v.w, a.out_scale, bs[3]));
      else { v.x += bs[0]; v.y += bs[1]; v.z += bs[2]; v.w += bs[3]; }
      if (relu) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
      if (grow >= row_lim) v = make_float4(0.f, 0.f, 0.f, 0.f);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsrc_c, (grow * a.ldc + c4) * 4 | dead, 0, 0);   // rows >= T dropped
    }
    // (no barrier here: pass q+1 writes the OTHER half, and pass q+2's writes to this half come after pass q+1's barrier, which every
    // thread reaches only after its pass-q reads)
  }
