// ITU-R BS.1770 integrated loudness and loudness normalisation on the device (input producer of `preprocess_input` when hparams['loud_norm'] is
// set, utils/audios/__init__.py:56-61: pyloudnorm, un-vendored: parity UNPINNED - the definition, the filter design, the block bounds and the
// tables are stylesinger_amd/loudness.py; and the writer's output LUFS target).
//
// K-weighting is a cascade of two biquads whose high-pass poles sit at ~0.995: the state is float64 throughout. Per sample, both stages in the
// transposed direct form II (state s = (s1, s2, t1, t2)):
//   y1 = b0 x + s1 ; s1 = b1 x - a1 y1 + s2 ; s2 = b2 x - a2 y1 ;   y = c0 y1 + t1 ; t1 = c1 y1 - d1 y + t2 ; t2 = c2 y1 - d2 y.
// That is a linear recurrence s' = A s + B x, so an item is cut into chunks of C samples and scanned:
//   1. lk_chunk_kernel<false>: every chunk runs the cascade from zero state and records its end state e_c (and max |x| of the chunk);
//   2. lk_carry_kernel: the true initial states S_0 = 0, S_{c+1} = M S_c + e_c with M = A^C (host, float64): one wave per item scans 64 chunks
//      at a time (Hillis-Steele over the lanes with the tabulated powers M, M^2, ..., M^32; the group's carry enters at lane 0);
//   3. lk_chunk_kernel<true>: every chunk runs again from S_c and sums y^2 into at most two gating segments;
//   4. lk_blocks_kernel: z_j = (sum over the block's four segments) / (T_g rate); 5. lk_gate_kernel: the two gates, L, the gain and max |x|.
// A chunk is one THREAD's walk (C <= 4096 samples); a workgroup owns 256 consecutive chunks = one contiguous span of the item and stages it
// through LDS 32 samples per chunk at a time: the global loads are 128-byte runs, and thread c reads LDS word 33 c + j (stride 33: conflict-free).
//
// Gating blocks overlap by 75 %: block j = [edges[j], edges[j + 4]), so an item's samples fall into SEGMENTS [edges[k], edges[k + 1]) and
// z_j is the sum of four segment sums. Consecutive edges are at least C apart (the host checks it; only the last one may be cut to n), so a chunk
// straddles at most one edge: it records (pre, post) = its sum before and from that edge on. A segment's sum is the `post` of the chunk the edge
// cuts, then the `pre` of every chunk that starts inside it, in ascending order: a fixed order with no atomics, so results are bit-identical from
// run to run and do not depend on B, on the buffer width or on the other items (they may depend on C).
#include "device_prims.h"
#include "../../include/stylesinger_hip.h"

namespace {
using namespace ss_dev;

constexpr int LK_THREADS = 256;
constexpr int LK_TS = 32;          // samples of every chunk staged per round
constexpr int LK_ROW = LK_TS + 1;  // LDS row stride in words
// the float64 table: [0..4] b0 b1 b2 a1 a2 of the shelf, [5..9] of the high pass (both normalised by a0), [10] T_g * rate, [11] unused,
// [12 + 16 i ...] M^(2^i) = A^(C 2^i) row-major for i = 0 .. 5 (108 doubles)
constexpr int LK_TAB_DIV = 10;
constexpr int LK_TAB_M = 12;

struct LkWs {
  double* E;    // [B][nchm][4] zero-state end state of every chunk
  double* S;    // [B][nchm][4] true initial state of every chunk
  double* PP;   // [B][nchm][2] (pre, post) sums of y^2
  float* MX;    // [B][nchm]    max |x|
  int64_t nchm;
};

__host__ __device__ inline int64_t lk_chunks(int64_t n, int C) { return (n + C - 1) / C; }

template <bool FINAL>
__global__ __launch_bounds__(LK_THREADS) void lk_chunk_kernel(const float* __restrict__ x, int64_t ldx, int Lx, const int32_t* __restrict__ n_,
                                                              const int32_t* __restrict__ nb_, const int32_t* __restrict__ edges, int lde,
                                                              const double* __restrict__ tab, int C, LkWs ws) {
  __shared__ float tile[LK_THREADS * LK_ROW];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t n = ss_uniform_len(n_, b, Lx);
  const int64_t c0 = (int64_t)blockIdx.x * LK_THREADS, S0 = c0 * C;   // first chunk / sample of this workgroup
  if (S0 >= n) return;
  int nb = 0;
  if (FINAL) {
    nb = ss_uniform_len(nb_, b, lde - 4);
    if (nb <= 0) return;   // too short for one block: nothing to sum
  }
  const int64_t c = c0 + tid, s = c * C;
  const int64_t slot = (int64_t)b * ws.nchm + c;
  const float* xb = x + (int64_t)b * ldx;
  const double b0 = tab[0], b1 = tab[1], b2 = tab[2], a1 = tab[3], a2 = tab[4];
  const double g0 = tab[5], g1 = tab[6], g2 = tab[7], d1 = tab[8], d2 = tab[9];
  double s1 = 0.0, s2 = 0.0, t1 = 0.0, t2 = 0.0, pre = 0.0, post = 0.0;
  float mx = 0.f;
  int64_t edge = INT64_MAX;   // the first segment edge past this chunk's first sample
  if (FINAL && s < n) {
    const double* si = ws.S + slot * 4;
    s1 = si[0]; s2 = si[1]; t1 = si[2]; t2 = si[3];
    const int32_t* eb = edges + (int64_t)b * lde;
    int lo = 0, hi = nb + 3;   // the largest k with edges[k] <= s (edges[0] = 0)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (eb[mid] <= s) lo = mid; else hi = mid - 1;
    }
    if (lo + 1 <= nb + 3) edge = eb[lo + 1];
  }
  for (int j0 = 0; j0 < C; j0 += LK_TS) {
    __syncthreads();
    for (int i = tid; i < LK_THREADS * LK_TS; i += LK_THREADS) {
      const int r = i >> 5, col = i & 31;
      const int64_t g = S0 + (int64_t)r * C + j0 + col;
      tile[r * LK_ROW + col] = g < n ? xb[g] : 0.f;   // (C is a multiple of LK_TS: the round stays inside the chunk)
    }
    __syncthreads();
    const int64_t base = s + j0;
    const int m = n - base < LK_TS ? (int)(n - base) : LK_TS;   // <= 0 past the item's end
    const float* row = tile + tid * LK_ROW;
    for (int j = 0; j < m; ++j) {
      const float xf = row[j];
      const double xv = (double)xf;
      const double y1 = b0 * xv + s1;
      s1 = b1 * xv - a1 * y1 + s2;
      s2 = b2 * xv - a2 * y1;
      const double y = g0 * y1 + t1;
      t1 = g1 * y1 - d1 * y + t2;
      t2 = g2 * y1 - d2 * y;
      if (FINAL) {
        const double v = y * y;
        if (base + j < edge) pre += v; else post += v;
      } else {
        mx = fmaxf(mx, fabsf(xf));
      }
    }
  }
  if (s >= n) return;
  if (FINAL) {
    ws.PP[slot * 2] = pre;
    ws.PP[slot * 2 + 1] = post;
  } else {
    double* e = ws.E + slot * 4;
    e[0] = s1; e[1] = s2; e[2] = t1; e[3] = t2;
    ws.MX[slot] = mx;
  }
}

// v += M t
__device__ __forceinline__ void lk_matvec_add(const double* __restrict__ M, const double (&t)[4], double (&v)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] += ((M[4 * r] * t[0] + M[4 * r + 1] * t[1]) + M[4 * r + 2] * t[2]) + M[4 * r + 3] * t[3];
}

__global__ __launch_bounds__(64) void lk_carry_kernel(const int32_t* __restrict__ n_, int Lx, const double* __restrict__ tab, int C, LkWs ws) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t nch = lk_chunks(ss_uniform_len(n_, b, Lx), C);
  if (nch <= 0) return;
  const double* E = ws.E + (int64_t)b * ws.nchm * 4;
  double* S = ws.S + (int64_t)b * ws.nchm * 4;
  if (lane < 4) S[lane] = 0.0;
  double carry[4] = {0.0, 0.0, 0.0, 0.0};   // S of the group's first chunk (the same in every lane)
  for (int64_t g = 0; g + 1 < nch; g += 64) {   // the last chunk's end state is nobody's carry
    const int64_t c = g + lane;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (c < nch) {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = E[c * 4 + k];
    }
    if (lane == 0) lk_matvec_add(tab + LK_TAB_M, carry, v);
#pragma unroll
    for (int i = 0; i < 6; ++i) {   // inclusive scan: v_l = sum_{m <= l} M^(l - m) e_m
      double t[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] = __shfl_up(v[k], 1 << i);
      if (lane >= (1 << i)) lk_matvec_add(tab + LK_TAB_M + 16 * i, t, v);
    }
    if (c + 1 < nch) {
#pragma unroll
      for (int k = 0; k < 4; ++k) S[(c + 1) * 4 + k] = v[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) carry[k] = __shfl(v[k], 63);
  }
}

__global__ __launch_bounds__(LK_THREADS) void lk_blocks_kernel(const int32_t* __restrict__ n_, int Lx, const int32_t* __restrict__ nb_,
                                                               const int32_t* __restrict__ edges, int lde, const double* __restrict__ tab, int C, LkWs ws,
                                                               double* __restrict__ z, int ldz) {
  const int b = blockIdx.y, j = blockIdx.x * LK_THREADS + threadIdx.x;
  if (j >= ldz) return;
  int nb = ss_uniform_len(nb_, b, lde - 4);
  if (nb > ldz) nb = ldz;
  double* zb = z + (int64_t)b * ldz;
  if (j >= nb) {
    zb[j] = 0.0;
    return;
  }
  const int64_t nch = lk_chunks(ss_uniform_len(n_, b, Lx), C);
  const int32_t* eb = edges + (int64_t)b * lde;
  const double* PP = ws.PP + (int64_t)b * ws.nchm * 2;
  double acc = 0.0;
  for (int k = j; k < j + 4; ++k) {
    const int64_t e0 = eb[k], e1 = eb[k + 1];
    double sg = 0.0;
    int64_t cf = e0 / C;
    if (e0 % C) {   // the chunk this edge cuts gives what it summed from the edge on
      if (cf < nch) sg = PP[cf * 2 + 1];
      ++cf;
    }
    int64_t cl = (e1 + C - 1) / C;   // the chunks that start inside the segment
    if (cl > nch) cl = nch;
    for (int64_t c = cf; c < cl; ++c) sg += PP[c * 2];
    acc += sg;
  }
  zb[j] = acc / tab[LK_TAB_DIV];
}

__global__ __launch_bounds__(64) void lk_gate_kernel(const int32_t* __restrict__ n_, int Lx, const int32_t* __restrict__ nb_, int lde, int C, LkWs ws,
                                                     const double* __restrict__ z, int ldz, double target, double* __restrict__ lufs,
                                                     float* __restrict__ gain, float* __restrict__ peak) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t nch = lk_chunks(ss_uniform_len(n_, b, Lx), C);
  int nb = ss_uniform_len(nb_, b, lde - 4);
  if (nb > ldz) nb = ldz;
  const float* MX = ws.MX + (int64_t)b * ws.nchm;
  float mx = 0.f;
  for (int64_t c = lane; c < nch; c += 64) mx = fmaxf(mx, MX[c]);
  mx = wave_max(mx);
  const double* zb = z + (int64_t)b * ldz;
  // absolute gate: J1 = {l_j >= -70}; every lane sums its blocks j = lane, lane + 64, ... in ascending order, then the fixed butterfly
  double s1 = 0.0, n1 = 0.0;
  for (int j = lane; j < nb; j += 64) {
    const double zj = zb[j];
    if (-0.691 + 10.0 * log10(zj) >= -70.0) { s1 += zj; n1 += 1.0; }
  }
  s1 = wave_sum(s1);
  n1 = wave_sum(n1);
  double L = nb > 0 ? -INFINITY : NAN;   // too short for a block: NaN; nothing passes a gate (digital silence): -inf
  if (n1 > 0.0) {
    const double rel = -0.691 + 10.0 * log10(s1 / n1) - 10.0;
    double s2 = 0.0, n2 = 0.0;
    for (int j = lane; j < nb; j += 64) {
      const double zj = zb[j], lj = -0.691 + 10.0 * log10(zj);
      if (lj > rel && lj > -70.0) { s2 += zj; n2 += 1.0; }
    }
    s2 = wave_sum(s2);
    n2 = wave_sum(n2);
    if (n2 > 0.0) L = -0.691 + 10.0 * log10(s2 / n2);
  }
  if (lane == 0) {
    lufs[b] = L;
    gain[b] = isfinite(L) ? (float)pow(10.0, (target - L) / 20.0) : 1.0f;
    peak[b] = mx;
  }
}

// y = fl32(g x); with P = fl32(g max|x|) (= max |y|: rounding is monotone) > 1, y = y / P as an IEEE division
__device__ __forceinline__ float lk_apply1(float xv, float g, float P) {
#pragma clang fp contract(off)
  const float y = g * xv;
  return P > 1.0f ? __fdiv_rn(y, P) : y;
}

template <bool VEC>
__global__ __launch_bounds__(LK_THREADS) void lk_apply_kernel(const float* __restrict__ x, int64_t ldx, int Lx, const int32_t* __restrict__ n_,
                                                              const float* __restrict__ gain, const float* __restrict__ peak, float* __restrict__ y,
                                                              int64_t ldy, int Ly) {
  const int b = blockIdx.y;
  const int64_t t = ((int64_t)blockIdx.x * LK_THREADS + threadIdx.x) * 4;
  if (t >= Ly) return;
  const int lim = Lx < Ly ? Lx : Ly;
  const int64_t n = ss_uniform_len(n_, b, lim);
  float g = gain[b];
  float P;
  {
#pragma clang fp contract(off)
    P = g * peak[b];
  }
  const float* xb = x + (int64_t)b * ldx;
  float* yb = y + (int64_t)b * ldy;
  if (VEC && t + 4 <= n) {   // (VEC: both rows 16-byte aligned at every t)
    const float4 v = *reinterpret_cast<const float4*>(xb + t);
    *reinterpret_cast<float4*>(yb + t) = make_float4(lk_apply1(v.x, g, P), lk_apply1(v.y, g, P), lk_apply1(v.z, g, P), lk_apply1(v.w, g, P));
    return;
  }
  if (VEC && t >= n && t + 4 <= Ly) {
    *reinterpret_cast<float4*>(yb + t) = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  for (int k = 0; k < 4 && t + k < Ly; ++k) yb[t + k] = t + k < n ? lk_apply1(xb[t + k], g, P) : 0.f;
}

int64_t lk_ws_doubles(int64_t B, int64_t nchm) { return B * nchm * 10; }   // E 4 + S 4 + PP 2 per chunk, then the floats

LkWs lk_carve(void* workspace, int B, int Lx, int C) {
  LkWs ws;
  ws.nchm = lk_chunks(Lx, C);
  const int64_t per = (int64_t)B * ws.nchm;
  ws.E = reinterpret_cast<double*>(workspace);
  ws.S = ws.E + per * 4;
  ws.PP = ws.S + per * 4;
  ws.MX = reinterpret_cast<float*>(ws.PP + per * 2);
  return ws;
}

}  // namespace

extern "C" int64_t ss_loudness_workspace_bytes(int B, int Lx, int C) {
  if (B <= 0 || Lx <= 0 || C < LK_TS || C > 4096 || C % LK_TS) return -1;
  const int64_t nchm = lk_chunks(Lx, C);
  return lk_ws_doubles(B, nchm) * (int64_t)sizeof(double) + ((int64_t)B * nchm * (int64_t)sizeof(float) + 7) / 8 * 8;
}

extern "C" int ss_loudness_measure(const float* x, int64_t ldx, int Lx, const int32_t* n, const int32_t* n_blocks, const int32_t* edges, int lde, int B,
                                   const double* tab, int C, double target, double* lufs, float* gain, float* peak, double* z, int ldz, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  SS_CHECK_ARG(x && n && n_blocks && edges && tab && lufs && gain && peak && z && workspace, "ss_loudness_measure: null argument");
  SS_CHECK_ARG(B > 0 && B <= 65535 && Lx > 0 && ldx >= Lx && lde >= 5 && ldz >= 1, "ss_loudness_measure: bad dims (B=%d Lx=%d ldx=%lld lde=%d ldz=%d)", B, Lx,
               (long long)ldx, lde, ldz);
  SS_CHECK_ARG(C >= LK_TS && C <= 4096 && C % LK_TS == 0, "ss_loudness_measure: bad chunk (C=%d: a multiple of %d in [%d, 4096])", C, LK_TS, LK_TS);
  SS_CHECK_ARG(target == target && target >= -200.0 && target <= 200.0, "ss_loudness_measure: bad target (%g LUFS)", target);
  SS_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 8 == 0 && workspace_bytes >= ss_loudness_workspace_bytes(B, Lx, C),
               "ss_loudness_measure: workspace of %lld bytes, need %lld (8-byte aligned)", (long long)workspace_bytes,
               (long long)ss_loudness_workspace_bytes(B, Lx, C));
  const LkWs ws = lk_carve(workspace, B, Lx, C);
  const int64_t groups = (ws.nchm + LK_THREADS - 1) / LK_THREADS;
  SS_CHECK_ARG(groups <= 0x7fffffff, "ss_loudness_measure: too many chunks");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)groups, (unsigned)B);
  hipLaunchKernelGGL(lk_chunk_kernel<false>, grid, dim3(LK_THREADS), 0, st, x, ldx, Lx, n, n_blocks, edges, lde, tab, C, ws);
  SS_CHECK_LAUNCH("lk_chunk_kernel<local>");
  hipLaunchKernelGGL(lk_carry_kernel, dim3((unsigned)B), dim3(64), 0, st, n, Lx, tab, C, ws);
  SS_CHECK_LAUNCH("lk_carry_kernel");
  hipLaunchKernelGGL(lk_chunk_kernel<true>, grid, dim3(LK_THREADS), 0, st, x, ldx, Lx, n, n_blocks, edges, lde, tab, C, ws);
  SS_CHECK_LAUNCH("lk_chunk_kernel<final>");
  hipLaunchKernelGGL(lk_blocks_kernel, dim3((unsigned)((ldz + LK_THREADS - 1) / LK_THREADS), (unsigned)B), dim3(LK_THREADS), 0, st, n, Lx, n_blocks, edges,
                     lde, tab, C, ws, z, ldz);
  SS_CHECK_LAUNCH("lk_blocks_kernel");
  hipLaunchKernelGGL(lk_gate_kernel, dim3((unsigned)B), dim3(64), 0, st, n, Lx, n_blocks, lde, C, ws, z, ldz, target, lufs, gain, peak);
  SS_CHECK_LAUNCH("lk_gate_kernel");
  return SS_OK;
}

extern "C" int ss_loudness_apply(const float* x, int64_t ldx, int Lx, const int32_t* n, const float* gain, const float* peak, float* y, int64_t ldy, int Ly,
                                 int B, void* stream) {
  SS_CHECK_ARG(x && n && gain && peak && y, "ss_loudness_apply: null argument");
  SS_CHECK_ARG(B > 0 && B <= 65535 && Lx > 0 && Ly > 0 && ldx >= Lx && ldy >= Ly, "ss_loudness_apply: bad dims (B=%d Lx=%d Ly=%d ldx=%lld ldy=%lld)", B, Lx, Ly,
               (long long)ldx, (long long)ldy);
  SS_CHECK_ARG(x != y, "ss_loudness_apply: input and output must not alias");
  const bool vec = reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(y) % 16 == 0 && ldx % 4 == 0 && ldy % 4 == 0;
  const dim3 grid((unsigned)(((int64_t)Ly + 4 * LK_THREADS - 1) / (4 * LK_THREADS)), (unsigned)B);
  if (vec)
    hipLaunchKernelGGL(lk_apply_kernel<true>, grid, dim3(LK_THREADS), 0, (hipStream_t)stream, x, ldx, Lx, n, gain, peak, y, ldy, Ly);
  else
    hipLaunchKernelGGL(lk_apply_kernel<false>, grid, dim3(LK_THREADS), 0, (hipStream_t)stream, x, ldx, Lx, n, gain, peak, y, ldy, Ly);
  SS_CHECK_LAUNCH("lk_apply_kernel");
  return SS_OK;
}
