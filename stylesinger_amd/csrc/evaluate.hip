// Objective metrics of a rendered item against a target recording (stylesinger_amd/evaluate.py holds the definitions; include/stylesinger_hip.h
// the summary): a quantised log-mel cepstrum per frame, a dynamic time warp over those frame vectors whose PATH is the product, and the
// reductions along that path (distance sum, voicing / gross-pitch counts, cents). Integer costs, so path / plen / cost / status are exact.
//
//   ss_eval_mcep       one thread per (frame, coefficient): the fp32 chain over the mel bins in ascending order, contraction off
//   ss_eval_cost_band  c(i, j) = isqrt(sum_k (qa_ik - qb_jk)^2) of every band cell, 64 x 64 tiles over all CUs, both operand tiles in LDS; a wave
//                      takes one anti-diagonal of the tile at a time (lane = row), so that its 64 uint16 results are neighbours in the
//                      diagonal-major workspace: ws[(d mod Wd) * Ta + i]
//   ss_eval_dtw        one workgroup per item, the sweep of contour_align.hip RESTATED (not shared: the tie order differs - diagonal, up, left - and
//                      the cost is read from the workspace, the next diagonal's one diagonal ahead, instead of computed from two LDS values):
//                      three rolling diagonals of D in LDS, one barrier per diagonal, one direction byte per cell; one lane walks back and
//                      writes the pairs at the END of the item's path buffer (last cell last), then all lanes move them to the front
//   ss_eval_reduce     one workgroup per item over the path (or the identity): S recomputed from q, thread t takes cells p = t (mod threads) ascending,
//                      then a fixed tree; no atomics
//   ss_cosine_rows     one wave per row, float64 sums in a fixed order
// None allocates or synchronises; plain vector stores only; an item reads and writes nothing of another item.
#include "common.h"
#include "../../include/stylesinger_hip.h"

namespace {

constexpr int EV_INF = 0x3FFFFFFF;       // D of a cell no path reaches (evaluate.EVAL_INF = pitch.ALIGN_INF)
constexpr int EV_DTW_THREADS = 512;
constexpr int EV_PASSES = SS_EVAL_MAX_T / EV_DTW_THREADS;   // rows of the longest diagonal per lane
static_assert(EV_PASSES * EV_DTW_THREADS == SS_EVAL_MAX_T, "the cap is a whole number of passes");
constexpr int EV_RED_THREADS = 256;
constexpr int EV_TILE = 64;              // rows and columns of a cost tile
constexpr int EV_COST_THREADS = 256;
constexpr int EV_MAX_LDS = 160 * 1024;
constexpr int EV_MAX_COST = 46341;       // isqrt(2^31 - 1) + 1: the largest cost of a legal S
static_assert((long long)(SS_EVAL_MAX_T + SS_EVAL_MAX_T) * EV_MAX_COST < EV_INF, "D overflows int32");
static_assert(14 * SS_EVAL_MAX_T <= EV_MAX_LDS, "the caps must fit the CU's LDS");
static_assert(SS_EVAL_MAX_T <= 32767, "band centres are kept as int16");

typedef short ev_short2 __attribute__((ext_vector_type(2)));

// the band of contour_align.hip: centre of row i, and the rule for an item that is not aligned
__device__ __forceinline__ int ev_centre(int i, int n_a, int n_b) { return (int)(((2 * (int64_t)i + 1) * n_b) / (2 * (int64_t)n_a)); }
__device__ __forceinline__ int ev_band_w(int band, int n_a, int n_b) {
  const int full = n_a > n_b ? n_a : n_b;
  return (band <= 0 || band > full) ? full : band;   // a band wider than the matrix is the full matrix
}
__device__ __forceinline__ bool ev_unaligned(int n_a, int n_b, int W) { return n_a == 0 || n_b == 0 || (int64_t)n_b > (int64_t)W * n_a; }

// ---- 1. quantised mel cepstrum ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void eval_mcep_kernel(const float* __restrict__ mel, int64_t ldm, int64_t mel_bs, const int32_t* __restrict__ lens,
                                                        const float* __restrict__ tab, int16_t* __restrict__ q, int B, int T, int N, int K, int Kp,
                                                        float s, float vmin, float vmax) {
#pragma clang fp contract(off)
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)B * T * Kp) return;
  const int k = (int)(e % Kp);
  const int64_t bt = e / Kp;
  const int t = (int)(bt % T), b = (int)(bt / T);
  int n = lens ? lens[b] : T;
  n = n < T ? n : T;
  int16_t v = 0;
  if (t < n && k < K) {
    const float* m = mel + (int64_t)b * mel_bs + (int64_t)t * ldm;
    const float* w = tab + (int64_t)k * N;
    float c = 0.f;
    for (int i = 0; i < N; ++i) {
      const float x = fminf(fmaxf(m[i], vmin), vmax);
      const float p = x * w[i];
      c = c + p;
    }
    const float r = rintf(c * s);
    v = (int16_t)(int)r;   // |r| <= 32767: the entry refuses ranges that could leave int16
  }
  q[e] = v;
}

// ---- 2. the costs of the band ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned ev_isqrt(unsigned S) {   // floor(sqrt(S)) for S < 2^31: sqrtf is within 1 of it, then an exact correction
  unsigned r = (unsigned)sqrtf((float)S);
  if (r * r > S) --r;
  if ((r + 1) * (r + 1) <= S) ++r;
  return r;
}

__global__ __launch_bounds__(EV_COST_THREADS) void eval_cost_kernel(const int16_t* __restrict__ qa, const int32_t* __restrict__ lens_a,
                                                                    const int16_t* __restrict__ qb, const int32_t* __restrict__ lens_b, int Kp, int band,
                                                                    int Ta, int Tb, uint16_t* __restrict__ wsc, int Wd) {
  extern __shared__ __align__(16) unsigned char ev_smem[];
  const int b = blockIdx.z, tid = threadIdx.x;
  const int n_a = ss_uniform_len(lens_a, b, Ta), n_b = ss_uniform_len(lens_b, b, Tb);
  const int W = ev_band_w(band, n_a, n_b);
  if (ev_unaligned(n_a, n_b, W)) return;
  const int i0 = blockIdx.x * EV_TILE, j0 = blockIdx.y * EV_TILE;
  if (i0 >= n_a || j0 >= n_b) return;
  const int i1 = (i0 + EV_TILE < n_a ? i0 + EV_TILE : n_a) - 1;
  // the columns the tile's rows can hold: lo of its first row .. hi of its last one (both grow with the row)
  const int c0 = ev_centre(i0, n_a, n_b), c1 = ev_centre(i1, n_a, n_b);
  const int lo0 = c0 - W > 0 ? c0 - W : 0, hi1 = c1 + W < n_b - 1 ? c1 + W : n_b - 1;
  if (j0 > hi1 || j0 + EV_TILE - 1 < lo0) return;   // uniform per workgroup: before any barrier

  const int K2 = Kp / 2, ld = K2 | 1;               // dwords per row in LDS, odd: the lanes of a wave read different rows
  uint32_t* A = reinterpret_cast<uint32_t*>(ev_smem);   // [64][ld]
  uint32_t* Bt = A + EV_TILE * ld;                       // [64][ld]
  const uint32_t* ga = reinterpret_cast<const uint32_t*>(qa + ((int64_t)b * Ta + i0) * Kp);   // Kp is even and the buffers are 4-byte aligned (checked)
  const uint32_t* gb = reinterpret_cast<const uint32_t*>(qb + ((int64_t)b * Tb + j0) * Kp);
  const int rows_a = i1 - i0 + 1, rows_b = (j0 + EV_TILE < n_b ? j0 + EV_TILE : n_b) - j0;
  for (int e = tid; e < EV_TILE * K2; e += EV_COST_THREADS) {
    const int r = e / K2, k = e - r * K2;
    A[r * ld + k] = r < rows_a ? ga[e] : 0u;          // rows at or past the item's length are never read
    Bt[r * ld + k] = r < rows_b ? gb[e] : 0u;
  }
  __syncthreads();

  const int lane = tid & 63, wave = tid >> 6;
  const int i = i0 + lane;
  const bool row_ok = i < n_a;
  const int ci = row_ok ? ev_centre(i, n_a, n_b) : 0;
  const int lo = ci - W > 0 ? ci - W : 0, hi = ci + W < n_b - 1 ? ci + W : n_b - 1;
  uint16_t* out = wsc + (int64_t)b * Wd * Ta;
  const uint32_t* arow = A + lane * ld;
  for (int dd = wave; dd < 2 * EV_TILE - 1; dd += EV_COST_THREADS / 64) {   // the tile's anti-diagonals: local column = dd - lane
    const int jl = dd - lane;
    const int j = j0 + jl;
    if (!row_ok || jl < 0 || jl >= EV_TILE || j < lo || j > hi) continue;
    const uint32_t* brow = Bt + jl * ld;
    int S = 0;
    for (int k = 0; k < K2; ++k) {
      const uint32_t ua = arow[k], ub = brow[k];
      ev_short2 va, vb;
      __builtin_memcpy(&va, &ua, 4);
      __builtin_memcpy(&vb, &ub, 4);
      const ev_short2 df = va - vb;                                   // packed int16 subtract: every difference fits (the entry's contract)
      S = __builtin_amdgcn_sdot2(df, df, S, false);
    }
    const int d = i + j;
    out[(int64_t)(d % Wd) * Ta + i] = (uint16_t)ev_isqrt((unsigned)S);
  }
}

// ---- 3. the sweep and the path -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EV_DTW_THREADS) void eval_dtw_kernel(const int32_t* __restrict__ lens_a, const int32_t* __restrict__ lens_b, int band,
                                                                  int32_t* __restrict__ path, int32_t* __restrict__ plen, int32_t* __restrict__ cost,
                                                                  int32_t* __restrict__ status, int Ta, int Tb, const uint16_t* __restrict__ wsc,
                                                                  unsigned char* __restrict__ wsd, int Wd) {
  extern __shared__ __align__(16) unsigned char ev_smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n_a = ss_uniform_len(lens_a, b, Ta), n_b = ss_uniform_len(lens_b, b, Tb);
  const int cap = Ta + Tb;                                           // pairs an item's path buffer holds; a path has at most n_a + n_b - 1
  int2* pth = reinterpret_cast<int2*>(path) + (int64_t)b * cap;
  const int W = ev_band_w(band, n_a, n_b);
  if (ev_unaligned(n_a, n_b, W)) {                                   // not aligned: the identity over the common frames (uniform per workgroup)
    const int P = n_a < n_b ? n_a : n_b;
    for (int p = tid; p < P; p += EV_DTW_THREADS) pth[p] = make_int2(p, p);
    if (tid == 0) {
      plen[b] = P;
      cost[b] = 0;
      status[b] = 1;
    }
    return;
  }
  int32_t* D = reinterpret_cast<int32_t*>(ev_smem);                  // [3][Ta]
  int16_t* ci = reinterpret_cast<int16_t*>(ev_smem + (size_t)12 * Ta);   // [Ta] band centres
  for (int i = tid; i < n_a; i += EV_DTW_THREADS) ci[i] = (int16_t)ev_centre(i, n_a, n_b);
  __syncthreads();

  const uint16_t* cst = wsc + (int64_t)b * Wd * Ta;
  unsigned char* dirs = wsd + (int64_t)b * Wd * Ta;
  const int n_diag = n_a + n_b - 1;
  const int den = 2 * (n_a + n_b);
  // rows of diagonal d, a superset (contour_align.hip derives it): 0 <= d - i < n_b, and inside the band
  //   i >= ((d - W) 2 n_a - n_b) / den and i < ((d + W + 1) 2 n_a - n_b) / den, one row of slack on both sides; the lane's own test is exact.
  // (d + W + 1) 2 n_a <= 24577 * 16384: int32 holds it.
  auto rows = [&](int d, int& a, int& e) {
    a = ((d - W) * 2 * n_a - n_b) / den - 1;
    e = ((d + W + 1) * 2 * n_a - n_b) / den + 1;
    const int rmin = d - (n_b - 1) > 0 ? d - (n_b - 1) : 0, rmax = d < n_a - 1 ? d : n_a - 1;
    a = a > rmin ? a : rmin;
    e = e < rmax ? e : rmax;
  };
  int a, e, slot = 0;                                                // slot = d mod Wd
  rows(0, a, e);
  // The costs of a diagonal are loaded ONE DIAGONAL AHEAD, all of this lane's rows of it (EV_PASSES registers; a band of at most 511 rows per
  // diagonal uses the first only): the loads are under way while the current diagonal is computed and end at its barrier. A cell outside the band
  // may be loaded (the row range is a superset; the address is inside the plane) and is never used.
  unsigned c_pre[EV_PASSES], c_nxt[EV_PASSES];
#pragma unroll
  for (int k = 0; k < EV_PASSES; ++k) c_pre[k] = c_nxt[k] = 0u;
  if (a + tid <= e) c_pre[0] = cst[a + tid];                        // diagonal 0: one cell
  for (int d = 0; d < n_diag; ++d) {
    int32_t* cur = D + (size_t)(d % 3) * Ta;
    const int32_t* p1 = D + (size_t)((d + 2) % 3) * Ta;              // diagonal d - 1
    const int32_t* p2 = D + (size_t)((d + 1) % 3) * Ta;              // diagonal d - 2
    int a1 = 0, e1 = -1;
    const int slot1 = slot + 1 == Wd ? 0 : slot + 1;
    if (d + 1 < n_diag) {
      rows(d + 1, a1, e1);
      const uint16_t* nx = cst + (int64_t)slot1 * Ta;                // inside the plane: slot1 < Wd, rows <= n_a - 1 < Ta
      if (a1 + tid <= e1) c_nxt[0] = nx[a1 + tid];
      if (e1 - a1 >= EV_DTW_THREADS) {                               // uniform: a diagonal longer than the workgroup
#pragma unroll
        for (int k = 1; k < EV_PASSES; ++k) {
          const int r = a1 + tid + k * EV_DTW_THREADS;
          if (r <= e1) c_nxt[k] = nx[r];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < EV_PASSES; ++k) {
      const int i = a + tid + k * EV_DTW_THREADS;
      if (a + k * EV_DTW_THREADS > e) break;                         // uniform
      if (i > e) continue;
      const int j = d - i, i1 = i > 0 ? i - 1 : 0;
      const int c_i = ci[i], c_1 = ci[i1];
      const int v_dg = p2[i1], v_up = p1[i1], v_lf = p1[i];
      const int lo = c_i - W > 0 ? c_i - W : 0, hi = c_i + W < n_b - 1 ? c_i + W : n_b - 1;
      if (j < lo || j > hi) continue;
      const int c = (int)c_pre[k];
      int best = 0, dir = 0;                                         // d == 0, the start cell: D = c(0, 0)
      if (d > 0) {
        const int lo1 = c_1 - W > 0 ? c_1 - W : 0, hi1 = c_1 + W < n_b - 1 ? c_1 + W : n_b - 1;
        const int dg = (i >= 1 && j - 1 >= lo1 && j - 1 <= hi1) ? v_dg : EV_INF;
        const int up = (i >= 1 && j >= lo1 && j <= hi1) ? v_up : EV_INF;
        const int lf = j - 1 >= lo ? v_lf : EV_INF;
        best = dg;                                                   // the first minimum in the order diagonal, up, left
        if (up < best) { best = up; dir = 1; }
        if (lf < best) { best = lf; dir = 2; }
      }
      cur[i] = best >= EV_INF ? EV_INF : best + c;
      dirs[(int64_t)slot * Ta + i] = (unsigned char)dir;
    }
    slot = slot1;
    a = a1;
    e = e1;
#pragma unroll
    for (int k = 0; k < EV_PASSES; ++k) c_pre[k] = c_nxt[k];         // (copying only c_pre[0] on short diagonals, behind a uniform test, measured 11 - 18 % slower)
    __syncthreads();
  }

  // the walk back: one lane, one dependent byte load per step; the pairs go to the END of the buffer, the last cell last, so they stand in forward
  // order. Every step lowers i + j by at least one: at most n_a + n_b - 1 <= cap - 1 pairs, k never reaches below 1.
  __threadfence_block();
  int32_t* shared_p = D + (size_t)(n_diag % 3) * Ta;                 // a word of the buffer the last diagonal did not use (Ta >= 1)
  if (tid == 0) {
    const int total = D[(size_t)((n_diag - 1) % 3) * Ta + (n_a - 1)];
    int i = n_a - 1, j = n_b - 1, k = cap;
    int s = (n_diag - 1) % Wd;
    while (true) {
      --k;
      pth[k] = make_int2(i, j);
      if (i == 0 && j == 0) break;
      const int dir = dirs[(int64_t)s * Ta + i];
      if (dir == 0 && i > 0 && j > 0) {
        --i; --j; s = s == 0 ? Wd - 1 : s - 1; s = s == 0 ? Wd - 1 : s - 1;
      } else if (dir == 1 && i > 0) {
        --i; s = s == 0 ? Wd - 1 : s - 1;
      } else if (j > 0 && dir == 2) {
        --j; s = s == 0 ? Wd - 1 : s - 1;
      } else {
        break;                                                       // cannot happen on a connected band; never walk out of the matrix
      }
    }
    shared_p[0] = cap - k;
    plen[b] = cap - k;
    cost[b] = total;
    status[b] = 0;
  }
  __syncthreads();
  const int P = shared_p[0], off = cap - P;                          // off >= 1
  // to the front, in ascending chunks: a chunk is read whole, then written whole. What it overwrites ([p0, p0 + threads)) lies below everything a
  // later chunk reads (from off + p0 + threads on), and the barrier keeps a write of this chunk off a pair another lane of it still has to read.
  for (int p0 = 0; p0 < P; p0 += EV_DTW_THREADS) {
    const int p = p0 + tid;
    int2 v = make_int2(0, 0);
    if (p < P) v = pth[off + p];
    __syncthreads();
    if (p < P) pth[p] = v;
  }
}

// ---- 4. the reductions along the path ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EV_RED_THREADS) void eval_reduce_kernel(const int16_t* __restrict__ qa, const float* __restrict__ f0a, int64_t ldfa,
                                                                     const int32_t* __restrict__ lens_a, const int16_t* __restrict__ qb,
                                                                     const float* __restrict__ f0b, int64_t ldfb, const int32_t* __restrict__ lens_b,
                                                                     int Kp, const int32_t* __restrict__ path, const int32_t* __restrict__ plen, int Ta,
                                                                     int Tb, int64_t* __restrict__ counts, double* __restrict__ sums) {
#pragma clang fp contract(off)
  __shared__ double s_d[2][EV_RED_THREADS];
  __shared__ int s_n[3][EV_RED_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n_a = ss_uniform_len(lens_a, b, Ta), n_b = ss_uniform_len(lens_b, b, Tb);
  const int cap = Ta + Tb;
  int P = n_a < n_b ? n_a : n_b;                                     // no path: the identity over the common frames
  const int2* pth = nullptr;
  if (path) {
    pth = reinterpret_cast<const int2*>(path) + (int64_t)b * cap;
    P = plen[b];
    P = P < 0 ? 0 : (P < cap ? P : cap);
    if (n_a == 0 || n_b == 0) P = 0;
  }
  const int16_t* A = qa + (int64_t)b * Ta * Kp;
  const int16_t* Bq = qb + (int64_t)b * Tb * Kp;
  const float* fa_row = f0a + (int64_t)b * ldfa;
  const float* fb_row = f0b + (int64_t)b * ldfb;
  double dist = 0.0, cents = 0.0;
  int n_both = 0, n_vde = 0, n_gpe = 0;
  for (int p = tid; p < P; p += EV_RED_THREADS) {
    int i = p, j = p;
    if (pth) {
      const int2 ij = pth[p];
      i = ij.x < 0 ? 0 : (ij.x < n_a ? ij.x : n_a - 1);              // a load must never leave the item's rows, whatever the path buffer holds
      j = ij.y < 0 ? 0 : (ij.y < n_b ? ij.y : n_b - 1);
    }
    const int16_t* ra = A + (int64_t)i * Kp;
    const int16_t* rb = Bq + (int64_t)j * Kp;
    int64_t S = 0;
    for (int k = 0; k < Kp; ++k) {
      const int df = (int)ra[k] - (int)rb[k];
      S += (int64_t)df * df;
    }
    dist = dist + sqrt((double)S);
    const float fa = fa_row[i], fb = fb_row[j];
    const bool va = fa > 0.f, vb = fb > 0.f;
    if (va && vb) {
      ++n_both;
      const float thr = 0.2f * fb;
      if (fabsf(fa - fb) > thr) ++n_gpe;
      const double c = 1200.0 * log2((double)fa / (double)fb);
      const double c2 = c * c;
      cents = cents + c2;
    } else if (va != vb) {
      ++n_vde;
    }
  }
  s_d[0][tid] = dist; s_d[1][tid] = cents;
  s_n[0][tid] = n_both; s_n[1][tid] = n_vde; s_n[2][tid] = n_gpe;
  __syncthreads();
  for (int h = EV_RED_THREADS / 2; h > 0; h >>= 1) {                 // the fixed tree: slot t += slot t + h
    if (tid < h) {
      s_d[0][tid] = s_d[0][tid] + s_d[0][tid + h];
      s_d[1][tid] = s_d[1][tid] + s_d[1][tid + h];
      s_n[0][tid] += s_n[0][tid + h]; s_n[1][tid] += s_n[1][tid + h]; s_n[2][tid] += s_n[2][tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    counts[4 * (int64_t)b + 0] = P;
    counts[4 * (int64_t)b + 1] = s_n[0][0];
    counts[4 * (int64_t)b + 2] = s_n[1][0];
    counts[4 * (int64_t)b + 3] = s_n[2][0];
    sums[2 * (int64_t)b + 0] = s_d[0][0];
    sums[2 * (int64_t)b + 1] = s_d[1][0];
  }
}

// ---- 5. cosine of row pairs ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void cosine_rows_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int C) {
#pragma clang fp contract(off)
  __shared__ double s[3][64];
  const int r = blockIdx.x, tid = threadIdx.x;
  const float* x = a + (int64_t)r * C;
  const float* y = b + (int64_t)r * C;
  double ab = 0.0, aa = 0.0, bb = 0.0;
  for (int c = tid; c < C; c += 64) {                                // lane t: columns c = t (mod 64) ascending
    const double u = (double)x[c], v = (double)y[c];
    ab = ab + u * v;
    aa = aa + u * u;
    bb = bb + v * v;
  }
  s[0][tid] = ab; s[1][tid] = aa; s[2][tid] = bb;
  __syncthreads();
  for (int h = 32; h > 0; h >>= 1) {
    if (tid < h) {
      s[0][tid] = s[0][tid] + s[0][tid + h];
      s[1][tid] = s[1][tid] + s[1][tid + h];
      s[2][tid] = s[2][tid] + s[2][tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double den = sqrt(s[1][0]) * sqrt(s[2][0]);
    out[r] = den > 0.0 ? (float)(s[0][0] / den) : 0.f;               // a zero row has no direction: 0
  }
}

int64_t ev_width(int Tb, int band) {   // band cells per row of an item
  if (band <= 0) return Tb;
  const int64_t w = 2 * (int64_t)band + 1;
  return w < Tb ? w : Tb;
}

bool ev_dims_ok(int B, int Ta, int Tb) { return B > 0 && B <= 65535 && Ta > 0 && Tb > 0 && Ta <= SS_EVAL_MAX_T && Tb <= SS_EVAL_MAX_T; }

}  // namespace

extern "C" int ss_eval_mcep(const float* mel, int64_t ldm, int64_t mel_bs, const int32_t* lens, const float* tab, int16_t* q, int B, int T, int n_mels,
                            int K, float s, float vmin, float vmax, void* stream) {
  SS_CHECK_ARG(mel && tab && q, "ss_eval_mcep: null pointer");
  SS_CHECK_ARG(B > 0 && T > 0 && n_mels > 0 && K > 0 && K <= SS_EVAL_MAX_K && ldm >= n_mels && mel_bs >= 0,
               "ss_eval_mcep: bad dims (B=%d T=%d n_mels=%d K=%d ldm=%lld)", B, T, n_mels, K, (long long)ldm);
  SS_CHECK_ARG(s > 0.f && vmin < vmax, "ss_eval_mcep: scale %g / range [%g, %g]", (double)s, (double)vmin, (double)vmax);
  // evaluate.mcep_bound. K < N: the rows are orthonormal and Parseval gives |c_k|, ||c - c'|| <= sqrt(N) * the largest |m|, |m - m'|. K >= N: rows
  // repeat (aliases) and one has norm sqrt(2): the bound per coefficient grows by sqrt(2) and S <= K * bound^2. + 1: the rounding of the chain and rint.
  const double span = fmax((double)vmax - (double)vmin, fmax(fabs((double)vmin), fabs((double)vmax)));
  const double bound = (double)s * sqrt((double)n_mels) * span * (K < n_mels ? 1.0 : sqrt(2.0)) + 1.0;
  SS_CHECK_ARG(bound <= 32767.0 && (K < n_mels || (double)K * bound * bound < 2147483648.0),
               "ss_eval_mcep: scale %g over [%g, %g] at %d bins, %d coefficients reaches %.0f: beyond int16 or a squared distance beyond int32 (never truncated)",
               (double)s, (double)vmin, (double)vmax, n_mels, K, bound);
  const int Kp = (K + 1) & ~1;
  const int64_t total = (int64_t)B * T * Kp;
  SS_CHECK_ARG(total / 256 < 0x7FFFFFFF, "ss_eval_mcep: %lld outputs in one launch", (long long)total);
  hipLaunchKernelGGL(eval_mcep_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mel, ldm, mel_bs, lens, tab, q, B, T,
                     n_mels, K, Kp, s, vmin, vmax);
  SS_CHECK_LAUNCH("ss_eval_mcep");
  return SS_OK;
}

extern "C" int64_t ss_eval_dtw_workspace_bytes(int B, int Ta, int Tb, int band) {
  if (!ev_dims_ok(B, Ta, Tb)) return 0;
  return 3 * (int64_t)B * Ta * ev_width(Tb, band);
}

extern "C" int ss_eval_cost_band(const int16_t* qa, const int32_t* lens_a, const int16_t* qb, const int32_t* lens_b, int Kp, int band, int Ta, int Tb,
                                 int B, void* ws, int64_t ws_bytes, void* stream) {
  SS_CHECK_ARG(qa && lens_a && qb && lens_b && ws, "ss_eval_cost_band: null pointer");
  SS_CHECK_ARG(B > 0 && B <= 65535 && Ta > 0 && Tb > 0 && Kp > 0 && Kp % 2 == 0 && Kp <= SS_EVAL_MAX_K, "ss_eval_cost_band: bad dims (B=%d Ta=%d Tb=%d Kp=%d)", B,
               Ta, Tb, Kp);
  SS_CHECK_ARG(Ta <= SS_EVAL_MAX_T && Tb <= SS_EVAL_MAX_T, "ss_eval_cost_band: Ta=%d / Tb=%d beyond the cap %d", Ta, Tb, SS_EVAL_MAX_T);
  SS_CHECK_ARG(((uintptr_t)qa & 3) == 0 && ((uintptr_t)qb & 3) == 0 && ((uintptr_t)ws & 1) == 0, "ss_eval_cost_band: qa / qb need 4-byte, ws 2-byte alignment");
  const int64_t need = ss_eval_dtw_workspace_bytes(B, Ta, Tb, band);
  SS_CHECK_ARG(ws_bytes >= need, "ss_eval_cost_band: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
  const size_t lds = (size_t)2 * EV_TILE * ((Kp / 2) | 1) * 4;
  hipLaunchKernelGGL(eval_cost_kernel, dim3((unsigned)ss_cdiv(Ta, EV_TILE), (unsigned)ss_cdiv(Tb, EV_TILE), (unsigned)B), dim3(EV_COST_THREADS), lds,
                     (hipStream_t)stream, qa, lens_a, qb, lens_b, Kp, band, Ta, Tb, static_cast<uint16_t*>(ws), (int)ev_width(Tb, band));
  SS_CHECK_LAUNCH("ss_eval_cost_band");
  return SS_OK;
}

extern "C" int ss_eval_dtw(const int32_t* lens_a, const int32_t* lens_b, int band, int32_t* path, int32_t* plen, int32_t* cost, int32_t* status, int Ta,
                           int Tb, int B, void* ws, int64_t ws_bytes, void* stream) {
  SS_CHECK_ARG(lens_a && lens_b && path && plen && cost && status && ws, "ss_eval_dtw: null pointer");
  SS_CHECK_ARG(B > 0 && B <= 65535 && Ta > 0 && Tb > 0, "ss_eval_dtw: bad dims (B=%d Ta=%d Tb=%d)", B, Ta, Tb);
  SS_CHECK_ARG(Ta <= SS_EVAL_MAX_T && Tb <= SS_EVAL_MAX_T, "ss_eval_dtw: Ta=%d / Tb=%d beyond the cap %d (the rolling diagonals live in LDS)", Ta, Tb,
               SS_EVAL_MAX_T);
  SS_CHECK_ARG(((uintptr_t)path & 7) == 0 && ((uintptr_t)ws & 1) == 0, "ss_eval_dtw: path needs 8-byte, ws 2-byte alignment");
  const int64_t need = ss_eval_dtw_workspace_bytes(B, Ta, Tb, band);
  SS_CHECK_ARG(ws_bytes >= need, "ss_eval_dtw: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
  const int Wd = (int)ev_width(Tb, band);
  const size_t lds = (size_t)14 * Ta + 2;   // (+ 2: the centres end on an int16; keeps the request even)
  // above the 64 KB a kernel gets without asking for long items; the attribute is per device and cheap, so it is set on every launch
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&eval_dtw_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) {
    ss_set_error("ss_eval_dtw: hipFuncSetAttribute(%d bytes of LDS): %s", (int)lds, hipGetErrorString(e));
    return SS_ERR_HIP;
  }
  unsigned char* base = static_cast<unsigned char*>(ws);
  hipLaunchKernelGGL(eval_dtw_kernel, dim3((unsigned)B), dim3(EV_DTW_THREADS), lds, (hipStream_t)stream, lens_a, lens_b, band, path, plen, cost, status, Ta,
                     Tb, reinterpret_cast<const uint16_t*>(base), base + 2 * (int64_t)B * Ta * Wd, Wd);
  SS_CHECK_LAUNCH("ss_eval_dtw");
  return SS_OK;
}

extern "C" int ss_eval_reduce(const int16_t* qa, const float* f0a, int64_t ldfa, const int32_t* lens_a, const int16_t* qb, const float* f0b, int64_t ldfb,
                              const int32_t* lens_b, int Kp, const int32_t* path, const int32_t* plen, int Ta, int Tb, int B, int64_t* counts,
                              double* sums, void* stream) {
  SS_CHECK_ARG(qa && f0a && lens_a && qb && f0b && lens_b && counts && sums, "ss_eval_reduce: null pointer");
  SS_CHECK_ARG((path == nullptr) == (plen == nullptr), "ss_eval_reduce: path and plen go together (both NULL: the identity path)");
  SS_CHECK_ARG(B > 0 && B <= 65535 && Ta > 0 && Tb > 0 && Kp > 0 && Kp % 2 == 0 && Kp <= SS_EVAL_MAX_K && ldfa >= Ta && ldfb >= Tb,
               "ss_eval_reduce: bad dims (B=%d Ta=%d Tb=%d Kp=%d ldfa=%lld ldfb=%lld)", B, Ta, Tb, Kp, (long long)ldfa, (long long)ldfb);
  SS_CHECK_ARG(Ta <= SS_EVAL_MAX_T && Tb <= SS_EVAL_MAX_T, "ss_eval_reduce: Ta=%d / Tb=%d beyond the cap %d", Ta, Tb, SS_EVAL_MAX_T);
  SS_CHECK_ARG(!path || ((uintptr_t)path & 7) == 0, "ss_eval_reduce: path needs 8-byte alignment");
  hipLaunchKernelGGL(eval_reduce_kernel, dim3((unsigned)B), dim3(EV_RED_THREADS), 0, (hipStream_t)stream, qa, f0a, ldfa, lens_a, qb, f0b, ldfb, lens_b, Kp,
                     path, plen, Ta, Tb, counts, sums);
  SS_CHECK_LAUNCH("ss_eval_reduce");
  return SS_OK;
}

extern "C" int ss_cosine_rows(const float* a, const float* b, float* out, int rows, int C, void* stream) {
  SS_CHECK_ARG(a && b && out, "ss_cosine_rows: null pointer");
  SS_CHECK_ARG(rows > 0 && C > 0, "ss_cosine_rows: bad dims (rows=%d C=%d)", rows, C);
  hipLaunchKernelGGL(cosine_rows_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, a, b, out, C);
  SS_CHECK_LAUNCH("ss_cosine_rows");
  return SS_OK;
}
