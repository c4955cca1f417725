// A guide vocal's pitch contour warped onto the score's per-frame notes by dynamic time warping (forward(pitch_hz=..., pitch_align="dtw")). The
// linear fit of pitch_fit.hip is right for a contour that already has the score's timing; a sung guide does not, and once it holds one note a little
// longer every later note lands on the wrong phones. The definition is `contour_align` in stylesinger_amd/pitch.py (include/stylesinger_hip.h has
// the summary): integer cents, integer costs, so idx / cost / status are exact and out is one fp32 product.
//
// One workgroup per item. The band |j - c_i| <= W of the (score frame i, guide frame j) matrix is swept by anti-diagonals d = i + j: the cells of a
// diagonal depend on the two diagonals before it only, so D lives in three rolling diagonals in LDS, indexed by the row i (cell (i, d - i) of
// diagonal d in slot i), with ONE workgroup barrier per diagonal: diagonal d writes the buffer diagonal d - 3 had, and reads d - 1 and d - 2.
// D never reaches memory. What does is the chosen predecessor of every band cell, one byte, at ws[(d mod Wd) * T + i] with
// Wd = min(Lc, 2 band + 1) >= the cells of any row: a row's cells lie on consecutive diagonals, so d mod Wd names them uniquely, and the rows of
// one diagonal are neighbours in memory (a wavefront stores 64 consecutive bytes). Then one lane walks the path back (at most n_t + n_c dependent
// byte loads) and all lanes gather out. Plain vector stores, no atomics; an item reads and writes nothing of another item.
//
// LDS: 3 x T int32 (D) + T int16 (c_i) + T int16 (score cents) + Lc int16 (guide cents) = 16 T + 2 Lc bytes; T = Lc = 8192 takes 144 KB of the
// CU's 160 KB. The rows active on diagonal d are a contiguous range (i + c_i grows strictly with i); every lane derives a superset [a, b] of it in
// closed form and tests its own row exactly.
#include "common.h"
#include "pitch_fit.h"
#include "../../include/stylesinger_hip.h"

namespace {

constexpr int CA_THREADS = 512;
constexpr int CA_INF = 0x3FFFFFFF;     // D of a cell no path reaches (pitch.ALIGN_INF)
constexpr int CA_UNVOICED = -32768;    // cents sentinel: unvoiced guide frame / rest (pitch.ALIGN_UNVOICED)
constexpr int CA_MAX_COST = 1200;      // upper limit of the cap / uv_cost arguments
constexpr int CA_MAX_LDS = 160 * 1024;
// int32 D cannot overflow: a path has fewer than SS_ALIGN_MAX_T + SS_ALIGN_MAX_LC cells of at most CA_MAX_COST each: 16384 * 1200 = 19 660 800
static_assert((long long)(SS_ALIGN_MAX_T + SS_ALIGN_MAX_LC) * CA_MAX_COST < CA_INF, "D overflows int32");
static_assert(CA_INF + CA_MAX_COST > 0, "INF + a cost must stay positive");
static_assert(16 * SS_ALIGN_MAX_T + 2 * SS_ALIGN_MAX_LC <= CA_MAX_LDS, "the caps must fit the CU's LDS");
static_assert(SS_ALIGN_MAX_T <= 32767 && SS_ALIGN_MAX_LC <= 32767, "band centres are kept as int16");

__device__ __forceinline__ int ca_guide_cents(float g, float shift100) {
#pragma clang fp contract(off)
  if (!(g > 0.f)) return CA_UNVOICED;
  const float r = g / 440.f;
  const float a = 1200.f * log2f(r);
  float x = a + shift100;
  x = fminf(fmaxf(x, -8900.f), 9100.f);   // cents in [-2000, 16000]: further than the cap from every note either way (also +inf)
  return 6900 + (int)rintf(x);
}

__global__ __launch_bounds__(CA_THREADS) void contour_align_kernel(const float* __restrict__ f0_hz, int64_t ldc, int Lc, const int32_t* __restrict__ lens_c,
                                                                   const int64_t* __restrict__ midi, int64_t ldm, const int32_t* __restrict__ lens_t,
                                                                   int band, int uv_cost, int cap, float shift100, float scale,
                                                                   float* __restrict__ out, int64_t ldo, int32_t* __restrict__ idx,
                                                                   int32_t* __restrict__ cost, int32_t* __restrict__ status, int T,
                                                                   unsigned char* __restrict__ ws, int Wd) {
  extern __shared__ __align__(16) unsigned char ca_smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n_c = ss_uniform_len(lens_c, b, Lc), n_t = ss_uniform_len(lens_t, b, T);   // clamped to [0, Lc] / [0, T]
  const float* g = f0_hz + (int64_t)b * ldc;
  const int64_t* m = midi + (int64_t)b * ldm;
  float* o = out + (int64_t)b * ldo;
  int32_t* ix = idx + (int64_t)b * T;
  const int full = n_t > n_c ? n_t : n_c;
  const int W = (band <= 0 || band > full) ? full : band;   // a band wider than the matrix is the full matrix
  if (n_t == 0 || n_c == 0 || (int64_t)n_c > (int64_t)W * n_t) {   // not aligned: the linear fit (uniform per workgroup: no barrier is skipped)
    for (int t = tid; t < T; t += CA_THREADS) {
      o[t] = (t < n_t && n_c > 0) ? ss_contour_fit_frame(g, n_c, n_t, t, scale) : 0.f;
      ix[t] = -1;
    }
    if (tid == 0) {
      cost[b] = 0;
      status[b] = 1;
    }
    return;
  }
  int32_t* D = reinterpret_cast<int32_t*>(ca_smem);                 // [3][T]
  int16_t* ci = reinterpret_cast<int16_t*>(ca_smem + (size_t)12 * T);   // [T] band centres
  int16_t* Mc = ci + T;                                             // [T] score cents
  int16_t* Gc = Mc + T;                                             // [Lc] guide cents
  for (int i = tid; i < n_t; i += CA_THREADS) {
    ci[i] = (int16_t)(((2 * (int64_t)i + 1) * n_c) / (2 * (int64_t)n_t));
    const int64_t mi = m[i];
    Mc[i] = (int16_t)(mi > 0 ? 100 * (int)(mi < 127 ? mi : 127) : CA_UNVOICED);
  }
  for (int j = tid; j < n_c; j += CA_THREADS) Gc[j] = (int16_t)ca_guide_cents(g[j], shift100);
  __syncthreads();

  unsigned char* wsb = ws + (int64_t)b * Wd * T;
  const int n_diag = n_t + n_c - 1;
  const int den = 2 * (n_t + n_c);
  int slot = 0;                                                      // d mod Wd
  for (int d = 0; d < n_diag; ++d) {
    int32_t* cur = D + (size_t)(d % 3) * T;
    const int32_t* p1 = D + (size_t)((d + 2) % 3) * T;               // diagonal d - 1
    const int32_t* p2 = D + (size_t)((d + 1) % 3) * T;               // diagonal d - 2
    // rows of this diagonal: 0 <= d - i < n_c, and inside the band d - W <= i + c_i <= d + W with (2i+1) n_c / (2 n_t) - 1 < c_i <= (2i+1) n_c / (2 n_t):
    //   i >= ((d - W) 2 n_t - n_c) / den and i < ((d + W + 1) 2 n_t - n_c) / den; one row of slack on both sides, the lane's own test is exact.
    // (d + W + 1) 2 n_t <= 24577 * 16384: int32 holds it. A negative numerator truncates to 0 where floor gives < 0: both clamp to the first row.
    int a = ((d - W) * 2 * n_t - n_c) / den - 1;
    int e = ((d + W + 1) * 2 * n_t - n_c) / den + 1;
    const int rmin = d - (n_c - 1) > 0 ? d - (n_c - 1) : 0, rmax = d < n_t - 1 ? d : n_t - 1;
    a = a > rmin ? a : rmin;
    e = e < rmax ? e : rmax;
    for (int i = a + tid; i <= e; i += CA_THREADS) {
      const int j = d - i, i1 = i > 0 ? i - 1 : 0;
      // every LDS operand up front, whether or not the cell or its predecessors exist: one round of LDS latency per diagonal instead of a chain of
      // three (band centre -> cents -> predecessors). All addresses are inside the arrays; what a cell outside the band holds is masked below.
      const int c_i = ci[i], c_1 = ci[i1];
      const int gc = Gc[j], mc = Mc[i];
      const int v_up = p1[i1], v_dg = p2[i1], v_lf = p1[i];
      asm volatile("" ::"v"(c_1), "v"(gc), "v"(mc), "v"(v_up), "v"(v_dg), "v"(v_lf));   // keeps the loads here: the compiler sinks them below the band test
      const int lo = c_i - W > 0 ? c_i - W : 0, hi = c_i + W < n_c - 1 ? c_i + W : n_c - 1;
      if (j < lo || j > hi) continue;
      const bool gv = gc != CA_UNVOICED, mv = mc != CA_UNVOICED;
      int c = 0;
      if (gv && mv) {
        const int df = gc > mc ? gc - mc : mc - gc;
        c = df < cap ? df : cap;
      } else if (gv != mv) {
        c = uv_cost;
      }
      int best = 0, dir = 0;                                         // d == 0, the start cell: D = c(0, 0)
      if (d > 0) {
        const int lo1 = c_1 - W > 0 ? c_1 - W : 0, hi1 = c_1 + W < n_c - 1 ? c_1 + W : n_c - 1;
        const int up = (i >= 1 && j >= lo1 && j <= hi1) ? v_up : CA_INF;
        const int dg = (i >= 1 && j - 1 >= lo1 && j - 1 <= hi1) ? v_dg : CA_INF;
        const int lf = j - 1 >= lo ? v_lf : CA_INF;
        best = up;                                                   // the first minimum in the order up, left, diagonal
        if (lf < best) { best = lf; dir = 1; }
        if (dg < best) { best = dg; dir = 2; }
      }
      cur[i] = best >= CA_INF ? CA_INF : best + c;
      wsb[(int64_t)slot * T + i] = (unsigned char)dir;
    }
    slot = slot + 1 == Wd ? 0 : slot + 1;
    __syncthreads();
  }

  // the walk back: one lane, one dependent byte load per step. The direction bytes were stored by this workgroup's own lanes before the barrier.
  __threadfence_block();
  int32_t* path = D + (size_t)(n_diag % 3) * T;                      // the buffer the last diagonal did not use: smallest j per row
  if (tid == 0) {
    const int total = D[(size_t)((n_diag - 1) % 3) * T + (n_t - 1)];
    int i = n_t - 1, j = n_c - 1;
    int s = (n_diag - 1) % Wd;
    while (true) {
      path[i] = j;                                                   // j only falls along the walk: a row's last write is its smallest j
      if (i == 0 && j == 0) break;
      const int dir = wsb[(int64_t)s * T + i];
      if (dir == 1 && j > 0) {
        --j; s = s == 0 ? Wd - 1 : s - 1;
      } else if (dir == 0 && i > 0) {
        --i; s = s == 0 ? Wd - 1 : s - 1;
      } else if (i > 0 && j > 0) {
        --i; --j; s = s == 0 ? Wd - 1 : s - 1; s = s == 0 ? Wd - 1 : s - 1;
      } else {
        break;                                                       // cannot happen on a connected band; never walk out of the matrix
      }
    }
    cost[b] = total;
    status[b] = 0;
  }
  __syncthreads();
  for (int t = tid; t < T; t += CA_THREADS) {
    float v = 0.f;
    int j = -1;
    if (t < n_t) {
      j = path[t];
      j = j < 0 ? 0 : (j < n_c ? j : n_c - 1);   // the walk visits every row, so this changes nothing; a load must never leave the item's row
      const float gj = g[j];
      v = gj > 0.f ? gj * scale : 0.f;
    }
    o[t] = v;
    ix[t] = j;
  }
}

int64_t ca_width(int Lc, int band) {   // direction bytes per row of an item
  if (band <= 0) return Lc;
  const int64_t w = 2 * (int64_t)band + 1;
  return w < Lc ? w : Lc;
}

bool ca_dims_ok(int B, int T, int Lc) { return B > 0 && B <= 65535 && T > 0 && Lc > 0 && T <= SS_ALIGN_MAX_T && Lc <= SS_ALIGN_MAX_LC; }

}  // namespace

extern "C" int64_t ss_contour_align_workspace_bytes(int B, int T, int Lc, int band) {
  if (!ca_dims_ok(B, T, Lc)) return 0;
  return (int64_t)B * T * ca_width(Lc, band);
}

extern "C" int ss_contour_align(const float* f0_hz, int64_t ldc, int Lc, const int32_t* lens_c, const int64_t* midi, int64_t ldm, const int32_t* lens_t,
                                int band, int uv_cost, int cap, float shift_semitones, float* out, int64_t ldo, int32_t* idx, int32_t* cost,
                                int32_t* status, int T, int B, void* ws, int64_t ws_bytes, void* stream) {
  SS_CHECK_ARG(f0_hz && lens_c && midi && lens_t && out && idx && cost && status && ws, "ss_contour_align: null pointer");
  SS_CHECK_ARG(B > 0 && B <= 65535 && Lc > 0 && T > 0 && ldc >= Lc && ldm >= T && ldo >= T,
               "ss_contour_align: bad dims (B=%d Lc=%d T=%d ldc=%lld ldm=%lld ldo=%lld)", B, Lc, T, (long long)ldc, (long long)ldm, (long long)ldo);
  SS_CHECK_ARG(T <= SS_ALIGN_MAX_T && Lc <= SS_ALIGN_MAX_LC, "ss_contour_align: T=%d / Lc=%d beyond the caps %d / %d (the rolling diagonals live in LDS)",
               T, Lc, SS_ALIGN_MAX_T, SS_ALIGN_MAX_LC);
  SS_CHECK_ARG(uv_cost >= 0 && uv_cost <= CA_MAX_COST && cap >= 0 && cap <= CA_MAX_COST, "ss_contour_align: uv_cost=%d / cap=%d outside [0, %d]", uv_cost,
               cap, CA_MAX_COST);
  SS_CHECK_ARG(shift_semitones >= -48.f && shift_semitones <= 48.f, "ss_contour_align: shift of %g semitones outside +-48", (double)shift_semitones);
  SS_CHECK_ARG(f0_hz != out, "ss_contour_align: input and output must not alias");
  const int64_t need = ss_contour_align_workspace_bytes(B, T, Lc, band);
  SS_CHECK_ARG(ws_bytes >= need, "ss_contour_align: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
  const float scale = (float)exp2((double)shift_semitones / 12.0);   // shift 0 -> exactly 1 (as ss_contour_fit)
  const float shift100 = 100.f * shift_semitones;
  const size_t lds = (size_t)16 * T + (size_t)2 * Lc;
  // above the 64 KB a kernel gets without asking for long items; the attribute is per device and cheap, so it is set on every launch
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&contour_align_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) {
    ss_set_error("ss_contour_align: hipFuncSetAttribute(%d bytes of LDS): %s", (int)lds, hipGetErrorString(e));
    return SS_ERR_HIP;
  }
  hipLaunchKernelGGL(contour_align_kernel, dim3((unsigned)B), dim3(CA_THREADS), lds, (hipStream_t)stream, f0_hz, ldc, Lc, lens_c, midi, ldm, lens_t, band,
                     uv_cost, cap, shift100, scale, out, ldo, idx, cost, status, T, static_cast<unsigned char*>(ws), (int)ca_width(Lc, band));
  SS_CHECK_LAUNCH("ss_contour_align");
  return SS_OK;
}
