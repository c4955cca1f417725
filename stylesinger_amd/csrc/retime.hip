// The score's phones laid out on a guide's frame axis (forward(pitch_hz=..., pitch_timing="guide")): ss_contour_align gave the guide frame under every
// score frame; this turns that path into a new mel2ph of the guide's length, so that the render follows the take's clock instead of the score's. The
// definition is `retime_to_guide` in stylesinger_amd/pitch.py (include/stylesinger_hip.h has the summary): integers only, every output is exact.
//
// One workgroup per item, three steps over chunks of RT_THREADS entries, the running count / maximum carried from chunk to chunk in a register
// (every thread reads all wave totals, so the carry is uniform without a round through LDS):
//   1. anchors: frame i is flagged where the score's pitch changes (i == 0, or Mc[i] != Mc[i-1]); a block-wide exclusive scan of the flags (ballot +
//      popcount inside a wave, the wave totals in LDS) gives every anchor its index k, and a[k] = i goes to LDS;
//   2. guide positions: h_k = idx[a_k] - k, an inclusive block-wide max scan, then the minimum with the pinned end h_m = n_c - m. The scanned
//      sequence does not decrease, so its suffix minimum against the pinned end IS that minimum: no second scan. g_k = h_k + k goes to LDS;
//   3. every guide frame j finds its span by an upper-bound binary search in g (at most 13 LDS reads) and writes mel2ph[src] and src.
// LDS: a and g as uint16 (both are frame numbers <= 8192), 2 x 16 KB, static: nothing depends on the padded sizes. a_m = n_t and g_m = n_c are the
// item's lengths and are not stored. Plain vector stores, no atomics; an item reads and writes nothing of another item, and every index that
// addresses memory is bounded by the item's own clamped lengths whatever idx holds.
#include "common.h"
#include "device_prims.h"
#include "../../include/stylesinger_hip.h"

namespace {

using namespace ss_dev;

constexpr int RT_THREADS = 512;
constexpr int RT_WAVES = RT_THREADS / 64;
constexpr int RT_UNVOICED = -32768;   // cents sentinel of a rest (pitch.ALIGN_UNVOICED)
static_assert(SS_ALIGN_MAX_T <= 65535 && SS_ALIGN_MAX_LC <= 65535, "anchors and guide positions are kept as uint16");
static_assert((2LL * SS_ALIGN_MAX_LC + 1) * SS_ALIGN_MAX_T <= 0x7fffffffLL, "(2 x + 1) s must fit int32");

__device__ __forceinline__ int rt_cents(int64_t m) { return m > 0 ? 100 * (int)(m < 127 ? m : 127) : RT_UNVOICED; }

__global__ __launch_bounds__(RT_THREADS) void retime_mel2ph_kernel(const int64_t* __restrict__ mel2ph, int64_t ldm, const int64_t* __restrict__ midi,
                                                                   int64_t ldn, const int32_t* __restrict__ idx,
                                                                   const int32_t* __restrict__ status_align, const int32_t* __restrict__ lens_t,
                                                                   const int32_t* __restrict__ lens_c, int64_t* __restrict__ out, int64_t ldo,
                                                                   int32_t* __restrict__ src, int32_t* __restrict__ status,
                                                                   int32_t* __restrict__ n_spans, int T, int Lc) {
  __shared__ uint16_t a_s[SS_ALIGN_MAX_T];   // a_k, k < m
  __shared__ uint16_t g_s[SS_ALIGN_MAX_T];   // g_k, k < m
  __shared__ int part[RT_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_t = ss_uniform_len(lens_t, b, T), n_c = ss_uniform_len(lens_c, b, Lc);   // clamped to [0, T] / [0, Lc]
  const int64_t* mp = mel2ph + (int64_t)b * ldm;
  const int64_t* md = midi + (int64_t)b * ldn;
  const int32_t* ix = idx + (int64_t)b * T;
  int64_t* o = out + (int64_t)b * ldo;
  int32_t* so = src + (int64_t)b * Lc;

  // 1. anchors, enumerated in frame order
  int m = 0;
  for (int base = 0; base < n_t; base += RT_THREADS) {
    const int i = base + tid;
    const bool flag = i < n_t && (i == 0 || rt_cents(md[i]) != rt_cents(md[i - 1]));
    int total;
    const int rank = wave_rank(flag, lane, total);
    if (lane == 0) part[wave] = total;
    __syncthreads();
    int off = m;
#pragma unroll
    for (int w = 0; w < RT_WAVES; ++w) {
      const int p = part[w];
      off += w < wave ? p : 0;
      m += p;
    }
    if (flag) a_s[off + rank] = (uint16_t)i;
    __syncthreads();   // the next chunk rewrites part; after the last one a_s is complete
  }

  const bool retimed = status_align[b] == 0 && n_t > 0 && n_c >= m;   // n_c >= m >= 1: not empty either. Uniform: no barrier is skipped
  if (tid == 0) {
    status[b] = retimed ? 0 : 1;
    n_spans[b] = m;
  }
  if (!retimed) {   // one span [0, n_t) -> [0, n_c): the linear stretch; an empty item writes nothing but zeros
    for (int j = tid; j < Lc; j += RT_THREADS) {
      const int s = (j < n_c && n_t > 0) ? ((2 * j + 1) * n_t) / (2 * n_c) : -1;
      o[j] = s >= 0 ? mp[s] : 0;
      so[j] = s;
    }
    return;
  }

  // 2. guide positions with at least one frame per span
  const int top = n_c - m;   // h_m
  int carry = 0;             // h_0 = 0 opens every prefix
  for (int base = 0; base < m; base += RT_THREADS) {
    const int k = base + tid;
    int h = -(1 << 30);
    if (k < m) {
      int j = k == 0 ? 0 : ix[a_s[k]];
      j = j < 0 ? 0 : (j < n_c ? j : n_c - 1);   // what ss_contour_align wrote lies inside already
      h = j - k;
    }
    h = wave_scan_max(h, lane);
    if (lane == 63) part[wave] = h;
    __syncthreads();
    int pre = carry;
#pragma unroll
    for (int w = 0; w < RT_WAVES; ++w) {
      const int p = part[w];
      pre = w < wave ? max(pre, p) : pre;
      carry = max(carry, p);
    }
    h = max(h, pre);
    if (k < m) g_s[k] = (uint16_t)((h < top ? h : top) + k);
    __syncthreads();
  }

  // 3. the map: k = the last span that starts at or before j (g_0 = 0, g strictly increasing)
  for (int j = tid; j < Lc; j += RT_THREADS) {
    int s = -1;
    if (j < n_c) {
      int lo = 0, hi = m;   // g_s[lo] <= j < g_s[hi] (g_m = n_c)
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int)g_s[mid] <= j) lo = mid; else hi = mid;
      }
      const int gk = g_s[lo], ak = a_s[lo];
      const int r = (lo + 1 < m ? (int)g_s[lo + 1] : n_c) - gk, sp = (lo + 1 < m ? (int)a_s[lo + 1] : n_t) - ak;
      s = ak + ((2 * (j - gk) + 1) * sp) / (2 * r);
    }
    o[j] = s >= 0 ? mp[s] : 0;
    so[j] = s;
  }
}

}  // namespace

extern "C" int ss_retime_mel2ph(const int64_t* mel2ph, int64_t ldm, const int64_t* midi, int64_t ldn, const int32_t* idx, const int32_t* status_align,
                                const int32_t* lens_t, const int32_t* lens_c, int64_t* out, int64_t ldo, int32_t* src, int32_t* status,
                                int32_t* n_spans, int T, int Lc, int B, void* stream) {
  SS_CHECK_ARG(mel2ph && midi && idx && status_align && lens_t && lens_c && out && src && status && n_spans, "ss_retime_mel2ph: null pointer");
  SS_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && Lc > 0 && ldm >= T && ldn >= T && ldo >= Lc,
               "ss_retime_mel2ph: bad dims (B=%d T=%d Lc=%d ldm=%lld ldn=%lld ldo=%lld)", B, T, Lc, (long long)ldm, (long long)ldn, (long long)ldo);
  SS_CHECK_ARG(T <= SS_ALIGN_MAX_T && Lc <= SS_ALIGN_MAX_LC, "ss_retime_mel2ph: T=%d / Lc=%d beyond the caps %d / %d (anchors and guide positions live in LDS)",
               T, Lc, SS_ALIGN_MAX_T, SS_ALIGN_MAX_LC);
  SS_CHECK_ARG(mel2ph != out, "ss_retime_mel2ph: input and output must not alias");
  hipLaunchKernelGGL(retime_mel2ph_kernel, dim3((unsigned)B), dim3(RT_THREADS), 0, (hipStream_t)stream, mel2ph, ldm, midi, ldn, idx, status_align, lens_t,
                     lens_c, out, ldo, src, status, n_spans, T, Lc);
  SS_CHECK_LAUNCH("ss_retime_mel2ph");
  return SS_OK;
}
