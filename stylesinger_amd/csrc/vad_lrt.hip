// A voice-activity decision on the device for ss_vad_trim's flags (vad_flags="lrt"): a per-window likelihood-ratio test in the maximum-likelihood
// form of Sohn, Kim & Sung (1999) against a noise spectrum taken from the item's own quietest windows. The definition is `lrt_statistic` in
// stylesinger_amd/vadtrim.py (float64 numpy), which also passes every constant; this is NOT webrtcvad's decision and claims no parity with it.
//
// Float64 throughout: a decision sits on a threshold, and the work is trivial (1000 windows of 512 points for a 30 s item). TWO launches:
//   (a) vl_spectrum_kernel, grid (windows / 4, B), 256 threads: ONE WAVE PER WINDOW. The wave quantises its window to 16-bit PCM values, multiplies by
//       the table's window, zero-pads to n_fft and runs a radix-2 transform in its own LDS slab (decimation in frequency, natural order in, bit-reversed
//       order out; the imaginary input is zero - the transform is a small fraction of a launch that is bound by its latency). P[w][k] = |X[k]|^2 for
//       the bins k_lo .. k_hi goes to the workspace (128 doubles per window), E[w] = their sum, added by one lane in ascending k, behind them.
//   (b) vl_decide_kernel, one workgroup of 1024 threads per item: E in LDS; rank[w] = number of v with E[v] < E[w], or equal and v < w, by counting;
//       the q windows of smallest rank as a list in ascending window index; N[k] = their mean, one thread per bin adding in list order; one thread
//       adds sum_k N[k] in ascending k; the peak rule and the floor; then one thread per window adds its statistic in ascending k.
// No atomics, every sum in the order the definition states, every window transformed by the same instruction sequence whatever its position:
// an item's row is bit-identical from run to run and does not depend on B, wav_stride, the other items or what the row holds beyond n_samples[b]
// (windows are whole: no sample at or beyond floor(n / spw) * spw is read).
#include "common.h"
#include "../../include/stylesinger_hip.h"

namespace {

constexpr int VL_WAVES = 4, VL_THREADS_A = 64 * VL_WAVES, VL_THREADS_B = 1024;
constexpr int VL_MAX_BINS = 128, VL_SLOT = VL_MAX_BINS + 1;   // workspace doubles per window: P[128], E
constexpr int VL_MAX_WINDOWS = 4096, VL_MAX_FFT = 1024, VL_MIN_FFT = 64;

__device__ __forceinline__ int vl_windows(const int32_t* n_, int b, int64_t wav_stride, int spw, int max_windows) {
  const int cap = wav_stride < (int64_t)0x7fffffff ? (int)wav_stride : 0x7fffffff;
  const int nw = ss_uniform_len(n_, b, cap) / spw;
  return nw < max_windows ? nw : max_windows;
}

__global__ __launch_bounds__(VL_THREADS_A) void vl_spectrum_kernel(const float* __restrict__ wav, int64_t wav_stride, const int32_t* __restrict__ n_,
                                                                   int max_windows, int spw, int n_fft, int logn, int k_lo, int nbins,
                                                                   const double* __restrict__ tab, double* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char vl_lds[];
  const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nw = vl_windows(n_, b, wav_stride, spw, max_windows);
  if ((int)blockIdx.x * VL_WAVES >= nw) return;                      // uniform over the workgroup: before any barrier
  const int w = blockIdx.x * VL_WAVES + wave;
  const bool live = w < nw;                                          // a wave beyond the item's last window transforms zeros and writes nothing
  double2* buf = reinterpret_cast<double2*>(vl_lds) + (size_t)wave * n_fft;
  const double2* tw = reinterpret_cast<const double2*>(tab);         // [s + j] = W_{2s}^j
  const double* win = tab + 2 * (size_t)n_fft;
  const float* x = wav + (int64_t)b * wav_stride + (int64_t)w * spw;
  for (int j = lane; j < n_fft; j += 64) {
    double2 z;
    z.x = 0.0; z.y = 0.0;
    if (live && j < spw) {
      double p = rint((double)x[j] * 32767.0);                       // exact product (24 + 15 bits), ties to even: np.rint
      p = p < -32768.0 ? -32768.0 : (p > 32767.0 ? 32767.0 : p);
      z.x = p * win[j];
    }
    buf[j] = z;
  }
  __syncthreads();
  const int half = n_fft >> 1;
  for (int s = half; s >= 1; s >>= 1) {
    for (int t = lane; t < half; t += 64) {
      const int j = t & (s - 1), base = ((t - j) << 1) + j;
      const double2 a = buf[base], c = buf[base + s], wj = tw[s + j];
      double2 u, d, r;
      u.x = a.x + c.x; u.y = a.y + c.y;
      d.x = a.x - c.x; d.y = a.y - c.y;
      r.x = d.x * wj.x - d.y * wj.y;
      r.y = d.x * wj.y + d.y * wj.x;
      buf[base] = u;
      buf[base + s] = r;
    }
    __syncthreads();
  }
  double pk[VL_MAX_BINS / 64];
#pragma unroll
  for (int i = 0; i < VL_MAX_BINS / 64; ++i) {
    const int bin = lane + 64 * i;
    pk[i] = 0.0;
    if (bin < nbins) {
      const double2 z = buf[__brev((unsigned)(k_lo + bin)) >> (32 - logn)];
      pk[i] = z.x * z.x + z.y * z.y;
    }
  }
  __syncthreads();
  double* pbuf = reinterpret_cast<double*>(buf);                     // the wave's slab again: its bins in natural order
  double* out = ws + ((int64_t)b * max_windows + w) * VL_SLOT;
#pragma unroll
  for (int i = 0; i < VL_MAX_BINS / 64; ++i) {
    const int bin = lane + 64 * i;
    if (bin < nbins) {
      pbuf[bin] = pk[i];
      if (live) out[bin] = pk[i];
    }
  }
  __syncthreads();
  if (live && lane == 0) {
    double e = 0.0;
    for (int i = 0; i < nbins; ++i) e += pbuf[i];                    // ascending k
    out[VL_MAX_BINS] = e;
  }
}

__global__ __launch_bounds__(VL_THREADS_B) void vl_decide_kernel(const int32_t* __restrict__ n_, int64_t wav_stride, int max_windows, int spw, int nbins,
                                                                 int q_div, double peak_ratio, double n_min, double eta, const double* __restrict__ ws,
                                                                 uint8_t* __restrict__ flags, int flags_stride, double* __restrict__ stat,
                                                                 int stat_stride) {
  extern __shared__ __attribute__((aligned(16))) unsigned char vl_lds[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nw = vl_windows(n_, b, wav_stride, spw, max_windows);
  uint8_t* fb = flags + (int64_t)b * flags_stride;
  double* sb = stat ? stat + (int64_t)b * stat_stride : nullptr;
  if (nw == 0) {
    for (int w = tid; w < max_windows; w += VL_THREADS_B) {
      fb[w] = 0;
      if (sb) sb[w] = 0.0;
    }
    return;
  }
  double* E = reinterpret_cast<double*>(vl_lds);                     // [max_windows]
  double* red = E + max_windows;                                     // [VL_THREADS_B]
  double* N = red + VL_THREADS_B;                                    // [VL_MAX_BINS]
  double* sc = N + VL_MAX_BINS;                                      // [2]: the peak rule's factor, (as an integer) the number of listed windows
  int* list = reinterpret_cast<int*>(sc + 2);                        // [max_windows]
  uint8_t* sel = reinterpret_cast<uint8_t*>(list + max_windows);     // [max_windows]
  const double* wsb = ws + (int64_t)b * max_windows * VL_SLOT;
  double emax = 0.0;                                                 // E >= 0
  for (int w = tid; w < nw; w += VL_THREADS_B) {
    const double e = wsb[(int64_t)w * VL_SLOT + VL_MAX_BINS];
    E[w] = e;
    emax = e > emax ? e : emax;
  }
  red[tid] = emax;
  __syncthreads();
  for (int s = VL_THREADS_B >> 1; s >= 1; s >>= 1) {                 // a maximum: the order does not matter
    if (tid < s) red[tid] = red[tid + s] > red[tid] ? red[tid + s] : red[tid];
    __syncthreads();
  }
  const int q = (nw + q_div - 1) / q_div;                            // >= 1: nw >= 1
  for (int w = tid; w < nw; w += VL_THREADS_B) {
    const double e = E[w];
    int r = 0;
    for (int v = 0; v < nw; ++v) {
      const double ev = E[v];
      r += (ev < e || (ev == e && v < w)) ? 1 : 0;
    }
    sel[w] = r < q ? 1 : 0;
  }
  __syncthreads();
  for (int w = tid; w < nw; w += VL_THREADS_B) {
    int pos = 0;
    for (int v = 0; v < w; ++v) pos += sel[v];
    if (sel[w]) list[pos] = w;                                       // pos < number of selected windows <= nw
    if (w == nw - 1) reinterpret_cast<int*>(sc + 1)[0] = pos + sel[w];   // q for finite E; counted, so that the list is never read past its end
  }
  __syncthreads();
  const int nsel = reinterpret_cast<const int*>(sc + 1)[0];
  for (int i = tid; i < nbins; i += VL_THREADS_B) {
    double a = 0.0;
    for (int j = 0; j < nsel; ++j) a += wsb[(int64_t)list[j] * VL_SLOT + i];   // ascending window index
    N[i] = a / (double)nsel;
  }
  __syncthreads();
  if (tid == 0) {
    double nsum = 0.0;
    for (int i = 0; i < nbins; ++i) nsum += N[i];                    // ascending k
    const double thr = red[0] * peak_ratio;
    sc[0] = nsum > thr ? thr / nsum : 1.0;
  }
  __syncthreads();
  const double f = sc[0];
  __syncthreads();
  for (int i = tid; i < nbins; i += VL_THREADS_B) {
    const double v = N[i] * f;                                       // f = 1: unchanged
    N[i] = v > n_min ? v : n_min;
  }
  __syncthreads();
  for (int w = tid; w < max_windows; w += VL_THREADS_B) {
    double s = 0.0;
    if (w < nw) {
      const double* pw = wsb + (int64_t)w * VL_SLOT;
      for (int i = 0; i < nbins; ++i) {                              // ascending k
        const double g = pw[i] / N[i];
        if (g > 1.0) s += (g - log(g)) - 1.0;
      }
      s = s / (double)nbins;
    }
    fb[w] = (w < nw && s > eta) ? 1 : 0;
    if (sb) sb[w] = s;
  }
}

bool vl_dims_ok(int B, int max_windows) { return B > 0 && B <= 65535 && max_windows > 0 && max_windows <= VL_MAX_WINDOWS; }

}  // namespace

extern "C" int64_t ss_vad_lrt_workspace_bytes(int B, int max_windows) {
  if (!vl_dims_ok(B, max_windows)) return 0;
  return (int64_t)B * max_windows * VL_SLOT * (int64_t)sizeof(double);
}

extern "C" int ss_vad_lrt(const float* wav, int64_t wav_stride, const int32_t* n_samples, int B, int max_windows, int samples_per_window, int n_fft,
                          int k_lo, int k_hi, int q_div, double peak_db, double n_min, double eta, const double* table, uint8_t* flags,
                          int flags_stride, double* stat, int stat_stride, void* ws, int64_t ws_bytes, void* stream) {
  SS_CHECK_ARG(wav && n_samples && table && flags && ws, "ss_vad_lrt: null argument");
  SS_CHECK_ARG(vl_dims_ok(B, max_windows), "ss_vad_lrt: bad dims (B=%d in [1, 65535], max_windows=%d in [1, %d])", B, max_windows, VL_MAX_WINDOWS);
  SS_CHECK_ARG(n_fft >= VL_MIN_FFT && n_fft <= VL_MAX_FFT && (n_fft & (n_fft - 1)) == 0, "ss_vad_lrt: bad n_fft (%d: a power of two in [%d, %d])", n_fft,
               VL_MIN_FFT, VL_MAX_FFT);
  SS_CHECK_ARG(samples_per_window >= 1 && samples_per_window <= n_fft, "ss_vad_lrt: n_fft = %d is smaller than samples_per_window = %d (or that is < 1)",
               n_fft, samples_per_window);
  SS_CHECK_ARG(k_lo >= 0 && k_lo <= k_hi && k_hi < n_fft / 2 + 1, "ss_vad_lrt: bad bin range (k_lo=%d, k_hi=%d: 0 <= k_lo <= k_hi <= n_fft / 2 = %d)", k_lo,
               k_hi, n_fft / 2);
  SS_CHECK_ARG(k_hi - k_lo + 1 <= VL_MAX_BINS, "ss_vad_lrt: %d bins, at most %d", k_hi - k_lo + 1, VL_MAX_BINS);
  SS_CHECK_ARG(q_div >= 1, "ss_vad_lrt: bad q_div (%d: at least 1)", q_div);
  SS_CHECK_ARG(peak_db == peak_db && n_min > 0.0 && n_min <= 1.0e300 && eta == eta, "ss_vad_lrt: bad constants (peak_db=%g, n_min=%g > 0, eta=%g)", peak_db,
               n_min, eta);
  // (a wav row may be shorter than max_windows windows: lengths are clamped to wav_stride, so no window reaches past its row)
  SS_CHECK_ARG(wav_stride >= 0 && flags_stride >= max_windows && (!stat || stat_stride >= max_windows),
               "ss_vad_lrt: bad strides (wav_stride=%lld >= 0; flags_stride=%d, stat_stride=%d: at least max_windows = %d)", (long long)wav_stride,
               flags_stride, stat_stride, max_windows);
  const int64_t need = ss_vad_lrt_workspace_bytes(B, max_windows);
  SS_CHECK_ARG(ws_bytes >= need, "ss_vad_lrt: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
  SS_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0 && (reinterpret_cast<uintptr_t>(table) & 15) == 0 && (!stat || (reinterpret_cast<uintptr_t>(stat) & 7) == 0),
               "ss_vad_lrt: misaligned workspace / stat (8 bytes) or table (16 bytes)");
  int logn = 0;
  while ((1 << logn) < n_fft) ++logn;
  const int nbins = k_hi - k_lo + 1;
  const double peak_ratio = pow(10.0, -peak_db / 10.0);
  hipStream_t st = (hipStream_t)stream;
  const size_t lds_a = (size_t)VL_WAVES * n_fft * sizeof(double2);                                    // <= 64 KiB at n_fft = 1024
  hipLaunchKernelGGL(vl_spectrum_kernel, dim3((unsigned)((max_windows + VL_WAVES - 1) / VL_WAVES), (unsigned)B), dim3(VL_THREADS_A), lds_a, st, wav,
                     wav_stride, n_samples, max_windows, samples_per_window, n_fft, logn, k_lo, nbins, table, static_cast<double*>(ws));
  SS_CHECK_LAUNCH("vl_spectrum_kernel");
  const size_t lds_b = (size_t)(max_windows + VL_THREADS_B + VL_MAX_BINS + 2) * sizeof(double) + (size_t)max_windows * (sizeof(int) + 1);   // <= 62 KiB
  hipLaunchKernelGGL(vl_decide_kernel, dim3((unsigned)B), dim3(VL_THREADS_B), lds_b, st, n_samples, wav_stride, max_windows, samples_per_window, nbins,
                     q_div, peak_ratio, n_min, eta, static_cast<const double*>(ws), flags, flags_stride, stat, stat_stride);
  SS_CHECK_LAUNCH("vl_decide_kernel");
  return SS_OK;
}
