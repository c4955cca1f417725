// Vocoder output denoise (tasks/tts/vocoder_infer/hifigan_nsf.py:14-22, 73-74: `denoise(wav_out, v=hparams['vocoder_denoise_c'])`): spectral
// subtraction between librosa 0.8's stft(center=True, pad_mode='constant') and istft(center=True) - un-vendored: parity UNPINNED, the definition is
// stylesinger_amd/denoise.py, restated in float64 by tests/denoise_ref.py.
//
// ONE launch, no workspace. A workgroup owns a run of TS output samples of one item (a whole number of hops; 4 N, 3 N at N = 2048) and computes
// every frame that reaches into it, halo frames included: frame i covers the padded positions [i H, i H + N), the run covers
// [O0 + N/2, O0 + TS + N/2). Per frame pair, all in LDS:
//   load + window + first radix-2 step (decimation in frequency, natural order in)  ->  log2 N - 1 DIF steps (bit-reversed order out), two at a
//   time as radix-4 butterflies  ->  the subtraction Y = X (m - v) / (m N) in place  ->  log2 N - 1 steps of the inverse (decimation in time with
//   conjugate twiddles, natural order out), grouped the same way  ->  last step, window, added to the run's accumulator in LDS.
// TWO consecutive frames share one N-point complex transform (real frames, so: frame i in the real part, frame i + 1 in the imaginary part; the
// two Hermitian spectra are separated from bins k and N - k for the subtraction and recombined, and the inverse returns the two frames in its real
// and imaginary part). The recombined spectra are Hermitian by construction with real bins 0 and N / 2: irfft's reading of the bins 0 .. N / 2.
// A frame's rounding depends on the frame it is paired with (at the level of fp32 rounding of the pair), and pairs are formed from the run's first
// frame on: fixed by the position in the item alone.
// Frames are added in ascending order, every accumulator slot has one writer per frame, and the run an output sample falls into depends on its
// position in the item only: results are bit-identical from run to run and do not depend on B, Lx, Ly or the other items. No atomics.
// Twiddles and window come from the caller's table (float64 on the host, rounded once for the fp32 kernel): the twiddles per step, W_{2s}^j at
// [s + j], so that a step reads consecutive entries (staged into LDS by the fp32 kernel: a step then waits for LDS only). N is a template
// argument: the butterfly loops unroll and a step's LDS reads are issued together.
// With H == N the envelope is w^2 alone and falls to 0 at every frame edge: the division by it amplifies the transform's rounding error by 1 / w
// (6.6e3 at k = 1, N = 256), which fp32 cannot carry inside 1e-5. That geometry runs the same kernel in float64 (T = double); every H < N has an
// envelope >= 0.5 (H = N / 2) or larger and runs in fp32.
#include "common.h"
#include "../../include/stylesinger_hip.h"

namespace {

constexpr int DN_THREADS = 256;

template <typename T> struct dn_vec2;
template <> struct dn_vec2<float> { typedef float2 type; };
template <> struct dn_vec2<double> { typedef double2 type; };

template <typename T2> __device__ __forceinline__ T2 dn_add(const T2& a, const T2& b) { T2 r; r.x = a.x + b.x; r.y = a.y + b.y; return r; }
template <typename T2> __device__ __forceinline__ T2 dn_sub(const T2& a, const T2& b) { T2 r; r.x = a.x - b.x; r.y = a.y - b.y; return r; }
// a * w and a * conj(w)
template <typename T2> __device__ __forceinline__ T2 dn_mul(const T2& a, const T2& w) { T2 r; r.x = a.x * w.x - a.y * w.y; r.y = a.x * w.y + a.y * w.x; return r; }
template <typename T2> __device__ __forceinline__ T2 dn_mulc(const T2& a, const T2& w) { T2 r; r.x = a.x * w.x + a.y * w.y; r.y = a.y * w.x - a.x * w.y; return r; }
// Y = X * (m - v) / (m N) where m = |X| > v, else 0 (m = 0 gives 0, not NaN: 0 > v is false for every v >= 0)
template <typename T, typename T2> __device__ __forceinline__ T2 dn_subtract(const T2& a, T v, T inv_n) {
  const T m = sqrt(a.x * a.x + a.y * a.y);
  const T s = m > v ? (m - v) / m * inv_n : (T)0;
  T2 r; r.x = a.x * s; r.y = a.y * s;
  return r;
}

// outputs per workgroup: a multiple of every hop (H | N). fp32: LDS = frame 8 N + run 4 TS + twiddles 8 N <= 56 KiB; float64 (H == N): the run is one
// hop, the twiddles stay in global memory, LDS = 16 N + 8 N
template <typename T, int N> constexpr int dn_run() { return sizeof(T) == 8 ? N : (N == 2048 ? 3 * N : 4 * N); }

template <typename T, int N>
__global__ __launch_bounds__(DN_THREADS) void wav_denoise_kernel(const float* __restrict__ x, int64_t ldx, int Lx, const int32_t* __restrict__ n_,
                                                                 float* __restrict__ y, int64_t ldy, int Ly, int32_t* __restrict__ n_out, int H, T v,
                                                                 const T* __restrict__ tab) {
  typedef typename dn_vec2<T>::type T2;
  constexpr int half = N >> 1, TS = dn_run<T, N>(), LOGN = N == 256 ? 8 : N == 512 ? 9 : N == 1024 ? 10 : 11;
  static_assert(N == 1 << LOGN, "N: 256, 512, 1024 or 2048");
  constexpr bool DN_ODD_STEPS = ((LOGN - 1) & 1) != 0;   // steps between the fused first / last one and the subtraction: log2 N - 1 per direction
  constexpr bool TW_LDS = sizeof(T) == 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char dn_lds[];
  T2* buf = reinterpret_cast<T2*>(dn_lds);       // N complex: the frame
  T* acc = reinterpret_cast<T*>(buf + N);        // TS: the run's overlap-added samples
  T2* tw_lds = reinterpret_cast<T2*>(acc + TS);  // N twiddles (fp32 only)
  const T2* tw_glb = reinterpret_cast<const T2*>(tab);   // [s + j] = W_{2s}^j for s = 1, 2, ..., N / 2 and j < s
  const T* win = tab + 2 * N;                            // N window values
  auto tw = [&](int k) -> T2 {
    if constexpr (TW_LDS) return tw_lds[k];
    else return tw_glb[k];
  };
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = ss_uniform_len(n_, b, Lx);
  const int nout = n / H * H, F = n / H + 1;
  if (blockIdx.x == 0 && tid == 0) n_out[b] = nout;
  const int64_t O0 = (int64_t)blockIdx.x * TS;                       // first output sample of the run
  const int64_t O1 = O0 + TS < Ly ? O0 + TS : Ly;
  float* yb = y + (int64_t)b * ldy;
  if (O0 >= nout) {
    for (int64_t o = O0 + tid; o < O1; o += DN_THREADS) yb[o] = 0.f;
    return;
  }
  const float* xb = x + (int64_t)b * ldx;
  for (int j = tid; j < TS; j += DN_THREADS) acc[j] = (T)0;   // (ordered before its first use by the barriers of the first frame)
  if constexpr (TW_LDS) {
    for (int j = tid; j < N; j += DN_THREADS) tw_lds[j] = tw_glb[j];
    __syncthreads();
  }
  const int64_t P0 = O0 + half;                                      // the run in padded positions: [P0, P0 + span)
  const int span = (int)((O0 + TS < nout ? O0 + TS : (int64_t)nout) - O0);
  const int i_lo = O0 >= half ? (int)((O0 - half) / H) + 1 : 0;      // first frame with i H + N > P0
  const int i_top = (int)((P0 + span - 1) / H);                      // last frame with i H < P0 + span
  const int i_hi = i_top < F - 1 ? i_top : F - 1;
  const T inv_n = (T)1 / (T)N;
  for (int i = i_lo; i <= i_hi; i += 2) {                            // frames i (real part) and i + 1 (imaginary part) share one transform
    const bool two = i + 1 <= i_hi;
    const int64_t S0 = (int64_t)i * H - half;                        // the item's sample under k = 0 of frame i
#pragma unroll
    for (int t = tid; t < half; t += DN_THREADS) {                   // load, window, DIF step of span N / 2
      const T w0 = win[t], w1 = win[t + half];
      const int64_t s0 = S0 + t, s1 = s0 + half, u0 = s0 + H, u1 = s1 + H;
      T2 z0, z1;
      z0.x = (s0 >= 0 && s0 < n) ? (T)xb[s0] * w0 : (T)0;
      z1.x = (s1 >= 0 && s1 < n) ? (T)xb[s1] * w1 : (T)0;
      z0.y = (two && u0 >= 0 && u0 < n) ? (T)xb[u0] * w0 : (T)0;
      z1.y = (two && u1 >= 0 && u1 < n) ? (T)xb[u1] * w1 : (T)0;
      buf[t] = dn_add(z0, z1);
      buf[t + half] = dn_mul(dn_sub(z0, z1), tw(half + t));
    }
    __syncthreads();
    // DIF steps of span half / 2 ... 1: two at a time as one radix-4 butterfly on four register-resident points (spans s and s / 2: the same
    // twiddles W_{2s}^j, W_{2s}^{j + s/2}, W_s^j and the same slots as the two radix-2 steps), a radix-2 step of span 1 where their number is odd
#pragma unroll
    for (int s = half >> 1; s >= 2; s >>= 2) {
      const int h = s >> 1;
#pragma unroll
      for (int t = tid; t < (N >> 2); t += DN_THREADS) {
        const int j = t & (h - 1), base = ((t - j) << 2) + j;
        const T2 e0 = buf[base], e1 = buf[base + h], e2 = buf[base + s], e3 = buf[base + s + h];
        const T2 a0 = dn_add(e0, e2), a2 = dn_mul(dn_sub(e0, e2), tw(s + j));
        const T2 a1 = dn_add(e1, e3), a3 = dn_mul(dn_sub(e1, e3), tw(s + j + h));
        buf[base] = dn_add(a0, a1);
        buf[base + s] = dn_add(a2, a3);
        if (h > 1) {
          const T2 w = tw(h + j);
          buf[base + h] = dn_mul(dn_sub(a0, a1), w);
          buf[base + s + h] = dn_mul(dn_sub(a2, a3), w);
        } else {
          buf[base + h] = dn_sub(a0, a1);
          buf[base + s + h] = dn_sub(a2, a3);
        }
      }
      __syncthreads();
    }
    if constexpr (DN_ODD_STEPS) {
#pragma unroll
      for (int t = tid; t < half; t += DN_THREADS) {
        const T2 a = buf[2 * t], c = buf[2 * t + 1];
        buf[2 * t] = dn_add(a, c);
        buf[2 * t + 1] = dn_sub(a, c);
      }
      __syncthreads();
    }
    // bin k sits at slot bitrev(k). Z = A + i B with A, B the two frames' Hermitian spectra: A[k] = (Z[k] + conj Z[N - k]) / 2,
    // B[k] = (Z[k] - conj Z[N - k]) / 2i. Both are scaled by their own magnitudes and put back as Y[k] = A' + i B', Y[N - k] = conj A' + i conj B':
    // the two scaled spectra stay exactly Hermitian (bins 0 and N / 2 real), so the inverse returns the frames in its real and imaginary part
    auto point = [&](int k) {
      const int kp = (N - k) & (N - 1);
      const int sk = (int)(__brev((unsigned)k) >> (32 - LOGN)), sp = (int)(__brev((unsigned)kp) >> (32 - LOGN));
      const T2 zk = buf[sk], zp = buf[sp];
      T2 A, B;
      A.x = (T)0.5 * (zk.x + zp.x); A.y = (T)0.5 * (zk.y - zp.y);
      B.x = (T)0.5 * (zk.y + zp.y); B.y = (T)0.5 * (zp.x - zk.x);
      A = dn_subtract<T, T2>(A, v, inv_n);
      B = dn_subtract<T, T2>(B, v, inv_n);
      T2 yk, yp;
      yk.x = A.x - B.y; yk.y = A.y + B.x;
      yp.x = A.x + B.y; yp.y = B.x - A.y;
      buf[sk] = yk;
      if (kp != k) buf[sp] = yp;
    };
    // thread t takes the bin at slot 2 t (the even slots hold the bins k < N / 2, each once): consecutive lanes read consecutive even slots and,
    // for the partner N - k, nearly consecutive ones - bins taken in natural order would sit N / 64 slots apart, 32 lanes to a bank pair
#pragma unroll
    for (int t = tid; t < half; t += DN_THREADS) {
      point((int)(__brev((unsigned)(2 * t)) >> (32 - LOGN)));
      if (t == 0) point(half);
    }
    __syncthreads();
    // the inverse: DIT steps of span 1 ... half / 2 with conjugate twiddles, in the mirrored grouping
    if constexpr (DN_ODD_STEPS) {
#pragma unroll
      for (int t = tid; t < half; t += DN_THREADS) {
        const T2 a = buf[2 * t], c = buf[2 * t + 1];
        buf[2 * t] = dn_add(a, c);
        buf[2 * t + 1] = dn_sub(a, c);
      }
      __syncthreads();
    }
#pragma unroll
    for (int s = DN_ODD_STEPS ? 4 : 2; s < half; s <<= 2) {          // spans s / 2, then s
      const int h = s >> 1;
#pragma unroll
      for (int t = tid; t < (N >> 2); t += DN_THREADS) {
        const int j = t & (h - 1), base = ((t - j) << 2) + j;
        const T2 e0 = buf[base], e2 = buf[base + s];
        T2 c1 = buf[base + h], c3 = buf[base + s + h];
        if (h > 1) {
          const T2 w = tw(h + j);
          c1 = dn_mulc(c1, w);
          c3 = dn_mulc(c3, w);
        }
        const T2 a0 = dn_add(e0, c1), a1 = dn_sub(e0, c1), a2 = dn_add(e2, c3), a3 = dn_sub(e2, c3);
        const T2 d2 = dn_mulc(a2, tw(s + j)), d3 = dn_mulc(a3, tw(s + j + h));
        buf[base] = dn_add(a0, d2);
        buf[base + s] = dn_sub(a0, d2);
        buf[base + h] = dn_add(a1, d3);
        buf[base + s + h] = dn_sub(a1, d3);
      }
      __syncthreads();
    }
    const int64_t rel = (int64_t)i * H - P0;                         // accumulator slot of k = 0 of frame i (may be negative or beyond the run)
    T2 r0[(half + DN_THREADS - 1) / DN_THREADS], r1[(half + DN_THREADS - 1) / DN_THREADS];
#pragma unroll
    for (int t = tid, q = 0; t < half; t += DN_THREADS, ++q) {       // span N / 2, window, overlap-add of frame i
      const T2 a = buf[t], c = dn_mulc(buf[t + half], tw(half + t));
      const T w0 = win[t], w1 = win[t + half];
      r0[q] = dn_add(a, c);
      r1[q] = dn_sub(a, c);
      r0[q].x *= w0; r0[q].y *= w0;
      r1[q].x *= w1; r1[q].y *= w1;
      const int64_t p0 = rel + t, p1 = p0 + half;
      if (p0 >= 0 && p0 < span) acc[p0] += r0[q].x;
      if (p1 >= 0 && p1 < span) acc[p1] += r1[q].x;
    }
    __syncthreads();                                                 // frame i + 1 after frame i: ascending order in every slot
    if (two) {
#pragma unroll
      for (int t = tid, q = 0; t < half; t += DN_THREADS, ++q) {
        const int64_t p0 = rel + H + t, p1 = p0 + half;
        if (p0 >= 0 && p0 < span) acc[p0] += r0[q].y;
        if (p1 >= 0 && p1 < span) acc[p1] += r1[q].y;
      }
    }
    __syncthreads();
  }
  for (int j = tid; O0 + j < O1; j += DN_THREADS) {
    float out = 0.f;
    if (j < span) {
      const int64_t p = P0 + j;
      const int ia = p >= N ? (int)((p - N) / H) + 1 : 0;
      const int ib = (int)(p / H) < F - 1 ? (int)(p / H) : F - 1;
      T e = (T)0;                                                    // the envelope: sum of w^2 over the frames that cover p, ascending
      for (int i = ia; i <= ib; ++i) {
        const T w = win[p - (int64_t)i * H];
        e += w * w;
      }
      const T a = acc[j];
      out = (float)(e > (T)1.17549435e-38f ? a / e : a);
    }
    yb[O0 + j] = out;
  }
}

template <typename T, int N>
void dn_launch(const float* x, int64_t ldx, int Lx, const int32_t* n, float* y, int64_t ldy, int Ly, int32_t* n_out, int B, int hop, T v, const T* tab,
               hipStream_t stream) {
  constexpr int TS = dn_run<T, N>();
  const size_t lds = (size_t)N * 2 * sizeof(T) + (size_t)TS * sizeof(T) + (sizeof(T) == 4 ? (size_t)N * 2 * sizeof(T) : 0);
  const dim3 grid((unsigned)(((int64_t)Ly + TS - 1) / TS), (unsigned)B);
  hipLaunchKernelGGL((wav_denoise_kernel<T, N>), grid, dim3(DN_THREADS), lds, stream, x, ldx, Lx, n, y, ldy, Ly, n_out, hop, v, tab);
}

bool dn_geometry_ok(int n_fft, int hop) {
  return n_fft >= 256 && n_fft <= 2048 && (n_fft & (n_fft - 1)) == 0 && hop >= 64 && hop <= n_fft && n_fft % hop == 0;
}

}  // namespace

extern "C" int64_t ss_wav_denoise_workspace_bytes(int B, int Lx, int n_fft, int hop) {
  if (B <= 0 || Lx <= 0 || !dn_geometry_ok(n_fft, hop)) return -1;
  return 0;   // the overlap-add lives in LDS
}

extern "C" int ss_wav_denoise(const float* x, int64_t ldx, int Lx, const int32_t* n, float* y, int64_t ldy, int Ly, int32_t* n_out, int B, int n_fft,
                              int hop, float v, const double* table, void* ws, int64_t ws_bytes, void* stream) {
  (void)ws;
  SS_CHECK_ARG(x && n && y && n_out && table, "ss_wav_denoise: null argument");
  SS_CHECK_ARG(n_fft >= 256 && n_fft <= 2048 && (n_fft & (n_fft - 1)) == 0, "ss_wav_denoise: bad fft_size (%d: a power of two in [256, 2048])", n_fft);
  SS_CHECK_ARG(hop >= 64 && hop <= n_fft && n_fft % hop == 0, "ss_wav_denoise: bad hop_size (%d: a divisor of fft_size = %d, at least 64)", hop, n_fft);
  SS_CHECK_ARG(B > 0 && B <= 65535 && Lx > 0 && Ly > 0 && ldx >= Lx && ldy >= Ly, "ss_wav_denoise: bad dims (B=%d Lx=%d Ly=%d ldx=%lld ldy=%lld)", B, Lx, Ly,
               (long long)ldx, (long long)ldy);
  SS_CHECK_ARG(Ly >= Lx / hop * hop, "ss_wav_denoise: Ly = %d is shorter than the longest possible output (%d samples)", Ly, Lx / hop * hop);
  SS_CHECK_ARG(v == v && v >= 0.f && v <= 3.0e38f, "ss_wav_denoise: bad v (%g: finite and >= 0)", (double)v);
  SS_CHECK_ARG(ws_bytes >= ss_wav_denoise_workspace_bytes(B, Lx, n_fft, hop), "ss_wav_denoise: workspace of %lld bytes, need %lld", (long long)ws_bytes,
               (long long)ss_wav_denoise_workspace_bytes(B, Lx, n_fft, hop));
  {   // the rows' byte ranges must be disjoint, not merely start at different addresses
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(x), x1 = x0 + ((uint64_t)(B - 1) * (uint64_t)ldx + (uint64_t)Lx) * sizeof(float);
    const uintptr_t y0 = reinterpret_cast<uintptr_t>(y), y1 = y0 + ((uint64_t)(B - 1) * (uint64_t)ldy + (uint64_t)Ly) * sizeof(float);
    SS_CHECK_ARG(x1 <= y0 || y1 <= x0, "ss_wav_denoise: input and output must not alias (their row ranges overlap)");
  }
  hipStream_t st = (hipStream_t)stream;
  const float* tab32 = reinterpret_cast<const float*>(table + 3 * (size_t)n_fft);
#define DN_CASE(N)                                                                                                     \
  case N:                                                                                                              \
    if (hop == n_fft) dn_launch<double, N>(x, ldx, Lx, n, y, ldy, Ly, n_out, B, hop, (double)v, table, st);            \
    else dn_launch<float, N>(x, ldx, Lx, n, y, ldy, Ly, n_out, B, hop, v, tab32, st);                                  \
    break;
  switch (n_fft) {
    DN_CASE(256)
    DN_CASE(512)
    DN_CASE(1024)
    DN_CASE(2048)
  }
#undef DN_CASE
  SS_CHECK_LAUNCH("wav_denoise_kernel");
  return SS_OK;
}
