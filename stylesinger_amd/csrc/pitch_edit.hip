// Pitch expression controls (forward(pitch_correct=, vibrato_scale=, vibrato_add=)): an edit of the merged log2-f0 between the pitch tail
// (ss_pitch_post / ss_pitch_given) and pitch_embed. The definition is `pitch_edit` in stylesinger_amd/pitch.py (float64; include/stylesinger_hip.h
// has the summary): a Hann moving average over each frame's sung neighbourhood splits the contour into a trend m and what rides on it, x - m; the
// result is m pulled toward the equally averaged score notes, the rest scaled, and an optional synthetic vibrato on held notes.
//
//   ss_pitch_edit_runs  one workgroup per item. Held-run bounds per frame: a frame opens a run where the key (min(midi, 127), 0 = rest or past the
//                       item) differs from its left neighbour's, so run_lo is an inclusive max scan of (opens ? t : -1) and run_hi a suffix min scan of
//                       (closes ? t + 1 : INT_MAX). Chunks of PR_THREADS frames, forward then backward, the carry in a register (every thread reads
//                       all wave totals, so it is uniform without a round through LDS). Any T.
//   ss_pitch_edit       ceil(T / TILE) x B workgroups of TILE threads, one frame per thread. The tile and its W halo of x (cents), c (note cents) and
//                       the sung flags are staged in LDS together with the 2 W + 1 weights; a thread walks the flags outward from its frame to find
//                       where its window leaves the region (at most W steps each way), then adds the three sums in ascending k in float64 with the
//                       product and the sum rounded separately, exactly as the definition does. One rounding to fp32 at the end.
//                       LDS: 2 x 766 doubles + 766 flag bytes + 511 weights = 17 KB static, whatever W is. The work is ~2 (2 W + 1) float64
//                       multiply-adds per frame: at W = 31 and 32 x 5625 frames 23 MFLOP over 704 workgroups - the launch is latency, not rate.
//   statistics          every tile reduces its six values in a fixed order (xor butterfly inside a wave, then the waves in ascending order) into
//                       stats_partial; pitch_edit_stats_kernel (one wave per item) adds the tiles in ascending order. No atomics.
// Nothing at or past lens[b] enters a result: those frames are staged as rests, and the only thing written there is f_out = f_in.
#include "common.h"
#include "device_prims.h"
#include "../../include/stylesinger_hip.h"

namespace {

using namespace ss_dev;

constexpr int PE_TILE = SS_PITCH_EDIT_TILE;
constexpr int PE_MAX_W = SS_PITCH_EDIT_MAX_W;
constexpr int PE_SPAN = PE_TILE + 2 * PE_MAX_W;
constexpr int PE_WAVES = PE_TILE / 64;
constexpr int PE_NSTAT = 6;
constexpr int PR_THREADS = 512;
constexpr int PR_WAVES = PR_THREADS / 64;
constexpr int PR_NONE = 0x7fffffff;
static_assert(PE_TILE % 64 == 0, "a tile is whole waves");

// the key of a frame: min(midi, 127) on sung frames of the item, 0 on rests and at or past the item's end
__device__ __forceinline__ int pe_key(const int64_t* __restrict__ md, int t, int n) {
  if (t < 0 || t >= n) return 0;
  const int64_t m = md[t];
  return m > 0 ? (int)(m < 127 ? m : 127) : 0;
}

__global__ __launch_bounds__(PR_THREADS) void pitch_edit_runs_kernel(const int64_t* __restrict__ midi, int64_t ldm, const int32_t* __restrict__ lens,
                                                                    int32_t* __restrict__ run_lo, int32_t* __restrict__ run_hi, int T) {
  __shared__ int part[PR_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = ss_uniform_len(lens, b, T);
  const int64_t* md = midi + (int64_t)b * ldm;
  int32_t* lo = run_lo + (int64_t)b * T;
  int32_t* hi = run_hi + (int64_t)b * T;
  const int n_chunks = (T + PR_THREADS - 1) / PR_THREADS;

  int carry = -1;   // forward: the last run start at or before the chunk
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int t = ch * PR_THREADS + tid;
    const int key = pe_key(md, t, n);
    int v = (t < T && (t == 0 || key != pe_key(md, t - 1, n))) ? t : -1;
    v = wave_scan_max(v, lane);
    if (lane == 63) part[wave] = v;
    __syncthreads();
    int pre = carry;
#pragma unroll
    for (int w = 0; w < PR_WAVES; ++w) {
      const int p = part[w];
      pre = w < wave ? max(pre, p) : pre;
      carry = max(carry, p);
    }
    if (t < T) lo[t] = key > 0 ? max(v, pre) : -1;
    __syncthreads();   // the next chunk rewrites part
  }

  carry = PR_NONE;   // backward: the first run end after the chunk
  for (int ch = n_chunks - 1; ch >= 0; --ch) {
    const int t = ch * PR_THREADS + tid;
    const int key = pe_key(md, t, n);
    int v = (t < T && (t == T - 1 || key != pe_key(md, t + 1, n))) ? t + 1 : PR_NONE;
    v = wave_scan_min_down(v, lane);
    if (lane == 0) part[wave] = v;
    __syncthreads();
    int post = carry;
#pragma unroll
    for (int w = 0; w < PR_WAVES; ++w) {
      const int p = part[w];
      post = w > wave ? min(post, p) : post;
      carry = min(carry, p);
    }
    if (t < T) hi[t] = key > 0 ? min(v, post) : -1;
    __syncthreads();
  }
}

__global__ __launch_bounds__(PE_TILE) void pitch_edit_kernel(const float* __restrict__ f_in, int64_t ld, const int64_t* __restrict__ midi, int64_t ldm,
                                                            const float* __restrict__ u, const int32_t* __restrict__ lens,
                                                            const int32_t* __restrict__ run_lo, const int32_t* __restrict__ run_hi,
                                                            const double* __restrict__ wtab, int W, double K0, double alpha, double kappa,
                                                            double vib_depth, double vib_omega, int vib_delay, int vib_fade,
                                                            float* __restrict__ f_out, double* __restrict__ stats_partial, int T) {
#pragma clang fp contract(off)
  __shared__ double x_s[PE_SPAN];
  __shared__ double c_s[PE_SPAN];
  __shared__ double w_s[2 * PE_MAX_W + 1];
  __shared__ double red[PE_WAVES][PE_NSTAT];
  __shared__ uint8_t sung_s[PE_SPAN];
  const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = ss_uniform_len(lens, b, T);
  const int t0 = tile * PE_TILE;
  const float* fi = f_in + (int64_t)b * ld;
  const int64_t* md = midi + (int64_t)b * ldm;

  for (int i = tid; i < PE_TILE + 2 * W; i += PE_TILE) {
    const int t = t0 - W + i;
    const int key = pe_key(md, t, n);
    sung_s[i] = key > 0;
    x_s[i] = key > 0 ? 1200.0 * (double)fi[t] : 0.0;
    c_s[i] = K0 + 100.0 * (double)(key - 69);
  }
  for (int i = tid; i < 2 * W + 1; i += PE_TILE) w_s[i] = wtab[i];
  __syncthreads();

  const int t = t0 + tid, i = tid + W;
  double cnt = 0.0, d2 = 0.0, dm = 0.0, dabs = 0.0, dmax = 0.0, cs = 0.0;
  if (t < T) {
    float o = fi[t];   // frames at or past lens[b] and rests: the input's bits
    if (sung_s[i]) {
      int l = 0, r = 0;   // how far the window reaches before it leaves the region
      while (l < W && sung_s[i - l - 1]) ++l;
      while (r < W && sung_s[i + r + 1]) ++r;
      double sx = 0.0, sc = 0.0, sw = 0.0;
      for (int k = -l; k <= r; ++k) {
        const double wk = w_s[k + W];
        sx = sx + wk * x_s[i + k];
        sc = sc + wk * c_s[i + k];
        sw = sw + wk;
      }
      const double x = x_s[i], m = sx / sw, nbar = sc / sw;
      double s = 0.0;
      if (vib_depth > 0.0) {
        const int a = run_lo[(int64_t)b * T + t], e = run_hi[(int64_t)b * T + t];
        const int on = a + vib_delay;
        if (a >= 0 && (int64_t)e - a >= (int64_t)vib_delay + 2 * (int64_t)vib_fade && t >= on) {
          const double up = fmin(1.0, (double)(t - on + 1) / (double)vib_fade), down = fmin(1.0, (double)(e - t) / (double)vib_fade);
          s = vib_depth * up * down * sin((double)(t - on) * vib_omega);
        }
      }
      const double xe = ((m + alpha * (nbar - m)) + kappa * (x - m)) + s;
      o = (float)(xe / 1200.0);
      dmax = fabs(xe - x);
      if (!(u[(int64_t)b * ld + t] > 0.0f)) {
        const double d = x - m, q = m - nbar;
        cnt = 1.0;
        d2 = d * d;
        dm = q;
        dabs = fabs(q);
        cs = s != 0.0 ? 1.0 : 0.0;
      }
    }
    f_out[(int64_t)b * ld + t] = o;
  }

  cnt = wave_sum(cnt);
  d2 = wave_sum(d2);
  dm = wave_sum(dm);
  dabs = wave_sum(dabs);
  cs = wave_sum(cs);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) dmax = fmax(dmax, __shfl_xor(dmax, s));
  if (lane == 0) {
    red[wave][0] = cnt; red[wave][1] = d2; red[wave][2] = dm; red[wave][3] = dabs; red[wave][4] = dmax; red[wave][5] = cs;
  }
  __syncthreads();
  if (tid < PE_NSTAT) {
    double v = red[0][tid];
    for (int w = 1; w < PE_WAVES; ++w) v = tid == 4 ? fmax(v, red[w][tid]) : v + red[w][tid];
    stats_partial[((int64_t)b * gridDim.x + tile) * PE_NSTAT + tid] = v;
  }
}

// one wave per item: lane j < 6 adds value j of the item's tiles in ascending tile order
__global__ __launch_bounds__(64) void pitch_edit_stats_kernel(const double* __restrict__ stats_partial, double* __restrict__ stats, int n_tiles) {
  const int b = blockIdx.x, j = threadIdx.x;
  double v = 0.0;
  if (j < PE_NSTAT) {
    const double* p = stats_partial + (int64_t)b * n_tiles * PE_NSTAT + j;
    for (int k = 0; k < n_tiles; ++k) v = j == 4 ? fmax(v, p[(int64_t)k * PE_NSTAT]) : v + p[(int64_t)k * PE_NSTAT];
  }
  const double cnt = __shfl(v, 0);
  if (j < PE_NSTAT) {
    double o = v;
    if (j == 1) o = cnt > 0.0 ? sqrt(v / cnt) : 0.0;
    if (j == 2 || j == 3) o = cnt > 0.0 ? v / cnt : 0.0;
    stats[(int64_t)b * PE_NSTAT + j] = o;
  }
}

}  // namespace

extern "C" int ss_pitch_edit_runs(const int64_t* midi, int64_t ldm, const int32_t* lens, int32_t* run_lo, int32_t* run_hi, int T, int B, void* stream) {
  SS_CHECK_ARG(midi && run_lo && run_hi, "ss_pitch_edit_runs: null pointer");
  SS_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && T < PR_NONE - PR_THREADS && ldm >= T, "ss_pitch_edit_runs: bad dims (B=%d T=%d ldm=%lld)", B, T, (long long)ldm);
  hipLaunchKernelGGL(pitch_edit_runs_kernel, dim3((unsigned)B), dim3(PR_THREADS), 0, (hipStream_t)stream, midi, ldm, lens, run_lo, run_hi, T);
  SS_CHECK_LAUNCH("ss_pitch_edit_runs");
  return SS_OK;
}

extern "C" int ss_pitch_edit(const float* f_in, int64_t ld, const int64_t* midi, int64_t ldm, const float* u, const int32_t* lens, const int32_t* run_lo,
                             const int32_t* run_hi, const double* w, int W, double K0, double alpha, double kappa, double vib_depth, double vib_omega,
                             int vib_delay, int vib_fade, float* f_out, double* stats_partial, double* stats, int T, int B, void* stream) {
  SS_CHECK_ARG(f_in && midi && u && w && f_out && stats_partial && stats, "ss_pitch_edit: null pointer");
  SS_CHECK_ARG(W >= 1 && W <= SS_PITCH_EDIT_MAX_W, "ss_pitch_edit: W=%d outside [1, %d] (the halo lives in LDS; a wider window is refused, not truncated)", W,
               SS_PITCH_EDIT_MAX_W);
  SS_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && T < PR_NONE - PE_SPAN && ld >= T && ldm >= T, "ss_pitch_edit: bad dims (B=%d T=%d ld=%lld ldm=%lld)", B, T,
               (long long)ld, (long long)ldm);
  SS_CHECK_ARG(f_in != f_out, "ss_pitch_edit: f_out must not alias f_in (a tile reads its neighbours' frames)");
  SS_CHECK_ARG(alpha >= 0.0 && alpha <= 1.0 && kappa >= 0.0, "ss_pitch_edit: alpha=%g outside [0, 1] or kappa=%g < 0", alpha, kappa);
  SS_CHECK_ARG(vib_depth >= 0.0 && (vib_depth == 0.0 || (run_lo && run_hi && vib_delay >= 0 && vib_fade >= 1)),
               "ss_pitch_edit: a synthetic vibrato (depth %g) needs run_lo / run_hi, delay=%d >= 0 and fade=%d >= 1", vib_depth, vib_delay, vib_fade);
  const int n_tiles = ss_cdiv(T, PE_TILE);
  hipLaunchKernelGGL(pitch_edit_kernel, dim3((unsigned)n_tiles, (unsigned)B), dim3(PE_TILE), 0, (hipStream_t)stream, f_in, ld, midi, ldm, u, lens, run_lo,
                     run_hi, w, W, K0, alpha, kappa, vib_depth, vib_omega, vib_delay, vib_fade, f_out, stats_partial, T);
  SS_CHECK_LAUNCH("ss_pitch_edit");
  hipLaunchKernelGGL(pitch_edit_stats_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, (const double*)stats_partial, stats, n_tiles);
  SS_CHECK_LAUNCH("ss_pitch_edit (statistics)");
  return SS_OK;
}
