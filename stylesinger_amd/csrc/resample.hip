// Sample-rate conversion of the reference audio on the device (input producer of `preprocess_input`): the polyphase form of the windowed-sinc
// interpolation that `librosa.core.load(path, sr=audio_sample_rate)` applies to a file of another rate (utils/audios/__init__.py:52; resampy's
// `kaiser_best`, un-vendored: parity UNPINNED - the definition, the table and the bank builder are stylesinger_amd/resample.py).
//
// Output t of an item sits at input position t * down / up = n + p / up. The bank row of phase p holds the weights of inputs n - left .. n - left +
// taps - 1, so   y[t] = sum_j bank[p][j] * xz[n - left + j],   xz zero outside the item.
//
// Lane mapping: the lanes of a wave SHARE A PHASE. A workgroup owns G * up consecutive outputs of one item (G periods of the phase pattern) and
// stages the G * down + taps inputs they touch into LDS, zero-filled outside [0, n_in). A work unit is (r, c): offset r < up inside the period,
// lane l of the unit computes the output of period g = 64 c + l. All 64 outputs of a unit have phase p = r * down mod up, so the weight is
// wave-uniform (scalar loads of the bank row, no vector memory traffic for it, no transposed copy of the bank) and the inner loop is one LDS read +
// one FMA per tap. Lane g reads LDS word g * down + (r * down) / up + j: a stride of `down` words between lanes. ds_read_b32 banks are
// (word mod 32) within a 32-lane half (MI355X_MICROARCH.md, LDS): an odd `down` (1, 3, 147: every standard rate up to 48 kHz, and 48 -> 16 kHz)
// is conflict-free, an even one is gcd(down, 32)-way (2: 96 -> 48 kHz runs its LDS reads at half rate).
// The stores of a unit are `up` floats apart; they are 1 / taps of the inner loop's work and merge in L2.
#include "common.h"
#include "../../include/stylesinger_hip.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_LDS_FLOATS = 16384;    // 64 KiB of dynamic LDS at most
constexpr int RS_TILE_OUTPUTS = 4096;   // outputs per workgroup aimed at (the staged wings are then a few % of the staged span)

typedef const __attribute__((address_space(4))) float* rs_const_ptr;

__global__ __launch_bounds__(RS_THREADS) void resample_poly_kernel(const float* __restrict__ x, int64_t ldx, int Lx, const int32_t* __restrict__ n_in,
                                                                   float* __restrict__ y, int64_t ldy, int Ly,
                                                                   const int32_t* __restrict__ n_out_computed, const int32_t* __restrict__ n_out,
                                                                   const float* __restrict__ bank, int up, int down, int taps, int left, int G) {
  extern __shared__ __attribute__((aligned(16))) float rs_x[];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t T0 = (int64_t)blockIdx.x * G * up;   // first output of this workgroup: a multiple of up, so it has phase 0
  const int64_t Tend = T0 + (int64_t)G * up < Ly ? T0 + (int64_t)G * up : Ly;
  int nc = ss_uniform_len(n_out_computed, b, Ly);
  if (n_out) nc = min(nc, ss_uniform_len(n_out, b, Ly));
  const int ni = ss_uniform_len(n_in, b, Lx);
  float* yb = y + (int64_t)b * ldy;
  for (int64_t t = (T0 > nc ? T0 : (int64_t)nc) + tid; t < Tend; t += RS_THREADS) yb[t] = 0.f;
  if (nc <= T0) return;
  // inputs (T0 / up) * down - left ... of the item, zero outside it
  const int span = (G - 1) * down + (int)(((int64_t)(up - 1) * down) / up) + taps;
  const int64_t N0 = (int64_t)blockIdx.x * G * down - left;
  const float* xb = x + (int64_t)b * ldx;
  for (int i = tid; i < span; i += RS_THREADS) {
    const int64_t s = N0 + i;
    rs_x[i] = (s >= 0 && s < ni) ? xb[s] : 0.f;
  }
  __syncthreads();
  const int C = (G + 63) >> 6, units = up * C;
  const int lane = tid & 63;
  for (int u = __builtin_amdgcn_readfirstlane(tid >> 6); u < units; u += RS_THREADS / 64) {
    const int r = u / C, g = (u - r * C) * 64 + lane;
    const int q = r * down, off = q / up, p = q - off * up;   // wave-uniform; r * down < 2^26
    const int64_t t = T0 + (int64_t)g * up + r;
    if (g < G && t < nc) {
      const rs_const_ptr w = reinterpret_cast<rs_const_ptr>(reinterpret_cast<uintptr_t>(bank + (int64_t)p * taps));
      const float* xp = rs_x + g * down + off;   // + taps - 1 <= span - 1
      float acc = 0.f;
      int j = 0;
      for (; j + 8 <= taps; j += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) acc = __builtin_fmaf(w[j + k], xp[j + k], acc);
      }
      for (; j < taps; ++j) acc = __builtin_fmaf(w[j], xp[j], acc);
      yb[t] = acc;
    }
  }
}

}  // namespace

extern "C" int ss_resample_poly(const float* x, int64_t ldx, int Lx, const int32_t* n_in, float* y, int64_t ldy, int Ly, const int32_t* n_out_computed,
                                const int32_t* n_out, int B, const float* bank, int up, int down, int taps, int left, void* stream) {
  SS_CHECK_ARG(x && n_in && y && n_out_computed && bank, "ss_resample_poly: null argument");
  SS_CHECK_ARG(B > 0 && B <= 65535 && Lx > 0 && Ly > 0 && ldx >= Lx && ldy >= Ly, "ss_resample_poly: bad dims (B=%d Lx=%d Ly=%d ldx=%lld ldy=%lld)", B, Lx,
               Ly, (long long)ldx, (long long)ldy);
  SS_CHECK_ARG(up >= 1 && up <= 4096 && down >= 1 && taps >= 1 && left >= 0 && left < taps, "ss_resample_poly: bad filter (up=%d down=%d taps=%d left=%d)",
               up, down, taps, left);
  SS_CHECK_ARG((int64_t)down + taps <= 16000, "ss_resample_poly: down + taps = %lld exceeds 16000 (the staged input span must fit 64 KiB of LDS)",
               (long long)down + taps);
  SS_CHECK_ARG(x != y, "ss_resample_poly: input and output must not alias");
  // periods per workgroup: ~RS_TILE_OUTPUTS outputs in whole waves of periods, fewer where the staged span G * down + taps would not fit
  int G = ((RS_TILE_OUTPUTS + up - 1) / up + 63) / 64 * 64;
  const int g_max = (RS_LDS_FLOATS - taps) / down;   // span < G * down + taps
  if (G > g_max) G = g_max >= 64 ? g_max / 64 * 64 : g_max;
  SS_CHECK_ARG(G >= 1, "ss_resample_poly: filter too long for one workgroup (down=%d taps=%d)", down, taps);
  const int64_t tile = (int64_t)G * up;
  const int64_t tiles = (Ly + tile - 1) / tile;
  const size_t lds = ((size_t)G * down + taps) * sizeof(float);
  hipLaunchKernelGGL(resample_poly_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(RS_THREADS), lds, (hipStream_t)stream, x, ldx, Lx, n_in, y, ldy, Ly,
                     n_out_computed, n_out, bank, up, down, taps, left, G);
  SS_CHECK_LAUNCH("resample_poly_kernel");
  return SS_OK;
}
