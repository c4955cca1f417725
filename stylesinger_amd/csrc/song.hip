// A whole song from separately rendered segments (StyleSingerInfer.sing_score): the segments of a score are rendered as rows of ordinary batches, in
// an order chosen for batching, and are put on ONE timeline here, on the device. The frame count of a segment is a device value (durations are the
// model's own), so both steps read lengths from device memory and neither needs a host sync.
//
// ss_song_offsets: offsets[s] = sum of max(lens[i], 0) over i < s, s = 0 .. S (an exclusive scan, 64-bit). One workgroup walks the array 256 entries
//   at a time (a Hillis-Steele scan in LDS per chunk, the running total carried from chunk to chunk), so S may be any size.
// ss_song_place: row b of `src` holds segment s = seg[b]; its first n = lens[s] * unit floats go to out[offsets[s] * unit ...]. The segments never
//   overlap - the timeline is their concatenation - so every output float has exactly one writer: no atomics, any launch order. At the joints the
//   waveform is faded through a table: f = min(fade, n / 2); a segment with s > 0 has float k < f multiplied by win[((2 k + 1) fade) / (2 f)]
//   (integer division; = win[k] when f == fade), a segment with s < S - 1 has float n - 1 - k multiplied by the same entry. One fp32 multiply by a
//   table value and nothing else: the host restatement (tests/song_ref.py) is bit-exact.
//   Reads stop at lds floats of a row, writes at cap floats of `out`; a row whose segment index is >= S or whose offset is negative is skipped. Each
//   of the three sets its bit in flags[0] (SS_SONG_FLAG_*), written by ONE thread of the launch (a read-modify-write in stream order).
//   16-byte loads and stores where unit, lds and both base pointers allow (the host decides; offsets[s] * unit is then a multiple of four floats),
//   else one float per access with consecutive lanes on consecutive floats.
#include "common.h"
#include "../../include/stylesinger_hip.h"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_PER_THREAD = 4;
constexpr int SP_SPAN = SP_THREADS * SP_PER_THREAD;   // floats of a row per workgroup

__global__ __launch_bounds__(SP_THREADS) void song_offsets_kernel(const int32_t* __restrict__ lens, int S, int64_t* __restrict__ offsets) {
  __shared__ int64_t sh[SP_THREADS];
  const int tid = threadIdx.x;
  int64_t carry = 0;
  for (int c = 0; c < S; c += SP_THREADS) {
    const int i = c + tid;
    const int64_t v = (i < S && lens[i] > 0) ? (int64_t)lens[i] : 0;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < SP_THREADS; d <<= 1) {
      const int64_t t = tid >= d ? sh[tid - d] : 0;
      __syncthreads();
      sh[tid] += t;
      __syncthreads();
    }
    if (i < S) offsets[i] = carry + sh[tid] - v;
    carry += sh[SP_THREADS - 1];
    __syncthreads();   // sh is rewritten by the next chunk
  }
  if (tid == 0) offsets[S] = carry;
}

struct SongRow {
  int s;          // song index
  int64_t n;      // floats of the segment
  int64_t n_ok;   // floats that are read and written: n after both clamps
  int64_t dst;    // first float in `out`
  int bits;       // SS_SONG_FLAG_* this row raises
};

// -> false: nothing of this row is placed (skipped on request, empty, or refused)
__device__ __forceinline__ bool song_row(const int32_t* __restrict__ seg, const int32_t* __restrict__ lens, const int64_t* __restrict__ offsets, int b,
                                         int S, int unit, int64_t lds, int64_t cap, SongRow& r) {
  r.bits = 0;
  r.n = r.n_ok = r.dst = 0;
  r.s = seg[b];
  if (r.s < 0) return false;
  if (r.s >= S) {
    r.bits = SS_SONG_FLAG_INDEX;
    return false;
  }
  const int len = lens[r.s];
  const int64_t off = offsets[r.s];
  if (len <= 0) return false;
  if (off < 0) {
    r.bits = SS_SONG_FLAG_INDEX;
    return false;
  }
  r.n = (int64_t)len * unit;
  r.n_ok = r.n;
  if (r.n_ok > lds) {
    r.n_ok = lds;
    r.bits |= SS_SONG_FLAG_READ;
  }
  int64_t room = 0;
  if (off <= cap / unit) {   // off * unit cannot overflow past this test
    r.dst = off * unit;
    room = cap - r.dst;
  }
  if (r.n_ok > room) {
    r.n_ok = room;
    r.bits |= SS_SONG_FLAG_WRITE;
  }
  return r.n_ok > 0;
}

// the joint gain of float k of a segment of n floats: head = faded floats at its start (0 for the song's first segment), tail = first faded float
// at its end (n for the song's last segment)
__device__ __forceinline__ float song_gain(float v, int64_t k, int64_t n, int64_t f, int64_t head, int64_t tail, const float* __restrict__ win, int fade) {
  int64_t j;
  if (k < head) j = k;
  else if (k >= tail) j = n - 1 - k;
  else return v;
  const int64_t idx = f == fade ? j : ((2 * j + 1) * (int64_t)fade) / (2 * f);
  return v * win[idx];
}

template <bool VEC>
__global__ __launch_bounds__(SP_THREADS) void song_place_kernel(const float* __restrict__ src, int64_t lds, const int32_t* __restrict__ seg, int B,
                                                                const int32_t* __restrict__ lens, const int64_t* __restrict__ offsets, int S, int unit,
                                                                const float* __restrict__ win, int fade, float* __restrict__ out, int64_t cap,
                                                                int32_t* __restrict__ flags) {
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  if (flags && blockIdx.x == 0 && b == 0) {   // one workgroup looks at every row's clamps; one thread of it updates the word
    __shared__ int sh_bits[SP_THREADS];
    int bits = 0;
    for (int r = tid; r < B; r += SP_THREADS) {
      SongRow row;
      song_row(seg, lens, offsets, r, S, unit, lds, cap, row);
      bits |= row.bits;
    }
    sh_bits[tid] = bits;
    __syncthreads();
    if (tid == 0) {
      for (int i = 1; i < SP_THREADS; ++i) bits |= sh_bits[i];
      if (bits) flags[0] = flags[0] | bits;
    }
  }
  SongRow r;
  if (!song_row(seg, lens, offsets, b, S, unit, lds, cap, r)) return;
  const int64_t base = (int64_t)blockIdx.x * SP_SPAN;
  if (base >= r.n_ok) return;
  const int64_t f = fade < r.n / 2 ? (int64_t)fade : r.n / 2;
  const int64_t head = r.s > 0 ? f : 0;
  const int64_t tail = r.s < S - 1 ? r.n - f : r.n;
  const float* sp = src + (int64_t)b * lds;
  float* dp = out + r.dst;
  if (VEC) {
    const int64_t k0 = base + (int64_t)tid * SP_PER_THREAD;
    if (k0 >= r.n_ok) return;
    if (k0 + SP_PER_THREAD <= r.n_ok) {
      float4 v = *reinterpret_cast<const float4*>(sp + k0);
      if (k0 < head || k0 + SP_PER_THREAD > tail) {
        v.x = song_gain(v.x, k0, r.n, f, head, tail, win, fade);
        v.y = song_gain(v.y, k0 + 1, r.n, f, head, tail, win, fade);
        v.z = song_gain(v.z, k0 + 2, r.n, f, head, tail, win, fade);
        v.w = song_gain(v.w, k0 + 3, r.n, f, head, tail, win, fade);
      }
      *reinterpret_cast<float4*>(dp + k0) = v;
    } else {   // the last floats before a clamp that is no multiple of four
      for (int64_t k = k0; k < r.n_ok; ++k) dp[k] = song_gain(sp[k], k, r.n, f, head, tail, win, fade);
    }
  } else {
#pragma unroll
    for (int j = 0; j < SP_PER_THREAD; ++j) {
      const int64_t k = base + j * SP_THREADS + tid;
      if (k < r.n_ok) dp[k] = song_gain(sp[k], k, r.n, f, head, tail, win, fade);
    }
  }
}

}  // namespace

extern "C" int ss_song_offsets(const int32_t* lens, int S, int64_t* offsets, void* stream) {
  SS_CHECK_ARG(S >= 0, "ss_song_offsets: S=%d", S);
  SS_CHECK_ARG(offsets && (lens || S == 0), "ss_song_offsets: null pointer");
  hipLaunchKernelGGL(song_offsets_kernel, dim3(1), dim3(SP_THREADS), 0, (hipStream_t)stream, lens, S, offsets);
  SS_CHECK_LAUNCH("ss_song_offsets");
  return SS_OK;
}

extern "C" int ss_song_place(const float* src, int64_t lds, const int32_t* seg, int B, const int32_t* lens, const int64_t* offsets, int S, int unit,
                             const float* win, int fade, float* out, int64_t cap, int32_t* flags, void* stream) {
  SS_CHECK_ARG(src && seg && lens && offsets && out, "ss_song_place: null pointer");
  SS_CHECK_ARG(B > 0 && B <= 65535 && S >= 0, "ss_song_place: bad dims (B=%d S=%d)", B, S);
  SS_CHECK_ARG(unit > 0 && unit <= (1 << 20), "ss_song_place: unit=%d floats per frame outside 1 .. 2^20", unit);
  SS_CHECK_ARG(lds > 0 && cap >= 0, "ss_song_place: bad sizes (lds=%lld cap=%lld)", (long long)lds, (long long)cap);
  SS_CHECK_ARG(fade >= 0 && fade <= (1 << 24), "ss_song_place: fade=%d floats outside 0 .. 2^24", fade);
  SS_CHECK_ARG(fade == 0 || win, "ss_song_place: fade=%d without a window table", fade);
  SS_CHECK_ARG(src != out, "ss_song_place: input and output must not alias");
  const int64_t gx = (lds + SP_SPAN - 1) / SP_SPAN;
  SS_CHECK_ARG(gx <= 0x7fffffffLL, "ss_song_place: lds=%lld floats per row is too wide", (long long)lds);
  const bool vec = unit % 4 == 0 && lds % 4 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)out % 16 == 0;
  const dim3 grid((unsigned)gx, (unsigned)B), block(SP_THREADS);
  if (vec)
    hipLaunchKernelGGL(song_place_kernel<true>, grid, block, 0, (hipStream_t)stream, src, lds, seg, B, lens, offsets, S, unit, win, fade, out, cap, flags);
  else
    hipLaunchKernelGGL(song_place_kernel<false>, grid, block, 0, (hipStream_t)stream, src, lds, seg, B, lens, offsets, S, unit, win, fade, out, cap, flags);
  SS_CHECK_LAUNCH("ss_song_place");
  return SS_OK;
}
