// stream.hip — streamed synthesis (include/bv2.h bv2_stream_chunk): what a window of the Generator needs besides the Generator itself.
//   stream_window_lens  the per-item length of a window of frames [w0, w0 + W): clamp(y_lengths[b] - w0, 1, W)
//   stream_emit         the window's KEPT samples out of the window's Generator output, as fp32 or as 16-bit PCM, zero past the item's end
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bv2_kernels.h"

namespace bv2 {

#define BV2_CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -1)

// The lower bound is 1, not 0: the Generator's kernels take lengths >= 1 (bv2_decode's y_lengths are clamp_min(.., 1), models.py:1057) — several
// clamp a column index to length - 1 for their unconditional loads (the split-K conv, conv_post), which a length of 0 would turn into an
// address in front of the tensor.  An item that ended before the window therefore runs as ONE frame of z * y_mask = 0; stream_emit writes
// its samples as zeros whatever the Generator left there.
__global__ void __launch_bounds__(64) stream_window_lens_kernel(const int64_t* y_lengths, int64_t* wlens, int w0, int W, int B) {
  for (int b = threadIdx.x; b < B; b += 64) {
    int64_t v = y_lengths[b] - w0;
    v = v < 1 ? 1 : (v > W ? W : v);
    wlens[b] = v;
  }
}

int launch_stream_window_lens(hipStream_t stream, const int64_t* y_lengths, int64_t* wlens, int w0, int W, int B) {
  if (B < 1 || W < 1 || w0 < 0) return -1;
  hipLaunchKernelGGL(stream_window_lens_kernel, dim3(1), dim3(64), 0, stream, y_lengths, wlens, w0, W, B);
  return BV2_CHECK_LAUNCH();
}

// One pass: dst[b][i] = i < valid_b ? f(src[b][src_off + i]) : 0 for i in [0, n), valid_b = y_lengths[b] * hop - start_sample (null: n).
// f is the identity (T = float) or the 16-bit PCM of bv2.h: (int16) trunc(clamp(x * gain, -32768, 32767)) — a fixed gain, no peak (a stream
// cannot know it; tanh bounds |x| <= 1).  A masked sample's source is never used: past an item's length the window output is whatever an
// earlier window left (the Generator's tiles past an item's length return without storing).
// The body is 16 bytes of DESTINATION per thread (4 floats / 8 samples of PCM), aligned on the destination; its source comes as float4 loads
// when it is 16-byte aligned at the same point (one flag per item, wave-uniform) and as dword loads otherwise — an odd product of upsample
// rates (5 * 5 * 5) or a PCM offset of t0 * 100 samples puts source and destination on different phases.  The < 16 bytes in front of and
// behind the body are written sample by sample by the first workgroup of the item.
template <typename T>
__device__ __forceinline__ T emit_one(float x, bool ok, float gain);
template <>
__device__ __forceinline__ float emit_one<float>(float x, bool ok, float) { return ok ? x : 0.f; }
template <>
__device__ __forceinline__ int16_t emit_one<int16_t>(float x, bool ok, float gain) {
  const float v = fminf(fmaxf(x * gain, -32768.f), 32767.f);       // NaN -> -32768 (fmaxf returns the other operand)
  return ok ? (int16_t)(int)v : (int16_t)0;
}

template <typename T>
__global__ void __launch_bounds__(256) stream_emit_kernel(const float* src, int64_t src_bstride, int64_t src_off, const int64_t* y_lengths,
                                                          int hop, int64_t start_sample, int64_t n, T* dst, int64_t dst_bstride,
                                                          float gain) {
  constexpr int V = 16 / (int)sizeof(T);
  const int b = blockIdx.y;
  const float* s = src + (int64_t)b * src_bstride + src_off;
  T* d = dst + (int64_t)b * dst_bstride;
  int64_t valid = n;
  if (y_lengths) {
    valid = y_lengths[b] * (int64_t)hop - start_sample;
    valid = valid < 0 ? 0 : (valid > n ? n : valid);
  }
  int64_t head = (int64_t)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(d) & 15u)) & 15u) / (unsigned)sizeof(T));
  head = head < n ? head : n;
  const int64_t nbody = (n - head) / V;
  const int64_t tail0 = head + nbody * V;
  if (blockIdx.x == 0) {                                           // head and tail: fewer than V samples each
    const int64_t t = threadIdx.x;
    if (t < head) d[t] = emit_one<T>(s[t], t < valid, gain);
    const int64_t i = tail0 + t;
    if (i < n) d[i] = emit_one<T>(s[i], i < valid, gain);
  }
  const bool src16 = (reinterpret_cast<uintptr_t>(s + head) & 15u) == 0;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < nbody; g += (int64_t)gridDim.x * 256) {
    const int64_t i = head + g * V;
    float x[V];
    if (src16) {
#pragma unroll
      for (int q = 0; q < V / 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(s + i + 4 * q);
        x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) x[e] = s[i + e];
    }
    T o[V];
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = emit_one<T>(x[e], i + e < valid, gain);
    uint4 pk;
    __builtin_memcpy(&pk, o, 16);
    *reinterpret_cast<uint4*>(d + i) = pk;
  }
}

int launch_stream_emit(hipStream_t stream, const float* src, int64_t src_bstride, int64_t src_off, const int64_t* y_lengths, int hop,
                       int64_t start_sample, int B, int64_t n, float* dst, int16_t* dst16, int64_t dst_bstride, float gain) {
  if (B < 1 || B > 65535 || n < 1 || hop < 1 || (dst != nullptr) == (dst16 != nullptr)) return -1;
  const int per_wg = 256 * (dst ? 4 : 8);
  int64_t gx = (n + per_wg - 1) / per_wg;
  gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
  if (dst)
    hipLaunchKernelGGL(stream_emit_kernel<float>, dim3((unsigned)gx, B), dim3(256), 0, stream, src, src_bstride, src_off, y_lengths, hop,
                       start_sample, n, dst, dst_bstride, gain);
  else
    hipLaunchKernelGGL(stream_emit_kernel<int16_t>, dim3((unsigned)gx, B), dim3(256), 0, stream, src, src_bstride, src_off, y_lengths, hop,
                       start_sample, n, dst16, dst_bstride, gain);
  return BV2_CHECK_LAUNCH();
}

}  // namespace bv2
