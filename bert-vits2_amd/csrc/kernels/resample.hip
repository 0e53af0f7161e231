// resample.hip — polyphase resampler (include/bv2.h bv2_resample): rate_in -> rate_out = L / M after the gcd, a Kaiser-windowed sinc of
// 2K + 1 taps per phase, table T[L][2K + 1] built on the host (bv2_resample_taps).
//   y[n] = sum_{jj = 0..2K} x[i0 + jj - K] * T[p][jj],   i0 = floor(n M / L),  p = (n M) mod L,   x = 0 outside [0, len_b)
// A workgroup owns a run of `tile` outputs of one item and stages their input span [i0(first) - K, i0(last) + K] in LDS once: the zero
// selection (an index outside [0, len_b), or outside the caller's buffer, is never loaded) and the int16 conversion happen there.  A thread
// owns four consecutive outputs of the tile, placed so that the four are one aligned 16-byte store on the body of the destination; each
// output is ONE fmaf chain over ascending jj, so a sum does not depend on where its tile starts, on the batch row, on n0 or on how a stream
// was cut (the bit-identity tests rest on this).  Input reads are near-contiguous LDS reads; a lane walks its own coefficient row (the
// table is at most 4 MB, 126 KB for the audio rates, and stays in L2).
// Any ratio inside the envelope runs on this one kernel: the launcher shrinks `tile` until the tile's own span fits the first
// TILE_SPAN floats of the buffer (a 441:1 decimation has one output per workgroup), and the tap loop runs in chunks of CHUNK taps
// (ascending, so the order of a sum is unchanged), each staged with the span it needs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bv2_kernels.h"

namespace bv2 {

#define BV2_CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -1)

constexpr int RS_THREADS = 256;
constexpr int RS_PER_THREAD = 4;
constexpr int RS_LDS_FLOATS = 8192;                         // 32 KB
constexpr int RS_TILE_SPAN = 6144;                          // floats a tile's own span may take: 1024 outputs of 44.1 -> 8 kHz need 5647
constexpr int RS_CHUNK = RS_LDS_FLOATS - RS_TILE_SPAN;      // taps per staging pass (2048: every audio rate pair is one pass)

template <typename T>
__device__ __forceinline__ float rs_load(const T* p);
template <>
__device__ __forceinline__ float rs_load<float>(const float* p) { return *p; }
template <>
__device__ __forceinline__ float rs_load<int16_t>(const int16_t* p) { return (float)*p * (1.f / 32768.f); }

template <typename T>
__global__ void __launch_bounds__(RS_THREADS) resample_kernel(const T* src, int64_t src_bstride, int64_t src_start, int64_t src_n,
                                                              const int64_t* src_lengths, const float* taps, int L, int M, int K,
                                                              int tile, int64_t n0, int64_t n1, float* dst, int64_t dst_bstride,
                                                              int64_t* dst_lengths_out) {
  __shared__ float xs[RS_LDS_FLOATS];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int ntaps = 2 * K + 1;
  const T* s = src + (int64_t)b * src_bstride;
  float* d = dst + (int64_t)b * dst_bstride;
  const int64_t src_end = src_start + src_n;
  int64_t len = src_lengths ? src_lengths[b] : src_end;
  len = len < 0 ? 0 : len;
  const int64_t n_out = (len * L + M - 1) / M;
  if (dst_lengths_out && blockIdx.x == 0 && tid == 0) dst_lengths_out[b] = n_out;

  // v = (n - n0) + shift counts floats from the 16-byte boundary at or below d: v % 4 == 0 is an aligned address
  const int shift = (int)((reinterpret_cast<uintptr_t>(d) >> 2) & 3u);
  const int64_t n = n1 - n0;
  const int64_t tile_v = (int64_t)blockIdx.x * tile;
  const int64_t oA = tile_v > shift ? tile_v - shift : 0;                   // the tile's outputs, as offsets o = n - n0 in [oA, oB)
  int64_t oB = tile_v + tile - shift;
  oB = oB > n ? n : oB;
  if (oB <= oA) return;                                                     // block-uniform
  const int64_t nA = n0 + oA;
  int64_t nB = n0 + oB;
  nB = nB > n_out ? n_out : nB;                                             // outputs at or past N_out(b) are zeros: nothing staged for them
  const bool any = nB > nA;                                                 // block-uniform
  const int64_t iA = any ? (nA * M) / L : 0;
  const int tile_span = any ? (int)(((nB - 1) * M) / L - iA) + 1 : 0;       // <= RS_TILE_SPAN by the launcher's choice of `tile`

  const int64_t v0 = tile_v + (int64_t)RS_PER_THREAD * tid;
  const bool mine = RS_PER_THREAD * tid < tile;
  float acc[RS_PER_THREAD];
  int off[RS_PER_THREAD];
  const float* row[RS_PER_THREAD];
  bool live[RS_PER_THREAD];
  {
    const int64_t nf = n0 + (v0 - shift);                                   // this thread's first output (may lie in front of n0)
    const int64_t nc = nf < 0 ? 0 : nf;
    int64_t i0 = (nc * M) / L;
    int p = (int)((nc * M) % L);
    const int mq = M / L, mr = M % L;
#pragma unroll
    for (int q = 0; q < RS_PER_THREAD; ++q) {
      const int64_t nq = nf + q;
      if (nq > nc) {                                                        // step from nc: one 64-bit division per thread
        i0 += mq; p += mr;
        if (p >= L) { p -= L; ++i0; }
      }
      live[q] = any && mine && RS_PER_THREAD * tid + q < tile && nq >= nA && nq < nB;
      off[q] = live[q] ? (int)(i0 - iA) : 0;
      row[q] = taps + (size_t)(live[q] ? p : 0) * ntaps;
      acc[q] = 0.f;
    }
  }

  if (any) {
    for (int j0 = 0; j0 < ntaps; j0 += RS_CHUNK) {
      const int jn = ntaps - j0 < RS_CHUNK ? ntaps - j0 : RS_CHUNK;
      const int64_t ib = iA + j0 - K;                                       // xs[e] = x[ib + e]
      const int count = tile_span + jn - 1;
      if (j0) __syncthreads();                                              // the previous chunk's reads are done
      for (int e = tid; e < count; e += RS_THREADS) {
        const int64_t i = ib + e;
        const bool ok = i >= 0 && i < len && i >= src_start && i < src_end;
        xs[e] = ok ? rs_load<T>(s + (i - src_start)) : 0.f;                 // selected, never multiplied in
      }
      __syncthreads();
#pragma unroll 4
      for (int j = 0; j < jn; ++j) {
#pragma unroll
        for (int q = 0; q < RS_PER_THREAD; ++q) acc[q] = fmaf(xs[off[q] + j], row[q][j0 + j], acc[q]);
      }
    }
  }

  if (!mine) return;
  const int64_t o = v0 - shift;                                             // offset of acc[0] in the destination
  if (o >= oA && o + RS_PER_THREAD <= oB && (v0 & 3) == 0) {
    float4 r;
    r.x = live[0] ? acc[0] : 0.f; r.y = live[1] ? acc[1] : 0.f; r.z = live[2] ? acc[2] : 0.f; r.w = live[3] ? acc[3] : 0.f;
    *reinterpret_cast<float4*>(d + o) = r;
  } else {
#pragma unroll
    for (int q = 0; q < RS_PER_THREAD; ++q) {
      const int64_t oq = o + q;
      if (RS_PER_THREAD * tid + q < tile && oq >= oA && oq < oB) d[oq] = live[q] ? acc[q] : 0.f;
    }
  }
}

int launch_resample(hipStream_t stream, const ResampleArgs& a) {
  const int64_t n = a.n1 - a.n0;
  if (a.B < 1 || a.B > 65535 || n < 1 || a.L < 1 || a.M < 1 || a.K < 1) return -1;
  // the largest tile whose own span, floor((tile - 1) M / L) + 2 at most, fits RS_TILE_SPAN
  int64_t tile = (int64_t)(RS_TILE_SPAN - 2) * a.L / a.M + 1;
  const int full = RS_THREADS * RS_PER_THREAD;
  tile = tile > full ? full : tile;
  if (tile >= RS_PER_THREAD) tile &= ~(int64_t)(RS_PER_THREAD - 1);         // whole threads, and every tile starts on a 16-byte boundary
  const int64_t gx = (n + 3 + tile - 1) / tile;                             // + 3: the destination's alignment shift
  if (gx > 0x7fffffff) return -1;
  const dim3 grid((unsigned)gx, (unsigned)a.B), block(RS_THREADS);
  if (a.input_format == 1)
    hipLaunchKernelGGL(resample_kernel<int16_t>, grid, block, 0, stream, static_cast<const int16_t*>(a.src), a.src_bstride, a.src_start,
                       a.src_n, a.src_lengths, a.taps, a.L, a.M, a.K, (int)tile, a.n0, a.n1, a.dst, a.dst_bstride, a.dst_lengths_out);
  else
    hipLaunchKernelGGL(resample_kernel<float>, grid, block, 0, stream, static_cast<const float*>(a.src), a.src_bstride, a.src_start,
                       a.src_n, a.src_lengths, a.taps, a.L, a.M, a.K, (int)tile, a.n0, a.n1, a.dst, a.dst_bstride, a.dst_lengths_out);
  return BV2_CHECK_LAUNCH();
}

}  // namespace bv2
