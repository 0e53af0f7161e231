// truepeak_taps.h — the staging and the tap loop that truepeak.hip and limiter.hip share: the F interpolated phases of every input
// position of a tile, in registers, as ONE fmaf chain each over ascending jj from 0.f (resample.hip's rule to the letter, so the values
// are bv2_resample's bits).  xs[e] = x[base - K + e] with samples outside [0, len) selected to zero and never loaded; tl[jj * F + p] =
// T[p][jj], the table transposed so that the F coefficients of a tap are one broadcast read.  A thread owns the positions
// tid + TP_THREADS r (r < TP_PER): at tap jj the lanes of a wave read consecutive words of xs, no bank conflict.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bv2_kernels.h"

namespace bv2 {

constexpr int TP_NT = 2 * TP_K + 1;                         // 73 taps per phase
constexpr int TP_XS = TP_TILE + 2 * TP_K;                   // the tile and its two halos
static_assert(TP_TILE == TP_THREADS * TP_PER, "a thread owns TP_PER positions, TP_THREADS apart");

template <typename T>
__device__ __forceinline__ float tp_load(const T* p);
template <>
__device__ __forceinline__ float tp_load<float>(const float* p) { return *p; }
template <>
__device__ __forceinline__ float tp_load<int16_t>(const int16_t* p) { return (float)*p * (1.f / 32768.f); }

__device__ __forceinline__ int64_t tp_item_len(const int64_t* lengths, int b, int64_t S) {
  int64_t n = lengths ? lengths[b] : S;
  n = n < 0 ? 0 : n;
  return n > S ? S : n;
}

// fills xs [TP_XS] and, for F > 1, tl [TP_NT * F]; the caller syncs
template <typename T, int F>
__device__ __forceinline__ void tp_stage(float* xs, float* tl, const T* src, int64_t base, int64_t len, const float* taps, int tid) {
  for (int e = tid; e < TP_XS; e += TP_THREADS) {
    const int64_t i = base - TP_K + e;
    xs[e] = (i >= 0 && i < len) ? tp_load<T>(src + i) : 0.f;                   // selected, never loaded outside the item
  }
  if (F > 1) {
    for (int e = tid; e < TP_NT * F; e += TP_THREADS) {
      const int p = e / TP_NT, jj = e - p * TP_NT;
      tl[jj * F + p] = taps[e];
    }
  }
}

// acc[r][p] = y[(base + tid + TP_THREADS r) F + p]
template <int F>
__device__ __forceinline__ void tp_phases(const float* xs, const float* tl, int tid, float (&acc)[TP_PER][F]) {
#pragma unroll
  for (int r = 0; r < TP_PER; ++r)
#pragma unroll
    for (int p = 0; p < F; ++p) acc[r][p] = 0.f;
#pragma unroll 1
  for (int jj = 0; jj < TP_NT; ++jj) {
    float t[F];
#pragma unroll
    for (int p = 0; p < F; ++p) t[p] = tl[jj * F + p];
#pragma unroll
    for (int r = 0; r < TP_PER; ++r) {
      const float x = xs[tid + TP_THREADS * r + jj];
#pragma unroll
      for (int p = 0; p < F; ++p) acc[r][p] = fmaf(x, t[p], acc[r][p]);
    }
  }
}

}  // namespace bv2
