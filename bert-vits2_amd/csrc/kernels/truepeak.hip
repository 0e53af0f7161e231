// truepeak.hip — true peak of mono audio (include/bv2.h bv2_true_peak; ITU-R BS.1770-4 annex 2 with the project's own interpolator).
//   true_peak(b) = max( max_k |x_b[k]| , max_n |y_b[n]| ),   y_b = what bv2_resample gives for rate -> F rate (L = F, M = 1, K = 36)
//   y[i F + p] = sum_{jj = 0..2K} x[i + jj - K] * T[p][jj]   — ONE fmaf chain over ascending jj from 0.f, fp32 table, x = 0 outside
//   [0, len_b): resample.hip's rule to the letter, so |y| here and there are the same bits.  The oversampled signal is never written.
// Specialised for integer upsampling: a workgroup owns TP_TILE input positions of one item, counted from the item's first sample, and
// stages them once with a halo of K samples on each side (the zero selection and the int16 conversion happen there); the F x 73 table
// sits in LDS, transposed to tl[jj][p], so the F coefficients of a tap are one broadcast read.  A thread owns the positions
// tid + 256 r (r < TP_PER) and forms their F phases: at tap jj the lanes of a wave read xs[tid + 256 r + jj], consecutive words, no
// bank conflict.  No 64-bit index arithmetic per output and no coefficient walk through L2.
// Reduction: |v| >= 0 orders as its bit pattern, so the workgroup's maximum is an integer atomicMax in LDS and one value per tile goes
// to tile_peak; a second small launch folds an item's tiles.  No floating-point atomics, no workgroup waits for another, and every slot
// that is read has been written by this call: nothing needs zeroing.
// Non-finite input follows the sample peak of loudness.hip: the maximum is fmaxf, which skips a NaN operand — a NaN sample (and the
// outputs it reaches) does not count; an infinite sample gives +inf.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bv2_kernels.h"
#include "truepeak_taps.h"

namespace bv2 {

#define BV2_CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -1)

template <typename T, int F>
__global__ void __launch_bounds__(TP_THREADS) true_peak_tile_kernel(const T* wav, int64_t bstride, const int64_t* lengths, int64_t S,
                                                                    int nt, const float* taps, float* tile_peak) {
  __shared__ float xs[TP_XS];                                                // xs[e] = x[base - K + e]
  __shared__ float tl[F > 1 ? TP_NT * F : 1];                                // tl[jj * F + p] = T[p][jj]
  __shared__ unsigned pk_bits;
  const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
  const int64_t len = tp_item_len(lengths, b, S);
  const int64_t base = (int64_t)k * TP_TILE;
  if (base >= len) return;                                                   // block-uniform: the tile lies behind the item
  const T* src = wav + (int64_t)b * bstride;
  if (tid == 0) pk_bits = 0u;
  tp_stage<T, F>(xs, tl, src, base, len, taps, tid);
  __syncthreads();

  float pk = 0.f;
  if (F > 1) {
    float acc[TP_PER][F];
    tp_phases<F>(xs, tl, tid, acc);                                          // truepeak_taps.h: shared with limiter.hip
#pragma unroll
    for (int r = 0; r < TP_PER; ++r) {
      if (base + tid + TP_THREADS * r < len) {                               // the F outputs of a position inside the item
#pragma unroll
        for (int p = 0; p < F; ++p) pk = fmaxf(pk, fabsf(acc[r][p]));
      }
    }
  }
#pragma unroll
  for (int r = 0; r < TP_PER; ++r) {
    const int i = tid + TP_THREADS * r;
    if (base + i < len) pk = fmaxf(pk, fabsf(xs[i + TP_K]));                 // the sample peak: phase 0 is not the identity
  }
  atomicMax(&pk_bits, __float_as_uint(pk));                                  // integers: pk >= 0 and never NaN
  __syncthreads();
  if (tid == 0) tile_peak[(size_t)b * nt + k] = __uint_as_float(pk_bits);
}

// one workgroup per item: the maximum over the tiles the item has (0 for an item of length 0)
__global__ void __launch_bounds__(TP_THREADS) true_peak_fold_kernel(const int64_t* lengths, int64_t S, int nt, const float* tile_peak,
                                                                    float* peak_out) {
  __shared__ unsigned pk_bits;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t len = tp_item_len(lengths, b, S);
  const int ntb = (int)((len + TP_TILE - 1) / TP_TILE);
  if (tid == 0) pk_bits = 0u;
  __syncthreads();
  float pk = 0.f;
  for (int k = tid; k < ntb; k += TP_THREADS) pk = fmaxf(pk, tile_peak[(size_t)b * nt + k]);
  atomicMax(&pk_bits, __float_as_uint(pk));
  __syncthreads();
  if (tid == 0) peak_out[b] = __uint_as_float(pk_bits);
}

template <typename T>
static void tp_launch_tiles(hipStream_t stream, const TruePeakArgs& a, int nt) {
  const dim3 grid((unsigned)nt, (unsigned)a.B), block(TP_THREADS);
  const T* w = static_cast<const T*>(a.wav);
  if (a.factor == 4)
    hipLaunchKernelGGL((true_peak_tile_kernel<T, 4>), grid, block, 0, stream, w, a.bstride, a.lengths, a.S, nt, a.taps, a.tile_peak);
  else if (a.factor == 2)
    hipLaunchKernelGGL((true_peak_tile_kernel<T, 2>), grid, block, 0, stream, w, a.bstride, a.lengths, a.S, nt, a.taps, a.tile_peak);
  else
    hipLaunchKernelGGL((true_peak_tile_kernel<T, 1>), grid, block, 0, stream, w, a.bstride, a.lengths, a.S, nt, a.taps, a.tile_peak);
}

int launch_true_peak(hipStream_t stream, const TruePeakArgs& a) {
  if (a.B < 1 || a.B > 65535 || a.S < 1 || (a.factor != 1 && a.factor != 2 && a.factor != 4) || (a.factor > 1 && !a.taps)) return -1;
  const int64_t nt = (a.S + TP_TILE - 1) / TP_TILE;
  if (nt > 0x7fffffff) return -1;
  if (a.input_format == 1) tp_launch_tiles<int16_t>(stream, a, (int)nt);
  else tp_launch_tiles<float>(stream, a, (int)nt);
  hipLaunchKernelGGL(true_peak_fold_kernel, dim3(a.B), dim3(TP_THREADS), 0, stream, a.lengths, a.S, (int)nt, a.tile_peak, a.peak);
  return BV2_CHECK_LAUNCH();
}

}  // namespace bv2
