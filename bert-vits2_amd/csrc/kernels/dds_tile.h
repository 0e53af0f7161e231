// dds_tile.h — the pieces every whole-DDSConv-layer kernel is built from (dds_fused.hip: the inference direction; sdp_forward.hip: the
// likelihood direction): the tile width, GELU, and the 1x1 GEMM of one 16-row tile on v_mfma_f32_16x16x4_f32.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "device_helpers.h"

namespace bv2 {

constexpr int DDS_NT = 16;                          // time steps per workgroup

__device__ __forceinline__ float gelu_erf(float y) { return 0.5f * y * (1.0f + erff(y * 0.70710678118654752440f)); }

// 1x1 GEMM of one 16-row tile against the [C][16] activation tile in LDS.  Weights: conv_w_index order with k = 1, i.e. float4
// index ((mt32*G + g)*2 + lh)*32 + (row & 31) holds channels 8g + 2q + lh (q = 0..3) of output row `row`.  Lane (m = l & 15,
// kk = l >> 4) supplies A[m][kk]; K step (unit u, q) covers channels 16u + 8*(kk >> 1) + 2q + (kk & 1), so one float4 per lane per
// unit feeds four MFMAs and the B operand of step q is row (16u + 8*(kk >> 1) + (kk & 1)) + 2q of the tile.
template <int NU>
__device__ __forceinline__ void load_tile_weights(const float* w, int row_tile16, int lane, f32x4 (&wr)[NU]) {
  const int m = lane & 15, kk = lane >> 4;
  constexpr int G = 2 * NU;
  const f32x4* wp = reinterpret_cast<const f32x4*>(w);
#pragma unroll
  for (int u = 0; u < NU; ++u)
    wr[u] = wp[((((row_tile16 >> 1) * G + 2 * u + (kk >> 1)) * 2 + (kk & 1)) * 32) + 16 * (row_tile16 & 1) + m];
}

template <int NU>
__device__ __forceinline__ f32x4 tile_gemm(const f32x4 (&wr)[NU], const float* ys, int lane) {
  const int n = lane & 15, kk = lane >> 4;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};       // two chains: the 16x16x4 f32 MFMA has 40-cycle latency
  const float* yb = ys + (8 * (kk >> 1) + (kk & 1)) * DDS_NT + n;
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const float* yu = yb + u * 16 * DDS_NT;
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[u].x, yu[0 * 2 * DDS_NT], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[u].y, yu[1 * 2 * DDS_NT], acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[u].z, yu[2 * 2 * DDS_NT], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[u].w, yu[3 * 2 * DDS_NT], acc1, 0, 0, 0);
  }
  return acc0 + acc1;
}

}  // namespace bv2
