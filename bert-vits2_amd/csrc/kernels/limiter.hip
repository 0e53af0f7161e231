// limiter.hip — look-ahead true-peak limiter of mono audio (include/bv2.h bv2_limit).  Per item, indices from its first sample:
//   e[i] = max(|x[i]|, max_p |y[i F + p]|)            y = bv2_resample's rate -> F rate outputs: truepeak_taps.h, the bits of truepeak.hip
//   r[i] = fminf(1, c / (e[i] g))                      1 outside [0, len)
//   m[j] = min r[j - H - 1 .. j + P + 1]               the hold: every m inside the window of s[i] has seen r[i - 1], r[i], r[i + 1]
//   d[j] = 1 - m[j]                                    0 outside [0, len)
//   A[i] = sum_{k = -P..H} w[k] d[i + k]               from 0.f over ascending k, product and sum rounded separately
//   s[i] = fminf(1 - A[i], fminf(r[i - 1], fminf(r[i], r[i + 1])))
//   out[i] = (x[i] g) s[i]                             bv2_loudness_apply's product times the gain curve; zeros behind the length
// Every fp32 operation is one separately rounded operation (plain operators with contraction off, below; IEEE division).
// Two launches:
//   1. limit_envelope_kernel  grid (tiles, B): true_peak_tile_kernel's staging and tap loop, r[i] per sample -> req (workspace [B][S]) and
//                             the tile's smallest r -> tile_min (an integer min in LDS, one store); tile 0 of an item also initialises
//                             the item's min_gain / limited_samples slots
//   2. limit_apply_kernel     grid (tiles, B): a workgroup stages r over its tile and the reach H + P + 1 on either side (s[i] depends on
//                             r[i - H - P - 1 .. i + H + P + 1]) in LDS — unless tile_min of every tile within that reach says 1, which a
//                             few loads tell.  All of it 1 (block-uniform): d = 0, A = 0, s = 1.0f exactly — the workgroup
//                             writes x g and is done; most tiles of speech take this path.  Otherwise the hold runs IN PLACE as
//                             passes a[u] = min(a[u], a[u + s]) for s = 1, 2, 4 .. span (the largest power of two <= W = H + P + 3), then
//                             s = W - span: a[u] = min r over W samples from u on (a minimum is exact in any order).  A pass walks the
//                             array in ascending chunks, reads of a chunk before its writes: a[u] only ever reads at or above u.  d
//                             replaces m in place; the FIR reads d as aligned float4 (a thread owns four consecutive outputs and re-uses
//                             the seven d values of four taps from registers) and the window through the scalar cache (the tap index is
//                             uniform).  LDS: LM_TILE + 2 LM_MAX_REACH + 4 floats = 53 264 bytes.
// min_gain is an integer atomicMin over the bit patterns of s (a positive float orders as its bits; a negative one, which 1 - A can only
// be by a rounding when r is 0, sorts below every positive), limited_samples an integer atomicAdd: no floating-point atomics, no
// workgroup waits for another.  Non-finite input follows truepeak.hip: fmaxf skips a NaN operand in the envelope, so a NaN sample asks
// for no reduction and leaves as NaN.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bv2_kernels.h"
#include "truepeak_taps.h"

// Device code contracts a * b + c into an FMA by default, and the __fmul_rn / __fadd_rn of the HIP headers are inline functions around
// plain * and + that were compiled under that default, so they fuse as well once inlined.  "One rounding per operation" is therefore
// written with plain operators under contraction OFF for this file (the interpolation's fmaf chains are explicit calls).
#pragma clang fp contract(off)

namespace bv2 {

#define BV2_CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -1)

static_assert(LM_TILE == TP_TILE && LM_THREADS == TP_THREADS && LM_PER == TP_PER, "the envelope launch is the true-peak tiling");
constexpr int LM_N = LM_TILE + 2 * LM_MAX_REACH + 2;        // staged r: the tile and H + P + 1 on either side
constexpr int LM_NA = (LM_N + 3) / 4 * 4;                   // whole float4s
constexpr int LM_CHUNK = 8;                                 // elements per thread and chunk of a hold pass
static_assert(LM_NA * 4 + 64 <= 64 * 1024, "the apply kernel's static LDS stays under 64 KB");

__device__ __forceinline__ float lm_item_gain(const int* groups, int n_gain, const float* gain, int b) {
  const int gi = groups ? groups[b] : b;
  return gi >= 0 && gi < n_gain ? gain[gi] : 1.f;
}

template <typename T, int F>
__global__ void __launch_bounds__(LM_THREADS) limit_envelope_kernel(const T* wav, int64_t bstride, const int64_t* lengths, int64_t S,
                                                                    const float* taps, const int* groups, int n_gain, const float* gain,
                                                                    float c, float* req, int nt, int* tile_min, float* min_gain,
                                                                    int64_t* limited) {
  __shared__ float xs[TP_XS];                                                // xs[e] = x[base - K + e]
  __shared__ float tl[F > 1 ? TP_NT * F : 1];                                // tl[jj * F + p] = T[p][jj]
  __shared__ int tmin;
  const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
  if (k == 0 && tid == 0) { min_gain[b] = 1.f; limited[b] = 0; }             // the slots the apply launch folds into
  const int64_t len = tp_item_len(lengths, b, S);
  const int64_t base = (int64_t)k * LM_TILE;
  if (base >= len) return;                                                   // block-uniform: the tile lies behind the item
  if (tid == 0) tmin = 0x3f800000;
  tp_stage<T, F>(xs, tl, wav + (int64_t)b * bstride, base, len, taps, tid);
  __syncthreads();

  float e[LM_PER];
#pragma unroll
  for (int r = 0; r < LM_PER; ++r) e[r] = fmaxf(0.f, fabsf(xs[tid + LM_THREADS * r + TP_K]));
  if (F > 1) {
    float acc[LM_PER][F];
    tp_phases<F>(xs, tl, tid, acc);
#pragma unroll
    for (int r = 0; r < LM_PER; ++r)
#pragma unroll
      for (int p = 0; p < F; ++p) e[r] = fmaxf(e[r], fabsf(acc[r][p]));
  }
  const float gn = lm_item_gain(groups, n_gain, gain, b);
  float* rq = req + (int64_t)b * S + base;
#pragma unroll
  for (int r = 0; r < LM_PER; ++r) {
    const int i = tid + LM_THREADS * r;
    if (base + i < len) {
      const float r1 = fminf(1.f, c / (e[r] * gn));                            // c / 0 = inf: 1
      rq[i] = r1;
      if (r1 < 1.f) atomicMin(&tmin, __float_as_int(r1));                      // integers: 0 <= r1 orders as its bit pattern
    }
  }
  __syncthreads();
  if (tid == 0) tile_min[(size_t)b * nt + k] = tmin;                         // the tile's smallest r: 1.0f's bits where nothing is asked
}

// a[u] = min(a[u], a[u + s]) for every u with u + s < n, in place
__device__ __forceinline__ void lm_hold_pass(float* a, int n, int s, int tid) {
  for (int c0 = 0; c0 < n; c0 += LM_THREADS * LM_CHUNK) {                    // uniform trip count
    float v[LM_CHUNK];
#pragma unroll
    for (int j = 0; j < LM_CHUNK; ++j) {
      const int u = c0 + tid + LM_THREADS * j;
      v[j] = u + s < n ? fminf(a[u], a[u + s]) : 0.f;
    }
    __syncthreads();                                                         // the chunk is read before it is written
#pragma unroll
    for (int j = 0; j < LM_CHUNK; ++j) {
      const int u = c0 + tid + LM_THREADS * j;
      if (u + s < n) a[u] = v[j];
    }
  }
  __syncthreads();
}

template <typename T>
__global__ void __launch_bounds__(LM_THREADS) limit_apply_kernel(const T* src, int64_t src_bstride, const int64_t* lengths, int64_t S,
                                                                 const float* req, int nt, const int* tile_min, int H, int P,
                                                                 const float* __restrict__ window,
                                                                 const int* groups, int n_gain, const float* gain, float* dst,
                                                                 int16_t* dst16, int64_t dst_bstride, float* curve, int* min_bits,
                                                                 unsigned long long* limited) {
  __shared__ __attribute__((aligned(16))) float a[LM_NA];                    // a[e] = r[base - (H + P + 1) + e], then m, then d
  __shared__ int mn_bits;
  __shared__ unsigned cnt;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t len = tp_item_len(lengths, b, S);
  const int64_t base = (int64_t)blockIdx.x * LM_TILE;
  const int R = H + P, n = LM_TILE + 2 * R + 2;
  const int li0 = LM_PER * tid;                                              // the thread's four consecutive outputs
  float* o32 = dst ? dst + (int64_t)b * dst_bstride + base : nullptr;
  int16_t* o16 = dst16 ? dst16 + (int64_t)b * dst_bstride + base : nullptr;
  float* oc = curve ? curve + (int64_t)b * S + base : nullptr;

  float v[LM_PER], s[LM_PER];
#pragma unroll
  for (int q = 0; q < LM_PER; ++q) { v[q] = 0.f; s[q] = 1.f; }
  bool engaged = false;
  if (base < len) {                                                          // block-uniform
    const float gn = lm_item_gain(groups, n_gain, gain, b);
    const T* x = src + (int64_t)b * src_bstride + base;
#pragma unroll
    for (int q = 0; q < LM_PER; ++q)
      if (base + li0 + q < len) v[q] = tp_load<T>(x + li0 + q) * gn;   // bv2_loudness_apply's product
    if (tid == 0) { mn_bits = 0x3f800000; cnt = 0u; }
    const float* rq = req + (int64_t)b * S;
    const int64_t t0 = base - (R + 1), t1 = base + LM_TILE + R;              // the reach: s of this tile depends on r[t0 .. t1]
    const int k_lo = (int)((t0 > 0 ? t0 : 0) / LM_TILE), k_hi = (int)((t1 < len ? t1 : len - 1) / LM_TILE);   // the item's tiles inside it
    int below = 0;
    for (int k = k_lo + tid; k <= k_hi; k += LM_THREADS) below |= tile_min[(size_t)b * nt + k] < 0x3f800000 ? 1 : 0;
    if (__syncthreads_or(below)) {                                           // block-uniform: a tile within reach asks for a reduction
      below = 0;
      for (int e = tid; e < n; e += LM_THREADS) {
        const int64_t t = t0 + e;
        const float r = (t >= 0 && t < len) ? rq[t] : 1.f;                   // selected, never loaded outside the item
        a[e] = r;
        below |= r < 1.f ? 1 : 0;
      }
      engaged = __syncthreads_or(below) != 0;                                // block-uniform: one of the samples within reach does
    }
  }

  if (engaged) {
    float rr[LM_PER + 2];                                                    // r[i - 1 .. i + 4] of the thread's outputs
#pragma unroll
    for (int q = 0; q < LM_PER + 2; ++q) rr[q] = a[li0 + R + q];
    const int W = R + 3;                                                     // the hold's length
    int span = 1;
    while (2 * span <= W) { lm_hold_pass(a, n, span, tid); span *= 2; }      // its first sync orders rr's reads before any write
    if (W - span) lm_hold_pass(a, n, W - span, tid);
    for (int u = tid; u < LM_TILE + R; u += LM_THREADS) {                    // d[base - P + u]
      const int64_t j = base - P + u;
      a[u] = (j >= 0 && j < len) ? 1.f - a[u] : 0.f;
    }
    __syncthreads();

    float acc[LM_PER];
#pragma unroll
    for (int q = 0; q < LM_PER; ++q) acc[q] = 0.f;
    float4 cur = *reinterpret_cast<const float4*>(a + li0);
    for (int kk0 = 0; kk0 <= R; kk0 += 4) {                                  // kk = k + P: output li reads d at a[li + kk]
      const float4 nxt = *reinterpret_cast<const float4*>(a + li0 + kk0 + 4);
      const float dv[8] = {cur.x, cur.y, cur.z, cur.w, nxt.x, nxt.y, nxt.z, nxt.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (kk0 + j <= R) {                                                  // uniform
          const float w = window[kk0 + j];
#pragma unroll
          for (int q = 0; q < LM_PER; ++q) acc[q] = acc[q] + w * dv[j + q];
        }
      }
      cur = nxt;
    }
    int mb = 0x3f800000;
    unsigned nlim = 0;
#pragma unroll
    for (int q = 0; q < LM_PER; ++q) {
      if (base + li0 + q < len) {
        s[q] = fminf(1.f - acc[q], fminf(rr[q], fminf(rr[q + 1], rr[q + 2])));
        const int bits = __float_as_int(s[q]);
        mb = bits < mb ? bits : mb;
        nlim += s[q] < 1.f ? 1u : 0u;
      }
    }
    if (mb != 0x3f800000) atomicMin(&mn_bits, mb);
    if (nlim) atomicAdd(&cnt, nlim);
    __syncthreads();
    if (tid == 0 && cnt) {
      atomicMin(min_bits + b, mn_bits);
      atomicAdd(limited + b, (unsigned long long)cnt);
    }
  }

#pragma unroll
  for (int q = 0; q < LM_PER; ++q) {
    const int li = li0 + q;
    if (base + li >= S) break;
    const float o = engaged ? v[q] * s[q] : v[q];                  // s = 1.0f exactly on the all-pass path
    if (o32) o32[li] = o;
    else o16[li] = (int16_t)(int)fminf(fmaxf(o * 32767.f, -32768.f), 32767.f);   // bv2_emit's rule
    if (oc) oc[li] = s[q];
  }
}

template <typename T>
static void lm_launch(hipStream_t stream, const LimitArgs& a, int nt) {
  const dim3 grid((unsigned)nt, (unsigned)a.B), block(LM_THREADS);
  const T* w = static_cast<const T*>(a.src);
  if (a.factor == 4)
    hipLaunchKernelGGL((limit_envelope_kernel<T, 4>), grid, block, 0, stream, w, a.src_bstride, a.lengths, a.S, a.taps, a.groups, a.n_gain,
                       a.gain, a.ceiling, a.req, nt, a.tile_min, a.min_gain, a.limited_samples);
  else if (a.factor == 2)
    hipLaunchKernelGGL((limit_envelope_kernel<T, 2>), grid, block, 0, stream, w, a.src_bstride, a.lengths, a.S, a.taps, a.groups, a.n_gain,
                       a.gain, a.ceiling, a.req, nt, a.tile_min, a.min_gain, a.limited_samples);
  else
    hipLaunchKernelGGL((limit_envelope_kernel<T, 1>), grid, block, 0, stream, w, a.src_bstride, a.lengths, a.S, a.taps, a.groups, a.n_gain,
                       a.gain, a.ceiling, a.req, nt, a.tile_min, a.min_gain, a.limited_samples);
  hipLaunchKernelGGL(limit_apply_kernel<T>, grid, block, 0, stream, w, a.src_bstride, a.lengths, a.S, a.req, nt, a.tile_min, a.H, a.P, a.window, a.groups,
                     a.n_gain, a.gain, a.dst, a.dst16, a.dst_bstride, a.curve, reinterpret_cast<int*>(a.min_gain),
                     reinterpret_cast<unsigned long long*>(a.limited_samples));
}

int launch_limit(hipStream_t stream, const LimitArgs& a) {
  if (a.B < 1 || a.B > 65535 || a.S < 1 || (a.factor != 1 && a.factor != 2 && a.factor != 4) || (a.factor > 1 && !a.taps)) return -1;
  if (a.H < 1 || a.P < a.H || a.H + a.P > LM_MAX_REACH || !a.window || !a.req || !a.tile_min || !a.min_gain || !a.limited_samples) return -1;
  if ((a.dst != nullptr) == (a.dst16 != nullptr) || a.dst_bstride < a.S) return -1;
  const int64_t nt = (a.S + LM_TILE - 1) / LM_TILE;
  if (nt > 0x7fffffff) return -1;
  if (a.input_format == 1) lm_launch<int16_t>(stream, a, (int)nt);
  else lm_launch<float>(stream, a, (int)nt);
  return BV2_CHECK_LAUNCH();
}

}  // namespace bv2
