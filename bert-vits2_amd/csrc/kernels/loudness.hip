// loudness.hip — ITU-R BS.1770-4 loudness of mono audio (include/bv2.h bv2_loudness_*): K-weighting, 400 ms blocks every 100 ms, the
// absolute and the relative gate, one gain per group, and the multiply that applies it.
//
// The K-weighting is two biquads in cascade, a 4-state linear recurrence s' = A s + B x.  Recurrence and every energy sum are fp64 (an fp32
// recurrence of the 38 Hz high pass, poles at radius 0.995, loses 6e-5 of a second's energy).  A sequential recurrence is made parallel by
// superposition: a thread filters its segment of LD_SEG samples from the ZERO state and keeps the end state z; the true start state of the
// next segment is A^LD_SEG s + z.  That chain runs in three levels with host-built powers of A — 16 segments (P = A^16), 16 groups of
// segments (Q = A^256), the tiles of an item (R = A^4096) — and the segment is then filtered again from its true state while its energy is
// summed.  Launches of a measurement:
//   1. loudness_tile_kernel<T, false>  grid (tiles, B): the tile's end state from the zero state                  -> tile_z
//   2. loudness_carry_kernel           one lane per item: the tiles' true start states, in order                  -> tile_s
//   3. loudness_tile_kernel<T, true>   grid (tiles, B): the second pass; per tile the energy of each 100 ms step it touches (at most
//                                      LD_MAX_PARTS) and the tile's sample peak                                   -> part, tile_peak
//   4. loudness_gate_kernel            one workgroup per group: block mean squares from the tiles' partial sums, both gates, lufs, gain
// A carry that crosses workgroups crosses a launch boundary: no workgroup ever waits for another one.  No floating-point atomics.
// Every sum has one order that depends on the item's own samples only: tiles and segments are counted from the ITEM's first sample, a
// step's energy is its tiles' partial sums in tile order (each a fixed tree over the tile's threads), a block is its four steps in order,
// an item's gated sum runs over its blocks in order, and a group's sum adds its items' sums in ascending order of value (so it does not
// depend on the rows the items sit in).  Samples at or behind an item's length are selected to zero, never loaded.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bv2_kernels.h"

namespace bv2 {

#define BV2_CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -1)

constexpr int LD_GROUPS = LD_THREADS / LD_SEG;               // 16 groups of 16 segments
constexpr int LD_XS = LD_TILE + LD_TILE / LD_SEG;            // a tile's samples, one pad float per segment: conflict-free segment reads
static_assert(LD_GROUPS == LD_SEG && LD_THREADS == 256, "the three-level chain below is written for 16 x 16 segments of 16 samples");

struct LdState { double s1, s2, t1, t2; };

template <typename T>
__device__ __forceinline__ float ld_load(const T* p);
template <>
__device__ __forceinline__ float ld_load<float>(const float* p) { return *p; }
template <>
__device__ __forceinline__ float ld_load<int16_t>(const int16_t* p) { return (float)*p * (1.f / 32768.f); }

// one sample through both biquads (transposed direct form II); returns the K-weighted sample
__device__ __forceinline__ double ld_step(const LoudnessFilter& f, LdState& s, double x) {
  const double y1 = fma(f.c[0], x, s.s1);
  s.s1 = fma(-f.c[3], y1, fma(f.c[1], x, s.s2));
  s.s2 = fma(-f.c[4], y1, f.c[2] * x);
  const double y2 = fma(f.c[5], y1, s.t1);
  s.t1 = fma(-f.c[8], y2, fma(f.c[6], y1, s.t2));
  s.t2 = fma(-f.c[9], y2, f.c[7] * y1);
  return y2;
}

// M s + z, M row-major 4 x 4: the state after a run of samples whose zero-state response ends in z
__device__ __forceinline__ LdState ld_advance(const double* M, const LdState& s, const LdState& z) {
  LdState r;
  r.s1 = fma(M[3], s.t2, fma(M[2], s.t1, fma(M[1], s.s2, fma(M[0], s.s1, z.s1))));
  r.s2 = fma(M[7], s.t2, fma(M[6], s.t1, fma(M[5], s.s2, fma(M[4], s.s1, z.s2))));
  r.t1 = fma(M[11], s.t2, fma(M[10], s.t1, fma(M[9], s.s2, fma(M[8], s.s1, z.t1))));
  r.t2 = fma(M[15], s.t2, fma(M[14], s.t1, fma(M[13], s.s2, fma(M[12], s.s1, z.t2))));
  return r;
}

__device__ __forceinline__ int64_t ld_item_len(const int64_t* lengths, int b, int64_t S) {
  int64_t n = lengths ? lengths[b] : S;
  n = n < 0 ? 0 : n;
  return n > S ? S : n;
}

template <typename T, bool SECOND>
__global__ void __launch_bounds__(LD_THREADS) loudness_tile_kernel(const T* wav, int64_t bstride, const int64_t* lengths, int64_t S, int nt,
                                                                   int step, int nparts, LoudnessFilter f, double* tile_z,
                                                                   const double* tile_s, double* part, float* tile_peak) {
  __shared__ float xs[LD_XS];
  __shared__ LdState zs[LD_THREADS];
  __shared__ LdState zg[LD_GROUPS];
  __shared__ double red[SECOND ? LD_MAX_PARTS * LD_THREADS : 1];
  __shared__ unsigned pk_bits;
  const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
  const int64_t len = ld_item_len(lengths, b, S);
  const int64_t base = (int64_t)k * LD_TILE;
  if (base >= len) return;                                                   // block-uniform: the tile lies behind the item
  const T* src = wav + (int64_t)b * bstride;
  if (SECOND && tid == 0) pk_bits = 0u;
#pragma unroll
  for (int r = 0; r < LD_SEG; ++r) {
    const int i = tid + LD_THREADS * r;
    xs[i + (i >> 4)] = base + i < len ? ld_load<T>(src + base + i) : 0.f;     // selected, never loaded behind the length
  }
  __syncthreads();

  const float* mine = xs + tid * (LD_SEG + 1);
  {
    LdState st = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < LD_SEG; ++q) ld_step(f, st, (double)mine[q]);
    zs[tid] = st;
  }
  __syncthreads();
  if (tid < LD_GROUPS) {                                                     // a group's end state from the zero state
    LdState s = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int i = 0; i < LD_SEG; ++i) s = ld_advance(f.P, s, zs[tid * LD_SEG + i]);
    zg[tid] = s;
  }
  __syncthreads();
  const size_t tix = (size_t)b * nt + k;
  if (!SECOND) {
    if (tid == 0) {
      LdState s = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
      for (int g = 0; g < LD_GROUPS; ++g) s = ld_advance(f.Q, s, zg[g]);
      double* o = tile_z + tix * 4;
      o[0] = s.s1; o[1] = s.s2; o[2] = s.t1; o[3] = s.t2;
    }
    return;
  }

  if (tid == 0) {                                                            // the groups' true start states from the tile's
    const double* t = tile_s + tix * 4;
    LdState s = {t[0], t[1], t[2], t[3]};
#pragma unroll 4
    for (int g = 0; g < LD_GROUPS; ++g) {
      const LdState z = zg[g];
      zg[g] = s;
      s = ld_advance(f.Q, s, z);
    }
  }
  __syncthreads();
  if (tid < LD_GROUPS) {                                                     // the segments' true start states from the group's
    LdState s = zg[tid];
#pragma unroll 4
    for (int i = 0; i < LD_SEG; ++i) {
      const LdState z = zs[tid * LD_SEG + i];
      zs[tid * LD_SEG + i] = s;
      s = ld_advance(f.P, s, z);
    }
  }
  __syncthreads();

  const int64_t i0 = base + (int64_t)tid * LD_SEG;
  const int64_t s0 = i0 / step;
  const int64_t bnd = (s0 + 1) * step;                                       // LD_SEG < step: a segment meets at most one step boundary
  const int j0 = (int)(s0 - base / step);
  double e0 = 0.0, e1 = 0.0;
  float pk = 0.f;
  {
    LdState st = zs[tid];
#pragma unroll
    for (int q = 0; q < LD_SEG; ++q) {
      const float x = mine[q];
      const double y = ld_step(f, st, (double)x);
      const int64_t i = i0 + q;
      if (i < len) {
        if (i < bnd) e0 = fma(y, y, e0); else e1 = fma(y, y, e1);
        pk = fmaxf(pk, fabsf(x));
      }
    }
  }
  for (int j = 0; j < nparts; ++j) red[j * LD_THREADS + tid] = j == j0 ? e0 : (j == j0 + 1 ? e1 : 0.0);
  atomicMax(&pk_bits, __float_as_uint(pk));                                  // integers: |x| >= 0 orders as its bit pattern
  __syncthreads();
  for (int stride = LD_THREADS / 2; stride >= 1; stride >>= 1) {             // one fixed tree per step
    for (int idx = tid; idx < nparts * stride; idx += LD_THREADS) {
      const int j = idx / stride, u = idx - j * stride;
      red[j * LD_THREADS + u] += red[j * LD_THREADS + u + stride];
    }
    __syncthreads();
  }
  if (tid < nparts) part[tix * LD_MAX_PARTS + tid] = red[tid * LD_THREADS];
  if (tid == 0) tile_peak[tix] = __uint_as_float(pk_bits);
}

__global__ void __launch_bounds__(64) loudness_carry_kernel(const int64_t* lengths, int64_t S, int B, int nt, LoudnessFilter f,
                                                            const double* tile_z, double* tile_s) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int64_t len = ld_item_len(lengths, b, S);
  const int ntb = (int)((len + LD_TILE - 1) / LD_TILE);
  LdState s = {0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < ntb; ++k) {
    const size_t tix = (size_t)b * nt + k;
    double* o = tile_s + tix * 4;
    o[0] = s.s1; o[1] = s.s2; o[2] = s.t1; o[3] = s.t2;
    const double* z = tile_z + tix * 4;
    const LdState zz = {z[0], z[1], z[2], z[3]};
    s = ld_advance(f.R, s, zz);
  }
}

__host__ __device__ __forceinline__ int64_t ld_blocks(int64_t n, int step) {
  const int64_t block = 4 * (int64_t)step;
  return n <= 0 ? 0 : (n < block ? 1 : (n - block) / step + 1);
}

// energy of step s of an item of n samples: its tiles' partial sums in tile order
__device__ __forceinline__ double ld_step_energy(const double* part_b, int64_t s, int64_t n, int step) {
  const int64_t lo = s * step;
  if (lo >= n) return 0.0;
  int64_t hi = lo + step;
  hi = hi > n ? n : hi;
  const int64_t k0 = lo / LD_TILE, k1 = (hi - 1) / LD_TILE;
  double e = 0.0;
  for (int64_t k = k0; k <= k1; ++k) e += part_b[k * LD_MAX_PARTS + (s - (k * LD_TILE) / step)];
  return e;
}

// the sum over the group's items of (item_s, item_c), added in ascending order of (sum, count): it does not depend on the items' rows
__device__ void ld_combine(const LoudnessGateArgs& a, int g, int b_lo, int b_hi, int offset, double* out_s, int64_t* out_c) {
  const int tid = threadIdx.x;
  for (int b = b_lo + tid; b < b_hi; b += LD_THREADS) {
    if (a.groups && a.groups[b] != g) continue;
    const double s = a.item_s[b];
    const int64_t c = a.item_c[b];
    int r = 0;
    for (int o = b_lo; o < b_hi; ++o) {
      if (a.groups && a.groups[o] != g) continue;
      const double so = a.item_s[o];
      const int64_t co = a.item_c[o];
      r += (so < s || (so == s && (co < c || (co == c && o < b)))) ? 1 : 0;
    }
    a.sort_s[offset + r] = s;
    a.sort_c[offset + r] = c;
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int b = b_lo; b < b_hi; ++b) n += (!a.groups || a.groups[b] == g) ? 1 : 0;
    double s = 0.0;
    int64_t c = 0;
    for (int i = 0; i < n; ++i) { s += a.sort_s[offset + i]; c += a.sort_c[offset + i]; }
    *out_s = s; *out_c = c;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(LD_THREADS) loudness_gate_kernel(LoudnessGateArgs a) {
  __shared__ double sum_s;
  __shared__ int64_t sum_c;
  __shared__ int offset_s;
  const int g = blockIdx.x, tid = threadIdx.x;
  const int b_lo = a.groups ? 0 : g, b_hi = a.groups ? a.B : g + 1;
  const int step = a.step;
  const int64_t block = 4 * (int64_t)step;

  if (a.part) {                                                              // block mean squares and peaks of the group's items
    for (int b = b_lo; b < b_hi; ++b) {
      if (a.groups && a.groups[b] != g) continue;                            // block-uniform
      const int64_t n = ld_item_len(a.lengths, b, a.S);
      const int64_t nb = ld_blocks(n, step);
      const double* pb = a.part + (size_t)b * a.nt * LD_MAX_PARTS;
      for (int64_t j = tid; j < a.ms_width; j += LD_THREADS) {
        double ms = 0.0;
        if (j < nb) {
          const int64_t s = n < block ? 0 : j;
          const double e = ((ld_step_energy(pb, s, n, step) + ld_step_energy(pb, s + 1, n, step)) + ld_step_energy(pb, s + 2, n, step)) +
                           ld_step_energy(pb, s + 3, n, step);
          ms = e / (double)(n < block ? n : block);
        }
        a.block_ms[(size_t)b * a.ms_bstride + j] = ms;
      }
      if (tid == 0) {
        const int64_t ntb = (n + LD_TILE - 1) / LD_TILE;
        float p = 0.f;
        for (int64_t k = 0; k < ntb; ++k) p = fmaxf(p, a.tile_peak[(size_t)b * a.nt + k]);
        a.peak[b] = p;
      }
    }
    __syncthreads();
  }
  if (!a.gate) return;

  if (tid == 0) {
    int off = g;
    if (a.groups) {
      off = 0;
      for (int b = 0; b < a.B; ++b) off += (a.groups[b] >= 0 && a.groups[b] < g) ? 1 : 0;
    }
    offset_s = off;
  }
  __syncthreads();
  const int offset = offset_s;

  double thr = 0.0;                                                          // pass 0: the absolute gate; pass 1: both gates
  double s_abs = 0.0;
  int64_t c_abs = 0;
  for (int pass = 0; pass < 2; ++pass) {
    for (int b = b_lo + tid; b < b_hi; b += LD_THREADS) {
      if (a.groups && a.groups[b] != g) continue;
      const int64_t nb = ld_blocks(ld_item_len(a.lengths, b, a.S), step);
      const double* ms = a.block_ms + (size_t)b * a.ms_bstride;
      double s = 0.0;
      int64_t c = 0;
      for (int64_t j = 0; j < nb; ++j) {
        const double v = ms[j];
        if (v > a.abs_ms && v > thr) { s += v; ++c; }
      }
      a.item_s[b] = s;
      a.item_c[b] = c;
    }
    __syncthreads();
    ld_combine(a, g, b_lo, b_hi, offset, &sum_s, &sum_c);
    if (pass == 0) {
      s_abs = sum_s; c_abs = sum_c;
      if (c_abs == 0) break;                                                 // block-uniform: a silent group
      thr = s_abs / (double)c_abs * 0.1;                                     // 10 LU below the absolute-gated loudness
      __syncthreads();
    }
  }

  if (tid == 0) {
    float pk = 0.f;
    for (int b = b_lo; b < b_hi; ++b)
      if (!a.groups || a.groups[b] == g) pk = fmaxf(pk, a.peak[b]);
    int flags = 0;
    double lufs = -INFINITY, gain = 1.0;
    if (c_abs == 0) {
      flags = LD_FLAG_SILENT;
    } else {
      lufs = -0.691 + 10.0 * log10(sum_s / (double)sum_c);
      gain = pow(10.0, (a.target_lufs - lufs) / 20.0);
      if ((double)pk * gain > a.ceiling) { gain = a.ceiling / (double)pk; flags = LD_FLAG_LIMITED; }
    }
    if (a.lufs) a.lufs[g] = lufs;
    if (a.gain) a.gain[g] = (float)gain;
    if (a.flags) a.flags[g] = flags;
  }
}

template <typename T>
__global__ void __launch_bounds__(LD_THREADS) loudness_apply_kernel(const T* src, int64_t src_bstride, const int64_t* lengths, int64_t S,
                                                                    const int* groups, int n_gain, const float* gain, float* dst,
                                                                    int16_t* dst16, int64_t dst_bstride) {
  const int b = blockIdx.y;
  const int64_t len = ld_item_len(lengths, b, S);
  const int gi = groups ? groups[b] : b;
  const float gn = gi >= 0 && gi < n_gain ? gain[gi] : 1.f;
  const T* s = src + (int64_t)b * src_bstride;
  const int64_t i_lo = ((int64_t)blockIdx.x * LD_THREADS) * 4 + threadIdx.x;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t i = i_lo + q * LD_THREADS;
    if (i >= S) break;
    const float v = i < len ? __fmul_rn(ld_load<T>(s + i), gn) : 0.f;        // one fp32 multiply, never contracted
    if (dst) dst[(int64_t)b * dst_bstride + i] = v;
    else dst16[(int64_t)b * dst_bstride + i] = (int16_t)(int)fminf(fmaxf(__fmul_rn(v, 32767.f), -32768.f), 32767.f);   // bv2_emit's rule
  }
}

// launches 1 to 3 of a measurement
static int launch_loudness_tiles(hipStream_t stream, const LoudnessArgs& a) {
  if (a.B < 1 || a.B > 65535 || a.S < 1 || a.step <= LD_SEG) return -1;
  const int64_t nt = (a.S + LD_TILE - 1) / LD_TILE;
  const int nparts = (LD_TILE - 1) / a.step + 2;
  if (nt > 0x7fffffff || nparts > LD_MAX_PARTS || a.gate.nt != (int)nt) return -1;
  const dim3 grid((unsigned)nt, (unsigned)a.B), block(LD_THREADS);
  if (a.input_format == 1) {
    const int16_t* w = static_cast<const int16_t*>(a.wav);
    hipLaunchKernelGGL((loudness_tile_kernel<int16_t, false>), grid, block, 0, stream, w, a.bstride, a.lengths, a.S, (int)nt, a.step, nparts,
                       a.filter, a.tile_z, a.tile_s, a.part, a.tile_peak);
    hipLaunchKernelGGL(loudness_carry_kernel, dim3((a.B + 63) / 64), dim3(64), 0, stream, a.lengths, a.S, a.B, (int)nt, a.filter, a.tile_z,
                       a.tile_s);
    hipLaunchKernelGGL((loudness_tile_kernel<int16_t, true>), grid, block, 0, stream, w, a.bstride, a.lengths, a.S, (int)nt, a.step, nparts,
                       a.filter, a.tile_z, a.tile_s, a.part, a.tile_peak);
  } else {
    const float* w = static_cast<const float*>(a.wav);
    hipLaunchKernelGGL((loudness_tile_kernel<float, false>), grid, block, 0, stream, w, a.bstride, a.lengths, a.S, (int)nt, a.step, nparts,
                       a.filter, a.tile_z, a.tile_s, a.part, a.tile_peak);
    hipLaunchKernelGGL(loudness_carry_kernel, dim3((a.B + 63) / 64), dim3(64), 0, stream, a.lengths, a.S, a.B, (int)nt, a.filter, a.tile_z,
                       a.tile_s);
    hipLaunchKernelGGL((loudness_tile_kernel<float, true>), grid, block, 0, stream, w, a.bstride, a.lengths, a.S, (int)nt, a.step, nparts,
                       a.filter, a.tile_z, a.tile_s, a.part, a.tile_peak);
  }
  return BV2_CHECK_LAUNCH();
}

int launch_loudness_measure(hipStream_t stream, const LoudnessArgs& a) {
  if (launch_loudness_tiles(stream, a)) return -1;
  return launch_loudness_gate(stream, a.gate);
}

int launch_loudness_gate(hipStream_t stream, const LoudnessGateArgs& a) {
  const int n = a.gate ? a.n_groups : a.B;                                   // blocks only: one workgroup per item
  if (a.B < 1 || n < 1 || n > 65535 || (a.gate && !a.groups && a.n_groups != a.B)) return -1;
  LoudnessGateArgs g = a;
  if (!a.gate) g.groups = nullptr;
  hipLaunchKernelGGL(loudness_gate_kernel, dim3(n), dim3(LD_THREADS), 0, stream, g);
  return BV2_CHECK_LAUNCH();
}

int launch_loudness_apply(hipStream_t stream, const LoudnessApplyArgs& a) {
  if (a.B < 1 || a.B > 65535 || a.S < 1) return -1;
  const int64_t gx = (a.S + 4 * LD_THREADS - 1) / (4 * LD_THREADS);
  if (gx > 0x7fffffff) return -1;
  const dim3 grid((unsigned)gx, (unsigned)a.B), block(LD_THREADS);
  if (a.input_format == 1)
    hipLaunchKernelGGL(loudness_apply_kernel<int16_t>, grid, block, 0, stream, static_cast<const int16_t*>(a.src), a.src_bstride, a.lengths,
                       a.S, a.groups, a.n_gain, a.gain, a.dst, a.dst16, a.dst_bstride);
  else
    hipLaunchKernelGGL(loudness_apply_kernel<float>, grid, block, 0, stream, static_cast<const float*>(a.src), a.src_bstride, a.lengths, a.S,
                       a.groups, a.n_gain, a.gain, a.dst, a.dst16, a.dst_bstride);
  return BV2_CHECK_LAUNCH();
}

// ---- step energies and loudness range (EBU Tech 3342; include/bv2.h bv2_loudness_steps / bv2_loudness_range) ----
// step_ss[b][k]: the energy of the item's whole step k — ld_step_energy, the sum the gate kernel forms for the same step, so four of
// them added in order and divided by the block are the bits of block_ms.  The range then works on step energies alone:
//   1. loudness_st_kernel     grid (steps, B): short-term energy s_j = (30 steps, added in ascending order) / (30 step)        -> st
//   2. loudness_range_kernel  one workgroup per group: both gates of Tech 3342 over the group's pooled short-term blocks, the two
//                             percentiles by a radix select over the fp64 bit patterns (a positive double orders as its uint64: 8
//                             passes of 8-bit histograms, integer atomics in LDS only — exact, the elements a sort would return), and
//                             the maxima of the short-term and the momentary (four steps) energies
__global__ void __launch_bounds__(LD_THREADS) loudness_steps_kernel(const double* part, const int64_t* lengths, int64_t S, int nt, int step,
                                                                    double* step_ss, int64_t ss_bstride, int64_t ss_width) {
  const int b = blockIdx.y;
  const int64_t k = (int64_t)blockIdx.x * LD_THREADS + threadIdx.x;
  if (k >= ss_width) return;
  const int64_t n = ld_item_len(lengths, b, S);
  step_ss[(size_t)b * ss_bstride + k] = k < n / step ? ld_step_energy(part + (size_t)b * nt * LD_MAX_PARTS, k, n, step) : 0.0;
}

__device__ __forceinline__ int64_t ld_st_blocks(int64_t n, int step) {
  const int64_t steps = n / step;
  return steps >= LD_ST_STEPS ? steps - (LD_ST_STEPS - 1) : 0;
}

__global__ void __launch_bounds__(LD_THREADS) loudness_st_kernel(LoudnessRangeArgs a) {
  const int b = blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * LD_THREADS + threadIdx.x;
  const int64_t stw = a.ss_width > 0 ? a.ss_width : 1;
  if (j >= stw) return;
  double v = 0.0;
  if (j < ld_st_blocks(ld_item_len(a.lengths, b, a.S), a.step)) {
    const double* e = a.step_ss + (size_t)b * a.ss_bstride + j;
    double s = 0.0;
    for (int q = 0; q < LD_ST_STEPS; ++q) s += e[q];
    v = s / ((double)LD_ST_STEPS * (double)a.step);
  }
  a.st[(size_t)b * stw + j] = v;
}

__device__ __forceinline__ double ld_block_sum(double* red, double v) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int stride = LD_THREADS / 2; stride >= 1; stride >>= 1) {
    if (tid < stride) red[tid] += red[tid + stride];
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ double ld_block_max(double* red, double v) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int stride = LD_THREADS / 2; stride >= 1; stride >>= 1) {
    if (tid < stride) red[tid] = fmax(red[tid], red[tid + stride]);
    __syncthreads();
  }
  return red[0];
}

// the element of rank `rank` (zero-based, ascending) among the group's short-term energies above both thresholds, as its bit pattern
__device__ unsigned long long ld_select(const LoudnessRangeArgs& a, int g, int b_lo, int b_hi, double thr, int64_t rank, unsigned* hist,
                                        unsigned* runs, unsigned long long* pick) {
  const int tid = threadIdx.x;
  const int64_t stw = a.ss_width > 0 ? a.ss_width : 1;
  unsigned long long prefix = 0;
  __syncthreads();
  if (tid == 0) pick[1] = (unsigned long long)rank;                          // the rank inside the bin that is still open
  for (int pass = 7; pass >= 0; --pass) {
    const int shift = 8 * pass;
    __syncthreads();
    hist[tid] = 0u;
    __syncthreads();
    for (int b = b_lo; b < b_hi; ++b) {
      if (a.groups && a.groups[b] != g) continue;                            // block-uniform
      const int64_t nst = ld_st_blocks(ld_item_len(a.lengths, b, a.S), a.step);
      const double* st = a.st + (size_t)b * stw;
      for (int64_t j = tid; j < nst; j += LD_THREADS) {
        const double v = st[j];
        if (!(v > a.abs_ms && v > thr)) continue;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
        if (pass == 7 || (bits >> (shift + 8)) == prefix) atomicAdd(&hist[(unsigned)(bits >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    if (tid < 16) {                                                          // the bin that holds the rank: 16 runs of 16 bins, then one run
      unsigned t = 0;
      for (int i = 0; i < 16; ++i) t += hist[tid * 16 + i];
      runs[tid] = t;
    }
    __syncthreads();
    if (tid == 0) {
      int64_t r = (int64_t)pick[1], cum = 0;
      int run = 0;
      for (; run < 15; ++run) {
        if (cum + (int64_t)runs[run] > r) break;
        cum += runs[run];
      }
      int bin = run * 16;
      for (; bin < run * 16 + 15; ++bin) {
        if (cum + (int64_t)hist[bin] > r) break;
        cum += hist[bin];
      }
      pick[0] = (prefix << 8) | (unsigned long long)bin;
      pick[1] = (unsigned long long)(r - cum);
    }
    __syncthreads();
    prefix = pick[0];
  }
  return prefix;
}

__global__ void __launch_bounds__(LD_THREADS) loudness_range_kernel(LoudnessRangeArgs a) {
  __shared__ double red[LD_THREADS];
  __shared__ unsigned hist[LD_THREADS];
  __shared__ unsigned runs[16];
  __shared__ unsigned long long pick[2];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int b_lo = a.groups ? 0 : g, b_hi = a.groups ? a.B : g + 1;
  const int64_t stw = a.ss_width > 0 ? a.ss_width : 1;
  const double block = 4.0 * (double)a.step;

  double s = 0.0, c = 0.0, total = 0.0, mx_st = 0.0, mx_mo = 0.0;            // counts as doubles: exact below 2^53
  for (int b = b_lo; b < b_hi; ++b) {
    if (a.groups && a.groups[b] != g) continue;                              // block-uniform
    const int64_t n = ld_item_len(a.lengths, b, a.S);
    const int64_t nst = ld_st_blocks(n, a.step);
    const int64_t nmo = n / a.step >= 4 ? n / a.step - 3 : 0;
    const double* st = a.st + (size_t)b * stw;
    const double* e = a.step_ss + (size_t)b * a.ss_bstride;
    for (int64_t j = tid; j < nst; j += LD_THREADS) {
      const double v = st[j];
      total += 1.0;
      mx_st = fmax(mx_st, v);
      if (v > a.abs_ms) { s += v; c += 1.0; }
    }
    for (int64_t j = tid; j < nmo; j += LD_THREADS) mx_mo = fmax(mx_mo, (((e[j] + e[j + 1]) + e[j + 2]) + e[j + 3]) / block);
  }
  s = ld_block_sum(red, s);
  c = ld_block_sum(red, c);
  total = ld_block_sum(red, total);
  mx_st = ld_block_max(red, mx_st);
  mx_mo = ld_block_max(red, mx_mo);

  int flags = 0;
  if (total == 0.0) flags = LD_RANGE_SHORT;
  else if (c == 0.0) flags = LD_RANGE_SILENT;
  double lra = 0.0, lo_l = -INFINITY, hi_l = -INFINITY, st_l = -INFINITY, mo_l = -INFINITY;
  if (!flags) {                                                              // block-uniform
    const double thr = s / c * 0.01;                                         // 20 LU below the absolute-gated mean
    double kept = 0.0;
    for (int b = b_lo; b < b_hi; ++b) {
      if (a.groups && a.groups[b] != g) continue;
      const int64_t nst = ld_st_blocks(ld_item_len(a.lengths, b, a.S), a.step);
      const double* st = a.st + (size_t)b * stw;
      for (int64_t j = tid; j < nst; j += LD_THREADS) {
        const double v = st[j];
        kept += (v > a.abs_ms && v > thr) ? 1.0 : 0.0;
      }
    }
    kept = ld_block_sum(red, kept);
    const int64_t nk = (int64_t)kept;                                        // >= 1: the largest gated block is above 0.01 of their mean
    const int64_t r_lo = ((nk - 1) * 10 + 50) / 100, r_hi = ((nk - 1) * 95 + 50) / 100;
    const double v_lo = __longlong_as_double((long long)ld_select(a, g, b_lo, b_hi, thr, r_lo, hist, runs, pick));
    const double v_hi = __longlong_as_double((long long)ld_select(a, g, b_lo, b_hi, thr, r_hi, hist, runs, pick));
    lra = 10.0 * log10(v_hi / v_lo);
    lo_l = -0.691 + 10.0 * log10(v_lo);
    hi_l = -0.691 + 10.0 * log10(v_hi);
    st_l = -0.691 + 10.0 * log10(mx_st);
    mo_l = -0.691 + 10.0 * log10(mx_mo);
  }
  if (tid == 0) {
    a.lra[g] = lra; a.st_low[g] = lo_l; a.st_high[g] = hi_l; a.max_short_term[g] = st_l; a.max_momentary[g] = mo_l; a.flags[g] = flags;
  }
}

int launch_loudness_steps(hipStream_t stream, const LoudnessStepsArgs& a) {
  if (launch_loudness_tiles(stream, a.m)) return -1;
  if (a.want_blocks && launch_loudness_gate(stream, a.m.gate)) return -1;
  if (a.ss_width < 1) return 0;                                              // S is shorter than a step: no item has one
  const int64_t gx = (a.ss_width + LD_THREADS - 1) / LD_THREADS;
  hipLaunchKernelGGL(loudness_steps_kernel, dim3((unsigned)gx, (unsigned)a.m.B), dim3(LD_THREADS), 0, stream, a.m.part, a.m.lengths, a.m.S,
                     a.m.gate.nt, a.m.step, a.step_ss, a.ss_bstride, a.ss_width);
  return BV2_CHECK_LAUNCH();
}

int launch_loudness_range(hipStream_t stream, const LoudnessRangeArgs& a) {
  if (a.B < 1 || a.B > 65535 || a.n_groups < 1 || a.n_groups > 65535 || a.step < 1 || (!a.groups && a.n_groups != a.B)) return -1;
  const int64_t stw = a.ss_width > 0 ? a.ss_width : 1;
  const int64_t gx = (stw + LD_THREADS - 1) / LD_THREADS;
  hipLaunchKernelGGL(loudness_st_kernel, dim3((unsigned)gx, (unsigned)a.B), dim3(LD_THREADS), 0, stream, a);
  hipLaunchKernelGGL(loudness_range_kernel, dim3(a.n_groups), dim3(LD_THREADS), 0, stream, a);
  return BV2_CHECK_LAUNCH();
}

}  // namespace bv2
