// assemble.hip — a document's audio joined on the device (include/bv2.h bv2_assemble): pieces that lie in several tensors, each under its
// level rule, and the pauses between them, written once into one buffer per document.
//   assemble_layout   the length of every segment from its device counter, an exclusive int64 scan per document -> offsets, totals
//   assemble_peaks    max|x| per piece or per level group (the two peak modes only), as the bit pattern of a non-negative float
//   assemble_write    the samples: 16-byte stores on the aligned body of the DESTINATION, every segment at its own source phase
// The piece lengths exist only on the device, so the layout is computed there; the host knows an upper bound (the capacity) and sizes
// the grids by it.  A workgroup owns AS_TILE destination samples of one document; tiles at or behind the document's total return.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bv2_kernels.h"

namespace bv2 {

#define BV2_CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -1)

// min(max(*length, 0) * hop, cap) without forming a product that could overflow: L * hop >= cap exactly when L >= ceil(cap / hop)
__device__ __forceinline__ int64_t as_seg_len(const AssembleSegment& g) {
  const int64_t cap = g.samples < 0 ? 0 : g.samples;
  if (!g.src) return cap;                                          // silence
  if (!g.length) return cap;
  const int64_t hop = g.hop < 1 ? 1 : g.hop;
  int64_t L = *g.length;
  L = L < 0 ? 0 : L;
  return L >= (cap + hop - 1) / hop ? cap : L * hop;
}

__device__ __forceinline__ int as_clamp_id(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// One workgroup.  run[i + 1] = lengths of segments [0, i] summed (run[0] = 0): a thread sums its own contiguous chunk, the chunk sums are
// scanned in LDS, the bases are added.  Integer sums: every order gives the same bits.  Then per document d: doc_seg[d] = its first segment
// (the first segment of a later document, or n, where d has none), doc_base[d] = run[doc_seg[d]]; offsets[i] = run[i] - doc_base[doc(i)],
// totals[d] = run[doc_seg[d + 1]] - doc_base[d].  peaks[] (one word per segment; the peak launch indexes it by piece or by group) is zeroed
// here, so the call needs no memset of its own.
__global__ void __launch_bounds__(AS_LAYOUT_THREADS) assemble_layout_kernel(const AssembleSegment* seg, int n, int n_docs, int64_t* run,
                                                                            int64_t* doc_base, int* doc_seg, unsigned* peaks,
                                                                            int64_t* offsets, int64_t* totals) {
  __shared__ int64_t part[2][AS_LAYOUT_THREADS];
  const int t = threadIdx.x;
  const int chunk = (n + AS_LAYOUT_THREADS - 1) / AS_LAYOUT_THREADS;
  const int i0 = t * chunk < n ? t * chunk : n, i1 = i0 + chunk < n ? i0 + chunk : n;
  int64_t sum = 0;
  for (int i = i0; i < i1; ++i) {
    sum += as_seg_len(seg[i]);
    run[i + 1] = sum;
    peaks[i] = 0u;
  }
  part[0][t] = sum;
  __syncthreads();
  int cur = 0;
  for (int o = 1; o < AS_LAYOUT_THREADS; o <<= 1) {                // inclusive scan of the chunk sums
    part[cur ^ 1][t] = part[cur][t] + (t >= o ? part[cur][t - o] : 0);
    cur ^= 1;
    __syncthreads();
  }
  const int64_t base = t ? part[cur][t - 1] : 0;
  for (int i = i0; i < i1; ++i) run[i + 1] += base;
  if (t == 0) run[0] = 0;
  __syncthreads();
  for (int i = t; i <= n; i += AS_LAYOUT_THREADS) {                // document boundaries: in front of segment i (i == n: behind the last)
    const int lo = i == 0 ? 0 : as_clamp_id(seg[i - 1].doc, n_docs) + 1;
    const int hi = i == n ? n_docs - 1 : as_clamp_id(seg[i].doc, n_docs);
    for (int d = lo; d <= hi; ++d) { doc_seg[d] = i; doc_base[d] = run[i]; }
  }
  if (t == 0) doc_seg[n_docs] = n;
  __syncthreads();
  for (int i = t; i < n; i += AS_LAYOUT_THREADS) offsets[i] = run[i] - doc_base[as_clamp_id(seg[i].doc, n_docs)];
  for (int d = t; d < n_docs; d += AS_LAYOUT_THREADS) totals[d] = run[doc_seg[d + 1]] - doc_base[d];
}

// What a workgroup of the peak and write launches knows about its document; ends(s) = run[s + 1] - base is the first sample behind
// segment s, non-decreasing along the document's segments [seg0, seg1).
struct AsDoc {
  const int64_t* run;
  int64_t base, limit;                                             // samples [0, limit) of the document are written
  int seg0, seg1;
  __device__ __forceinline__ int64_t start(int s) const { return run[s] - base; }
  __device__ __forceinline__ int64_t end(int s) const { return run[s + 1] - base; }
  // the segment that holds sample p (0 <= p < limit): the first s in [lo, hi] with end(s) > p; the caller guarantees end(hi) > p
  __device__ __forceinline__ int find(int64_t p, int lo, int hi) const {
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if (end(mid) > p) hi = mid; else lo = mid + 1;
    }
    return lo;
  }
};

__device__ __forceinline__ bool as_open_doc(const AssembleArgs& a, int d, AsDoc* D) {
  D->run = a.run;
  D->seg0 = a.doc_seg[d];
  D->seg1 = a.doc_seg[d + 1];
  D->base = a.doc_base[d];
  const int64_t total = D->seg1 > D->seg0 ? a.run[D->seg1] - D->base : 0, cap = a.capacity[d];
  D->limit = total < cap ? total : cap;                            // total <= capacity whenever the device table is the planned one
  return D->limit > 0;
}

// ---- peaks -------------------------------------------------------------------------------------------------------------------------
// The same walk as the write launch, over the same tiles; a thread carries the running max of the key it is in (the piece, or its group)
// and hands it over with an integer atomic max when the key changes — non-negative floats order like their bit patterns, so the result
// does not depend on the order of arrival.  Atomics on one word serialise (measured: one per wave of a 4.46 s piece, 400 per word, made
// this launch four times as long as the write launch), so a workgroup walks AS_PEAK_TILES tiles and merges its waves before it sends one.
// The word only ever grows, so a value read first — however stale — can only say "not needed" when that is true.
__device__ __forceinline__ void as_raise_peak(unsigned* peaks, int key, float m) {
  if (m > 0.f && __float_as_uint(m) > __hip_atomic_load(peaks + key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(peaks + key, __float_as_uint(m));
}

template <int V>
__global__ void __launch_bounds__(AS_THREADS) assemble_peaks_kernel(AssembleArgs a) {
  const int d = blockIdx.y;
  AsDoc D;
  if (!as_open_doc(a, d, &D)) return;
  const int mis = (int)((reinterpret_cast<uintptr_t>(a.dst_bases[d]) & 15u) / (16 / V));
  constexpr int64_t SPAN = (int64_t)AS_TILE * AS_PEAK_TILES;       // samples [t0, t0 + SPAN): AS_PEAK_TILES tiles of the write launch
  const int64_t t0 = (int64_t)blockIdx.x * SPAN - mis;
  if (t0 >= D.limit) return;
  const int64_t tl = t0 + SPAN < D.limit ? t0 + SPAN : D.limit;
  const int sA = D.find(t0 < 0 ? 0 : t0, D.seg0, D.seg1 - 1), sB = D.find(tl - 1, sA, D.seg1 - 1);
  int key = -1;
  float m = 0.f;
  for (int64_t q = t0 + (int64_t)threadIdx.x * V; q < tl; q += (int64_t)AS_THREADS * V) {
    int64_t p = q < 0 ? 0 : q;
    const int64_t pe = q + V < tl ? q + V : tl;
    if (p >= pe) continue;
    int s = D.find(p, sA, sB);
    while (p < pe) {
      int64_t e = D.end(s);
      while (e <= p && s < sB) e = D.end(++s);                     // zero-length segments; ends inside [sA, sB] because end(sB) > tl - 1
      const AssembleSegment g = a.seg[s];
      const int64_t stop = e < pe ? e : pe;
      if (stop <= p) break;                                        // cannot happen with this call's own layout
      if (g.src) {
        const int k = a.level == AS_LEVEL_PIECE_PEAK ? s : as_clamp_id(g.group, a.n_groups);
        if (k != key) {
          as_raise_peak(a.peaks, key, m);
          key = k; m = 0.f;
        }
        const float* x = g.src + (p - D.start(s));
        const int64_t cnt = stop - p;
        if (cnt == V && V % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15u) == 0) {
#pragma unroll
          for (int j = 0; j < V / 4; ++j) {
            const float4 v = *reinterpret_cast<const float4*>(x + 4 * j);
            m = fmaxf(fmaxf(m, fabsf(v.x)), fmaxf(fabsf(v.y), fmaxf(fabsf(v.z), fabsf(v.w))));
          }
        } else {
          for (int64_t j = 0; j < cnt; ++j) m = fmaxf(m, fabsf(x[j]));
        }
      }
      p = stop;
    }
  }
  // hand-over: a wave whose lanes all ended in one key reduces to one value, the workgroup's waves merge theirs through LDS, and one
  // thread raises each distinct key once; lanes of a wave that ended in several keys (a tile of many short pieces) raise their own
  __shared__ int w_key[AS_THREADS / 64];
  __shared__ float w_max[AS_THREADS / 64];
  const unsigned long long has = __ballot(m > 0.f);
  int wkey = -1;
  float wmax = 0.f;
  if (has) {
    const int kref = __shfl(key, __ffsll((long long)has) - 1);
    if (__all(m == 0.f || key == kref)) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
      wkey = kref; wmax = m;
    } else {
      as_raise_peak(a.peaks, key, m);
    }
  }
  if ((threadIdx.x & 63) == 0) { w_key[threadIdx.x >> 6] = wkey; w_max[threadIdx.x >> 6] = wmax; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 0; w < AS_THREADS / 64; ++w) {
      float v = w_max[w];
      if (!(v > 0.f)) continue;
      for (int u = w + 1; u < AS_THREADS / 64; ++u)
        if (w_key[u] == w_key[w]) { v = fmaxf(v, w_max[u]); w_max[u] = 0.f; }
      as_raise_peak(a.peaks, w_key[w], v);
    }
  }
}

// ---- write -------------------------------------------------------------------------------------------------------------------------
// The value rules of include/bv2.h, each one numpy reproduces bit for bit: no contraction, IEEE division.
//   peak modes  pk > 0 ? x / pk : 0                      16 bit: (int16)(int)((x / pk) * 32767.f)             (bv2_pcm16's rule)
//   gain modes  v = x * gain                             16 bit: (int16)(int) clamp(v * 32767.f, -32768, 32767) (bv2_loudness_apply's rule)
template <typename T, bool PEAK>
__device__ __forceinline__ T as_value(float x, float k);
template <>
__device__ __forceinline__ float as_value<float, true>(float x, float pk) { return pk > 0.f ? __fdiv_rn(x, pk) : 0.f; }
template <>
__device__ __forceinline__ int16_t as_value<int16_t, true>(float x, float pk) {
  return pk > 0.f ? (int16_t)(int)__fmul_rn(__fdiv_rn(x, pk), 32767.f) : (int16_t)0;
}
template <>
__device__ __forceinline__ float as_value<float, false>(float x, float gain) { return __fmul_rn(x, gain); }
template <>
__device__ __forceinline__ int16_t as_value<int16_t, false>(float x, float gain) {
  return (int16_t)(int)fminf(fmaxf(__fmul_rn(__fmul_rn(x, gain), 32767.f), -32768.f), 32767.f);
}

// A thread owns one 16-byte vector of the destination per pass.  It finds the segment of its first sample by binary search between the
// tile's first and last segment (found once per workgroup, over the whole document), then walks: a run of samples inside one piece is
// loaded as float4 where source and destination share the 16-byte phase and as dwords otherwise, silence is zeros.  A vector that lies
// wholly inside [0, limit) leaves as one 16-byte store; the at most two vectors per document that do not (in front of a base that is
// off the boundary, across the document's end) are stored sample by sample, and nothing at or behind `limit` is written.
template <typename T, bool PEAK>
__global__ void __launch_bounds__(AS_THREADS) assemble_write_kernel(AssembleArgs a) {
  constexpr int V = 16 / (int)sizeof(T);
  const int d = blockIdx.y;
  AsDoc D;
  if (!as_open_doc(a, d, &D)) return;
  T* dst = static_cast<T*>(a.dst_bases[d]);
  const int mis = (int)((reinterpret_cast<uintptr_t>(dst) & 15u) / sizeof(T));
  const int64_t t0 = (int64_t)blockIdx.x * AS_TILE - mis;
  if (t0 >= D.limit) return;
  const int64_t tl = t0 + AS_TILE < D.limit ? t0 + AS_TILE : D.limit;
  const int sA = D.find(t0 < 0 ? 0 : t0, D.seg0, D.seg1 - 1), sB = D.find(tl - 1, sA, D.seg1 - 1);
  for (int64_t q = t0 + (int64_t)threadIdx.x * V; q < tl; q += (int64_t)AS_THREADS * V) {
    int64_t p = q < 0 ? 0 : q;
    const int64_t pe = q + V < tl ? q + V : tl;
    if (p >= pe) continue;
    const int first = (int)(p - q);                                // o[first .. first + (pe - p)) are the samples to store
    T o[V];
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = (T)0;
    int s = D.find(p, sA, sB);
    while (p < pe) {
      int64_t e = D.end(s);
      while (e <= p && s < sB) e = D.end(++s);
      const AssembleSegment g = a.seg[s];
      const int64_t stop = e < pe ? e : pe;
      if (stop <= p) break;                                        // cannot happen with this call's own layout
      if (g.src) {
        float k;
        if (PEAK) k = __uint_as_float(a.peaks[a.level == AS_LEVEL_PIECE_PEAK ? s : as_clamp_id(g.group, a.n_groups)]);
        else k = a.gain ? a.gain[as_clamp_id(g.group, a.n_groups)] : 1.f;
        const float* x = g.src + (p - D.start(s));
        if (stop - p == V && (reinterpret_cast<uintptr_t>(x) & 15u) == 0) {      // the whole vector, source on the same phase
#pragma unroll
          for (int j = 0; j < V / 4; ++j) {
            const float4 v = *reinterpret_cast<const float4*>(x + 4 * j);
            o[4 * j] = as_value<T, PEAK>(v.x, k); o[4 * j + 1] = as_value<T, PEAK>(v.y, k);
            o[4 * j + 2] = as_value<T, PEAK>(v.z, k); o[4 * j + 3] = as_value<T, PEAK>(v.w, k);
          }
        } else if (stop - p == V) {
#pragma unroll
          for (int j = 0; j < V; ++j) o[j] = as_value<T, PEAK>(x[j], k);
        } else {
          const int at = (int)(p - q), cnt = (int)(stop - p);
#pragma unroll
          for (int j = 0; j < V; ++j)
            if (j >= at && j < at + cnt) o[j] = as_value<T, PEAK>(x[j - at], k);
        }
      }
      p = stop;
    }
    if (first == 0 && pe - q == V) {
      uint4 pk;
      __builtin_memcpy(&pk, o, 16);
      *reinterpret_cast<uint4*>(dst + q) = pk;
    } else {
      const int cnt = (int)(pe - q);
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (j >= first && j < cnt) dst[q + j] = o[j];
    }
  }
}

int launch_assemble(hipStream_t stream, const AssembleArgs& a) {
  if (a.n_segments < 1 || a.n_segments > AS_MAX_SEGMENTS || a.n_docs < 1 || a.n_docs > AS_MAX_DOCS || a.n_groups < 1 ||
      a.n_groups > a.n_segments || a.max_capacity < 0 || a.max_capacity > AS_MAX_CAPACITY)
    return -1;
  hipLaunchKernelGGL(assemble_layout_kernel, dim3(1), dim3(AS_LAYOUT_THREADS), 0, stream, a.seg, a.n_segments, a.n_docs, a.run, a.doc_base,
                     a.doc_seg, a.peaks, a.offsets, a.totals);
  if (a.max_capacity > 0) {
    const int V = a.pcm16 ? 8 : 4;
    const dim3 grid((unsigned)((a.max_capacity + V - 1 + AS_TILE - 1) / AS_TILE), (unsigned)a.n_docs), block(AS_THREADS);
    const bool peak = a.level == AS_LEVEL_PIECE_PEAK || a.level == AS_LEVEL_GROUP_PEAK;
    if (peak) {
      const dim3 pgrid((grid.x + AS_PEAK_TILES - 1) / AS_PEAK_TILES, grid.y);
      if (a.pcm16) hipLaunchKernelGGL(assemble_peaks_kernel<8>, pgrid, block, 0, stream, a);
      else hipLaunchKernelGGL(assemble_peaks_kernel<4>, pgrid, block, 0, stream, a);
    }
    if (a.pcm16) {
      if (peak) hipLaunchKernelGGL((assemble_write_kernel<int16_t, true>), grid, block, 0, stream, a);
      else hipLaunchKernelGGL((assemble_write_kernel<int16_t, false>), grid, block, 0, stream, a);
    } else {
      if (peak) hipLaunchKernelGGL((assemble_write_kernel<float, true>), grid, block, 0, stream, a);
      else hipLaunchKernelGGL((assemble_write_kernel<float, false>), grid, block, 0, stream, a);
    }
  }
  return BV2_CHECK_LAUNCH();
}

}  // namespace bv2
