// align.hip — the two kernels of the reference's forced aligner (SynthesizerTrn.forward, models.py:960-991): the negative cross-entropy
// matrix between a recording's latent frames and the text's prior (neg_cent), and monotonic_align.maximum_path over it (maximum_path).
// The noise-scaled-MAS term of models.py:976-982 (use_noise_scaled_mas, a training-time perturbation drawn with randn_like) is NOT
// implemented: the matrix is the deterministic one.
//
// neg_cent (models.py:962-975).  For item b, frame y, symbol x, D = inter_channels, r[d,x] = exp(-2 logs_p[d,x]):
//     out[b,y,x] = c1[x] + sum_d (-1/2 z_p[d,y]^2) r[d,x] + sum_d z_p[d,y] (m_p[d,x] r[d,x]) + c4[x]
//     c1[x] = sum_d (-1/2 log 2pi - logs_p[d,x]),   c4[x] = sum_d -1/2 m_p[d,x]^2 r[d,x]
// which is the reference's neg_cent1 + neg_cent2 + neg_cent3 + neg_cent4 in that order of addition; the two matrix products are the two
// halves of one K = 2 D product with A rows [-1/2 z_p^2, z_p] and B columns [r, m r], kept in two accumulators (two independent MFMA
// chains, and the reference's own grouping of the sum).  Both operands differ per batch item, so this is not a conv.  A workgroup of four
// waves owns 64 frames x 16 symbols: its prologue forms the B operand [2 D][16] and the two column constants in LDS straight from
// m_p / logs_p (no intermediate tensor), then every wave runs D / 4 steps of two v_mfma_f32_16x16x4_f32 — A[m = l & 15][k = l >> 4] read
// from z_p (16 consecutive frames per lane group: 64-byte segments), B[k = l >> 4][n = l & 15] from LDS (64 consecutive words: no bank
// conflict), D register i = frame 4 (l >> 4) + i, symbol l & 15.  Cells outside y < y_lengths[b], x < x_lengths[b] are written as 0.
//
// maximum_path (monotonic_align/core.py).  One workgroup per batch item; thread t owns the symbols x = t + j NT, j < XPT.
//   forward   rows y in sequence, the previous row of cumulative values in LDS (two rows, ping-pong: ONE barrier per row), inside the
//             reference's band max(0, t_x + y - t_y) <= x < min(t_x, y + 1):
//                 v_cur = x == y ? -1e9 : prev[x];   v_prev = x == 0 ? (y == 0 ? 0 : -1e9) : prev[x - 1]
//                 cur[x] = neg_cent[y][x] + max(v_prev, v_cur)
//             plain fp32 add and max, one chain per cell: the result does not depend on NT or XPT.  neg_cent is only read (const): the
//             cumulative matrix is never stored.  What the backtrack needs of it is ONE bit per cell,
//                 move[y][x] = x != 0 && (x == y || prev[x] < prev[x - 1])       (the reference's tie rule: strictly greater on the left)
//             recorded as a wave ballot per row into the workspace ([Ty][ceil(T / 64)] 64-bit words per item).  The matrix values of the
//             next MP_PF rows are loaded into registers while the current MP_PF rows run, so a row does not wait for global memory.
//   backtrack chunks of rows, last to first: all threads stage the chunk's bit rows into LDS, thread 0 walks them (an LDS read per
//             row — never a chain of dependent global loads), leaving the chosen symbol of every row and the frame count of every
//             symbol in LDS; then all threads write the chunk's one-hot attn rows (when asked for).
//   outputs   durations [B][T] int64 (0 past x_lengths), attn [B][Ty][T] fp32 one-hot (optional), score [B] = the cumulative value of
//             the last cell (optional).
// Precondition x_lengths[b] <= y_lengths[b] (the reference's band is empty otherwise); lengths are clamped to [0, T] / [0, Ty], an item
// with a zero length gets zero durations and a zero score, and no index leaves its array whatever the lengths say.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../bv2_kernels.h"
#include "rng.h"

namespace bv2 {

#define BV2_CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -1)

// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int NC_WAVES = 4;                       // 16 frames each
constexpr int NC_THREADS = 64 * NC_WAVES;
constexpr int NC_TY = 16 * NC_WAVES, NC_TX = 16;  // the workgroup's tile: frames x symbols

__global__ void __launch_bounds__(NC_THREADS) neg_cent_kernel(const NegCentArgs A) {
  extern __shared__ __attribute__((aligned(16))) float nc_smem[];
  const int D = A.D, T = A.T, Ty = A.Ty;
  float* Br = nc_smem;                            // [D][16]  r
  float* Bm = Br + (size_t)D * NC_TX;             // [D][16]  m r
  float* cp = Bm + (size_t)D * NC_TX;             // [2][16 parts][16]  partial column constants
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b = blockIdx.z, x0 = blockIdx.x * NC_TX, y0 = blockIdx.y * NC_TY;
  int tx = A.x_lengths ? (int)A.x_lengths[b] : T, ty = A.y_lengths ? (int)A.y_lengths[b] : Ty;
  tx = tx < 0 ? 0 : (tx > T ? T : tx);
  ty = ty < 0 ? 0 : (ty > Ty ? Ty : ty);

  {
    // prologue: thread (part, n) walks the channels d = part, part + 16, ... of symbol x0 + n; a symbol past x_lengths is never loaded
    const int n = tid & 15, part = tid >> 4, x = x0 + n;
    const bool ok = x < tx;
    const float* mp = A.m_p + ((int64_t)b * D) * T + x;
    const float* lp = A.logs_p + ((int64_t)b * D) * T + x;
    float c1 = 0.f, c4 = 0.f;
    for (int d = part; d < D; d += NC_THREADS / 16) {
      float r = 0.f, mr = 0.f;
      if (ok) {
        const float m = mp[(int64_t)d * T], ls = lp[(int64_t)d * T];
        r = expf(-2.f * ls);
        mr = m * r;
        c1 += -0.91893853320467274178f - ls;      // -1/2 log(2 pi)
        c4 += -0.5f * (m * m) * r;
      }
      Br[d * NC_TX + n] = r;
      Bm[d * NC_TX + n] = mr;
    }
    cp[part * NC_TX + n] = c1;
    cp[(16 + part) * NC_TX + n] = c4;
  }
  __syncthreads();

  const int n = lane & 15, g = lane >> 4;
  const int ya = y0 + 16 * wid + n;               // the frame of this lane's A row
  const bool ya_ok = ya < ty;
  const float* zp = A.z_p + ((int64_t)b * D) * Ty + (ya_ok ? ya : 0);
  typedef float f4 __attribute__((ext_vector_type(4)));
  f4 acc2 = {0.f, 0.f, 0.f, 0.f}, acc3 = {0.f, 0.f, 0.f, 0.f};
  if (y0 + 16 * wid < ty) {                       // wave-uniform: a tile of padded frames has nothing to multiply
    for (int s = 0; s < D / 4; ++s) {
      const int d = 4 * s + g;
      const float z = ya_ok ? zp[(int64_t)d * Ty] : 0.f;
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(-0.5f * (z * z), Br[d * NC_TX + n], acc2, 0, 0, 0);
      acc3 = __builtin_amdgcn_mfma_f32_16x16x4f32(z, Bm[d * NC_TX + n], acc3, 0, 0, 0);
    }
  }
  float c1 = 0.f, c4 = 0.f;
#pragma unroll
  for (int p = 0; p < 16; ++p) { c1 += cp[p * NC_TX + n]; c4 += cp[(16 + p) * NC_TX + n]; }   // fixed order
  const int x = x0 + n;
  if (x < T) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int y = y0 + 16 * wid + 4 * g + i;
      if (y < Ty) {
        const float v = ((c1 + acc2[i]) + acc3[i]) + c4;
        A.out[((int64_t)b * Ty + y) * T + x] = (y < ty && x < tx) ? v : 0.f;
      }
    }
  }
}

int64_t neg_cent_lds_bytes(int D) { return (int64_t)sizeof(float) * (2 * (int64_t)D * NC_TX + 2 * 16 * NC_TX); }

int launch_neg_cent(hipStream_t stream, const NegCentArgs& a) {
  if (a.B < 1 || a.B > 65535 || a.T < 1 || a.Ty < 1 || a.D < 4 || a.D % 4 || a.D > NC_MAX_D) return -1;
  const int64_t gy = (a.Ty + NC_TY - 1) / NC_TY;
  if (gy > 65535) return -1;
  const dim3 grid((unsigned)((a.T + NC_TX - 1) / NC_TX), (unsigned)gy, (unsigned)a.B), block(NC_THREADS);
  hipLaunchKernelGGL(neg_cent_kernel, grid, block, (size_t)neg_cent_lds_bytes(a.D), stream, a);
  return BV2_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int MP_PF = 4;                          // rows of matrix values in flight ahead of the row being computed
constexpr int MP_BITS_LDS = 2048;                 // 64-bit words of a staged backtrack chunk (16 KB)
constexpr float MP_NEG = -1e9f;                   // the reference's max_neg_val (exact in fp32)

inline int mp_words(int T) { return (T + 63) / 64; }
inline int mp_chunk_rows(int T) { const int r = MP_BITS_LDS / mp_words(T); return r > 1024 ? 1024 : r; }

template <int XPT>
__global__ void __launch_bounds__(1024) maximum_path_kernel(const MaxPathArgs A, const int chunk_rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mp_smem[];
  const int T = A.T, Ty = A.Ty, W = (T + 63) / 64;
  float* row = reinterpret_cast<float*>(mp_smem);                               // [2][T] cumulative values, ping-pong
  int* cnt = reinterpret_cast<int*>(mp_smem);                                   // [T] frames per symbol (the backtrack reuses the rows)
  unsigned long long* bits = reinterpret_cast<unsigned long long*>(mp_smem + sizeof(float) * 2 * (size_t)((T + 1) & ~1));   // [chunk_rows][W]
  int* sel = reinterpret_cast<int*>(bits + (size_t)chunk_rows * W);             // [chunk_rows] the path's symbol per row
  const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63;
  const int b = blockIdx.x;
  int tx = A.x_lengths ? (int)A.x_lengths[b] : T, ty = A.y_lengths ? (int)A.y_lengths[b] : Ty;
  tx = tx < 0 ? 0 : (tx > T ? T : tx);
  ty = ty < 0 ? 0 : (ty > Ty ? Ty : ty);
  const float* val = A.neg_cent + (int64_t)b * Ty * T;
  unsigned long long* gbits = A.bits + (int64_t)b * Ty * W;
  int64_t* dur = A.durations + (int64_t)b * T;

  for (int e = tid; e < 2 * T; e += NT) row[e] = MP_NEG;
  __syncthreads();

  // ---- forward
  float cur[XPT][MP_PF], nxt[XPT][MP_PF];
  auto fetch = [&](float (&dst)[XPT][MP_PF], int yb) {
#pragma unroll
    for (int j = 0; j < XPT; ++j) {
      const int x = tid + j * NT;
#pragma unroll
      for (int q = 0; q < MP_PF; ++q) {
        const int y = yb + q;
        dst[j][q] = (x < tx && y < ty) ? val[(int64_t)y * T + x] : 0.f;
      }
    }
  };
  fetch(cur, 0);
  for (int yb = 0; yb < ty; yb += MP_PF) {
    fetch(nxt, yb + MP_PF);
#pragma unroll
    for (int q = 0; q < MP_PF; ++q) {
      const int y = yb + q;
      if (y < ty) {                                                             // block-uniform
        const float* prev = row + ((y + 1) & 1) * T;
        float* out = row + (y & 1) * T;
        const int lo = tx + y - ty > 0 ? tx + y - ty : 0, hi = tx < y + 1 ? tx : y + 1;
#pragma unroll
        for (int j = 0; j < XPT; ++j) {
          const int x = tid + j * NT;
          const bool in = x >= lo && x < hi;
          bool move = false;
          if (in) {
            const float v_cur = x == y ? MP_NEG : prev[x];
            const float v_prev = x == 0 ? (y == 0 ? 0.f : MP_NEG) : prev[x - 1];
            move = x != 0 && (x == y || v_cur < v_prev);
            out[x] = cur[j][q] + fmaxf(v_prev, v_cur);
          }
          const unsigned long long m = __ballot(move);
          const int w = (tid >> 6) + j * (NT >> 6);                             // the word of this wave's 64 symbols
          if (lane == 0 && w < W) gbits[(int64_t)y * W + w] = m;
        }
        __syncthreads();
      }
    }
#pragma unroll
    for (int j = 0; j < XPT; ++j)
#pragma unroll
      for (int q = 0; q < MP_PF; ++q) cur[j][q] = nxt[j][q];
  }
  if (A.score && tid == 0) A.score[b] = (tx > 0 && ty > 0) ? row[((ty - 1) & 1) * T + tx - 1] : 0.f;
  __syncthreads();                                                              // the rows are read; every bit row is written

  // ---- backtrack
  for (int e = tid; e < T; e += NT) cnt[e] = 0;
  int index = tx - 1;                                                           // thread 0's walk state
  for (int y1 = ty; y1 > 0; y1 -= chunk_rows) {
    const int yc = y1 - chunk_rows > 0 ? y1 - chunk_rows : 0, nr = y1 - yc;
    __syncthreads();                                                            // the previous chunk's sel / bits are consumed
    for (int e = tid; e < nr * W; e += NT) bits[e] = gbits[(int64_t)yc * W + e];
    __syncthreads();
    if (tid == 0 && tx > 0) {
      for (int r = nr - 1; r >= 0; --r) {
        const int y = yc + r;
        sel[r] = index;
        cnt[index] += 1;
        if (index != 0 && (index == y || ((bits[r * W + (index >> 6)] >> (index & 63)) & 1ull))) --index;
      }
    }
    __syncthreads();
    if (A.attn && tx > 0) {
      float* at = A.attn + ((int64_t)b * Ty + yc) * T;
      for (int e = tid; e < nr * T; e += NT) {
        const int r = e / T, x = e - r * T;
        at[e] = sel[r] == x ? 1.f : 0.f;
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < T; e += NT) dur[e] = (e < tx && ty > 0) ? (int64_t)cnt[e] : 0;
  if (A.attn) {                                                                 // rows past y_lengths (all rows of an empty item) are zeros
    const int yz = tx > 0 ? ty : 0;
    float* at = A.attn + ((int64_t)b * Ty + yz) * T;
    const int64_t n = (int64_t)(Ty - yz) * T;
    for (int64_t e = tid; e < n; e += NT) at[e] = 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// PosteriorEncoder's last line (models.py:486): z = (m + noise * exp(logs) * scale) * mask; the noise is the caller's draw (null: z = m * mask)
// or, with seeds [B], the value of (seeds[b], RNG_NOISE_Q, channel, frame) computed here (kernels/rng.h)
__global__ void __launch_bounds__(256) posterior_sample_kernel(const float* m, const float* logs, const float* noise, float scale,
                                                               const float* mask, float* z, int C, int T, const int64_t* seeds) {
  const int b = blockIdx.z, ch = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const int64_t i = ((int64_t)b * C + ch) * T + t;
  const float mk = mask[(int64_t)b * T + t];
  float v = m[i];
  if (noise || seeds) {
    const float nz = seeds ? seeded_normal(seeds[b], RNG_NOISE_Q, ch, t) : noise[i];
    v = v + nz * expf(logs[i]) * scale;
  }
  z[i] = mk != 0.f ? v * mk : 0.f;                    // a masked frame is selected to zero: its noise may hold anything
}

int launch_posterior_sample(hipStream_t stream, const float* m, const float* logs, const float* noise, float scale, const float* mask,
                            float* z, int B, int C, int T, const int64_t* seeds) {
  if (B < 1 || B > 65535 || C < 1 || C > 65535 || T < 1) return -1;
  hipLaunchKernelGGL(posterior_sample_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)C, (unsigned)B), dim3(256), 0, stream, m, logs, noise,
                     scale, mask, z, C, T, seeds);
  return BV2_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The KL term of SynthesizerTrn.forward() along the path (losses.py:45-61), per frame.  A workgroup owns 256 frames of one item: it
// forms the inclusive cumulative durations of the item's symbols in LDS (wave 0, 64 symbols per step, integer adds: exact), every thread
// then finds its frame's symbol by bisection — the gather `expand` does, no [Ty x T] product — and walks the channels.
constexpr int KL_THREADS = 256;

__global__ void __launch_bounds__(KL_THREADS) kl_path_kernel(const KlPathArgs A) {
  __shared__ int cum[MP_MAX_T];                                      // cum[s] = frames of symbols 0 .. s
  const int tid = threadIdx.x, b = blockIdx.y, T = A.T, Ty = A.Ty, D = A.D;
  int tx = A.x_lengths ? (int)A.x_lengths[b] : T, ty = A.y_lengths ? (int)A.y_lengths[b] : Ty;
  tx = tx < 0 ? 0 : (tx > T ? T : tx);
  ty = ty < 0 ? 0 : (ty > Ty ? Ty : ty);
  if (tid < 64) {
    int carry = 0;
    for (int s0 = 0; s0 < tx; s0 += 64) {
      const int s = s0 + tid;
      float wf = s < tx ? A.w_ceil[(int64_t)b * T + s] : 0.f;
      wf = wf > 0.f ? (wf < 16777216.f ? wf : 16777216.f) : 0.f;   // negative / NaN durations count as 0
      int v = (int)wf;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(v, off);
        if (tid >= off) v += u;
      }
      v += carry;
      if (s < tx) cum[s] = v;
      carry = __shfl(v, 63);
    }
  }
  __syncthreads();
  const int j = blockIdx.x * KL_THREADS + tid;
  if (j >= Ty) return;
  float* out = A.kl_frame + (int64_t)b * Ty + j;
  if (j >= ty || tx < 1) { *out = 0.f; return; }
  int lo = 0, hi = tx - 1;                                           // the first symbol whose cumulative duration exceeds j; the last one otherwise
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cum[mid] > j) hi = mid; else lo = mid + 1;
  }
  const int s = lo;
  const float* zp = A.z_p + ((int64_t)b * D) * Ty + j;
  const float* lq = A.logs_q + ((int64_t)b * D) * Ty + j;
  const float* mp = A.m_p + ((int64_t)b * D) * T + s;
  const float* lp = A.logs_p + ((int64_t)b * D) * T + s;
  double a[4] = {0.0, 0.0, 0.0, 0.0};                                  // fp32 terms as the reference forms them, fp64 sums
  for (int c0 = 0; c0 < D; c0 += 4) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = c0 + q;
      if (c < D) {
        const float l = lp[(int64_t)c * T], d = zp[(int64_t)c * Ty] - mp[(int64_t)c * T];
        float k = (l - lq[(int64_t)c * Ty]) - 0.5f;
        k = k + (0.5f * (d * d)) * expf(-2.f * l);
        a[q] = a[q] + (double)k;
      }
    }
  }
  *out = (float)((a[0] + a[1]) + (a[2] + a[3]));
}

int launch_kl_path(hipStream_t stream, const KlPathArgs& a) {
  if (a.B < 1 || a.B > 65535 || a.T < 1 || a.T > MP_MAX_T || a.Ty < 1 || a.D < 1) return -1;
  if (!a.z_p || !a.logs_q || !a.m_p || !a.logs_p || !a.w_ceil || !a.kl_frame || !a.kl) return -1;
  hipLaunchKernelGGL(kl_path_kernel, dim3((unsigned)((a.Ty + KL_THREADS - 1) / KL_THREADS), (unsigned)a.B), dim3(KL_THREADS), 0, stream, a);
  if (BV2_CHECK_LAUNCH()) return -1;
  return launch_row_sum(stream, a.kl_frame, a.kl, a.B, a.Ty);
}

int64_t maximum_path_workspace_bytes(int B, int T, int Ty) { return (int64_t)B * Ty * mp_words(T) * 8; }

int64_t maximum_path_lds_bytes(int T) {
  return (int64_t)sizeof(float) * 2 * ((T + 1) & ~1) + (int64_t)mp_chunk_rows(T) * mp_words(T) * 8 + (int64_t)mp_chunk_rows(T) * 4;
}

int launch_maximum_path(hipStream_t stream, const MaxPathArgs& a) {
  if (a.B < 1 || a.B > 65535 || a.T < 1 || a.T > MP_MAX_T || a.Ty < 1) return -1;
  int nt = (a.T + 63) / 64 * 64;
  nt = nt > 1024 ? 1024 : nt;
  const int xpt = (a.T + nt - 1) / nt;
  const int rows = mp_chunk_rows(a.T);
  const size_t lds = (size_t)maximum_path_lds_bytes(a.T);
  const dim3 grid((unsigned)a.B), block((unsigned)nt);
  if (xpt <= 1) hipLaunchKernelGGL(maximum_path_kernel<1>, grid, block, lds, stream, a, rows);
  else if (xpt <= 2) hipLaunchKernelGGL(maximum_path_kernel<2>, grid, block, lds, stream, a, rows);
  else hipLaunchKernelGGL(maximum_path_kernel<4>, grid, block, lds, stream, a, rows);     // T <= MP_MAX_T = 4096
  return BV2_CHECK_LAUNCH();
}

}  // namespace bv2
