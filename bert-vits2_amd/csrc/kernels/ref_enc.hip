// ref_enc.hip — ReferenceEncoder (reference models.py:752-808): the speaker vector g of a model without a speaker table, computed from a
// linear spectrogram y [B, spec, L] viewed as a one-channel image [B, 1, L, spec].
//
//   six weight-normed Conv2d(3x3, stride 2, pad 1) + ReLU, widths 1 -> 32 -> 32 -> 64 -> 64 -> 128 -> 128   (activations [B][C][H = time][W = freq])
//   transpose to [B, H6, 128 * W6], GRU(128 * W6 -> 128), final hidden state -> Linear(128 -> gin)
//
// A short chain of small launches (0.5 GMAC at L = 400), EIGHT per call: conv 1 (direct, 9 taps), convs 2-6 (one launch each), the GRU input
// projection for all steps at once, and the recurrence + proj.  Everything is plain fp32 FMA: g feeds the text encoder and both duration
// predictors, and durations go through ceil().
//
// Summation order.  Every output element is produced by ONE thread (conv) or one wave (GEMM rows) in an order that depends on the layer's
// channel counts only — never on L, B or the lengths.  Convs 2-6 sum K = 9 * C_in in chunks of 16 input channels (144 terms into a fresh
// accumulator, chunk totals added in order), which keeps the rounding error of the long sums at the level of a blocked CPU GEMM.
//
// Ragged batches (y_lengths).  Item b's length at the input of layer i is n_i = (n_{i-1} - 1) / 2 + 1, n_0 = y_lengths[b]; every layer reads
// rows >= n_i as zero padding and does not produce rows >= n_{i+1}, the GRU runs n_6 steps.  Masking changes which taps are zero, not the
// order of a sum, so each item of a padded batch gets bit for bit the g it gets alone.  (The reference has no mask here: bias and ReLU make
// the padded region non-zero and it leaks into g.)
#include <hip/hip_runtime.h>
#include <math.h>
#include "../bv2_kernels.h"

namespace bv2 {

#define BV2_CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -1)

namespace {

constexpr int RE_CK = 16;                 // input channels per LDS-staged chunk (every C_in of convs 2-6 is a multiple of it)
constexpr int RE_TW = 64;                 // output columns per workgroup of convs 2-6 (one per lane)
constexpr int RE_PW = 2 * RE_TW + 1;      // staged input columns
constexpr int RE_NC = 8;                  // output channels per wave (weights of one tap: 8 consecutive floats, wave-uniform)
constexpr int RE_HID = 128;               // GRU hidden size (256 // 2, models.py:782)
constexpr int RE_GATES = 3 * RE_HID;

__host__ __device__ inline int re_down(int n) { return (n - 1) / 2 + 1; }

// length of item b on the time axis after `layer` convs (layer 0 = the spectrogram itself)
__device__ __forceinline__ int re_len(const int64_t* yl, int b, int L, int layer) {
  long long n = yl ? (long long)yl[b] : (long long)L;
  n = n < 1 ? 1 : (n > L ? L : n);
  int v = (int)n;
  for (int i = 0; i < layer; ++i) v = re_down(v);
  return v;
}

// ---- conv 1: C_in = 1, 32 output channels in registers; a 16 x 16 output tile per workgroup, its 33 x 33 input patch through LDS
// (the spectrogram is time-contiguous, the image frequency-contiguous: the patch is loaded along time and read along frequency)
__global__ void __launch_bounds__(256) ref_conv1_kernel(const float* __restrict__ y, int64_t sb, int64_t sf, int64_t st,
                                                        const int64_t* __restrict__ yl, int L, int spec, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ out, int H1, int W1) {
  __shared__ float p[33][34];                       // [freq][time]
  const int b = blockIdx.z, h0 = blockIdx.y * 16, w0 = blockIdx.x * 16;
  const int n0 = re_len(yl, b, L, 0), n1 = re_down(n0);
  if (h0 >= n1) return;                             // uniform: rows past this item's end are never read
  for (int i = threadIdx.x; i < 33 * 33; i += 256) {
    const int fl = i / 33, tl = i - fl * 33;
    const int f = 2 * w0 - 1 + fl, t = 2 * h0 - 1 + tl;
    float v = 0.f;
    if (f >= 0 && f < spec && t >= 0 && t < n0) v = y[(int64_t)b * sb + (int64_t)f * sf + (int64_t)t * st];
    p[fl][tl] = v;
  }
  __syncthreads();
  const int hl = threadIdx.x >> 4, wl = threadIdx.x & 15;
  const int ho = h0 + hl, wo = w0 + wl;
  float x[9];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) x[kh * 3 + kw] = p[2 * wl + kw][2 * hl + kh];
  if (ho >= n1 || wo >= W1) return;
  float* o = out + ((int64_t)b * 32 * H1 + ho) * W1 + wo;
#pragma unroll 4
  for (int co = 0; co < 32; ++co) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 9; ++j) acc = fmaf(w[j * 32 + co], x[j], acc);     // w [tap][32]: wave-uniform
    acc += bias[co];
    o[(int64_t)co * H1 * W1] = acc > 0.f ? acc : 0.f;
  }
}

// ---- convs 2-6: implicit GEMM, K = 9 * C_in.  A workgroup owns one output row, 64 output columns and 32 output channels: lane = column,
// wave = 8 channels.  Per chunk of 16 input channels the 3-row input patch AND the chunk's weights are staged in LDS (the patch row by row,
// independent loads in flight; the weights of a wave are one contiguous run of the packed tensor); the 8 weights of a (channel, tap) are
// then two broadcast 16-byte LDS reads.  Bias and ReLU in the epilogue.
// in [B][Cin][Hin][Win], out [B][Cout][Hout][Wout], w [Cout/8][Cin][9][8]; grid (column tiles * Cout/32, Hout, B); `layer` = index of the
// INPUT tensor in the length chain (1 for conv 2).
__global__ void __launch_bounds__(256) ref_conv_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ out,
                                                       const int64_t* __restrict__ yl, int L, int layer, int Cin, int Cout, int Hin,
                                                       int Win, int Hout, int Wout, int ncg) {
  __shared__ float patch[RE_CK * 3][RE_PW + 3];                               // row = channel * 3 + kernel row
  __shared__ __attribute__((aligned(16))) float wl[4][RE_CK * 9 * RE_NC];     // per wave: [channel][tap][8]
  const int b = blockIdx.z, ho = blockIdx.y;
  const int cgrp = (int)blockIdx.x % ncg, w0 = ((int)blockIdx.x / ncg) * RE_TW;
  const int nin = re_len(yl, b, L, layer), nout = re_down(nin);
  if (ho >= nout) return;                           // uniform per workgroup
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int c8 = cgrp * 4 + wave;                   // this wave's group of 8 output channels
  const float* wg = w + (int64_t)c8 * Cin * 9 * RE_NC;
  const float* inb = in + (int64_t)b * Cin * Hin * Win;
  const int win0 = 2 * w0 - 1;
  float tot[RE_NC];
#pragma unroll
  for (int j = 0; j < RE_NC; ++j) tot[j] = 0.f;
  for (int c0 = 0; c0 < Cin; c0 += RE_CK) {
    __syncthreads();                                // the previous chunk's reads are done
    // this wave's weights of the chunk: RE_CK * 72 consecutive floats
    {
      const float4* src = reinterpret_cast<const float4*>(wg + (int64_t)c0 * 9 * RE_NC);
      float4* dst = reinterpret_cast<float4*>(wl[wave]);
      for (int i = lane; i < RE_CK * 9 * RE_NC / 4; i += 64) dst[i] = src[i];
    }
    // the patch: wave v stages rows v, v + 4, ... (a row = 129 input columns of one channel and kernel row; columns lane, lane + 64, 128).
    // All loads are issued before the first LDS write, from clamped (always valid) addresses; padding is a select, not a branch.
    {
      constexpr int NR = RE_CK * 3 / 4;
      const int wa = win0 + lane, wb = wa + 64, wc = win0 + 128;
      const int ia = wa < 0 ? 0 : (wa < Win ? wa : Win - 1), ib = wb < Win ? wb : Win - 1, ic = wc < Win ? wc : Win - 1;
      float va[NR], vb[NR], vc[NR];
#pragma unroll
      for (int q = 0; q < NR; ++q) {
        const int row = wave + 4 * q, ci = row / 3, r = row - 3 * ci;
        const int hin = 2 * ho - 1 + r;
        const int hc = hin < 0 ? 0 : (hin < nin ? hin : nin - 1);
        const float* src = inb + ((int64_t)(c0 + ci) * Hin + hc) * Win;
        va[q] = src[ia]; vb[q] = src[ib]; vc[q] = src[ic];
      }
#pragma unroll
      for (int q = 0; q < NR; ++q) {
        const int row = wave + 4 * q, r = row % 3;
        const int hin = 2 * ho - 1 + r;
        const bool rok = hin >= 0 && hin < nin;       // wave-uniform
        patch[row][lane] = (rok && wa >= 0 && wa < Win) ? va[q] : 0.f;
        patch[row][lane + 64] = (rok && wb < Win) ? vb[q] : 0.f;
        if (lane == 0) patch[row][128] = (rok && wc < Win) ? vc[q] : 0.f;
      }
    }
    __syncthreads();
    float acc[RE_NC];
#pragma unroll
    for (int j = 0; j < RE_NC; ++j) acc[j] = 0.f;
#pragma unroll 8
    for (int ci = 0; ci < RE_CK; ++ci) {            // unrolled deep: the LDS reads of many taps are in flight at once
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const float x = patch[ci * 3 + kh][2 * lane + kw];
          const float4* wt = reinterpret_cast<const float4*>(&wl[wave][(ci * 9 + kh * 3 + kw) * RE_NC]);
          const float4 u = wt[0], v = wt[1];
          acc[0] = fmaf(u.x, x, acc[0]); acc[1] = fmaf(u.y, x, acc[1]); acc[2] = fmaf(u.z, x, acc[2]); acc[3] = fmaf(u.w, x, acc[3]);
          acc[4] = fmaf(v.x, x, acc[4]); acc[5] = fmaf(v.y, x, acc[5]); acc[6] = fmaf(v.z, x, acc[6]); acc[7] = fmaf(v.w, x, acc[7]);
        }
    }
#pragma unroll
    for (int j = 0; j < RE_NC; ++j) tot[j] += acc[j];
  }
  const int wo = w0 + lane;
  if (wo >= Wout) return;
#pragma unroll
  for (int j = 0; j < RE_NC; ++j) {
    const int co = c8 * RE_NC + j;
    const float v = tot[j] + bias[co];
    out[(((int64_t)b * Cout + co) * Hout + ho) * Wout + wo] = v > 0.f ? v : 0.f;
  }
}

// ---- GRU input projection for all steps at once: gi[b][t][j] = b_ih[j] + sum_k W_ih[j][k] * X[b][t][k], k = c * W6 + f (the reference's
// transpose(1, 2).view(N, T, -1), models.py:795-798, as an index change on conv 6's own [B][128][H6][W6] layout).  One wave per gate row j
// and up to 8 steps; lanes split K (lane, lane + 64, ...), then a fixed butterfly.  grid (384 / 4, ceil(H6 / 8), B).
__global__ void __launch_bounds__(256) ref_gru_in_kernel(const float* __restrict__ x, const float* __restrict__ w_ih,
                                                         const float* __restrict__ b_ih, float* __restrict__ gi,
                                                         const int64_t* __restrict__ yl, int L, int H6, int W6) {
  const int b = blockIdx.z, t0 = blockIdx.y * 8;
  const int n6 = re_len(yl, b, L, 6);
  if (t0 >= n6) return;
  const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int K = RE_HID * W6;
  const float* wr = w_ih + (int64_t)j * K;
  const float* xb = x + (int64_t)b * RE_HID * H6 * W6;
  const int nt = n6 - t0 < 8 ? n6 - t0 : 8;
  float acc[8];
  int toff[8];                                      // steps past the item's end read its last step (a valid address); their sums are dropped
#pragma unroll
  for (int s = 0; s < 8; ++s) { acc[s] = 0.f; toff[s] = (s < nt ? t0 + s : n6 - 1) * W6; }
#pragma unroll 4
  for (int k = lane; k < K; k += 64) {              // K = 128 * W6 is a multiple of 64: every lane runs the same trip count, no branches
    const int c = k / W6, f = k - c * W6;
    const float wv = wr[k];
    const float* xp = xb + (int64_t)c * H6 * W6 + f;
#pragma unroll
    for (int s = 0; s < 8; ++s) acc[s] = fmaf(wv, xp[toff[s]], acc[s]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int s = 0; s < 8; ++s) acc[s] += __shfl_xor(acc[s], off);
  if (lane == 0) {
    const float bj = b_ih[j];
#pragma unroll
    for (int s = 0; s < 8; ++s)
      if (s < nt) gi[((int64_t)b * H6 + t0 + s) * RE_GATES + j] = acc[s] + bj;
  }
}

// ---- the recurrence and proj: one workgroup of 768 threads per batch item.  W_hh [384][128] fp32 is 192 KB — more than the LDS — and is
// held in REGISTERS for the whole launch: thread (row j = tid / 2, half = tid % 2) keeps 64 weights.  PyTorch's gate order (r, z, n),
// n = tanh(W_in x + b_in + r * (W_hn h + b_hn)), h' = (h - n) * z + n (ATen RNN.cpp gru cell).  Linear(128 -> gin) on the final state.
__global__ void __launch_bounds__(768) ref_gru_kernel(const float* __restrict__ gi, const float* __restrict__ w_hh,
                                                      const float* __restrict__ b_hh, const float* __restrict__ pw,
                                                      const float* __restrict__ pb, float* __restrict__ g_out,
                                                      const int64_t* __restrict__ yl, int L, int H6, int gin) {
  __shared__ __attribute__((aligned(16))) float h[RE_HID];
  __shared__ float gh[RE_GATES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int j = tid >> 1, half = tid & 1;
  const int n6 = re_len(yl, b, L, 6);
  float w[64];
  {
    const float4* wr = reinterpret_cast<const float4*>(w_hh + (int64_t)j * RE_HID + half * 64);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float4 v = wr[q];
      w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
  }
  const float bh = b_hh[j];
  if (tid < RE_HID) h[tid] = 0.f;
  __syncthreads();
  const float* gib = gi + (int64_t)b * H6 * RE_GATES;
  for (int t = 0; t < n6; ++t) {
    float gr = 0.f, gz = 0.f, gn = 0.f;
    if (tid < RE_HID) {                             // issued early: the loads fly while the matrix-vector product runs
      gr = gib[(int64_t)t * RE_GATES + tid];
      gz = gib[(int64_t)t * RE_GATES + RE_HID + tid];
      gn = gib[(int64_t)t * RE_GATES + 2 * RE_HID + tid];
    }
    const float4* hv = reinterpret_cast<const float4*>(h + half * 64);
    float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;   // four chains of 16 terms each
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float4 v = hv[q];
      p0 = fmaf(w[4 * q], v.x, p0);
      p1 = fmaf(w[4 * q + 1], v.y, p1);
      p2 = fmaf(w[4 * q + 2], v.z, p2);
      p3 = fmaf(w[4 * q + 3], v.w, p3);
    }
    float p = (p0 + p1) + (p2 + p3);
    p += __shfl_xor(p, 1);                          // the row's two halves (a + b == b + a: both lanes hold the same sum)
    if (half == 0) gh[j] = p + bh;
    __syncthreads();
    if (tid < RE_HID) {
      const float r = 1.f / (1.f + expf(-(gr + gh[tid])));
      const float z = 1.f / (1.f + expf(-(gz + gh[RE_HID + tid])));
      const float n = tanhf(gn + r * gh[2 * RE_HID + tid]);
      h[tid] = (h[tid] - n) * z + n;
    }
    __syncthreads();
  }
  // proj: wave v takes rows v, v + 12, ...; a lane holds two of the 128 products, fixed butterfly
  const int lane = tid & 63, wave = tid >> 6;
  for (int o = wave; o < gin; o += 12) {
    const float* pr = pw + (int64_t)o * RE_HID;
    float p = fmaf(pr[lane], h[lane], pr[lane + 64] * h[lane + 64]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) p += __shfl_xor(p, off);
    if (lane == 0) g_out[(int64_t)b * gin + o] = p + pb[o];
  }
}

}  // namespace

void ref_enc_dims(int L, int spec, int* H, int* W) {
  H[0] = L; W[0] = spec;
  for (int i = 1; i <= 6; ++i) { H[i] = re_down(H[i - 1]); W[i] = re_down(W[i - 1]); }
}

int64_t ref_enc_workspace_floats(int B, int L, int spec) {
  int H[7], W[7];
  ref_enc_dims(L, spec, H, W);
  const int C[7] = {1, 32, 32, 64, 64, 128, 128};
  int64_t odd = 0, even = 0;                         // outputs of convs 1, 3, 5 / 2, 4, 6 ping-pong between two buffers
  for (int i = 1; i <= 6; ++i) {
    const int64_t n = (int64_t)B * C[i] * H[i] * W[i];
    if (i & 1) odd = n > odd ? n : odd; else even = n > even ? n : even;
  }
  auto up = [](int64_t n) { return (n + 63) / 64 * 64; };
  return up(odd) + up(even) + up((int64_t)B * H[6] * RE_GATES);
}

int launch_ref_enc(hipStream_t s, const RefEncArgs& a) {
  if (a.B < 1 || a.L < 1 || a.spec < 1 || a.gin < 1 || !a.y || !a.g_out || !a.ws) return -1;
  int H[7], W[7];
  ref_enc_dims(a.L, a.spec, H, W);
  const int C[7] = {1, 32, 32, 64, 64, 128, 128};
  int64_t odd = 0;
  for (int i = 1; i <= 6; i += 2) { const int64_t n = (int64_t)a.B * C[i] * H[i] * W[i]; odd = n > odd ? n : odd; }
  int64_t even = 0;
  for (int i = 2; i <= 6; i += 2) { const int64_t n = (int64_t)a.B * C[i] * H[i] * W[i]; even = n > even ? n : even; }
  auto up = [](int64_t n) { return (n + 63) / 64 * 64; };
  float* buf[2] = {a.ws + up(odd), a.ws};            // buf[i & 1] holds conv i's output
  float* gi = a.ws + up(odd) + up(even);
  if (H[1] > 65535 * 16 || a.B > 65535) return -1;
  hipLaunchKernelGGL(ref_conv1_kernel, dim3((W[1] + 15) / 16, (H[1] + 15) / 16, a.B), dim3(256), 0, s, a.y, a.sb, a.sf, a.st,
                     a.y_lengths, a.L, a.spec, a.cw[0], a.cb[0], buf[1], H[1], W[1]);
  if (int rc = BV2_CHECK_LAUNCH()) return rc;
  for (int i = 2; i <= 6; ++i) {
    const int ncg = C[i] / 32;
    if (H[i] > 65535) return -1;
    hipLaunchKernelGGL(ref_conv_kernel, dim3(((W[i] + RE_TW - 1) / RE_TW) * ncg, H[i], a.B), dim3(256), 0, s, buf[(i - 1) & 1],
                       a.cw[i - 1], a.cb[i - 1], buf[i & 1], a.y_lengths, a.L, i - 1, C[i - 1], C[i], H[i - 1], W[i - 1], H[i], W[i],
                       ncg);
    if (int rc = BV2_CHECK_LAUNCH()) return rc;
  }
  if ((H[6] + 7) / 8 > 65535) return -1;
  hipLaunchKernelGGL(ref_gru_in_kernel, dim3(RE_GATES / 4, (H[6] + 7) / 8, a.B), dim3(256), 0, s, buf[0], a.w_ih, a.b_ih, gi,
                     a.y_lengths, a.L, H[6], W[6]);
  if (int rc = BV2_CHECK_LAUNCH()) return rc;
  hipLaunchKernelGGL(ref_gru_kernel, dim3(a.B), dim3(768), 0, s, gi, a.w_hh, a.b_hh, a.pw, a.pb, a.g_out, a.y_lengths, a.L, H[6],
                     a.gin);
  return BV2_CHECK_LAUNCH();
}

}  // namespace bv2
