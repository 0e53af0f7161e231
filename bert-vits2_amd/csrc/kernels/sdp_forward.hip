// sdp_forward.hip — the StochasticDurationPredictor in its FORWARD direction (reference models.py:206-244): the negative log-likelihood of
// observed durations w given the text, nll + logq, decomposed per symbol.  The inference direction (dds_fused.hip) samples a duration from
// noise; this one pushes a given duration through the same flows and adds up what every step contributes:
//     h_w  = post_proj(post_convs(post_pre(w))) * mask                                      (the trunk of the posterior side)
//     z_q  = post_flows(e_q * mask; g = x + h_w)          ElementwiseAffine, then four ConvFlows with the channel Flips
//     u    = sigmoid(z_q[0]) * mask;   z0 = (w - u) * mask;   y = log(clamp_min(z0, 1e-5)) * mask                  (the Log flow)
//     z    = flows([y, z_q[1]]; g = x)                    ElementwiseAffine, then ALL FOUR ConvFlows (inference drops one)
// Launch form of the inference path: one DDSConv layer per launch (dds_fwd_layer_kernel, the layer kernel of dds_fused.hip with a
// second instantiation's worth of differences: the first layer's conditioning may be absent (post_pre on w) or any tensor (x + h_w), the
// closing projection may add a tensor to its output (h_w + x, formed once), and the spline epilogue runs the forward spline and subtracts
// that position's logabsdet * mask from the per-position accumulator row).  Three pointwise launches carry everything between the flows.
//
// Reductions.  Every term lands in acc[b][t], one read-modify-write per launch by the one thread that owns the position (launches are
// ordered by the stream): no atomics, nothing depends on the tiling or on the batch.  The closing launch (one wave per item) adds the
// last Gaussian term, writes nll_sym[b][t] (exactly 0 at masked positions) and sums the row in a fixed order: lane l adds the positions
// l, l + 64, l + 128, ... in sequence, then the 64 partial sums meet in a butterfly (xor 32, 16, 8, 4, 2, 1).  The row sums (this one and
// launch_row_sum) run on fp64 accumulators and are rounded to fp32 once: the sum of a few hundred fp32 terms then carries the terms'
// own error and one rounding, not the summation's.
#include <hip/hip_runtime.h>
#include <cmath>
#include "../bv2_kernels.h"
#include "dds_tile.h"
#include "rng.h"
#include "spline.h"

namespace bv2 {

#define BV2_CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -1)

constexpr float kHalfLog2Pi = 0.91893853320467274178f;

template <int NU>   // C = 16*NU channels; NU waves per workgroup
__global__ void __launch_bounds__(64 * NU) dds_fwd_layer_kernel(const DdsFwdArgs A) {
  constexpr int C = 16 * NU, NW = NU, CG = 4 * NU;
  __shared__ __attribute__((aligned(16))) float ys[C * DDS_NT];
  __shared__ float xres[C * DDS_NT];
  __shared__ float red[4][NW][DDS_NT];
  __shared__ float prm[32 * DDS_NT];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y, t0 = blockIdx.x * DDS_NT;
  const int T = A.T;

  f32x4 wr[NU];
  if constexpr (NU <= 12) load_tile_weights<NU>(A.w, wv, lane, wr);

  // ---- phase 1: (input transform) + depthwise conv + LN1 + GELU on thread (tl = time step, cg = channel group)
  const int tl = tid & 15, cg = tid >> 4;
  const float* maskb = A.mask + (int64_t)b * T;
  float pg1[4], pb1[4], pg2[4], pb2[4], pbias[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    pg1[i] = A.g1[cg + CG * i]; pb1[i] = A.b1[cg + CG * i];
    const int row = 16 * wv + 4 * (lane >> 4) + i;
    pg2[i] = A.g2[row]; pb2[i] = A.b2[row]; pbias[i] = A.bias[row];
  }
  float v[4], xc[4];
  {
    const int t = t0 + tl;
    const bool tok = t < T;
    const int tcl = tok ? t : T - 1;
    float mk3[3];
    int tt3[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int tt = t + (j - 1) * A.dil;
      const bool ok = tok && tt >= 0 && tt < T;
      tt3[j] = ok ? tt : tcl;
      const float mv = maskb[tt3[j]];
      mk3[j] = ok ? mv : 0.f;
    }
    const bool has_pre = A.pre_w != nullptr;
    const bool has_src = has_pre ? A.g != nullptr : true;          // post_pre(w) has no conditioning: its residual stream starts at pre alone
    float z3[3];
    {
      const float* zr = has_pre ? A.z + ((int64_t)b * A.z_rows + A.z_src) * T : maskb;
#pragma unroll
      for (int j = 0; j < 3; ++j) z3[j] = zr[tt3[j]];
    }
    float x3[4][3], dw[4][3], db[4], pw[4], pb[4];
    const float* const src = has_src ? (has_pre ? A.g : A.x) + (int64_t)b * C * T : nullptr;
    const float* const pwp = has_pre ? A.pre_w : A.dwb;
    const float* const pbp = has_pre ? A.pre_b : A.dwb;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = cg + CG * i;
#pragma unroll
      for (int j = 0; j < 3; ++j) dw[i][j] = A.dww[c * 3 + j];
      db[i] = A.dwb[c]; pw[i] = pwp[c]; pb[i] = pbp[c];
    }
    if (has_src) {                                                  // kernel-uniform
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float* xp = src + (int64_t)(cg + CG * i) * T;
#pragma unroll
        for (int j = 0; j < 3; ++j) x3[i][j] = xp[tt3[j]];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) x3[i][j] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (has_pre) {
#pragma unroll
        for (int j = 0; j < 3; ++j) x3[i][j] = has_src ? pw[i] * z3[j] + pb[i] + x3[i][j] : pw[i] * z3[j] + pb[i];
      }
      xc[i] = x3[i][1];
      float acc = db[i];
#pragma unroll
      for (int j = 0; j < 3; ++j) acc += dw[i][j] * (x3[i][j] * mk3[j]);
      v[i] = acc;
    }
  }
  {
    float s = (v[0] + v[1]) + (v[2] + v[3]);
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (lane < DDS_NT) red[0][wv][lane] = s;
    __syncthreads();
    float m = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) m += red[0][w][tl];
    const float mean = m / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const float d = v[i] - mean; q += d * d; }
    q += __shfl_xor(q, 16);
    q += __shfl_xor(q, 32);
    if (lane < DDS_NT) red[1][wv][lane] = q;
    __syncthreads();
    float qs = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) qs += red[1][w][tl];
    const float rstd = 1.0f / sqrtf(qs / (float)C + A.eps);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = cg + CG * i;
      const float y = (v[i] - mean) * rstd * pg1[i] + pb1[i];
      ys[c * DDS_NT + tl] = gelu_erf(y);
      xres[c * DDS_NT + tl] = xc[i];
    }
  }
  __syncthreads();

  // ---- phase 2: 1x1 conv, wave wv -> output rows [16 wv, 16 wv + 16)
  if constexpr (NU > 12) load_tile_weights<NU>(A.w, wv, lane, wr);
  f32x4 acc = tile_gemm<NU>(wr, ys, lane);

  const bool post = A.post_w != nullptr;
  const bool post_wave = post && 16 * wv < A.post_cout_pad;       // wave-uniform
  f32x4 pw[NU];
  if (post_wave) load_tile_weights<NU>(A.post_w, wv, lane, pw);

  // ---- phase 3: bias + LN2 + GELU + residual on the MFMA output layout
  const int n = lane & 15, rg = lane >> 4;
  const int t = t0 + n;
  const bool tok = t < T;
  const float mkc = tok ? maskb[t] : 0.f;
  float o[4];
  {
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = acc[r] + pbias[r];
    float s = (o[0] + o[1]) + (o[2] + o[3]);
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (lane < DDS_NT) red[2][wv][lane] = s;
    __syncthreads();
    float m = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) m += red[2][w][n];
    const float mean = m / (float)C;
    float q = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) { const float d = o[r] - mean; q += d * d; }
    q += __shfl_xor(q, 16);
    q += __shfl_xor(q, 32);
    if (lane < DDS_NT) red[3][wv][lane] = q;
    __syncthreads();
    float qs = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) qs += red[3][w][n];
    const float rstd = 1.0f / sqrtf(qs / (float)C + A.eps);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wv + 4 * rg + r;
      const float y = gelu_erf((o[r] - mean) * rstd * pg2[r] + pb2[r]);
      float val = xres[row * DDS_NT + n] + y;
      if (A.last_mask) val *= mkc;
      o[r] = val;
      if (A.out && tok) A.out[((int64_t)b * C + row) * T + t] = val;
    }
  }
  if (!post) return;                                               // kernel-uniform

  // ---- phase 4: the 1x1 projection that follows the DDSConv, on this tile
#pragma unroll
  for (int r = 0; r < 4; ++r) ys[(16 * wv + 4 * rg + r) * DDS_NT + n] = o[r];
  __syncthreads();
  if (post_wave) {
    const f32x4 pa = tile_gemm<NU>(pw, ys, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * wv + 4 * rg + r;
      const float val = (pa[r] + A.post_b[row]) * mkc;
      if (A.post_out) {
        if (tok && row < A.post_cout) {
          const int64_t oi = ((int64_t)b * A.post_cout + row) * T + t;
          A.post_out[oi] = A.post_add ? A.post_add[oi] + val : val;     // x + h_w, the post flows' conditioning (models.py:220)
        }
      } else if (row < 32) {
        prm[row * DDS_NT + n] = val;
      }
    }
  }
  if (A.post_out || !A.zio) return;                               // kernel-uniform
  __syncthreads();
  if (tid < DDS_NT) {
    const int ts = t0 + tid;
    if (ts < T) {
      const float cst = A.cst, wscale = A.wscale;
      float uw[SPK], uh[SPK], ud[SPK + 1];
#pragma unroll
      for (int i = 0; i < SPK; ++i) { uw[i] = prm[i * DDS_NT + tid] / A.sqrt_fc; uh[i] = prm[(SPK + i) * DDS_NT + tid] / A.sqrt_fc; }
      ud[0] = cst; ud[SPK] = cst;
#pragma unroll
      for (int i = 1; i < SPK; ++i) ud[i] = prm[(2 * SPK + i - 1) * DDS_NT + tid];
      const float mk = maskb[ts];
      float* zs = A.zio + ((int64_t)b * 2 + A.z_src) * T + ts;
      float* zd = A.zio + ((int64_t)b * 2 + A.z_dst) * T + ts;
      float lad;
      const float outv = rq_spline_forward_one(*zd, uw, uh, ud, A.tail, wscale, &lad);
      *zd = outv * mk;
      *zs = *zs * mk;
      float* ap = A.acc + (int64_t)b * T + ts;
      *ap = *ap - lad * mk;                                        // both sides subtract their flows' log-determinants (models.py:231, 242)
    }
  }
}

int launch_dds_fwd_layer(hipStream_t stream, const DdsFwdArgs& a) {
  if (!dds_fused_supported(a.C) || a.B < 1 || a.B > 65535 || a.T < 1 || a.dil < 1 || !a.mask || !a.w || !a.bias) return -2;
  if (!a.x && !a.pre_w) return -1;
  if (a.pre_w && (!a.z || a.z_rows < 1 || a.z_src < 0 || a.z_src >= a.z_rows)) return -1;
  if (a.out && a.out == a.x) return -1;
  if (a.post_w && (a.post_cout_pad % 16 || a.post_cout_pad > a.C || (!a.post_out && (!a.zio || !a.acc || a.post_cout_pad < 32)))) return -1;
  if (a.post_w && a.zio && (a.z_src < 0 || a.z_src > 1 || a.z_dst < 0 || a.z_dst > 1)) return -1;
  if ((int64_t)a.C * a.T >= (1ll << 31)) return -1;
  const dim3 grid((a.T + DDS_NT - 1) / DDS_NT, a.B);
  DdsFwdArgs k = a;
  k.cst = (float)std::log(std::exp(1.0 - 1e-3) - 1.0);
  k.wscale = (float)(1.0 - 1e-3 * SPK);
  switch (a.C) {
    case 128: hipLaunchKernelGGL((dds_fwd_layer_kernel<8>), grid, dim3(512), 0, stream, k); break;
    case 192: hipLaunchKernelGGL((dds_fwd_layer_kernel<12>), grid, dim3(768), 0, stream, k); break;
    default:  hipLaunchKernelGGL((dds_fwd_layer_kernel<16>), grid, dim3(1024), 0, stream, k); break;
  }
  return BV2_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the pointwise steps between the flows; thread = one position (b, t)
__device__ __forceinline__ float logsigmoid_f(float x) { return fminf(x, 0.f) - log1pf(expf(-fabsf(x))); }

// e_q (the caller's draw, or the value of (seeds[b], RNG_NOISE_E, row, t)) * mask -> the posterior side's ElementwiseAffine;
// acc = the e_q Gaussian term minus that layer's log-determinant (models.py:214-221, 229)
__global__ void __launch_bounds__(256) sdp_fwd_begin_kernel(const SdpFwdPointArgs A) {
  const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x, T = A.T;
  if (t >= T) return;
  const int64_t i0 = ((int64_t)b * 2) * T + t, i1 = i0 + T;
  const float mk = A.mask[(int64_t)b * T + t];
  float e0, e1;
  if (A.seeds) { e0 = seeded_normal(A.seeds[b], RNG_NOISE_E, 0, t); e1 = seeded_normal(A.seeds[b], RNG_NOISE_E, 1, t); }
  else { e0 = A.noise[i0]; e1 = A.noise[i1]; }
  e0 = mk != 0.f ? e0 * mk : 0.f;                                   // a masked position is selected to zero: its noise may hold anything
  e1 = mk != 0.f ? e1 * mk : 0.f;
  const float l0 = A.ea_logs[0], l1 = A.ea_logs[1];
  A.zq[i0] = (A.ea_m[0] + expf(l0) * e0) * mk;
  A.zq[i1] = (A.ea_m[1] + expf(l1) * e1) * mk;
  float a = (-0.5f * (2.f * kHalfLog2Pi + e0 * e0)) * mk;
  a = a + (-0.5f * (2.f * kHalfLog2Pi + e1 * e1)) * mk;
  a = a - (l0 * mk + l1 * mk);
  A.acc[(int64_t)b * T + t] = a;
}

// z_u, z1 = z_q;  u = sigmoid(z_u) * mask;  z0 = (w - u) * mask;  the two logsigmoid terms;  the Log flow;  the main side's
// ElementwiseAffine (models.py:222-238)
__global__ void __launch_bounds__(256) sdp_fwd_mid_kernel(const SdpFwdPointArgs A) {
  const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x, T = A.T;
  if (t >= T) return;
  const int64_t i0 = ((int64_t)b * 2) * T + t, i1 = i0 + T, ia = (int64_t)b * T + t;
  const float mk = A.mask[ia];
  const float zu = A.zq[i0], z1 = A.zq[i1];
  const float u = (1.f / (1.f + expf(-zu))) * mk;
  const float z0 = (A.w[ia] - u) * mk;
  float a = A.acc[ia];
  a = a - (logsigmoid_f(zu) + logsigmoid_f(-zu)) * mk;
  const float y = logf(fmaxf(z0, 1e-5f)) * mk;
  a = a + y;                                                        // the Log flow's log-determinant is -y
  const float l0 = A.ea_logs[0], l1 = A.ea_logs[1];
  A.z[i0] = (A.ea_m[0] + expf(l0) * y) * mk;
  A.z[i1] = (A.ea_m[1] + expf(l1) * z1) * mk;
  a = a - (l0 * mk + l1 * mk);
  A.acc[ia] = a;
}

// the fixed-order sum of the 64 per-lane partial sums of a row
__device__ __forceinline__ double wave_butterfly_sum(double s) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_xor(s, off);
  return s;
}

// the z Gaussian term, nll_sym and nll; one wave per item
__global__ void __launch_bounds__(64) sdp_fwd_end_kernel(const SdpFwdPointArgs A) {
  const int b = blockIdx.x, lane = threadIdx.x, T = A.T;
  double s = 0.0;
  for (int t = lane; t < T; t += 64) {
    const int64_t i0 = ((int64_t)b * 2) * T + t, i1 = i0 + T, ia = (int64_t)b * T + t;
    const float mk = A.mask[ia];
    const float z0 = A.z[i0], z1 = A.z[i1];
    float a = A.acc[ia];
    a = a + (0.5f * (2.f * kHalfLog2Pi + z0 * z0)) * mk;
    a = a + (0.5f * (2.f * kHalfLog2Pi + z1 * z1)) * mk;
    a = mk != 0.f ? a : 0.f;
    A.nll_sym[ia] = a;
    s = s + (double)a;
  }
  s = wave_butterfly_sum(s);
  if (lane == 0) A.nll[b] = (float)s;
}

int launch_sdp_fwd_point(hipStream_t stream, int step, const SdpFwdPointArgs& a) {
  if (a.B < 1 || a.B > 65535 || a.T < 1 || !a.mask || !a.acc) return -1;
  const dim3 grid((unsigned)((a.T + 255) / 256), (unsigned)a.B);
  if (step == 0) {
    if ((!a.noise && !a.seeds) || !a.zq || !a.ea_m || !a.ea_logs) return -1;
    hipLaunchKernelGGL(sdp_fwd_begin_kernel, grid, dim3(256), 0, stream, a);
  } else if (step == 1) {
    if (!a.zq || !a.z || !a.w || !a.ea_m || !a.ea_logs) return -1;
    hipLaunchKernelGGL(sdp_fwd_mid_kernel, grid, dim3(256), 0, stream, a);
  } else {
    if (!a.z || !a.nll_sym || !a.nll) return -1;
    hipLaunchKernelGGL(sdp_fwd_end_kernel, dim3((unsigned)a.B), dim3(64), 0, stream, a);
  }
  return BV2_CHECK_LAUNCH();
}

// out[b] = the fixed-order sum of row b of x [B][n] (the order of sdp_fwd_end_kernel); one wave per item
__global__ void __launch_bounds__(64) row_sum_kernel(const float* x, float* out, int n) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* r = x + (int64_t)b * n;
  double s = 0.0;
  for (int t = lane; t < n; t += 64) s = s + (double)r[t];
  s = wave_butterfly_sum(s);
  if (lane == 0) out[b] = (float)s;
}

int launch_row_sum(hipStream_t stream, const float* x, float* out, int B, int n) {
  if (B < 1 || B > 65535 || n < 1 || !x || !out) return -1;
  hipLaunchKernelGGL(row_sum_kernel, dim3((unsigned)B), dim3(64), 0, stream, x, out, n);
  return BV2_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the forward spline alone, one element per thread (tests): uw / uh [N][10] unnormalised widths / heights as the spline takes them
// (already divided by sqrt(filter_channels)), ud [N][9] raw interior derivatives
__global__ void __launch_bounds__(256) spline_forward_kernel(const float* x, const float* uw, const float* uh, const float* ud, float tail,
                                                             float cst, float wscale, int64_t N, float* y, float* lad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  float w[SPK], h[SPK], d[SPK + 1];
#pragma unroll
  for (int k = 0; k < SPK; ++k) { w[k] = uw[i * SPK + k]; h[k] = uh[i * SPK + k]; }
  d[0] = cst; d[SPK] = cst;
#pragma unroll
  for (int k = 1; k < SPK; ++k) d[k] = ud[i * (SPK - 1) + k - 1];
  float l;
  y[i] = rq_spline_forward_one(x[i], w, h, d, tail, wscale, &l);
  lad[i] = l;
}

int launch_spline_forward(hipStream_t stream, const float* x, const float* uw, const float* uh, const float* ud, float tail, int64_t N,
                          float* y, float* lad) {
  if (N < 1 || N > (1ll << 30) || !x || !uw || !uh || !ud || !y || !lad) return -1;
  hipLaunchKernelGGL(spline_forward_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, x, uw, uh, ud, tail,
                     (float)std::log(std::exp(1.0 - 1e-3) - 1.0), (float)(1.0 - 1e-3 * SPK), N, y, lad);
  return BV2_CHECK_LAUNCH();
}

}  // namespace bv2
