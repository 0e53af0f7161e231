// stft.hip — the spectrogram the ReferenceEncoder reads, from a waveform (reference mel_processing.py:43-78 spectrogram_torch and :95-142
// mel_spectrogram_torch): reflect padding by pad = (n_fft - hop) / 2, periodic Hann window of `win` samples centred in n_fft, one-sided
// STFT (center = False), sqrt(re^2 + im^2 + 1e-6), and for the mel form log(max(M . spec, 1e-5)).
//
// Two launches per call, both asynchronous on the caller's stream:
//
//   stft_prepare_kernel   fills the call's workspace: the twiddles exp(-2 pi i m / n_fft), m < n_fft / 2 (sincospi in fp64, rounded once to
//                         fp32), the window (torch.hann_window's own fp32 recipe: the argument n * (float)(2 pi / win) rounded to fp32, its
//                         cosine rounded to fp32, * -0.5 + 0.5 — a window from the exact argument differs from the reference's by up to 2e-7,
//                         which at a spectral peak of 200 is the size of the whole error budget), and per mel row the range of its non-zeros.
//   stft_kernel<N>        one workgroup of 256 threads owns ST_TF = 8 consecutive frames of one item.  Frames (2p, 2p + 1) are the real and
//                         imaginary part of ONE complex N-point transform; a Stockham autosort chain of radix-8 / radix-4 passes
//                         (2048 = 8.8.8.4, 1024 = 8.8.4.4) runs in place in LDS with the butterflies in registers (read, barrier, butterfly,
//                         write, barrier); the two spectra are untangled by conjugate symmetry (additions and an exact halving), magnitudes
//                         go to an LDS block [f][frame] that reuses the transform's space, and are stored from there — frequency-fastest when
//                         the output's frequency stride is 1, frame-fastest otherwise — or, for the mel form, contracted with the filterbank
//                         rows over their non-zero ranges.  Padding, int16 conversion (x / 32768, exact), window, magnitude, mel, log and the
//                         zero fill of frames past an item's end are all inside this launch.
//
// LDS per workgroup at N = 2048: 4 pairs x (N + N / 16) float2 (one float2 of padding per 16 keeps the strided writes of the early passes at a
// 2-way bank conflict) = 69 632 B + the half twiddle table 8 192 B = 77 824 B: two workgroups per CU.  N = 1024: 38 912 B.
//
// Bounds.  A workgroup reads samples [0, S_b) of its own item only (S_b = wav_lengths[b] clamped to [0, S]): a frame index is reflected at most
// once at either end (pad < S_b is what makes a frame exist at all) and clamped after that; frames >= L_b are never loaded.  Every store is
// guarded by f < C and t < L (the frame capacity of the output).  The summation order of every output depends on n_fft only, never on B,
// S or the lengths, so an item of a ragged batch gets bit for bit what it gets alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../bv2_kernels.h"

namespace bv2 {

#define BV2_CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -1)

namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_TF = 8;                    // frames per workgroup
constexpr int ST_P = ST_TF / 2;             // complex transforms per workgroup
constexpr int ST_MS = ST_TF + 1;            // row stride of the magnitude block [f][frame] (odd: conflict-free both ways)

__host__ __device__ constexpr int st_pad(int i) { return i + (i >> 4); }
__host__ __device__ constexpr int st_pair_stride(int N) { return N + N / 16; }

struct cf { float x, y; };
__device__ __forceinline__ cf cadd(cf a, cf b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cf csub(cf a, cf b) { return {a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ cf cmul(cf a, cf b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cf mul_mi(cf a) { return {a.y, -a.x}; }          // a * (-i)

// forward 4-point DFT in place (e^{-2 pi i / 4} = -i)
__device__ __forceinline__ void dft4(cf& a0, cf& a1, cf& a2, cf& a3) {
  const cf t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3), t3 = mul_mi(csub(a1, a3));
  a0 = cadd(t0, t2); a2 = csub(t0, t2); a1 = cadd(t1, t3); a3 = csub(t1, t3);
}

template <int R>
__device__ __forceinline__ void dft(cf (&u)[R]) {
  if constexpr (R == 4) {
    dft4(u[0], u[1], u[2], u[3]);
  } else {
    static_assert(R == 8, "radix 4 or 8");
    dft4(u[0], u[2], u[4], u[6]);             // even samples -> E[0..3] in u[0], u[2], u[4], u[6]
    dft4(u[1], u[3], u[5], u[7]);             // odd samples  -> O[0..3] in u[1], u[3], u[5], u[7]
    constexpr float s = 0.70710678118654752440f;
    const cf o0 = u[1];
    const cf o1 = {(u[3].x + u[3].y) * s, (u[3].y - u[3].x) * s};       // * (1 - i) / sqrt 2
    const cf o2 = mul_mi(u[5]);
    const cf o3 = {(u[7].y - u[7].x) * s, -(u[7].x + u[7].y) * s};      // * (-1 - i) / sqrt 2
    const cf e0 = u[0], e1 = u[2], e2 = u[4], e3 = u[6];
    u[0] = cadd(e0, o0); u[4] = csub(e0, o0);
    u[1] = cadd(e1, o1); u[5] = csub(e1, o1);
    u[2] = cadd(e2, o2); u[6] = csub(e2, o2);
    u[3] = cadd(e3, o3); u[7] = csub(e3, o3);
  }
}

// exp(-2 pi i m / N), m < N, from the half table
template <int N>
__device__ __forceinline__ cf twiddle(const cf* tw, int m) {
  cf v = tw[m & (N / 2 - 1)];
  if (m & (N / 2)) { v.x = -v.x; v.y = -v.y; }
  return v;
}

// One Stockham pass of radix R over the ST_P transforms of the workgroup; P_ = product of the radices of the passes before it.  Butterfly i of
// a transform reads elements i + r * (N / R), multiplies element r by exp(-2 pi i r k / (P_ R)), k = i mod P_, and writes output q of the
// R-point DFT to (i - k) * R + k + q * P_.  FIRST: the elements come from `first` (the windowed frames) instead of LDS.
template <int N, int R, int P_, bool FIRST, typename Load>
__device__ __forceinline__ void fft_pass(cf* __restrict__ data, const cf* __restrict__ tw, Load first) {
  constexpr int T = N / R;                                  // butterflies per transform
  constexpr int ITEMS = ST_P * T / ST_THREADS;              // butterflies per thread
  static_assert(ST_P * T % ST_THREADS == 0, "whole butterflies per thread");
  cf u[ITEMS][R];
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const int w = threadIdx.x + ST_THREADS * j, pr = w / T, i = w % T;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if constexpr (FIRST) u[j][r] = first(pr, i + r * T);
      else u[j][r] = data[pr * st_pair_stride(N) + st_pad(i + r * T)];
    }
  }
  if constexpr (!FIRST) __syncthreads();                    // every element is in a register before any is overwritten
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const int w = threadIdx.x + ST_THREADS * j, pr = w / T, i = w % T;
    const int k = i & (P_ - 1), base = (i - k) * R + k;
    if constexpr (P_ > 1) {
#pragma unroll
      for (int r = 1; r < R; ++r) u[j][r] = cmul(u[j][r], twiddle<N>(tw, r * k * (N / (P_ * R))));
    }
    dft<R>(u[j]);
#pragma unroll
    for (int q = 0; q < R; ++q) data[pr * st_pair_stride(N) + st_pad(base + q * P_)] = u[j][q];
  }
  __syncthreads();
}

__global__ void __launch_bounds__(ST_THREADS) stft_prepare_kernel(int n_fft, int win, float win_step, int n_mels, int C,
                                                                  const float* __restrict__ mel, cf* __restrict__ tw,
                                                                  float* __restrict__ window, int* __restrict__ mel_range) {
  const int nb = (n_fft + ST_THREADS - 1) / ST_THREADS;
  if ((int)blockIdx.x < nb) {
    const int n = blockIdx.x * ST_THREADS + threadIdx.x;
    if (n < n_fft) {
      const int off = (n_fft - win) / 2, j = n - off;       // torch.stft centres a shorter window
      float v = 0.f;
      if (j >= 0 && j < win) {
        const float arg = __fmul_rn((float)j, win_step);
        v = __fadd_rn(__fmul_rn((float)cos((double)arg), -0.5f), 0.5f);
      }
      window[n] = v;
    }
    if (n < n_fft / 2) {
      double s, c;
      sincospi(2.0 * (double)n / (double)n_fft, &s, &c);
      tw[n] = {(float)c, (float)-s};
    }
    return;
  }
  // one workgroup per mel row: [first non-zero, last non-zero + 1)
  __shared__ int lo, hi;
  const int m = blockIdx.x - nb;
  if (threadIdx.x == 0) { lo = C; hi = 0; }
  __syncthreads();
  int l = C, h = 0;
  for (int f = threadIdx.x; f < C; f += ST_THREADS)
    if (mel[(int64_t)m * C + f] != 0.f) { l = min(l, f); h = max(h, f + 1); }
  if (l < C) { atomicMin(&lo, l); atomicMax(&hi, h); }
  __syncthreads();
  if (threadIdx.x == 0) { mel_range[2 * m] = min(lo, hi); mel_range[2 * m + 1] = hi; }
}

struct StftK {
  const void* wav; int64_t wav_bstride; const int64_t* wav_lengths; int64_t S;
  int hop, pad, fmt, n_mels, L;
  const cf* tw; const float* window; const int* mel_range; const float* mel;
  float* spec; int64_t sb, sf, st;
  int64_t* lengths_out;
};

__device__ __forceinline__ int64_t st_frames(int64_t Sb, int pad, int n_fft, int hop) {
  if (Sb <= pad) return 0;
  const int64_t n = Sb + 2 * (int64_t)pad - n_fft;
  return n < 0 ? 0 : 1 + n / hop;
}

template <int N>
__global__ void __launch_bounds__(ST_THREADS) stft_kernel(const StftK a) {
  constexpr int C = N / 2 + 1;
  extern __shared__ __align__(16) unsigned char st_smem[];
  cf* data = reinterpret_cast<cf*>(st_smem);                                     // [ST_P][N + N / 16]
  cf* tw = data + ST_P * st_pair_stride(N);                                      // [N / 2]
  float* mag = reinterpret_cast<float*>(st_smem);                                // [C][ST_MS], after the transforms
  static_assert(C * ST_MS * sizeof(float) <= ST_P * st_pair_stride(N) * sizeof(cf), "the magnitude block fits the transform space");

  const int b = blockIdx.y, t0 = blockIdx.x * ST_TF, tid = threadIdx.x;
  int64_t Sb = a.wav_lengths ? a.wav_lengths[b] : a.S;
  Sb = Sb < 0 ? 0 : (Sb > a.S ? a.S : Sb);
  int64_t Lb64 = st_frames(Sb, a.pad, N, a.hop);
  const int Lb = (int)(Lb64 > a.L ? a.L : Lb64);
  if (blockIdx.x == 0 && tid == 0 && a.lengths_out) a.lengths_out[b] = Lb;
  float* out = a.spec + (int64_t)b * a.sb;
  const int Cout = a.n_mels ? a.n_mels : C;

  if (t0 >= Lb) {                                                                // uniform: nothing but zeros to write, no sample is read
    for (int i = tid; i < Cout * ST_TF; i += ST_THREADS) {
      const int f = i / ST_TF, t = t0 + i % ST_TF;
      if (t < a.L) out[(int64_t)f * a.sf + (int64_t)t * a.st] = 0.f;
    }
    return;
  }

  for (int i = tid; i < N / 2; i += ST_THREADS) tw[i] = a.tw[i];

  // windowed frames: transform pr carries frame t0 + 2 pr in its real part and t0 + 2 pr + 1 in its imaginary part
  const int64_t wbase = (int64_t)b * a.wav_bstride;
  auto sample = [&](int t, int n) -> float {
    if (t >= Lb) return 0.f;
    int64_t i = (int64_t)t * a.hop + n - a.pad;
    if (i < 0) i = -i;
    if (i >= Sb) i = 2 * (Sb - 1) - i;
    i = i < 0 ? 0 : (i >= Sb ? Sb - 1 : i);                                      // unreachable for a frame that exists; keeps every read inside the item
    return a.fmt ? (float)static_cast<const int16_t*>(a.wav)[wbase + i] * (1.f / 32768.f) : static_cast<const float*>(a.wav)[wbase + i];
  };
  auto first = [&](int pr, int n) -> cf {
    const float w = a.window[n];
    const int t = t0 + 2 * pr;
    return {w * sample(t, n), w * sample(t + 1, n)};
  };

  if constexpr (N == 2048) {
    fft_pass<N, 8, 1, true>(data, tw, first);
    fft_pass<N, 8, 8, false>(data, tw, first);
    fft_pass<N, 8, 64, false>(data, tw, first);
    fft_pass<N, 4, 512, false>(data, tw, first);
  } else {
    fft_pass<N, 8, 1, true>(data, tw, first);
    fft_pass<N, 8, 8, false>(data, tw, first);
    fft_pass<N, 4, 64, false>(data, tw, first);
    fft_pass<N, 4, 256, false>(data, tw, first);
  }

  // untangle: with Z = A + i B (A, B the spectra of the two real frames), A[k] = (Z[k] + conj Z[N - k]) / 2, B[k] = (Z[k] - conj Z[N - k]) / 2i
  constexpr int KJ = N / 2 / ST_THREADS + 1;                                     // the last round holds k = N / 2 alone
  float ma[ST_P][KJ], mb[ST_P][KJ];
#pragma unroll
  for (int pr = 0; pr < ST_P; ++pr)
#pragma unroll
    for (int j = 0; j < KJ; ++j) {
      const int k = tid + ST_THREADS * j;
      ma[pr][j] = mb[pr][j] = 0.f;
      if (k <= N / 2) {
        const cf z = data[pr * st_pair_stride(N) + st_pad(k)], y = data[pr * st_pair_stride(N) + st_pad((N - k) & (N - 1))];
        const float ar = 0.5f * (z.x + y.x), ai = 0.5f * (z.y - y.y), br = 0.5f * (z.y + y.y), bi = 0.5f * (y.x - z.x);
        ma[pr][j] = sqrtf(ar * ar + ai * ai + 1e-6f);
        mb[pr][j] = sqrtf(br * br + bi * bi + 1e-6f);
      }
    }
  __syncthreads();
#pragma unroll
  for (int pr = 0; pr < ST_P; ++pr)
#pragma unroll
    for (int j = 0; j < KJ; ++j) {
      const int k = tid + ST_THREADS * j;
      if (k <= N / 2) {
        mag[k * ST_MS + 2 * pr] = ma[pr][j];
        mag[k * ST_MS + 2 * pr + 1] = mb[pr][j];
      }
    }
  __syncthreads();

  if (a.n_mels) {
    for (int i = tid; i < a.n_mels * ST_TF; i += ST_THREADS) {
      const int m = i / ST_TF, tl = i % ST_TF, t = t0 + tl;
      if (t >= a.L) continue;
      float v = 0.f;
      if (t < Lb) {
        int lo = a.mel_range[2 * m], hi = a.mel_range[2 * m + 1];
        lo = lo < 0 ? 0 : lo; hi = hi > C ? C : hi;
        const float* row = a.mel + (int64_t)m * C;
        float acc = 0.f;
        for (int f = lo; f < hi; ++f) acc = fmaf(row[f], mag[f * ST_MS + tl], acc);
        v = logf(fmaxf(acc, 1e-5f));
      }
      out[(int64_t)m * a.sf + (int64_t)t * a.st] = v;
    }
    return;
  }
  if (a.sf == 1) {                                                               // [B, L, C] memory: a frame's C values are one contiguous run
    for (int tl = 0; tl < ST_TF; ++tl) {
      const int t = t0 + tl;
      if (t >= a.L) break;
      float* row = out + (int64_t)t * a.st;
      const bool live = t < Lb;
      for (int f = tid; f < C; f += ST_THREADS) row[f] = live ? mag[f * ST_MS + tl] : 0.f;
    }
  } else {                                                                       // frame-fastest: ST_TF consecutive frames of a frequency row
    for (int i = tid; i < C * ST_TF; i += ST_THREADS) {
      const int f = i / ST_TF, tl = i % ST_TF, t = t0 + tl;
      if (t < a.L) out[(int64_t)f * a.sf + (int64_t)t * a.st] = t < Lb ? mag[f * ST_MS + tl] : 0.f;
    }
  }
}

template <int N>
constexpr int st_lds_bytes() { return (int)(ST_P * st_pair_stride(N) * sizeof(cf) + N / 2 * sizeof(cf)); }

}  // namespace

int64_t stft_workspace_bytes(int n_fft, int n_mels) {
  return (int64_t)(n_fft / 2) * 8 + (int64_t)n_fft * 4 + (int64_t)(n_mels > 0 ? n_mels : 0) * 8;
}

int launch_stft(hipStream_t stream, const StftArgs& a) {
  const int N = a.n_fft, C = N / 2 + 1;
  unsigned char* ws = static_cast<unsigned char*>(a.ws);
  cf* tw = reinterpret_cast<cf*>(ws);
  float* window = reinterpret_cast<float*>(ws + (size_t)(N / 2) * 8);
  int* mel_range = reinterpret_cast<int*>(ws + (size_t)(N / 2) * 8 + (size_t)N * 4);
  const float win_step = (float)(2.0 * 3.14159265358979323846 / (double)a.win);     // the fp32 scalar torch.hann_window multiplies arange by
  const int nb = (N + ST_THREADS - 1) / ST_THREADS;
  hipLaunchKernelGGL(stft_prepare_kernel, dim3(nb + (a.n_mels > 0 ? a.n_mels : 0)), dim3(ST_THREADS), 0, stream, N, a.win, win_step, a.n_mels,
                     C, a.mel, tw, window, mel_range);
  if (int rc = BV2_CHECK_LAUNCH()) return rc;
  StftK k;
  k.wav = a.wav; k.wav_bstride = a.wav_bstride; k.wav_lengths = a.wav_lengths; k.S = a.S;
  k.hop = a.hop; k.pad = (N - a.hop) / 2; k.fmt = a.input_format; k.n_mels = a.n_mels; k.L = a.L;
  k.tw = tw; k.window = window; k.mel_range = mel_range; k.mel = a.mel;
  k.spec = a.spec; k.sb = a.sb; k.sf = a.sf; k.st = a.st; k.lengths_out = a.lengths_out;
  const dim3 grid((a.L + ST_TF - 1) / ST_TF, a.B);
  if (N == 2048) {
    ensure_dyn_lds(reinterpret_cast<const void*>(&stft_kernel<2048>), st_lds_bytes<2048>());
    hipLaunchKernelGGL(stft_kernel<2048>, grid, dim3(ST_THREADS), st_lds_bytes<2048>(), stream, k);
  } else {
    hipLaunchKernelGGL(stft_kernel<1024>, grid, dim3(ST_THREADS), st_lds_bytes<1024>(), stream, k);
  }
  return BV2_CHECK_LAUNCH();
}

}  // namespace bv2
