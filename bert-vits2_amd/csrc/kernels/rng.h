// rng.h — the counter-based N(0,1) generator behind per-utterance noise seeds (DESIGN.md "Seeded noise").
// The value at (utterance seed, draw, row, frame) is a pure function of those four numbers: Philox4x32-10 (Salmon et al., SC'11; the
// standard constants) keyed by the seed, counter (t, row >> 2, which, 0), then Box-Muller on one pair of its four words.  One Philox
// call therefore yields the four normals of rows 4q .. 4q+3 of one frame.  Every kernel that needs a value calls seeded_normal /
// seeded_normal4 below and nothing else: the bits are the same wherever they are computed (tests/test_seeded_noise_gpu.py).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BV2_RNG_HD __host__ __device__ inline
#else
#define BV2_RNG_HD inline
#endif

namespace bv2 {

enum { RNG_NOISE_W = 0, RNG_NOISE_Z = 1, RNG_NOISE_Q = 2 };   // `which`: the SDP draw, the prior draw, the posterior draw
enum { RNG_NOISE_E = 3 };                                     // e_q of the duration likelihood (models.py:214-217); 0-2 and their values do not move

struct Philox4 { uint32_t x, y, z, w; };

// 32 x 32 -> 64: the low word is one v_mul_lo_u32, the high word one v_mul_hi_u32 (no 64-bit multiply is formed)
BV2_RNG_HD uint32_t rng_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

BV2_RNG_HD Philox4 philox4x32_10(Philox4 c, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = rng_mulhi(M0, c.x), lo0 = M0 * c.x, hi1 = rng_mulhi(M1, c.z), lo1 = M1 * c.z;
    c = Philox4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += W0; k1 += W1;
  }
  return c;
}

// the four words of (seed, which, rows 4q .. 4q+3, frame t)
BV2_RNG_HD Philox4 seeded_words(int64_t seed, int which, int q, int t) {
  const uint64_t s = (uint64_t)seed;
  return philox4x32_10(Philox4{(uint32_t)t, (uint32_t)q, (uint32_t)which, 0u}, (uint32_t)(s & 0xffffffffu), (uint32_t)(s >> 32));
}

// Box-Muller on one word pair: u = ((word >> 9) + 0.5) * 2^-23 is exact in fp32 and inside (0, 1); even = r cos(2 pi u2), odd = r sin(2 pi u2).
// The last product is a rounded multiply of its own (__fmul_rn): inlined into a consumer it is never contracted into the consumer's
// arithmetic, so the value has the same bits in every kernel.  |value| <= sqrt(48 ln 2) ~ 5.77.
BV2_RNG_HD void box_muller_pair(uint32_t a, uint32_t b, float* even, float* odd) {
  const float u1 = ((float)(a >> 9) + 0.5f) * 1.1920928955078125e-07f;
  const float u2 = ((float)(b >> 9) + 0.5f) * 1.1920928955078125e-07f;
  const float r = sqrtf(-2.f * logf(u1));
#if defined(__HIP_DEVICE_COMPILE__)
  float s, c;
  sincospif(2.f * u2, &s, &c);
  *even = __fmul_rn(r, c);
  *odd = __fmul_rn(r, s);
#else
  // host instantiation (include/bv2_testing.h): the integer core is the device's; the two circular functions through the host's double ones
  const double x = 3.14159265358979323846 * (double)(2.f * u2);
  *even = r * (float)cos(x);
  *odd = r * (float)sin(x);
#endif
}

// rows 4q .. 4q+3 of frame t
BV2_RNG_HD void seeded_normal4(int64_t seed, int which, int q, int t, float* v0, float* v1, float* v2, float* v3) {
  const Philox4 w = seeded_words(seed, which, q, t);
  box_muller_pair(w.x, w.y, v0, v1);
  box_muller_pair(w.z, w.w, v2, v3);
}

// one value: its pair only, through the same function as seeded_normal4
BV2_RNG_HD float seeded_normal(int64_t seed, int which, int row, int t) {
  const Philox4 w = seeded_words(seed, which, row >> 2, t);
  const bool p = (row >> 1) & 1;
  float e, o;
  box_muller_pair(p ? w.z : w.x, p ? w.w : w.y, &e, &o);
  return (row & 1) ? o : e;
}

}  // namespace bv2
