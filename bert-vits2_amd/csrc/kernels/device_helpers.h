// device_helpers.h — the numeric primitives every kernel file shares, each defined ONCE: the native vector types, bf16 / fp16 pack and
// unpack, the bf16x3 / fp16x2 operand splits of the x6 / x3 convs, leaky-ReLU, the byte-offset loads, the 32x32x16 MFMA overloads, the
// wave max and the max |x| slot publish, and the timeline record.  These few lines decide rounding, and the bit-identity tests between
// the layer-wise and the fused kernels (tests/test_x6_gpu.py and its siblings) assume both sides round alike.  A few call sites keep an
// open-coded copy, each marked with a comment, because the call changed the order of the emitted instructions there; the one that
// matters for bit-identity is conv_x6.hip store_x, whose three-plane split must stay in step with split3_bf16 below by hand.
#pragma once
#include <hip/hip_runtime.h>
#include "../bv2_kernels.h"

namespace bv2 {

// native vectors (HIP's float4 struct defeats SROA in the conv kernels)
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ---- bf16: a 32-bit word holds two values, [15:0] and [31:16]
__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ unsigned bf_pack(float a, float b) {     // round-to-nearest-even (v_cvt_pk_bf16_f32)
  bf16x2 r;
  r[0] = (__bf16)a; r[1] = (__bf16)b;
  return __builtin_bit_cast(unsigned, r);
}
__device__ __forceinline__ float bf_round(float v) { return (float)(__bf16)v; }     // round-to-nearest-even to a bf16 value

// ---- fp16: round-to-nearest-even (v_cvt_f16_f32 x 2 + pack)
__device__ __forceinline__ unsigned f16_pack(float a, float b) {
  f32x2 v = {a, b};
  const f16x2 r = __builtin_convertvector(v, f16x2);
  return __builtin_bit_cast(unsigned, r);
}
__device__ __forceinline__ f32x2 f16_unpack(unsigned u) { return __builtin_convertvector(__builtin_bit_cast(f16x2, u), f32x2); }

__device__ __forceinline__ float lrelu(float v, float slope) { return v < 0.f ? v * slope : v; }

// load base[byte_off]: wave-uniform base (SGPR pair) + 32-bit per-lane BYTE offset -> the `global_load v, v_off, s[base]`
// addressing form (one VGPR per address instead of a 64-bit pair)
__device__ __forceinline__ float ld_off(const float* base, unsigned byte_off) {
  return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off);
}
__device__ __forceinline__ f32x4 ld_off4(const float* base, unsigned byte_off) {
  return *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(base) + byte_off);
}

__device__ __forceinline__ f32x16 mfma_32x32x16(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma_32x32x16(f16x8 a, f16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }

// max over the wave's 64 lanes, in every lane
__device__ __forceinline__ float wave_max(float m) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
  return m;
}

// ConvProb::omax: the wave's max |v| into its XCD's line of the slot (bv2_kernels.h).  |v| >= 0, so fp32 bit patterns order like the
// values.  `seen`: the word as read at the start of the kernel (stale is fine: it only filters redundant atomics).
__device__ __forceinline__ unsigned* x3_slot_word(unsigned* slot) {
  return slot + X3_LINE_WORDS * (__builtin_amdgcn_s_getreg((31 << 11) | 20) & 7u);      // XCC_ID
}
__device__ __forceinline__ void x3_publish(unsigned* word, unsigned seen, float vmx, int lane) {
  const unsigned bits = __float_as_uint(wave_max(vmx));
  if (lane == 0 && bits > seen) __hip_atomic_fetch_max(word, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ---- the operand splits of the fp32 convs on the bf16 / fp16 matrix core, a pair of values at a time (word = {a, b})
constexpr float X6_BF16_MAX = 3.38953139e38f;   // 0x7f7f0000
// x6: the three bf16 planes.  Plane 1 saturates at the largest bf16 (x6_split, bv2_kernels.h): a finite value never rounds to +-inf, its
// remainder a - h1 (< 2^120) is exact in planes 2 and 3; inf / NaN leave the clamp finite but their remainders are inf / NaN
__device__ __forceinline__ void split3_bf16(float a, float b, unsigned& u1, unsigned& u2, unsigned& u3) {
  u1 = bf_pack(__builtin_amdgcn_fmed3f(a, -X6_BF16_MAX, X6_BF16_MAX), __builtin_amdgcn_fmed3f(b, -X6_BF16_MAX, X6_BF16_MAX));
  a -= bf_lo(u1); b -= bf_hi(u1);
  u2 = bf_pack(a, b);
  a -= bf_lo(u2); b -= bf_hi(u2);
  u3 = bf_pack(a, b);
}
// x3 (bv2_kernels.h): the two fp16 halves of SCALED values, |a|, |b| < 2^15: g0 = fp16(a), g1 = fp16(a - g0); the remainder is exact in fp32
__device__ __forceinline__ void split2_f16(float a, float b, unsigned& u1, unsigned& u2) {
  u1 = f16_pack(a, b);
  const f32x2 f = f16_unpack(u1);
  u2 = f16_pack(a - f[0], b - f[1]);
}

// tools/timeline.py's record of one workgroup (8 words at d; the kernel's dbg pointer is null in the product): the caller's three stamps,
// now, where the workgroup ran, and the caller's word 6 = taps (or units) | ticks of a phase of its choice << 16
__device__ __forceinline__ void timeline_record(unsigned long long* d, unsigned long long ts0, unsigned long long ts1,
                                                unsigned long long ts2, int taps, unsigned long long ticks = 0) {
  d[0] = ts0; d[1] = ts1; d[2] = ts2; d[3] = __builtin_amdgcn_s_memtime();
  d[4] = __builtin_amdgcn_s_getreg((31 << 11) | 4);               // HW_ID
  d[5] = __builtin_amdgcn_s_getreg((31 << 11) | 20);              // XCC_ID
  d[6] = (unsigned long long)taps | (ticks << 16); d[7] = 1;
}

}  // namespace bv2
