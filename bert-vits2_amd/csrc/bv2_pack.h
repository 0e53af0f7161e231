// bv2_pack.h — the host-side writers of the packed weight formats, one per format, next to the index functions (bv2_kernels.h) that
// define each stream's element order.  The packers (bv2_model.cpp, bv2_bert.cpp) and the tests' kernel entry points (bv2_testing.cpp) fill through
// these, so a kernel held to its bar on a test-packed weight is held on what the product packs.  Host only.
//
// A weight source is any callable src(co, ci, j) -> float, a bias source bsrc(co) -> float.  Every writer stores exactly the elements
// its index function names for co < cout, ci < cin, j < k and nothing else: the destination's padding is the caller's to zero.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>

#include "bv2_internal.h"
#include "bv2_kernels.h"

namespace bv2 {

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// ---- the header every packed blob opens with (kBlobHeaderFloats floats, zeroed by the caller): magic, ABI version, config hash, the
// blob's own layout number, then its length in floats.  The inference blob (kBlobMagic, BV2_PACK_LAYOUT), the posterior encoder's
// (kPosteriorMagic, BV2_POSTERIOR_LAYOUT) and the forward duration predictor's (kSdpForwardMagic, BV2_SDP_FORWARD_LAYOUT) differ in the
// two numbers only; the attach calls read it back with blob_header_matches.
inline void write_blob_header(float* blob, uint32_t magic, uint32_t layout, uint32_t cfg_hash, int64_t total_floats) {
  uint32_t* hdr = reinterpret_cast<uint32_t*>(blob);
  hdr[0] = magic; hdr[1] = BV2_ABI_VERSION; hdr[2] = cfg_hash; hdr[3] = layout;
  std::memcpy(hdr + 4, &total_floats, sizeof(total_floats));
}
inline bool blob_header_matches(const uint32_t hdr[8], uint32_t magic, uint32_t layout, uint32_t cfg_hash, int64_t total_floats) {
  int64_t tf;
  std::memcpy(&tf, hdr + 4, sizeof(tf));
  return hdr[0] == magic && hdr[1] == BV2_ABI_VERSION && hdr[2] == cfg_hash && hdr[3] == layout && tf == total_floats;
}

// ---- descriptors (offsets left unset)
inline ConvW conv_desc(int cin, int cout, int k) {               // fp32 stream, with its optional bf16 / fp16 / x6 / x3 companions
  ConvW c;
  c.cin = cin; c.cout = cout; c.k = k;
  c.cin_pad = round_up(cin, 16); c.cout_pad = round_up(cout, 32); c.w_ld = round_up(cout, 128);
  return c;
}
inline ConvW conv_cl_desc(int cin, int cout, int k) {            // channels-last stream only (no fp32 copy)
  ConvW c;
  c.cin = cin; c.cout = cout; c.k = k;
  c.cin_pad = cin; c.cout_pad = round_up(cout, 32); c.w_ld = c.cout_pad;
  return c;
}

// ---- the WN gate order (ACT_GATE, bv2_kernels.h): packed row n of an in_layer (2 * hid rows; also of a layer's cond_layer slice) is source
// row wn_gate_row(hid, n) — every 32-row tile holds the tanh rows of 16 channels, then the sigmoid rows (source row hid + c) of the same 16
inline int wn_gate_row(int hid, int n) {
  const int mt = n / 32, j = n % 32;
  return j < 16 ? 16 * mt + j : hid + 16 * mt + (j - 16);
}

// ---- sizes, in floats unless the name says otherwise
inline int64_t conv_w_floats(const ConvW& c) { return (int64_t)c.k * c.cin_pad * c.w_ld; }
inline int64_t cl_w_floats(const ConvW& c) { return (cl_w_elems(c.cin, c.cout_pad, c.k) + 1) / 2; }
inline int64_t x6_w_floats(const ConvW& c) { return (x6_w_elems(c.cin, c.cout_pad, c.k) + 1) / 2; }
inline int64_t x3_region_floats(const ConvW& c) { return X3_HDR_FLOATS + (x3_w_elems(c.cin, c.cout_pad, c.k) + 1) / 2; }   // 1 / S_w, then the planes
constexpr int kRbclBiasRow = 32, kRb16BiasRow = 16;              // floats per conv in the two whole-ResBlock bias blocks
inline int64_t rbcl_stream_units(int C, int k, int nd) { return (int64_t)2 * nd * resblock_cl_bf16_units(C, k) + RBCL_PD; }   // 512 bf16 each
inline int64_t rb16_stream_units(int k, int nd) { return (int64_t)2 * nd * rb16_units(k); }

// ---- one writer per format
template <class F>
inline void for_each_weight(int cin, int cout, int k, const F& f) {
  for (int j = 0; j < k; ++j)
    for (int ci = 0; ci < cin; ++ci)
      for (int co = 0; co < cout; ++co) f(co, ci, j);
}
template <class Src>
inline void pack_f32(float* dst, int cin, int cout, int k, const Src& src, int co0 = 0) {   // co0: the rows land at [co0, co0 + cout) of a fused matrix
  const int cin_pad = round_up(cin, 16);
  for_each_weight(cin, cout, k, [&](int co, int ci, int j) { dst[conv_w_index(j, ci, co0 + co, cin_pad, k)] = src(co, ci, j); });
}
template <class Src>
inline void pack_cl_bf16(uint16_t* dst, int cin, int cout, int k, const Src& src) {
  for_each_weight(cin, cout, k, [&](int co, int ci, int j) { dst[cl_w_index(j, ci, co, cin, k)] = f2bf(src(co, ci, j)); });
}
template <class Src>
inline void pack_cl_f16(uint16_t* dst, int cin, int cout, int k, const Src& src) {
  for_each_weight(cin, cout, k, [&](int co, int ci, int j) { dst[cl_w_index(j, ci, co, cin, k)] = f2h(src(co, ci, j)); });
}
// w = h1 + h2 + h3 exactly, one bf16 plane each
template <class Src>
inline void pack_x6(uint16_t* dst, int cin, int cout, int k, const Src& src) {
  for_each_weight(cin, cout, k, [&](int co, int ci, int j) {
    uint16_t h[3];
    x6_split(src(co, ci, j), h);
    for (int pl = 0; pl < 3; ++pl) dst[x6_w_index(j, ci, co, cin, k, pl)] = h[pl];
  });
}
// w * S_w = g0 + g1 in two fp16 planes, S_w from the tensor's largest magnitude; returns 1 / S_w (the float in front of the planes)
template <class Src>
inline float pack_x3(uint16_t* dst, int cin, int cout, int k, const Src& src) {
  float wmax = 0.f;
  for_each_weight(cin, cout, k, [&](int co, int ci, int j) { wmax = std::max(wmax, std::fabs(src(co, ci, j))); });
  uint32_t mb;
  std::memcpy(&mb, &wmax, 4);
  const unsigned e = x3_scale_exp(mb);
  const float S = x3_scale(e);
  for_each_weight(cin, cout, k, [&](int co, int ci, int j) {
    const float v = src(co, ci, j) * S;                          // exact: S is a power of two, |v| < 2^15
    const uint16_t g0 = f2h(v);
    dst[x3_w_index(j, ci, co, cin, k, 0)] = g0;
    dst[x3_w_index(j, ci, co, cin, k, 1)] = f2h(v - h2f(g0));
  });
  return x3_scale_inv(e);
}
template <class BSrc>
inline void pack_bias(float* dst, int cout, const BSrc& bsrc) {  // the first cout floats of a row of cout_pad
  for (int co = 0; co < cout; ++co) dst[co] = bsrc(co);
}

// ---- the whole-ResBlock streams, rearranged from a conv's bf16 channels-last stream `cl` (C -> C, k taps) and its bias `b`;
// `slot` = 2 * d + e, the conv's place among the block's 2 * nd
// TAP-MAJOR unit order (tap j outer, 16-channel group s inner; kernels/resblock_cl_bf16.hip): the kernel's LDS walk then needs one pointer
// add per tap and immediate offsets for the groups; the per-conv stream is group-major (unit = s * k + j; m-tile 0 = the whole channel dim)
inline void rbcl_put_conv(uint16_t* stream, float* bias, int slot, const uint16_t* cl, const float* b, int C, int k) {
  const int G = C / 16;
  uint16_t* dst = stream + (int64_t)slot * resblock_cl_bf16_units(C, k) * 512;
  for (int j = 0; j < k; ++j)
    for (int s = 0; s < G; ++s) std::memcpy(dst + ((int64_t)j * G + s) * 512, cl + ((int64_t)s * k + j) * 512, sizeof(uint16_t) * 512);
  std::memcpy(bias + slot * kRbclBiasRow, b, sizeof(float) * (size_t)C);
}
// C = 16: the tap-pair stream of kernels/resblock_c16_bf16.hip
inline void rb16_put_conv(uint16_t* stream, float* bias, int slot, const uint16_t* cl, const float* b, int k) {
  uint16_t* dst = stream + (int64_t)slot * rb16_units(k) * 512;
  for_each_weight(16, 16, k, [&](int co, int ci, int j) { dst[rb16_w_index(j, ci, co)] = cl[cl_w_index(j, ci, co, 16, k)]; });
  std::memcpy(bias + slot * kRb16BiasRow, b, sizeof(float) * 16);
}

}  // namespace bv2
