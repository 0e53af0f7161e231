// bv2_testing.cpp — the test-only kernel entry points declared in include/bv2_testing.h: single kernels and host-side packers behind
// plain C launchers, for tests/ and tools/.  The product's C ABI (include/bv2.h) is bv2_api.cpp.
#include <cmath>
#include <cstddef>
#include <cstring>
#include <functional>
#include <vector>

#include "bv2_internal.h"
#include "bv2_pack.h"
#include "../../include/bv2_testing.h"
#include "kernels/rng.h"

using namespace bv2;

// a dense weight [cout][cin][k] / bias [cout] (null: zeros) as the sources the writers of bv2_pack.h take
static auto t_dense(const float* w, int cin, int k) {
  return [=](int co, int ci, int j) { return w[((size_t)co * cin + ci) * k + j]; };
}
static auto t_bias(const float* b) { return [=](int co) { return b ? b[co] : 0.f; }; }

extern "C" {

int64_t bv2_test_conv_pack_floats(int cin, int cout, int k) {
  const ConvW c = conv_desc(cin, cout, k);
  // + 2048 floats: the register-ring conv kernel prefetches up to 4 units (4 KB) past the last weight unit
  // + the three split-bf16 planes of conv_x6.hip (tile >= TILE_X6), 6 bytes per weight of the 32-row padded matrix
  const int64_t base = conv_w_floats(c) + c.cout_pad + 2048;
  // + the x3 form's region (tile == TILE_X3): two slots (max |x| in, max |out| back), 1 / S_w, the two fp16 planes
  return base + (cin % 32 == 0 ? x6_w_floats(c) + 64 + 2 * X3_SLOT_WORDS + x3_region_floats(c) + 64 : 0);
}
void bv2_test_x6_split(float v, uint16_t* h3) { x6_split(v, h3); }
int bv2_test_convert(int kind, const void* in, void* out, int64_t n) {
  if (!in || !out || n < 0 || kind < 0 || kind > 2) return -1;
  const float* f = static_cast<const float*>(in);
  const uint16_t* u = static_cast<const uint16_t*>(in);
  for (int64_t i = 0; i < n; ++i) {
    if (kind == 0) static_cast<uint16_t*>(out)[i] = f2bf(f[i]);
    else if (kind == 1) static_cast<uint16_t*>(out)[i] = f2h(f[i]);
    else static_cast<float*>(out)[i] = h2f(u[i]);
  }
  return 0;
}
int bv2_test_x6_regions(const bv2_handle* h, int64_t* off_floats, int64_t* n_floats, int max_regions) {
  if (!h || !off_floats || !n_floats) return -1;
  const Model& m = h->model;
  int n = 0;
  auto add = [&](const ConvW& w) {
    if (w.wx_off < 0) return;
    if (n < max_regions) { off_floats[n] = w.wx_off; n_floats[n] = x6_w_floats(w); }
    ++n;
  };
  for (int i = 0; i < m.n_ups; ++i)
    for (int j = 0; j < m.n_rbk; ++j)
      for (int d = 0; d < m.n_rbd; ++d)
        for (int e = 0; e < 2; ++e) add(m.rb[i][j][d][e]);
  return n;
}
int bv2_test_x3_regions(const bv2_handle* h, int64_t* off_floats, int64_t* n_floats, int max_regions) {
  if (!h || !off_floats || !n_floats) return -1;
  const Model& m = h->model;
  int n = 0;
  for (int i = 0; i < m.n_ups; ++i)
    for (int j = 0; j < m.n_rbk; ++j)
      for (int d = 0; d < m.n_rbd; ++d)
        for (int e = 0; e < 2; ++e) {
          const ConvW& w = m.rb[i][j][d][e];
          if (w.wy_off < 0 || w.wx_off < 0) continue;
          if (n < max_regions) { off_floats[n] = w.wy_off; n_floats[n] = x3_region_floats(w); }
          ++n;
        }
  return n;
}
static int64_t t_x6_off(int cin, int cout, int k) {
  const ConvW c = conv_desc(cin, cout, k);
  return (conv_w_floats(c) + c.cout_pad + 2048 + 63) / 64 * 64;
}
static int64_t t_x3_off(int cin, int cout, int k) {                 // the x3 region: [slot in] [slot out] (X3_SLOT_WORDS each) [1 / S_w (64)] [planes]
  return (t_x6_off(cin, cout, k) + x6_w_floats(conv_desc(cin, cout, k)) + 64 + 63) / 64 * 64;
}
int64_t bv2_test_x3_omax_off(int cin, int cout, int k) { return t_x3_off(cin, cout, k) + X3_SLOT_WORDS; }

// one conv w_host [cout][cin][k] + bias_host [cout] (or null) into a zeroed region of bv2_test_conv_pack_floats(cin, cout, k) floats: the
// packed fp32 stream, the bias behind it, with x6 the three bf16 planes at t_x6_off, and with x3 the region at t_x3_off:
// [max |x| slot] [max |out| slot] (X3_SLOT_WORDS each, left zero) [1 / S_w] (X3_HDR_FLOATS) [the two scaled fp16 planes]
// (rowmap: packed row co is row rowmap(co) of w_host / bias_host, as Packer::conv1d's; null: co itself)
static void t_pack_conv(float* pk, const float* w_host, const float* bias_host, int cin, int cout, int k, bool x6, bool x3 = false,
                        const std::function<int(int)>* rowmap = nullptr) {
  const auto dense = t_dense(w_host, cin, k);
  const auto src = [&](int co, int ci, int j) { return dense(rowmap ? (*rowmap)(co) : co, ci, j); };
  pack_f32(pk, cin, cout, k, src);
  if (bias_host) pack_bias(pk + conv_w_floats(conv_desc(cin, cout, k)), cout, [&](int co) { return bias_host[rowmap ? (*rowmap)(co) : co]; });
  if (!x6) return;
  pack_x6(reinterpret_cast<uint16_t*>(pk + t_x6_off(cin, cout, k)), cin, cout, k, src);
  if (!x3) return;
  float* reg = pk + t_x3_off(cin, cout, k) + 2 * X3_SLOT_WORDS;
  reg[0] = pack_x3(reinterpret_cast<uint16_t*>(reg + X3_HDR_FLOATS), cin, cout, k, src);
}
// the descriptor of a conv packed by t_pack_conv at float offset `off` of a scratch that plays the blob
static ConvW t_conv_w(int64_t off, int cin, int cout, int k, bool bias, bool x6) {
  ConvW w = conv_desc(cin, cout, k);
  w.w_off = off; w.b_off = bias ? off + conv_w_floats(w) : -1;
  w.wx_off = x6 ? off + t_x6_off(cin, cout, k) : -1;
  return w;
}

// "kernarg_head" for the launch entries of this file (they have no handle): 0 = every launch below takes its generic kernel
static int g_test_no_head = 0;
void bv2_test_set_kernarg_head(int on) { g_test_no_head = on ? 0 : 1; }
// host only: the split-K head's packed fields (bv2_kernels.h sk_head_pack / sk_head_unpack).  Returns 1 and the six unpacked fields
// {k, dil, pad_left, ksplit, cin, cin_pad} when a one-problem launch with these values takes the head form, 0 when it falls back
int bv2_test_splitk_head(int k, int dil, int pad_left, int ksplit, int cin, int cin_pad, int B, int has_lens, int nprob, int32_t* out6) {
  ConvLaunch cl;
  std::memset(&cl, 0, sizeof(cl));
  static const int64_t one_len = 1;
  ConvProb& p = cl.p[0];
  p.nsrc = 1; p.k = k; p.dil = dil; p.pad_left = pad_left; p.cin = cin; p.cin_pad = cin_pad;
  cl.nprob = nprob; cl.B = B; cl.L = 1; cl.ksplit = ksplit; cl.lens = has_lens ? &one_len : nullptr;
  SkHead h;
  if (!sk_head_pack(cl, 1, 1, 1, &h)) return 0;
  const SkSmall q = sk_head_unpack(h.pk0, h.pk1);
  if (out6) { out6[0] = q.k; out6[1] = q.dil; out6[2] = q.pad_left; out6[3] = q.ksplit; out6[4] = q.cin; out6[5] = q.cin_pad; }
  return 1;
}

int bv2_test_conv1d(void* stream, const float* x, const float* w_host, const float* bias_host, float* out, float* wpack_dev,
                    int B, int cin, int cout, int k, int dil, int pad_left, int L, int tile, float lrelu_slope, int relu,
                    const float* res, int res_mode, const float* in_mask, const float* out_mask, int mask_pre,
                    int mask_post, const float* bias2, int nsrc, const float* x1, const float* x2, float in_scale, int ksplit,
                    int64_t slab_stride) {
  try {
    if (relu != ACT_NONE && relu != ACT_RELU && relu != ACT_GATE && relu != ACT_GELU) return -1;
    const ConvW c = conv_desc(cin, cout, k);
    std::vector<float> pk;
    const size_t boff = (size_t)conv_w_floats(c);
    const bool x6 = tile >= TILE_X6 && cin % 32 == 0;
    const bool x3 = tile == TILE_X3 && x6;
    if (w_host) {                                 // w_host == NULL: wpack_dev already holds the packed weight (timing loops)
      pk.assign((size_t)bv2_test_conv_pack_floats(cin, cout, k), 0.f);
      t_pack_conv(pk.data(), w_host, bias_host, cin, cout, k, x6, x3);
    }
    if (w_host && hipMemcpy(wpack_dev, pk.data(), sizeof(float) * pk.size(), hipMemcpyHostToDevice) != hipSuccess) return -6;
    ConvLaunch cl;
    std::memset(&cl, 0, sizeof(cl));
    ConvProb& p = cl.p[0];
    if (cin % 32 == 0 && ksplit <= 1) {
      // every kernel's max |out| lands in the region's second slot (bv2_test_x3_omax_off); the x3 form reads max |x| from the first: the
      // product's producers publish it from their epilogues, here a reduction launch fills the (zeroed) slot
      float* reg = wpack_dev + t_x3_off(cin, cout, k);
      if (launch_x3_zero_slots(static_cast<hipStream_t>(stream), reinterpret_cast<unsigned*>(reg), 2)) return -6;
      p.omax = reinterpret_cast<unsigned*>(reg + X3_SLOT_WORDS);
      if (x3) {
        if (nsrc != 1 || launch_absmax(static_cast<hipStream_t>(stream), x, (int64_t)B * cin * L, reinterpret_cast<unsigned*>(reg))) return -2;
        p.xmax = reinterpret_cast<const unsigned*>(reg);
        p.w3inv = reg + 2 * X3_SLOT_WORDS; p.w3 = reinterpret_cast<const uint16_t*>(reg + 2 * X3_SLOT_WORDS + X3_HDR_FLOATS);
      }
    }
    p.x[0] = x; p.x[1] = x1; p.x[2] = x2; p.nsrc = nsrc; p.in_scale = in_scale;
    p.x_bstride = (int64_t)cin * L; p.x_rstride = L; p.Lin = L;
    p.in_mask = in_mask; p.in_mask_bstride = L; p.out_mask = out_mask; p.out_mask_bstride = L;
    p.w = wpack_dev; p.bias = bias_host ? wpack_dev + boff : nullptr;
    if (x6) p.w6 = reinterpret_cast<const uint16_t*>(wpack_dev + t_x6_off(cin, cout, k));
    p.bias2 = bias2; p.bias2_bstride = cout;
    p.out = out; p.out_bstride = (int64_t)(relu == ACT_GATE ? cout / 2 : cout) * L; p.out_rstride = L; p.out_tstride = 1; p.out_toff = 0;
    p.res = res; p.res_bstride = p.out_bstride; p.res_mode = res_mode;
    p.cin = cin; p.cin_pad = c.cin_pad; p.cout = cout; p.cout_pad = c.cout_pad; p.w_ld = c.w_ld; p.k = k; p.dil = dil;
    p.pad_left = pad_left < 0 ? ((k - 1) / 2) * dil : pad_left;
    p.pre_act = lrelu_slope != 0.f ? PRE_LRELU : PRE_NONE; p.slope = lrelu_slope;
    p.act = relu; p.mask_pre = mask_pre; p.mask_post = mask_post;
    cl.nprob = 1; cl.B = B; cl.L = L; cl.ksplit = ksplit < 1 ? 1 : ksplit; cl.slab_stride = slab_stride; cl.no_head = g_test_no_head;
    const char* vn = nullptr;
    return launch_conv1d(static_cast<hipStream_t>(stream), cl, tile, &vn);
  } catch (...) { return -100; }
}

int bv2_test_resblock_fused(void* stream, const float* x, float* out, const float* w1_host, const float* b1_host,
                            const float* w2_host, const float* b2_host, float* wpack_dev, int B, int C, int k, int dil, int L,
                            float slope) {
  try {
    const size_t one = (size_t)bv2_test_conv_pack_floats(C, C, k), boff = (size_t)conv_w_floats(conv_desc(C, C, k));
    std::vector<float> pk(2 * one, 0.f);
    t_pack_conv(pk.data(), w1_host, b1_host, C, C, k, false);
    t_pack_conv(pk.data() + one, w2_host, b2_host, C, C, k, false);
    if (hipMemcpy(wpack_dev, pk.data(), sizeof(float) * pk.size(), hipMemcpyHostToDevice) != hipSuccess) return -6;
    FusedLaunch F;
    std::memset(&F, 0, sizeof(F));
    F.nprob = 1; F.B = B; F.C = C; F.L = L; F.slope = slope;
    F.p[0].x = x; F.p[0].out = out; F.p[0].w1 = wpack_dev; F.p[0].b1 = wpack_dev + boff;
    F.p[0].w2 = wpack_dev + one; F.p[0].b2 = wpack_dev + one + boff; F.p[0].k = k; F.p[0].dil = dil;
    return launch_resblock_fused(static_cast<hipStream_t>(stream), F);
  } catch (...) { return -100; }
}

int64_t bv2_test_resblock_cl_pack_bytes(int C, int k, int nd) {
  int64_t units = (int64_t)2 * nd * ((C / 16) * k + RBCL_PD) + RBCL_PD;                 // the largest of the stream formats
  return units * 1024 + (int64_t)2 * nd * (C > 32 ? C : 32) * 4 + 256;
}

int bv2_test_resblock_cl(void* stream, const void* x, void* out, const float* w_host, const float* bias_host, void* wpack_dev, int B,
                         int C, int k, const int* dil, int nd, int L, float slope, int variant, const int64_t* lens) {
  try {
    if (nd < 1 || nd > BV2_RBCL_MAX_D) return -2;
    if (variant != 0 && variant != 1) return -2;
    if (variant == 1 ? !resblock_c16_bf16_supported(C, k, dil, nd) : !resblock_cl_bf16_supported(C, k, dil, nd)) return -2;
    // as the packer (bv2_model.cpp): each conv's channels-last bf16 stream, then rearranged into the block's stream
    const int64_t wunits = variant == 1 ? rb16_stream_units(k, nd) : rbcl_stream_units(C, k, nd);
    std::vector<uint16_t> pk((size_t)wunits * 512, 0);
    std::vector<float> pb((size_t)2 * nd * (variant == 1 ? kRb16BiasRow : kRbclBiasRow), 0.f);
    for (int s = 0; s < 2 * nd; ++s) {
      std::vector<uint16_t> cl((size_t)cl_w_elems(C, round_up(C, 32), k), 0);
      pack_cl_bf16(cl.data(), C, C, k, t_dense(w_host + (size_t)s * C * C * k, C, k));
      if (variant == 1) rb16_put_conv(pk.data(), pb.data(), s, cl.data(), bias_host + (size_t)s * C, k);
      else rbcl_put_conv(pk.data(), pb.data(), s, cl.data(), bias_host + (size_t)s * C, C, k);
    }
    char* base = static_cast<char*>(wpack_dev);
    const size_t wbytes = pk.size() * 2, boff = (wbytes + 255) / 256 * 256;
    if (hipMemcpy(base, pk.data(), wbytes, hipMemcpyHostToDevice) != hipSuccess) return -6;
    if (hipMemcpy(base + boff, pb.data(), pb.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return -6;
    RbClLaunch F;
    std::memset(&F, 0, sizeof(F));
    F.nprob = 1; F.B = B; F.C = C; F.L = L; F.nd = nd; F.slope = slope; F.lens = lens; F.len_mul = 1;
    F.p[0].x = static_cast<const uint16_t*>(x); F.p[0].out = static_cast<uint16_t*>(out);
    F.p[0].w = reinterpret_cast<const uint16_t*>(base); F.p[0].bias = reinterpret_cast<const float*>(base + boff);
    F.p[0].k = k;
    for (int d = 0; d < nd; ++d) F.p[0].dil[d] = dil[d];
    return variant == 1 ? launch_resblock_c16_bf16(static_cast<hipStream_t>(stream), F)
                        : launch_resblock_cl_bf16(static_cast<hipStream_t>(stream), F);
  } catch (...) { return -100; }
}

// ---- direct kernel-level entries for the round-4 fused kernels (they were only held to the layer-wise kernels)
int bv2_test_respair_cl(void* stream, const void* x, void* out, const float* w_host, const float* bias_host, void* wpack_dev, int B,
                        int C, int k, int dil, int L, float slope, int form, const int64_t* lens) {
  try {
    if (!respair_cl_bf16_supported(C, k, dil)) return -2;
    const int64_t ne = cl_w_elems(C, C, k);
    std::vector<uint16_t> pk((size_t)2 * ne, 0);
    for (int e = 0; e < 2; ++e) pack_cl_bf16(pk.data() + e * ne, C, C, k, t_dense(w_host + (size_t)e * C * C * k, C, k));
    char* base = static_cast<char*>(wpack_dev);
    const size_t wbytes = pk.size() * 2 + 8192, boff = (wbytes + 255) / 256 * 256;     // + slack: the rings run a few units past a stream's end
    if (hipMemset(base, 0, boff + (size_t)2 * C * 4) != hipSuccess) return -6;
    if (hipMemcpy(base, pk.data(), pk.size() * 2, hipMemcpyHostToDevice) != hipSuccess) return -6;
    if (hipMemcpy(base + boff, bias_host, (size_t)2 * C * 4, hipMemcpyHostToDevice) != hipSuccess) return -6;
    RpClLaunch F;
    std::memset(&F, 0, sizeof(F));
    F.nprob = 1; F.B = B; F.C = C; F.L = L; F.slope = slope; F.lens = lens; F.len_mul = 1; F.form = form; F.mix = 1;
    RpClProb& q = F.p[0];
    q.x = static_cast<const uint16_t*>(x); q.out = static_cast<uint16_t*>(out);
    q.w1 = reinterpret_cast<const uint16_t*>(base); q.w2 = q.w1 + ne;
    q.b1 = reinterpret_cast<const float*>(base + boff); q.b2 = q.b1 + C;
    q.k = k; q.dil = dil;
    return launch_respair_cl_bf16(static_cast<hipStream_t>(stream), F, nullptr);
  } catch (...) { return -100; }
}
int64_t bv2_test_respair_cl_pack_bytes(int C, int k) { return cl_w_elems(C, C, k) * 4 + 8192 + 256 + (int64_t)2 * C * 4; }

int64_t bv2_test_respair_x6_pack_bytes(int C, int k) { return x6_w_elems(C, (C + 31) / 32 * 32, k) * 4 + 16384 + 256 + (int64_t)2 * 32 * 4 + (int64_t)2 * C * 4 + 1024; }
// the C = 32 pair from the three bf16 planes of each conv (x3 = false) or from their two scaled fp16 planes.  Scratch: [planes of conv 1]
// [of conv 2] [16 KB ring slack], then 256-byte aligned [b1] [b2] (cout_pad floats each) [1 / S_w of conv 1] [of conv 2] (64 floats each)
static int t_respair_x(bool x3, void* stream, const float* x, float* out, const float* w_host, const float* bias_host, void* wpack_dev,
                       int B, int C, int k, int dil, int L, float slope, const int64_t* lens) {
  try {
    if (!respair_x6_supported(C, k, dil)) return -2;
    const int cout_pad = round_up(C, 32);
    const int64_t ne = x3 ? x3_w_elems(C, cout_pad, k) : x6_w_elems(C, cout_pad, k);
    std::vector<uint16_t> pk((size_t)2 * ne, 0);
    std::vector<float> pb((size_t)2 * cout_pad + 128, 0.f);
    for (int e = 0; e < 2; ++e) {
      const auto src = t_dense(w_host + (size_t)e * C * C * k, C, k);
      if (x3) pb[(size_t)2 * cout_pad + 64 * e] = pack_x3(pk.data() + e * ne, C, C, k, src);
      else pack_x6(pk.data() + e * ne, C, C, k, src);
      pack_bias(pb.data() + (size_t)e * cout_pad, C, t_bias(bias_host + (size_t)e * C));
    }
    char* base = static_cast<char*>(wpack_dev);
    const size_t wbytes = pk.size() * 2 + 16384, boff = (wbytes + 255) / 256 * 256;
    if (hipMemset(base, 0, boff + pb.size() * 4) != hipSuccess) return -6;
    if (hipMemcpy(base, pk.data(), pk.size() * 2, hipMemcpyHostToDevice) != hipSuccess) return -6;
    if (hipMemcpy(base + boff, pb.data(), pb.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return -6;
    FusedLaunch F;
    std::memset(&F, 0, sizeof(F));
    F.nprob = 1; F.B = B; F.C = C; F.L = L; F.slope = slope; F.lens = lens; F.len_mul = 1;
    FusedProb& q = F.p[0];
    q.x = x; q.out = out; q.k = k; q.dil = dil;
    q.w61 = reinterpret_cast<const uint16_t*>(base); q.w62 = q.w61 + ne;      // (the launcher insists on them; not read by the x3 form)
    q.b1 = reinterpret_cast<const float*>(base + boff); q.b2 = q.b1 + cout_pad;
    if (x3) { q.w31 = q.w61; q.w32 = q.w62; q.w3inv1 = q.b1 + 2 * cout_pad; q.w3inv2 = q.w3inv1 + 64; }
    q.w1 = q.b1; q.w2 = q.b1;                        // the fp32 streams are not read by this kernel
    return launch_respair_x6(static_cast<hipStream_t>(stream), F);
  } catch (...) { return -100; }
}
int bv2_test_respair_x3(void* stream, const float* x, float* out, const float* w_host, const float* bias_host, void* wpack_dev, int B,
                        int C, int k, int dil, int L, float slope, const int64_t* lens) {
  return t_respair_x(true, stream, x, out, w_host, bias_host, wpack_dev, B, C, k, dil, L, slope, lens);
}
int bv2_test_respair_x6(void* stream, const float* x, float* out, const float* w_host, const float* bias_host, void* wpack_dev, int B,
                        int C, int k, int dil, int L, float slope, const int64_t* lens) {
  return t_respair_x(false, stream, x, out, w_host, bias_host, wpack_dev, B, C, k, dil, L, slope, lens);
}

int bv2_test_flow_boundary(void* stream, const float* a, int nslab, int64_t slab_stride, const float* gamma, const float* beta,
                           const float* mask, float* x1, int64_t z_bstride, const float* post_w_host, const float* post_b_host,
                           const float* pre_w_host, const float* pre_b_host, float* pre_out, float* wpack_dev, int B, int C, int T) {
  try {
    const int C1 = C / 2;
    // two 1x1 convs in the packed conv layout (conv_w_index, k = 1): post C -> C1, pre C1 -> C
    const size_t npost = (size_t)conv_w_floats(conv_desc(C, C1, 1)), npre = (size_t)conv_w_floats(conv_desc(C1, C, 1));
    std::vector<float> pk((size_t)bv2_test_flow_boundary_pack_floats(C), 0.f);
    pack_f32(pk.data(), C, C1, 1, t_dense(post_w_host, C, 1));
    if (pre_w_host) pack_f32(pk.data() + npost, C1, C, 1, t_dense(pre_w_host, C1, 1));
    pack_bias(pk.data() + npost + npre, C1, t_bias(post_b_host));
    if (pre_b_host) pack_bias(pk.data() + npost + npre + C1, C, t_bias(pre_b_host));
    if (hipMemcpy(wpack_dev, pk.data(), pk.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return -6;
    FbArgs F;
    std::memset(&F, 0, sizeof(F));
    F.a = a; F.nslab = nslab; F.slab_stride = slab_stride; F.gamma = gamma; F.beta = beta; F.eps = 1e-5f; F.mask = mask;
    F.x1 = x1; F.x1_out = x1; F.z_bstride = z_bstride; F.post_w = wpack_dev; F.post_b = wpack_dev + npost + npre;
    if (pre_w_host) { F.pre_w = wpack_dev + npost; F.pre_b = wpack_dev + npost + npre + C1; F.pre_out = pre_out; }
    F.B = B; F.C = C; F.T = T; F.C1 = C1; F.no_head = g_test_no_head;
    if (!flow_boundary_supported(F)) return -2;
    return launch_flow_boundary(static_cast<hipStream_t>(stream), F);
  } catch (...) { return -100; }
}
int64_t bv2_test_flow_boundary_pack_floats(int C) {
  const int C1 = C / 2;
  return conv_w_floats(conv_desc(C, C1, 1)) + conv_w_floats(conv_desc(C1, C, 1)) + C1 + C + 64;
}

int64_t bv2_test_conv_cl_pack_bytes(int cin, int cout, int k) {
  return cl_w_elems(cin, round_up(cout, 32), k) * 2 + (int64_t)round_up(cout, 32) * 4;
}
}  // extern "C"
// a conv's channels-last stream (bf16, or fp16) and, behind it, its zero-padded bias row to the device: bv2_test_conv_cl_pack_bytes bytes
template <class Src, class BSrc>
static bool t_upload_cl(void* dev, bool f16, int cin, int cout, int k, const Src& src, const BSrc& bsrc) {
  const int cout_pad = round_up(cout, 32);
  const int64_t ne = cl_w_elems(cin, cout_pad, k);
  std::vector<uint16_t> pk((size_t)ne, 0);
  if (f16) pack_cl_f16(pk.data(), cin, cout, k, src);
  else pack_cl_bf16(pk.data(), cin, cout, k, src);
  std::vector<float> bb((size_t)cout_pad, 0.f);
  pack_bias(bb.data(), cout, bsrc);
  return hipMemcpy(dev, pk.data(), (size_t)ne * 2, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(static_cast<char*>(dev) + ne * 2, bb.data(), (size_t)cout_pad * 4, hipMemcpyHostToDevice) == hipSuccess;
}
extern "C" {

int bv2_test_conv_cl_bf16(void* stream, const void* x0, const void* x1, const void* x2, int nsrc, const float* w_host,
                          const float* bias_host, void* wpack_dev, void* out, const void* res, const float* bias2, int B, int cin,
                          int cout, int k, int dil, int pad_left, int L, int pre_lrelu, float slope) {
  try {
    if (!conv_cl_bf16_supported(cin, cout, k, dil)) return -2;
    const int cout_pad = round_up(cout, 32);
    const int64_t ne = cl_w_elems(cin, cout_pad, k);
    // w_host == NULL: wpack_dev already holds the packed weight (timing loops)
    if (w_host && !t_upload_cl(wpack_dev, false, cin, cout, k, t_dense(w_host, cin, k), t_bias(bias_host))) return -6;
    ClLaunch cl;
    std::memset(&cl, 0, sizeof(cl));
    ClProb& p = cl.p[0];
    p.x[0] = static_cast<const uint16_t*>(x0); p.x[1] = static_cast<const uint16_t*>(x1); p.x[2] = static_cast<const uint16_t*>(x2);
    p.nsrc = nsrc; p.in_scale = 1.f / (float)nsrc; p.x_bstride = (int64_t)cin * L; p.Lin = L;
    p.w = static_cast<const uint16_t*>(wpack_dev);
    p.bias = bias_host ? reinterpret_cast<const float*>(static_cast<char*>(wpack_dev) + ne * 2) : nullptr;
    p.bias2 = bias2; p.bias2_bstride = cout;
    p.out = static_cast<uint16_t*>(out); p.out_bstride = (int64_t)cout * L;
    p.res = static_cast<const uint16_t*>(res); p.res_bstride = p.out_bstride;
    p.cin = cin; p.cout = cout; p.cout_pad = cout_pad; p.k = k; p.dil = dil;
    p.pad_left = pad_left < 0 ? ((k - 1) / 2) * dil : pad_left;
    p.pre_lrelu = pre_lrelu; p.slope = slope;
    cl.nprob = 1; cl.B = B; cl.L = L;
    return launch_conv_cl_bf16(static_cast<hipStream_t>(stream), cl, nullptr);
  } catch (...) { return -100; }
}

int bv2_test_conv_f16(void* stream, const void* x, int in_ct, const float* in_mask, const float* w_host, const float* bias_host,
                      void* wpack_dev, void* out, int out_ct, const float* res, int res_mode, const float* out_mask, int mask_pre,
                      int mask_post, int act, int B, int cin, int cout, int k, int dil, int L, int out_rstride) {
  return bv2_test_conv_f16_ex(stream, x, in_ct, in_mask, w_host, bias_host, wpack_dev, out, out_ct, res, res_mode, out_mask, mask_pre,
                              mask_post, act, B, cin, cout, k, dil, L, out_rstride, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                              0, 0, 0, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 0);
}

int bv2_test_dump_cl_conv(bv2_handle* h, const void* host_blob, int kind, int i, int j, int d, int e, int32_t* dims,
                          float* w_out, float* bias_out) {
  if (!h || !host_blob || !dims) return -1;
  try {
    const Model& m = h->model;
    const ConvW* w = nullptr;
    int pad_left = 0;
    if (kind == 0) { w = &m.conv_pre; pad_left = (w->k - 1) / 2; }
    else if (kind == 1 && i >= 0 && i < m.n_ups) { w = &m.ups[i].cl; pad_left = m.ups[i].cl_pad_left; }
    else if (kind == 2 && i >= 0 && i < m.n_ups && j >= 0 && j < m.n_rbk && d >= 0 && d < m.n_rbd && (e == 0 || e == 1)) {
      w = &m.rb[i][j][d][e];
      pad_left = ((w->k - 1) / 2) * (e == 0 ? m.cfg.resblock_dilation_sizes[j][d] : 1);
    }
    // kind 3: fp16 stream of a transformer-flow Encoder conv — coupling i (application order), layer j, d = 0 qkv / 1 o /
    //         2 ffn conv_1 / 3 ffn conv_2.   kind 4: resblock conv rb[i][j][d][e] read back from the TAP-MAJOR whole-ResBlock
    //         stream (must equal kind 2).
    bool half = false, tapmajor = false, tappair = false;
    if (kind == 3 && i >= 0 && i < m.n_coupling && m.cfg.use_transformer_flow && j >= 0 && j < m.coupling[i].enc.n_layers &&
        d >= 0 && d < 4) {
      const EncLayerW& L = m.coupling[i].enc.layer[j];
      w = d == 0 ? &L.qkv : (d == 1 ? &L.o : (d == 2 ? &L.ffn1 : &L.ffn2));
      pad_left = (w->k - 1) / 2;
      half = true;
      if (w->wh_off < 0) return -2;
    } else if (kind == 4 && i >= 0 && i < m.n_ups && j >= 0 && j < m.n_rbk && d >= 0 && d < m.n_rbd && (e == 0 || e == 1)) {
      w = &m.rb[i][j][d][e];
      pad_left = ((w->k - 1) / 2) * (e == 0 ? m.cfg.resblock_dilation_sizes[j][d] : 1);
      tapmajor = true;
      if (m.rbcl_w_off[i][j] < 0) return -2;
    }
    else if (kind == 5 && i >= 0 && i < m.n_ups && j >= 0 && j < m.n_rbk && d >= 0 && d < m.n_rbd && (e == 0 || e == 1)) {
      // kind 5: rb[i][j][d][e] read back from the tap-PAIR stream of kernels/resblock_c16_bf16.hip (must equal kind 2)
      w = &m.rb[i][j][d][e];
      pad_left = ((w->k - 1) / 2) * (e == 0 ? m.cfg.resblock_dilation_sizes[j][d] : 1);
      tappair = true;
      if (m.rb16_w_off[i][j] < 0) return -2;
    }
    if (!w || (!half && w->wb_off < 0)) return -2;
    dims[0] = w->cin; dims[1] = w->cout; dims[2] = w->k; dims[3] = pad_left;
    const float* blob = static_cast<const float*>(host_blob);
    const uint16_t* wb = reinterpret_cast<const uint16_t*>(blob + (half ? w->wh_off : w->wb_off));
    if (tapmajor) wb = reinterpret_cast<const uint16_t*>(blob + m.rbcl_w_off[i][j]) +
                       (int64_t)(2 * d + e) * resblock_cl_bf16_units(w->cin, w->k) * 512;
    if (tappair) wb = reinterpret_cast<const uint16_t*>(blob + m.rb16_w_off[i][j]) + (int64_t)(2 * d + e) * rb16_units(w->k) * 512;
    if (w_out)
      for (int co = 0; co < w->cout; ++co)
        for (int ci = 0; ci < w->cin; ++ci)
          for (int jj = 0; jj < w->k; ++jj) {
            int64_t idx = cl_w_index(jj, ci, co, w->cin, w->k);
            if (tappair) idx = rb16_w_index(jj, ci, co);
            if (tapmajor) {                           // unit (group s, tap jj) sits at jj*G + s instead of s*k + jj
              const int G = w->cin / 16, sg = ci / 16;
              idx = ((int64_t)jj * G + sg) * 512 + idx % 512;
            }
            float f;
            if (half) {
              f = h2f(wb[idx]);
            } else {
              const uint32_t u = (uint32_t)wb[idx] << 16;
              std::memcpy(&f, &u, 4);
            }
            w_out[((size_t)co * w->cin + ci) * w->k + jj] = f;
          }
    if (bias_out)
      for (int co = 0; co < w->cout; ++co)
        bias_out[co] = tappair ? blob[m.rb16_b_off[i][j] + (2 * d + e) * 16 + co] : (w->b_off >= 0 ? blob[w->b_off + co] : 0.f);
    return 0;
  } catch (...) { return -100; }
}

int bv2_test_attention(void* stream, const float* qkv, int ld, const float* mask, const float* erv, float* out,
                       int B, int H, int D, int T, int W) {
  return bv2_test_attention_q(stream, qkv, ld, mask, erv, out, B, H, D, T, W, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                              0, 0, 1, nullptr, 0);
}

int bv2_test_attention_f16(void* stream, const float* qkv, int ld, const float* mask, const float* erv, float* out,
                           int B, int H, int D, int T, int W) {
  return bv2_test_attention_q(stream, qkv, ld, mask, erv, out, B, H, D, T, W, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                              0, 0, 1, nullptr, 0);
}

int bv2_test_layernorm(void* stream, const float* a, const float* add, int mode, const float* dww, const float* dwb, int dil,
                       const float* in_mask, const float* gamma, const float* beta, int post_gelu, const float* res,
                       const float* vec, const float* mask, float* out, int B, int C, int T, int nslab, int64_t slab_stride) {
  return bv2_test_layernorm_ex(stream, a, add, mode, dww, dwb, dil, in_mask, gamma, beta, post_gelu, res, vec, mask, out, B, C, T, nslab,
                               slab_stride, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 0);
}

// ---- the Encoder layer's fused launch forms (tests/test_encoder_forms_gpu.py): the three launchers above with every field of the
// fused forms exposed.  Status of the kernel launchers is passed through unchanged.
int bv2_test_attention_ex(void* stream, const float* qkv, int ld, const float* mask, const float* erv, float* out, int B, int H, int D,
                          int T, int W, int f16, const void* kh, const void* vh, const float* wo_host, float* wo_pack_dev,
                          const float* bo, const float* res, float* o_out, int64_t o_slab_stride, int Co, int ksplit, float* ml_out) {
  return bv2_test_attention_q(stream, qkv, ld, mask, erv, out, B, H, D, T, W, f16, kh, vh, wo_host, wo_pack_dev, bo, res, o_out, o_slab_stride,
                              Co, ksplit, ml_out, 0);
}

int bv2_test_attention_pick_qtile(int B, int H, int T, int D, int ksplit, int f16) {
  return attention_pick_qtile(B, H, T, D, ksplit, f16 != 0);
}

int bv2_test_attention_q(void* stream, const float* qkv, int ld, const float* mask, const float* erv, float* out, int B, int H, int D,
                         int T, int W, int f16, const void* kh, const void* vh, const float* wo_host, float* wo_pack_dev,
                         const float* bo, const float* res, float* o_out, int64_t o_slab_stride, int Co, int ksplit, float* ml_out, int qtile) {
  try {
    AttnArgs a;
    a.qtile = qtile;
    a.qkv = qkv; a.ld = ld; a.mask = mask; a.erv = erv; a.out = out; a.B = B; a.H = H; a.D = D; a.T = T; a.W = W; a.f16 = f16;
    a.kh = static_cast<const uint16_t*>(kh); a.vh = static_cast<const uint16_t*>(vh);
    if (wo_host) {
      if (!wo_pack_dev || Co < 1 || H < 1 || D < 1) return -1;
      const int cin = H * D, cin_pad = round_up(cin, 16);
      std::vector<float> pk((size_t)round_up(Co, 32) * cin_pad, 0.f);        // rows padded to whole 32-row tiles (zero)
      pack_f32(pk.data(), cin, Co, 1, t_dense(wo_host, cin, 1));
      if (hipMemcpy(wo_pack_dev, pk.data(), sizeof(float) * pk.size(), hipMemcpyHostToDevice) != hipSuccess) return -6;
      a.wo = wo_pack_dev; a.wo_groups = cin_pad / 8;
    }
    a.bo = bo; a.res = res; a.o_out = o_out; a.o_slab_stride = o_slab_stride; a.Co = Co;
    a.ksplit = ksplit; a.ml_out = ml_out; a.no_head = g_test_no_head;
    return launch_attention(static_cast<hipStream_t>(stream), a);
  } catch (...) { return -100; }
}

int bv2_test_layernorm_ex(void* stream, const float* a, const float* add, int mode, const float* dww, const float* dwb, int dil,
                          const float* in_mask, const float* gamma, const float* beta, int post_gelu, const float* res,
                          const float* vec, const float* mask, float* out, int B, int C, int T, int nslab, int64_t slab_stride,
                          const float* ml, int ml_H, int ml_ks, const float* bias, float* out2, const float* vec2,
                          const void* pf_ptr, unsigned pf_bytes) {
  LnArgs l;
  std::memset(&l, 0, sizeof(l));
  l.a = a; l.add = add; l.nslab = nslab; l.slab_stride = slab_stride; l.mode = mode; l.dww = dww; l.dwb = dwb; l.dil = dil; l.in_mask = in_mask;
  l.gamma = gamma; l.beta = beta; l.eps = 1e-5f; l.post_gelu = post_gelu; l.res = res; l.vec = vec; l.vec_bstride = C;
  l.mask = mask; l.out = out; l.B = B; l.C = C; l.T = T;
  l.ml = ml; l.ml_H = ml_H; l.ml_ks = ml_ks; l.bias = bias;
  l.out2 = out2; l.vec2 = vec2; l.vec2_bstride = C;
  l.pf = Prefetch{pf_ptr, pf_bytes}; l.no_head = g_test_no_head;
  return launch_layernorm(static_cast<hipStream_t>(stream), l);
}

int bv2_test_conv_f16_ex(void* stream, const void* x, int in_ct, const float* in_mask, const float* w_host, const float* bias_host,
                         void* wpack_dev, void* out, int out_ct, const float* res, int res_mode, const float* out_mask, int mask_pre,
                         int mask_post, int act, int B, int cin, int cout, int k, int dil, int L, int out_rstride,
                         const float* ln_gamma, const float* ln_beta, const float* ln_vec, const float* ln_mask, void* k16, void* v16,
                         int kv_row0, int kv_rows, int k16_ld, const float* bias2, int bias2_bstride, int no_ksplit,
                         const float* p1_w_host, const float* p1_bias_host, void* p1_out, const float* p1_res, int p1_res_mode) {
  try {
    if (!conv_f16_supported(cin, cout, k, dil, !out_ct)) return -2;
    const int cout_pad = round_up(cout, 32);
    const int64_t ne = cl_w_elems(cin, cout_pad, k);
    const int64_t one = bv2_test_conv_cl_pack_bytes(cin, cout, k);          // problem i's weights + bias at wpack_dev + i * one
    HcLaunch hl;
    std::memset(&hl, 0, sizeof(hl));
    hl.nprob = p1_w_host ? 2 : 1;
    const float* ws[2] = {w_host, p1_w_host};
    const float* bs[2] = {bias_host, p1_bias_host};
    for (int i = 0; i < hl.nprob; ++i) {
      char* base = static_cast<char*>(wpack_dev) + (size_t)i * one;
      // w_host == NULL (problem 0 only): wpack_dev already holds the packed weight (timing loops)
      if (ws[i] && !t_upload_cl(base, true, cin, cout, k, t_dense(ws[i], cin, k), t_bias(bs[i]))) return -6;
      HcProb& p = hl.p[i];
      p.x = x; p.in_ct = in_ct; p.x_bstride = (int64_t)cin * L; p.x_rstride = L; p.Lin = L;
      p.in_mask = in_mask; p.in_mask_bstride = L;
      p.w = reinterpret_cast<const uint16_t*>(base);
      p.bias = bs[i] ? reinterpret_cast<const float*>(base + ne * 2) : nullptr;
      p.out_ct = out_ct;
      p.out_rstride = out_ct ? (out_rstride > 0 ? out_rstride : L) : 0;
      p.out_bstride = out_ct ? (int64_t)cout * p.out_rstride : (int64_t)(act == ACT_GATE ? cout / 2 : cout) * L;
      p.res_bstride = p.out_bstride;
      p.out_mask = out_mask; p.out_mask_bstride = L; p.mask_pre = mask_pre; p.mask_post = mask_post; p.act = act;
      p.cin = cin; p.cout = cout; p.cout_pad = cout_pad; p.k = k; p.dil = dil; p.pad_left = ((k - 1) / 2) * dil;
    }
    HcProb& p = hl.p[0];
    p.out = out; p.res = res; p.res_mode = res_mode;
    p.bias2 = bias2; p.bias2_bstride = bias2_bstride;
    p.ln_gamma = ln_gamma; p.ln_beta = ln_beta; p.ln_eps = 1e-5f; p.ln_vec = ln_vec; p.ln_vec_bstride = cout; p.ln_mask = ln_mask;
    p.k16 = static_cast<uint16_t*>(k16); p.v16 = static_cast<uint16_t*>(v16); p.kv_row0 = kv_row0; p.kv_rows = kv_rows; p.k16_ld = k16_ld;
    if (hl.nprob == 2) { hl.p[1].out = p1_out; hl.p[1].res = p1_res; hl.p[1].res_mode = p1_res_mode; }
    hl.B = B; hl.L = L; hl.no_ksplit = no_ksplit;
    return launch_conv_f16(static_cast<hipStream_t>(stream), hl, nullptr);
  } catch (...) { return -100; }
}

// ---- the BERT / DeBERTa-v2 feature extractor's own kernels (tests/test_bert_kernels_gpu.py): the launchers of kernels/deberta_attn.hip
// and kernels/bert.hip, status passed through unchanged
int bv2_test_deberta_attn(void* stream, const float* qkv, int ld, const float* mask, const float* pk, const float* pq, const float* tab,
                          float* out, int B, int H, int D, int T, int P, int span) {
  DebertaAttnArgs a;
  a.qkv = qkv; a.ld = ld; a.mask = mask; a.pk = pk; a.pq = pq; a.tab = tab; a.out = out;
  a.B = B; a.H = H; a.D = D; a.T = T; a.P = P; a.span = span;
  return launch_deberta_attn(static_cast<hipStream_t>(stream), a);
}

int bv2_test_bert_ln(void* stream, const float* a, int nslab, int64_t slab_stride, const float* gamma, const float* beta, float eps,
                     const float* mask, float* out, int B, int C, int T, const void* pf_ptr, unsigned pf_bytes) {
  BertLnArgs l;
  l.a = a; l.nslab = nslab; l.slab_stride = slab_stride; l.gamma = gamma; l.beta = beta; l.eps = eps; l.mask = mask; l.out = out;
  l.B = B; l.C = C; l.T = T;
  l.pf = Prefetch{pf_ptr, pf_bytes};
  return launch_bert_ln(static_cast<hipStream_t>(stream), l);
}

int bv2_test_bert_embed_ln(void* stream, const int64_t* input_ids, const int64_t* token_type_ids, const float* word, const float* pos,
                           const float* type, const int64_t* lengths, const float* gamma, const float* beta, float eps, float* out,
                           int B, int S, int C, int vocab, int max_pos, int type_vocab, const void* pf_ptr, unsigned pf_bytes) {
  BertEmbedArgs e;
  e.input_ids = input_ids; e.token_type_ids = token_type_ids; e.word = word; e.pos = pos; e.type = type; e.lengths = lengths;
  e.gamma = gamma; e.beta = beta; e.eps = eps; e.out = out;
  e.B = B; e.S = S; e.C = C; e.vocab = vocab; e.max_pos = max_pos; e.type_vocab = type_vocab;
  e.pf = Prefetch{pf_ptr, pf_bytes};
  return launch_bert_embed_ln(static_cast<hipStream_t>(stream), e);
}

void bv2_test_conv_timeline(void* dev_buf, long long capacity_u64) {
  conv_set_timeline(static_cast<unsigned long long*>(dev_buf), capacity_u64);
}
int bv2_test_conv_timeline_report(long long* meta, int max_launches) { return conv_timeline_report(meta, max_launches); }

void bv2_test_set_tuning(int splitk_waves, int force_ck, long tile_target) { conv_set_tuning(splitk_waves, force_ck, tile_target); }
int bv2_test_splitk_stage(void) { return conv_last_splitk_stage(); }
int bv2_test_splitk_waves(void) { return conv_last_splitk_waves(); }
void bv2_test_set_x6_tuning(int t256, int t128, int t64, int ck) { conv_x6_set_tuning(t256, t128, t64, ck); }
void bv2_test_x6_occupancy(int* out4) { conv_x6_occupancy(out4); }
void bv2_test_set_variants(const char* cl_spec, int cl_generic, int hc_generic) {
  conv_cl_set_tuning(cl_spec, cl_generic);
  conv_f16_set_tuning(hc_generic);
}

int64_t bv2_test_dds_pack_floats(int C) {
  // [dww 3C][dwb C][g1 C][b1 C][g2 C][b2 C][pre_w C][pre_b C] + conv pack (1x1 C->C) + post conv pack (1x1 C->C rows max)
  return 10 * (int64_t)C + 2 * bv2_test_conv_pack_floats(C, C, 1);
}

int bv2_test_dds_layer(void* stream, const float* x, const float* pre_w_host, const float* pre_b_host, const float* z, int z_src,
                       const float* g, const float* mask, const float* dww_host, const float* dwb_host, const float* g1_host,
                       const float* b1_host, const float* g2_host, const float* b2_host, const float* w_host,
                       const float* bias_host, float* out, int dil, int last_mask, const float* post_w_host,
                       const float* post_b_host, int post_cout, float* post_out, float* zio, int z_dst, float* wpack_dev,
                       int B, int C, int T) {
  try {
    const int64_t one = bv2_test_conv_pack_floats(C, C, 1);
    std::vector<float> pk((size_t)bv2_test_dds_pack_floats(C), 0.f);
    size_t o = 0;
    auto put = [&](const float* src, size_t n) { size_t at = o; if (src) std::memcpy(&pk[o], src, n * sizeof(float)); o += n; return at; };
    const size_t o_dww = put(dww_host, 3 * (size_t)C), o_dwb = put(dwb_host, C), o_g1 = put(g1_host, C), o_b1 = put(b1_host, C),
                 o_g2 = put(g2_host, C), o_b2 = put(b2_host, C), o_pw = put(pre_w_host, C), o_pb = put(pre_b_host, C);
    const size_t o_w = o, boff = (size_t)conv_w_floats(conv_desc(C, C, 1));   // both convs keep their bias boff behind their weights
    t_pack_conv(&pk[o_w], w_host, bias_host, C, C, 1, false);
    const size_t o_p = o_w + (size_t)one;
    if (post_w_host) {
      pack_f32(&pk[o_p], C, post_cout, 1, t_dense(post_w_host, C, 1));
      if (post_b_host) pack_bias(&pk[o_p + boff], post_cout, t_bias(post_b_host));
    }
    if (hipMemcpy(wpack_dev, pk.data(), sizeof(float) * pk.size(), hipMemcpyHostToDevice) != hipSuccess) return -6;
    DdsArgs a;
    std::memset(&a, 0, sizeof(a));
    a.x = x;
    if (pre_w_host) { a.pre_w = wpack_dev + o_pw; a.pre_b = wpack_dev + o_pb; a.z = z; a.z_src = z_src; a.g = g; a.x = nullptr; }
    a.mask = mask; a.dww = wpack_dev + o_dww; a.dwb = wpack_dev + o_dwb; a.g1 = wpack_dev + o_g1; a.b1 = wpack_dev + o_b1;
    a.g2 = wpack_dev + o_g2; a.b2 = wpack_dev + o_b2; a.w = wpack_dev + o_w; a.bias = wpack_dev + o_w + boff;
    a.out = out; a.dil = dil; a.last_mask = last_mask; a.eps = 1e-5f;
    if (post_w_host) {
      a.post_w = wpack_dev + o_p; a.post_b = wpack_dev + o_p + boff; a.post_cout = post_cout; a.post_cout_pad = round_up(post_cout, 32);
      a.post_out = post_out; a.zio = zio; a.z_src = z_src; a.z_dst = z_dst; a.sqrt_fc = std::sqrt((float)C); a.tail = 5.0f;
    }
    a.B = B; a.C = C; a.T = T;
    return launch_dds_layer(static_cast<hipStream_t>(stream), a);
  } catch (...) { return -100; }
}

// ---- the Generator's stage glue: ConvTranspose1d, multi-problem conv launches, conv_post (tests/test_generator_glue_*.py)
// dense weights of the polyphase split from the ConvTranspose1d weight w [cin][cout][k]: phase ph's conv [cout][cin][ntaps] and the
// channels-last union-window conv [u * cout][cin][cl_k], through UpsGeom's tap maps like the packer (bv2_model.cpp)
static void t_ups_phase_dense(const UpsGeom& G, int ph, int cin, int cout, const float* w, float* out) {
  for (int co = 0; co < cout; ++co)
    for (int ci = 0; ci < cin; ++ci)
      for (int j = 0; j < G.ntaps; ++j) out[((size_t)co * cin + ci) * G.ntaps + j] = w[((size_t)ci * cout + co) * G.k + G.tap(ph, j)];
}
static void t_ups_cl_dense(const UpsGeom& G, int cin, int cout, const float* w, float* out) {
  for (int cop = 0; cop < G.u * cout; ++cop)
    for (int ci = 0; ci < cin; ++ci)
      for (int jw = 0; jw < G.cl_k; ++jw) {
        const int tap = G.cl_tap(cop / cout, jw);
        out[((size_t)cop * cin + ci) * G.cl_k + jw] = tap < 0 ? 0.f : w[((size_t)ci * cout + cop % cout) * G.k + tap];
      }
}
static int64_t t_region(int cin, int cout, int k) { return (bv2_test_conv_pack_floats(cin, cout, k) + 63) / 64 * 64; }

int bv2_test_ups_split(int u, int k, int cin, int cout, const float* w, float* phase_w, int32_t* pad_left, float* cl_w, int32_t* cl_dims,
                       int32_t* cl_offs) {
  UpsGeom G;
  if (!ups_geometry(u, k, G)) return -2;
  if (cin < 1 || cout < 1) return -1;
  for (int ph = 0; ph < u; ++ph) {
    if (pad_left) pad_left[ph] = G.pad_left[ph];
    if (cl_offs) cl_offs[ph] = G.cl_off[ph];
    if (w && phase_w) t_ups_phase_dense(G, ph, cin, cout, w, phase_w + (size_t)ph * cout * cin * G.ntaps);
  }
  if (cl_dims) { cl_dims[0] = G.cl_pad_left; cl_dims[1] = G.cl_k; }
  if (w && cl_w) t_ups_cl_dense(G, cin, cout, w, cl_w);
  return 0;
}

int64_t bv2_test_conv_multi_pack_floats(int cin, int cout, const int32_t* k, int nprob) {
  int64_t n = 0;
  for (int i = 0; i < nprob; ++i) n += t_region(cin, cout, k[i]);
  return n;
}
int bv2_test_conv_multi(void* stream, const bv2_test_conv_prob* probs, int nprob, int cin, int cout, const float* x0, const float* x1,
                        const float* x2, int nsrc, float in_scale, float lrelu_slope, const int64_t* lens, int len_mul, int B, int L,
                        int tile, int ksplit, int64_t slab_stride, const float* out_mask, unsigned* omax, float* wpack_dev, int32_t* info) {
  try {
    if (!probs || nprob < 1 || nprob > BV2_MAX_PROBS || nsrc < 1 || nsrc > 3) return -2;
    if (tile == TILE_SPLITK && nsrc != 1) return -2;             // the split-K kernel reads x[0] only
    const bool x6 = tile >= TILE_X6 && cin % 32 == 0;
    const bool x3 = tile == TILE_X3 && x6;                       // every problem reads max |x| from a slot of its own region, filled here
    if (x3 && nsrc != 1) return -2;
    ConvLaunch cl;
    std::memset(&cl, 0, sizeof(cl));
    int64_t off = 0;
    for (int i = 0; i < nprob; ++i) {
      const bv2_test_conv_prob& q = probs[i];
      if (!q.w_host || q.k < 1 || q.dil < 1 || !q.out) return -2;
      std::vector<float> pk((size_t)t_region(cin, cout, q.k), 0.f);
      t_pack_conv(pk.data(), q.w_host, q.bias_host, cin, cout, q.k, x6, x3);
      if (hipMemcpy(wpack_dev + off, pk.data(), sizeof(float) * pk.size(), hipMemcpyHostToDevice) != hipSuccess) return -6;
      const ConvW w = t_conv_w(off, cin, cout, q.k, q.bias_host != nullptr, x6);
      ConvProb p = conv_prob(w, wpack_dev, x0, q.out, L, q.dil);
      p.x[1] = x1; p.x[2] = x2; p.nsrc = nsrc; p.in_scale = in_scale;
      if (x6) p.w6 = reinterpret_cast<const uint16_t*>(wpack_dev + w.wx_off);
      if (x3) {
        float* reg = wpack_dev + off + t_x3_off(cin, cout, q.k);
        if (launch_absmax(static_cast<hipStream_t>(stream), x0, (int64_t)B * cin * L, reinterpret_cast<unsigned*>(reg))) return -6;
        p.xmax = reinterpret_cast<const unsigned*>(reg);
        p.w3inv = reg + 2 * X3_SLOT_WORDS; p.w3 = reinterpret_cast<const uint16_t*>(reg + 2 * X3_SLOT_WORDS + X3_HDR_FLOATS);
      }
      if (q.pad_left >= 0) p.pad_left = q.pad_left;
      p.out_rstride = q.out_rstride; p.out_bstride = (int64_t)cout * q.out_rstride; p.out_tstride = q.out_tstride; p.out_toff = q.out_toff;
      p.res = q.res; p.res_bstride = p.out_bstride; p.res_mode = q.res_mode;
      p.out_mask = out_mask; p.mask_post = out_mask ? 1 : 0;
      p.pre_act = lrelu_slope != 0.f ? PRE_LRELU : PRE_NONE; p.slope = lrelu_slope;
      p.omax = omax;
      cl.p[i] = p;
      off += t_region(cin, cout, q.k);
    }
    cl.nprob = nprob; cl.B = B; cl.L = L; cl.lens = lens; cl.len_mul = len_mul < 1 ? 1 : len_mul;
    cl.ksplit = ksplit >= 1 ? ksplit : conv_pick_ksplit(cl, BV2_MAX_KSPLIT);      // ksplit 0: the split the executor would take (Ctx::conv)
    cl.slab_stride = slab_stride; cl.no_head = g_test_no_head;
    const char* vn = nullptr;
    const int rc = launch_conv1d(static_cast<hipStream_t>(stream), cl, tile, &vn);
    if (info) { info[0] = conv_last_placement(); info[1] = cl.ksplit; }
    return rc;
  } catch (...) { return -100; }
}

int64_t bv2_test_conv_transpose_pack_floats(int u, int k, int cin, int cout) {
  UpsGeom G;
  return ups_geometry(u, k, G) ? (int64_t)u * t_region(cin, cout, G.ntaps) : -2;
}
int bv2_test_conv_transpose(void* stream, const float* w_host, const float* bias_host, int u, int k, int cin, int cout, const float* x0,
                            const float* x1, const float* x2, int nsrc, float* out, const int64_t* lens, int len_mul, int B, int L,
                            int tile, int only_phase, unsigned* omax, float* wpack_dev, int32_t* info) {
  try {
    UpsGeom G;
    if (!ups_geometry(u, k, G) || !w_host || nsrc < 1 || nsrc > 3 || only_phase >= u || tile >= TILE_X6) return -2;
    UpW U;
    U.u = u; U.k = k; U.cin = cin; U.cout = cout; U.ntaps = G.ntaps; U.cl_pad_left = G.cl_pad_left;
    const int64_t one = t_region(cin, cout, G.ntaps);
    std::vector<float> pk((size_t)(u * one), 0.f), dense((size_t)cout * cin * G.ntaps);
    for (int ph = 0; ph < u; ++ph) {
      t_ups_phase_dense(G, ph, cin, cout, w_host, dense.data());
      t_pack_conv(pk.data() + ph * one, dense.data(), bias_host, cin, cout, G.ntaps, false);
      U.phase[ph] = t_conv_w(ph * one, cin, cout, G.ntaps, bias_host != nullptr, false);
      U.pad_left[ph] = G.pad_left[ph];
    }
    if (hipMemcpy(wpack_dev, pk.data(), sizeof(float) * pk.size(), hipMemcpyHostToDevice) != hipSuccess) return -6;
    const float* src[3] = {x0, nsrc > 1 ? x1 : nullptr, nsrc > 2 ? x2 : nullptr};
    ConvLaunch cl = ups_conv_launch(U, wpack_dev, src, nsrc, out, B, L, lens, len_mul < 1 ? 1 : len_mul, omax);
    if (only_phase >= 0) { cl.p[0] = cl.p[only_phase]; cl.nprob = 1; }
    const char* vn = nullptr;
    const int rc = launch_conv1d(static_cast<hipStream_t>(stream), cl, tile, &vn);
    if (info) { info[0] = conv_last_placement(); info[1] = cl.ksplit; }
    return rc;
  } catch (...) { return -100; }
}

int64_t bv2_test_conv_transpose_cl_pack_bytes(int u, int k, int cin, int cout) {
  UpsGeom G;
  if (!ups_geometry(u, k, G) || cin % 16) return -2;
  return bv2_test_conv_cl_pack_bytes(cin, u * cout, G.cl_k);
}
int bv2_test_conv_transpose_cl(void* stream, const float* w_host, const float* bias_host, int u, int k, int cin, int cout, const void* x0,
                               const void* x1, const void* x2, int nsrc, void* out, const int64_t* lens, int len_mul, int B, int L,
                               int phase_taps, void* wpack_dev) {
  try {
    UpsGeom G;
    if (!ups_geometry(u, k, G) || !w_host || !bias_host || nsrc < 1 || nsrc > 3) return -2;
    if (!conv_cl_bf16_supported(cin, u * cout, G.cl_k, 1)) return -2;
    std::vector<float> dense((size_t)u * cout * cin * G.cl_k);
    t_ups_cl_dense(G, cin, cout, w_host, dense.data());
    if (!t_upload_cl(wpack_dev, false, cin, u * cout, G.cl_k, t_dense(dense.data(), cin, G.cl_k), [&](int co) { return bias_host[co % cout]; }))
      return -6;
    UpW U;
    U.u = u; U.k = k; U.cin = cin; U.cout = cout; U.ntaps = G.ntaps; U.cl_pad_left = G.cl_pad_left;
    for (int ph = 0; ph < u; ++ph) U.pad_left[ph] = G.pad_left[ph];
    U.cl = conv_cl_desc(cin, u * cout, G.cl_k);
    U.cl.wb_off = 0; U.cl.b_off = cl_w_elems(cin, U.cl.cout_pad, G.cl_k) / 2;   // float offsets from wpack_dev, which plays the blob
    const uint16_t* src[3] = {static_cast<const uint16_t*>(x0), nsrc > 1 ? static_cast<const uint16_t*>(x1) : nullptr,
                              nsrc > 2 ? static_cast<const uint16_t*>(x2) : nullptr};
    const ClLaunch cl = ups_cl_launch(U, static_cast<const float*>(wpack_dev), src, nsrc, static_cast<uint16_t*>(out), B, L, lens,
                                      len_mul < 1 ? 1 : len_mul, phase_taps != 0);
    if (phase_taps && !cl.p[0].ph_cout) return -2;               // the restriction was asked for and does not fit its nibbles
    return launch_conv_cl_bf16(static_cast<hipStream_t>(stream), cl, nullptr);
  } catch (...) { return -100; }
}

int bv2_test_conv_post(void* stream, const float* x0, const float* x1, const float* x2, int nsrc, const float* w_host, float* w_dev,
                       float* out, const int64_t* lens, int len_mul, int B, int C, int k, int L) {
  if (!w_host || !w_dev || nsrc < 1 || nsrc > 3 || C < 1 || k < 1) return -2;
  if (hipMemcpy(w_dev, w_host, sizeof(float) * (size_t)C * k, hipMemcpyHostToDevice) != hipSuccess) return -6;
  const float* src[3] = {x0, nsrc > 1 ? x1 : nullptr, nsrc > 2 ? x2 : nullptr};
  return launch_conv_post(static_cast<hipStream_t>(stream), conv_post_args(src, nsrc, w_dev, out, C, k, B, L, lens, len_mul < 1 ? 1 : len_mul));
}
int bv2_test_conv_post_cl(void* stream, const void* x0, const void* x1, const void* x2, int nsrc, const float* w_host, float* w_dev,
                          float* out, const int64_t* lens, int len_mul, int B, int C, int k, int L, int generic) {
  if (!w_host || !w_dev || nsrc < 1 || nsrc > 3 || C < 1 || k < 1) return -2;
  if (hipMemcpy(w_dev, w_host, sizeof(float) * (size_t)C * k, hipMemcpyHostToDevice) != hipSuccess) return -6;
  const uint16_t* src[3] = {static_cast<const uint16_t*>(x0), nsrc > 1 ? static_cast<const uint16_t*>(x1) : nullptr,
                            nsrc > 2 ? static_cast<const uint16_t*>(x2) : nullptr};
  return launch_conv_post_cl(static_cast<hipStream_t>(stream),
                             conv_post_cl_args(src, nsrc, w_dev, out, C, k, B, L, lens, len_mul < 1 ? 1 : len_mul, generic != 0));
}

// ---- the fp32 WN layer's two launches as run_wn builds them (tests/test_wn_forms_*.py)
int bv2_test_wn_gate_row(int hid, int n) { return wn_gate_row(hid, n); }
int64_t bv2_test_wn_in_pack_floats(int B, int H) { return t_region(H, 2 * H, kFlowKernel) + (int64_t)B * 2 * H; }
int bv2_test_wn_in_layer(void* stream, const float* x, const float* w_host, const float* bias_host, const float* gl_host, float* acts,
                         float* wpack_dev, int B, int H, int L, int tile) {
  try {
    if (!x || !w_host || !bias_host || !gl_host || !acts || !wpack_dev || B < 1 || H < 16 || H % 16 || L < 1 || tile >= TILE_X6) return -2;
    const int k = kFlowKernel;
    const int64_t one = t_region(H, 2 * H, k);
    const std::function<int(int)> gate_row = [H](int n) { return wn_gate_row(H, n); };
    std::vector<float> pk((size_t)bv2_test_wn_in_pack_floats(B, H), 0.f);
    t_pack_conv(pk.data(), w_host, bias_host, H, 2 * H, k, false, false, &gate_row);
    for (int b = 0; b < B; ++b)                    // the layer's cond_layer slice: the same rows (Packer::gemv with pack_wn's cond_row)
      for (int n = 0; n < 2 * H; ++n) pk[(size_t)one + (size_t)b * 2 * H + n] = gl_host[(size_t)b * 2 * H + gate_row(n)];
    if (hipMemcpy(wpack_dev, pk.data(), sizeof(float) * pk.size(), hipMemcpyHostToDevice) != hipSuccess) return -6;
    ConvLaunch cl{};
    cl.p[0] = wn_in_prob(t_conv_w(0, H, 2 * H, k, true, false), wpack_dev, x, acts, wpack_dev + one, 2 * H, L);
    cl.nprob = 1; cl.B = B; cl.L = L; cl.ksplit = 1; cl.no_head = g_test_no_head;
    const char* vn = nullptr;
    return launch_conv1d(static_cast<hipStream_t>(stream), cl, tile, &vn);
  } catch (...) { return -100; }
}
int64_t bv2_test_wn_res_skip_pack_floats(int H) { return 2 * t_region(H, H, 1); }
int bv2_test_wn_res_skip(void* stream, const float* acts, const float* w_host, const float* bias_host, float* x, float* outacc,
                         const float* mask, float* wpack_dev, int B, int H, int L, int tile, int first, int last) {
  try {
    if (!acts || !w_host || !bias_host || !x || !outacc || !mask || !wpack_dev || B < 1 || H < 1 || L < 1 || tile >= TILE_X6) return -2;
    // as pack_wn: rows [0,H) the x update, rows [H,2H) the skip rows, two convs of H rows; the last layer's H rows are all skip rows
    const int64_t one = t_region(H, H, 1);
    std::vector<float> pk((size_t)(2 * one), 0.f);
    if (!last) t_pack_conv(pk.data(), w_host, bias_host, H, H, 1, false);
    t_pack_conv(pk.data() + one, w_host + (last ? 0 : (size_t)H * H), bias_host + (last ? 0 : H), H, H, 1, false);
    if (hipMemcpy(wpack_dev, pk.data(), sizeof(float) * pk.size(), hipMemcpyHostToDevice) != hipSuccess) return -6;
    const ConvW res = t_conv_w(0, H, H, 1, true, false), skip = t_conv_w(one, H, H, 1, true, false);
    ConvLaunch cl = wn_res_skip_launch(last ? nullptr : &res, skip, first != 0, wpack_dev, acts, x, outacc, mask, B, L);
    cl.ksplit = 1; cl.slab_stride = 0; cl.no_head = g_test_no_head;
    const char* vn = nullptr;
    return launch_conv1d(static_cast<hipStream_t>(stream), cl, tile, &vn);
  } catch (...) { return -100; }
}

int bv2_test_spline(void* stream, float* z, int src, int dst, const float* params, int prow, const float* mask,
                    float sqrt_fc, float tail, int B, int T) {
  return launch_spline(static_cast<hipStream_t>(stream), z, src, dst, params, prow, mask, sqrt_fc, tail, B, T);
}
int bv2_test_spline_forward(void* stream, const float* x, const float* uw, const float* uh, const float* ud, float tail, long long N,
                            float* y, float* logabsdet) {
  return launch_spline_forward(static_cast<hipStream_t>(stream), x, uw, uh, ud, tail, N, y, logabsdet);
}


// kernels/rng.h on the host
void bv2_test_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  const Philox4 w = philox4x32_10(Philox4{ctr[0], ctr[1], ctr[2], ctr[3]}, key[0], key[1]);
  out[0] = w.x; out[1] = w.y; out[2] = w.z; out[3] = w.w;
}
float bv2_test_seeded_normal(int64_t seed, int which, int row, int t) { return seeded_normal(seed, which, row, t); }

}  // extern "C"
