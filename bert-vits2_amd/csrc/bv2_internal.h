// bv2_internal.h — host-side model description (packed-weight layout), handle, and executor interfaces of libbv2.so.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/bv2.h"
#include "bv2_kernels.h"

namespace bv2 {

constexpr int kAttnWindow = 4;       // reference attentions.py:46
constexpr int kCondLayer = 2;        // reference attentions.py:69-71
constexpr int kSdpLayers = 3;        // DDSConv n_layers, reference models.py:171-173
constexpr int kSdpKernel = 3;
constexpr int kSdpBins = 10;
constexpr int kSdpFlowsUsed = 3;     // ConvFlows applied at inference (the 4th is the dropped "useless vflow")
constexpr int kDpFilter = 256;       // reference models.py:929-931
constexpr int kDpKernel = 3;
constexpr int kFlowKernel = 5;       // reference models.py:903-924
constexpr int kMaxLayers = 16;
constexpr int kMaxFlows = 8;
constexpr uint32_t kBlobMagic = 0x32765642u;  // "BVv2"
constexpr int kBlobHeaderFloats = 64;

// ---- packed-weight descriptors: offsets are in floats from the start of the blob ----
struct ConvW {
  int cin = 0, cin_pad = 0, cout = 0, cout_pad = 0, w_ld = 0, k = 1;
  int64_t w_off = -1, b_off = -1;    // b_off < 0: no bias
  int64_t wb_off = -1;               // Generator convs only: bf16 fragment stream (cl_w_index), offset in floats
  int64_t wh_off = -1;               // flow Encoder convs only: fp16 fragment stream (cl_w_index), offset in floats
  int64_t wx_off = -1;               // wide Generator ResBlock convs only: three bf16 planes (x6_w_index), offset in floats
  int64_t wy_off = -1;               // fp32 Generator ResBlock convs with x6 planes: 1 / S_w, then (X3_HDR_FLOATS in) two fp16 planes (x3_w_index)
};
struct VecW { int64_t off = -1; int64_t n = 0; };
struct GemvW { int cout = 0, cin = 0; int64_t w_off = -1, b_off = -1; };

struct EncLayerW {
  ConvW qkv, o, ffn1, ffn2;
  VecW erv, g1, b1, g2, b2;
};
struct EncoderW {
  int n_layers = 0, ksize = 1, hidden = 0, filter = 0, heads = 0;
  GemvW spk;
  EncLayerW layer[kMaxLayers];
};
struct DDSLayerW { VecW dww, dwb; ConvW c1x1; VecW g1, b1, g2, b2; int dil = 1; };
struct DDSW { DDSLayerW l[kSdpLayers]; };
struct ConvFlowW { VecW pre_w, pre_b; DDSW convs; ConvW proj; };

// modules.WN (modules.py:160-210), the stack of the residual flow's couplings and of the posterior encoder
struct WnW {
  GemvW cond;                        // cond_layer: 2 * hidden * layers rows, each layer's slice in the gate order of `in`
  ConvW in[kMaxLayers];              // rows in gate order (ACT_GATE): per 32-row tile 16 tanh rows then their 16 sigmoid rows
  ConvW res[kMaxLayers], skip[kMaxLayers];   // res_skip_layers split into its x-update rows and its output rows
  int layers = 0;
};

struct CouplingW {
  bool flipped = false;              // channel Flip folded into pre/post weight permutations
  ConvW pre, post;
  EncoderW enc;                      // transformer flow
  WnW wn;                            // residual (WN) flow
};

struct UpW {
  int u = 1, k = 1, cin = 0, cout = 0, ntaps = 1;
  ConvW phase[BV2_MAX_UPS];          // one conv problem per output phase (polyphase ConvTranspose1d)
  int pad_left[BV2_MAX_UPS];
  // channels-last form (bf16 path): ONE conv cin -> u*cout over the union of the phases' tap windows (zero weights where
  // a phase does not use a tap); row t of its output is rows t*u .. t*u+u-1 of the upsampled tensor
  ConvW cl;
  int cl_pad_left = 0;
};

// Polyphase geometry of ConvTranspose1d(stride u, kernel k, padding (k - u) / 2), said once for the packer (bv2_model.cpp), the executors
// (bv2_exec.cpp) and the tests' entry points (bv2_testing.cpp).  Output n = u*s + ph gathers x[s + shift - mtap] * W[ci][co][pp + u*mtap]
// (SURVEY.md §7.3 K2): phase ph is a stride-1 conv of ntaps = k / u taps with pad_left = ntaps - 1 - shift whose tap j reads W[..][tap(ph, j)].
// Channels-last form: ONE conv over the union of the phases' tap windows, cl_k = cl_pad_left + max right reach + 1 taps, in which phase ph
// owns the window taps [cl_off, cl_off + ntaps), cl_off = cl_pad_left - pad_left[ph] (the other taps of its rows are zero).
struct UpsGeom {
  int u = 1, k = 1, ntaps = 1, pad = 0;
  int pp[BV2_MAX_UPS], shift[BV2_MAX_UPS], pad_left[BV2_MAX_UPS];
  int cl_pad_left = 0, cl_k = 1, cl_off[BV2_MAX_UPS];
  // index into the k taps of the ConvTranspose1d weight: tap j of phase ph / window tap jw of phase ph (-1: a zero of the window)
  int tap(int ph, int j) const { return pp[ph] + u * (ntaps - 1 - j); }
  int cl_tap(int ph, int jw) const { const int j = jw - cl_off[ph]; return j < 0 || j >= ntaps ? -1 : tap(ph, j); }
  // ClProb::ph_offs: nibble ph = cl_off[ph]; false when a phase or an offset does not fit a nibble
  bool ph_offs(unsigned long long* out) const {
    unsigned long long offs = 0;
    bool fits = u <= 16;
    for (int ph = 0; ph < u && fits; ++ph) {
      fits = cl_off[ph] >= 0 && cl_off[ph] <= 15;
      offs |= (unsigned long long)(cl_off[ph] & 15) << (4 * ph);
    }
    if (fits) *out = offs;
    return fits;
  }
};
// false outside the envelope (bv2_model.cpp validate_config: u = 2..8, k = 1..4 x u, (k - u) even)
inline bool ups_geometry(int u, int k, UpsGeom& g) {
  if (u < 2 || u > BV2_MAX_UPS || k < u || k % u || (k - u) % 2 || k / u > 4) return false;
  g.u = u; g.k = k; g.ntaps = k / u; g.pad = (k - u) / 2;
  int plmax = 0, right = 0;
  for (int ph = 0; ph < u; ++ph) {
    g.pp[ph] = (ph + g.pad) % u; g.shift[ph] = (ph + g.pad) / u;
    g.pad_left[ph] = (g.ntaps - 1) - g.shift[ph];
    plmax = g.pad_left[ph] > plmax ? g.pad_left[ph] : plmax;
    const int r = g.ntaps - 1 - g.pad_left[ph];
    right = r > right ? r : right;
  }
  g.cl_pad_left = plmax; g.cl_k = plmax + right + 1;
  for (int ph = 0; ph < u; ++ph) g.cl_off[ph] = plmax - g.pad_left[ph];
  return true;
}

// ReferenceEncoder (n_speakers == 0 only; kernels/ref_enc.hip)
struct RefEncW {
  bool present = false;
  VecW cw[6], cb[6];                 // conv 1 [9][32], convs 2-6 [Cout/8][Cin][9][8] (weight-norm folded); biases
  VecW w_ih, b_ih, w_hh, b_hh;       // GRU(128 * W6 -> 128), PyTorch's layout and gate order (r, z, n)
  VecW pw, pb;                       // proj [gin][128]
};

// PosteriorEncoder enc_q (reference models.py:448-487): its own, optional blob — the inference blob does not carry it
constexpr uint32_t kPosteriorMagic = 0x71765642u;  // "BVvq"
constexpr int kPosteriorLayers = 16;               // modules.WN(hidden, 5, 1, 16): = kMaxLayers
struct PosteriorW {
  int spec = 0;                      // spec_channels: pre's input rows (odd widths ride on cin_pad, rows >= cin read as zero)
  ConvW pre;                         // Conv1d(spec -> hidden, 1)
  WnW wn;                            // enc: kPosteriorLayers layers
  ConvW proj_m, proj_logs;           // proj (hidden -> 2 inter, 1) split into its halves
};

// What the StochasticDurationPredictor needs in its FORWARD direction and the inference blob does not hold (models.py:176-187, 206-244):
// post_pre / post_convs / post_proj / post_flows and the ConvFlow sdp.flows.1 that inference drops — a third, optional blob
constexpr uint32_t kSdpForwardMagic = 0x66765642u;  // "BVvf"
constexpr int kSdpFlows = 4;                        // ConvFlows per side (models.py:155, 183)
struct SdpForwardW {
  VecW post_pre_w, post_pre_b;       // Conv1d(1 -> C, k = 1)
  DDSW post_convs;
  ConvW post_proj;
  VecW post_ea_m, post_ea_logs;      // post_flows.0
  ConvFlowW post_cf[kSdpFlows];      // post_flows.1, .3, .5, .7 in forward order
  ConvFlowW cf_first;                // flows.1; flows.3 / .5 / .7 are Model::cf[2] / [1] / [0] of the inference blob
};

struct Model {
  bv2_config cfg;
  bool flow_flip_first = false;      // odd number of couplings: the reverse pass starts with a real channel Flip of z (bv2_model.cpp)
  // enc_p
  VecW emb, tone_emb, lang_emb;
  ConvW bert[3];
  EncoderW enc;
  ConvW proj_m, proj_logs;
  // durations
  ConvW sdp_pre, sdp_proj;
  GemvW sdp_cond;
  DDSW sdp_convs;
  ConvFlowW cf[kSdpFlowsUsed];       // application order: flows.7, flows.5, flows.3
  VecW ea_m, ea_logs;
  GemvW dp_cond;
  ConvW dp_c1, dp_c2, dp_proj;
  VecW dp_g1, dp_b1, dp_g2, dp_b2;
  VecW emb_g;                        // absent (off -1) when n_speakers == 0
  RefEncW ref_enc;
  // flow: application order (reverse pass): a = 0 is reference flows.{2(n-1)}
  int n_coupling = 0;
  CouplingW coupling[kMaxFlows];
  // dec
  ConvW conv_pre;
  GemvW dec_cond;
  int n_ups = 0, n_rbk = 0, n_rbd = 0;
  int rb_type = 1;                   // 1 = ResBlock1 ((dilated conv, conv) pairs), 2 = ResBlock2 (one conv per dilation: rb[..][d][0] only)
  UpW ups[BV2_MAX_UPS];
  ConvW rb[BV2_MAX_UPS][BV2_MAX_RESBLOCK_KERNELS][BV2_MAX_RESBLOCK_DILATIONS][2];
  // whole-ResBlock bf16 streams of the narrow stages (kernels/resblock_cl_bf16.hip); -1 where the stage is too wide
  int64_t rbcl_w_off[BV2_MAX_UPS][BV2_MAX_RESBLOCK_KERNELS];
  int64_t rbcl_b_off[BV2_MAX_UPS][BV2_MAX_RESBLOCK_KERNELS];
  // the C = 16 stage once more in the tap-pair layout of kernels/resblock_c16_bf16.hip (rb16_w_index); -1 elsewhere
  int64_t rb16_w_off[BV2_MAX_UPS][BV2_MAX_RESBLOCK_KERNELS];
  int64_t rb16_b_off[BV2_MAX_UPS][BV2_MAX_RESBLOCK_KERNELS];
  VecW conv_post;
  int post_c = 0, post_k = 7;
  int total_up = 1;
};

// ---- shared by the two host executors (bv2_exec.cpp, bv2_bert.cpp) ----
// a caller's workspace carved in 256-byte steps; base == nullptr: sizes only
struct Arena {
  char* base;
  int64_t off = 0, cap;
  Arena(void* b, int64_t c) : base(static_cast<char*>(b)), cap(c) {}
  template <class T> T* get(int64_t n) {
    const int64_t bytes = (n * (int64_t)sizeof(T) + 255) / 256 * 256;
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += bytes;
    return p;
  }
  bool ok() const { return base == nullptr || off <= cap; }
};

// conv problem with the defaults of a "same"-padded Conv1d on a dense [B,C,L] tensor (an offset < 0 is a null pointer)
inline ConvProb conv_prob(const ConvW& w, const float* blob, const float* x, float* out, int L, int dil = 1) {
  ConvProb p;
  std::memset(&p, 0, sizeof(p));
  p.x[0] = x; p.nsrc = 1; p.in_scale = 1.f;
  p.x_bstride = (int64_t)w.cin * L; p.x_rstride = L; p.Lin = L;
  p.in_mask_bstride = L; p.out_mask_bstride = L;
  p.w = w.w_off < 0 ? nullptr : blob + w.w_off; p.bias = w.b_off < 0 ? nullptr : blob + w.b_off;
  p.out = out; p.out_bstride = (int64_t)w.cout * L; p.out_rstride = L; p.out_tstride = 1; p.out_toff = 0;
  p.res_bstride = p.out_bstride;
  p.cin = w.cin; p.cin_pad = w.cin_pad; p.cout = w.cout; p.cout_pad = w.cout_pad; p.w_ld = w.w_ld;
  p.k = w.k; p.dil = dil; p.pad_left = ((w.k - 1) / 2) * dil;
  p.slope = 0.1f;
  return p;
}
// the same for the bf16 channels-last path (kernels/gen_bf16.hip): x / out [B][L][C]
inline ClProb cl_prob(const ConvW& w, const float* blob, const uint16_t* x, uint16_t* out, int L, int dil = 1) {
  ClProb p;
  std::memset(&p, 0, sizeof(p));
  p.x[0] = x; p.nsrc = 1; p.in_scale = 1.f; p.x_bstride = (int64_t)w.cin * L; p.Lin = L;
  p.w = w.wb_off < 0 ? nullptr : reinterpret_cast<const uint16_t*>(blob + w.wb_off); p.bias = w.b_off < 0 ? nullptr : blob + w.b_off;
  p.out = out; p.out_bstride = (int64_t)w.cout * L; p.res_bstride = p.out_bstride;
  p.cin = w.cin; p.cout = w.cout; p.cout_pad = w.cout_pad; p.k = w.k; p.dil = dil; p.pad_left = ((w.k - 1) / 2) * dil;
  p.slope = 0.1f;
  return p;
}
// the packed fp32 stream of a conv (m-tile-major: what the split-K kernel's XCDs read in contiguous eighths) as the prefetch target of the
// launch before it (bv2_kernels.h Prefetch); nothing when `on` is false or there is no such conv
inline Prefetch weight_prefetch(const ConvW* w, const float* blob, bool on) {
  if (!on || !w || w->w_off < 0) return Prefetch{nullptr, 0};
  return Prefetch{blob + w->w_off, (unsigned)((int64_t)(w->cout_pad / 32) * (w->cin_pad / 8) * w->k * 1024)};
}

struct HostTensor { std::vector<float> data; std::vector<int64_t> shape; };

// A packed weight blob as the handle holds it, whatever it packs: the host tensors its load call took, its length and config hash once its
// layout is built (total_floats == 0: not yet), the attached device copy.  The typed descriptor of its contents (Model, PosteriorW,
// SdpForwardW) stands beside it on the handle.
struct WeightBlob {
  std::map<std::string, HostTensor> tensors;
  const float* dev = nullptr;
  int64_t total_floats = 0;
  uint32_t cfg_hash = 0;
};
// ... and what tells the three kinds apart: the two header numbers (bv2_pack.h write_blob_header), the keys it takes, its name in messages
enum BlobKind { kInference = 0, kPosterior, kSdpForward, kBlobKinds };
struct BlobDesc {
  uint32_t magic, layout;
  bool (*mine)(const std::string& key);
  const char* noun;
};
bool inference_key(const std::string& key);                        // everything but the other two kinds' (training-only) tensors
bool posterior_key(const std::string& key);                        // enc_q.*
bool sdp_forward_key(const std::string& key);                      // sdp.post_* and sdp.flows.1.*
constexpr BlobDesc kBlobDesc[kBlobKinds] = {
    {kBlobMagic, BV2_PACK_LAYOUT, inference_key, "inference"},
    {kPosteriorMagic, BV2_POSTERIOR_LAYOUT, posterior_key, "posterior encoder"},
    {kSdpForwardMagic, BV2_SDP_FORWARD_LAYOUT, sdp_forward_key, "forward duration predictor"},
};

struct ProfileRec { hipEvent_t e0, e1; int fam; double flops, bytes; };

struct Tap { float* dst; int64_t cap; };

}  // namespace bv2

struct bv2_handle {
  bv2::Model model;                  // laid out by bv2_create
  bv2::PosteriorW post;              // laid out once spec_channels is known (bv2_posterior_*), again when it changes
  bv2::SdpForwardW sdpf;             // laid out on first use (bv2_sdp_forward_*)
  bv2::WeightBlob blob[bv2::kBlobKinds];
  std::string err;
  std::map<std::string, bv2::Tap> taps;
  int gen_dtype = BV2_F32;           // Generator arithmetic: BV2_F32 (conv_mfma.hip) or BV2_BF16 (gen_bf16.hip)
  int flow_dtype = BV2_F32;          // transformer-flow Encoder convs: BV2_F32 (conv_mfma.hip) or BV2_F16 (enc_f16.hip)
  // bv2_set_option switches (tests compare the fused kernels with the layer-wise ones)
  bool no_conv_x6 = false;           // "conv_x6" = 0: wide Generator convs on the fp32 matrix core (conv_mfma.hip) instead of the bf16x6 form
  bool no_conv_x3 = false;           // "conv_x3" = 0: the wide fp32 Generator convs on the three-plane bf16 form (six products) instead of the two-plane fp16 form
  bool x6_narrow = true;             // "conv_x6_c32" = 0: the C = 32 stage on the fused fp32 pair kernel instead of layer-wise on conv_x6.hip
  bool no_fused_resblock = false;    // "fused_resblock" = 0: narrow Generator stages layer by layer
  int prefetch = 0;                  // "prefetch": bit 0 LayerNorm launches, bit 1 split-K launches carry the next launch's weight stream (batch 1); measured: nothing at config 2 (profiles/r05_ab_prefetch_c2.txt), off
  bool no_xcd_affine = false;        // "xcd_affine" = 0: plain grids for the fp16 Encoder stacks (default: batch item b on XCD b % 8 when B >= 8 && (B % 8 == 0 || B >= 32), Ctx::xcd_affine)
  bool no_f16_fused_ln = false;      // "f16_fused_ln" = 0: LayerNorm-1 / the plain LayerNorm-2s of the fp16 Encoder stacks as launches of their own instead of in conv_o's / conv_2's epilogue
  int f16_wn = 0, f16_ni = 0;        // "f16_wn" / "f16_ni": tile tuning of the fp16 Encoder convs (HcLaunch wn_pref / ni_pref); 0 = the launcher's choice
  bool no_f16_kv = false;            // "f16_kv" = 0: the fp16 Encoder stacks' q/k/v projection writes K and V as fp32 rows and the attention kernel rounds them in registers
  bool no_f16_ksplit = false;        // "f16_ksplit" = 0: the fp16 FFN conv_2 (768 -> 192 rows, 64-column tiles) as 6 waves over three staged chunks instead of 12 waves on K halves of one tile
  bool no_conv_post_rows = false;    // "conv_post_rows" = 0: the bf16 path's conv_post + tanh on the any-width kernel also at C = 16 (default: the row-wise kernel, gen_bf16.hip)
  bool no_ups_phase_taps = false;    // "ups_phase_taps" = 0: the bf16 ConvTranspose1d launches multiply through the zero taps of the union window (A/B and bit-identity tests)
  bool no_stage_sum = true;          // "stage_sum" = 1: the launch that finishes a bf16 Generator stage writes ONE tensor, the branch mean (default 0: the n branch tensors are handed over and
  // the next launch forms the mean).  Measured round 6 (profiles/r06_ab_stage_sum.txt, r06_fam_stage_sum.txt, B = 32): the consumers gain 228 us per step (four
  // ConvTranspose1d launches read 1/3 of the bytes), the producers lose 346 us — a workgroup that runs three branches back to back lives 3x as long (tail rounds of
  // a 416-workgroup grid, no k = 11 / k = 3 tiles side by side on a CU any more), every branch pays the widest branch's halo, the running sum is re-read through L2:
  // 14.65 vs 14.66-14.72 ms at config 3, 15.7-15.9 vs 15.6 at config 5.  Bit-identical either way (tests/test_stage_sum_gpu.py).
  bool no_resblock_c16 = false;      // "resblock_c16" = 0: the C = 16 bf16 stage on the 32x32x16 whole-ResBlock kernel (resblock_cl_bf16.hip) instead of resblock_c16_bf16.hip
  bool no_respair_c32 = false;       // "respair_c32" = 0: the C = 32 bf16 stage as whole-ResBlock launches (resblock_cl_bf16.hip) instead of pair by pair
  int respair_form = 1;              // "respair_form": 1 = 64 x 128 wave tiles (respair2_cl_bf16_kernel), 0 = 32-channel waves
  bool respair_problem_major = false; // "respair_mix" = 0: the pair kernel's branches dispatched one after the other (A/B only)
  bool x6_pair_c128 = false;         // "x6_pair_c128" = 1: the pair kernel also on the C = 128 stage (one 8-wave workgroup per CU; measured, see DESIGN)
  bool no_x6_pair_c16 = false;       // "x6_pair_c16" = 0: the C = 16 stage on the fused fp32-MFMA pair kernel (resblock_fused.hip)
  bool no_x6_pair_c64 = false;       // "x6_pair_c64" = 0: the pair kernel on the C = 32 stage only
  bool no_x6_pair = false;           // "x6_pair" = 0: the C = 32 fp32 stage as two conv_x6 launches per ResBlock pair instead of one respair_x6 launch
  bool no_fused_boundary = false;    // "fused_boundary" = 0: LayerNorm-2, post and the next pre of the transformer flow as three launches
  bool no_fused_respair = false;     // "fused_respair" = 0: the wide bf16 Generator stages one conv per launch (gen_bf16.hip) instead of one pair per launch
  bool no_fused_attn_o = false;      // "fused_attn_o" = 0: conv_o as its own launch after the attention kernel
  int attn_ksplit = -1;              // "attn_ksplit": key ranges per (head, query tile) of the fused attention; -1 = picked per shape, 0 / 1 = off
  bool no_kernarg_head = false;      // "kernarg_head" = 0: the split-K conv, LayerNorm, fp32 attention and flow boundary launches take their generic kernels (bv2_kernels.h SkHead)
  int attn_qtile = 0;                // "attn_qtile": queries per workgroup of the fp32 attention; 0 = picked per shape (attention_pick_qtile), 16, 32
  bool no_fused_dds = false;         // "fused_dds" = 0: DDSConv layers as 3 launches each
  bool no_overlap_dp = true;         // "overlap_dp" = 1: the (independent) DurationPredictor on an internal side stream, forked from and
  // joined back into the caller's stream with events (created on first use; capturable).  OFF by default: measured on MI355X at
  // batch 1 the fork/join costs more than the 5 short launches it hides (4.70 -> 4.82 ms per step eager, 4.75 -> 4.78 replayed).
  bool no_lean_durations = false;    // "lean_durations" = 0: both duration predictors always run (default: at a host-known sdp_ratio of exactly 0 or 1 the one
  // whose term is multiplied by 0.0f is not launched, run_encode)
  bool no_phase_b_front = false;     // "phase_b_front" = 0: the head of phase B as five launches (frame_index, expand, attn_path, gemv, x3 slots) instead of one
  // bv2_set_noise_seeds: [B] device int64, read by the kernels when a call runs (null: off, every call takes its noise tensors)
  const int64_t* seeds = nullptr;
  int seeds_B = 0;
  hipStream_t side_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // profiling
  bool prof_on = false;
  int prof_mode = 1;                 // 1: every MFMA kernel launch, 2: Generator (dec.*) launches only, 3: per site, 4: dec.ups per site
  std::vector<bv2::ProfileRec> prof_pool;
  size_t prof_used = 0;
  std::vector<std::string> prof_names;
};

namespace bv2 {

// bv2_model.cpp
// first pass: every descriptor, b.total_floats and b.cfg_hash; on an error nothing is touched
int build_layout(Model& m, WeightBlob& b, std::string& err);
int build_posterior_layout(const bv2_config& cfg, int spec_channels, PosteriorW& w, WeightBlob& b, std::string& err);
int build_sdp_forward_layout(const bv2_config& cfg, SdpForwardW& w, WeightBlob& b, std::string& err);
// second pass: b.tensors into `blob` (b.total_floats floats), header included
int pack_blob(const Model& m, const WeightBlob& b, float* blob, std::string& err);
int pack_posterior_blob(const bv2_config& cfg, const PosteriorW& w, const WeightBlob& b, float* blob, std::string& err);
int pack_sdp_forward_blob(const bv2_config& cfg, const SdpForwardW& w, const WeightBlob& b, float* blob, std::string& err);

// bv2_exec.cpp
// active seeds (bv2_set_noise_seeds) against a call's batch and its noise pointer: non-zero with h->err set on a mismatch
int check_seeds(bv2_handle* h, int B, const void* noise, const char* what, const char* noise_name);
int64_t workspace_bytes(const Model& m, int B, int T, int Ty);
// ic: per-utterance controls (may be null: the scalars of in); a null member keeps that scalar
// g_in: a caller's speaker vectors [B][gin] (null: emb_g(in.sid)); copied to out.g
int run_encode(bv2_handle* h, hipStream_t s, const bv2_encode_in& in, const bv2_encode_out& out, void* ws, int64_t wsb,
               const bv2_item_controls* ic = nullptr, const float* g_in = nullptr);
int run_ref_encode(bv2_handle* h, hipStream_t s, const float* y, const int64_t* strides, const int64_t* y_lengths, int B, int L,
                   float* g_out, void* ws, int64_t wsb);
int run_decode(bv2_handle* h, hipStream_t s, const bv2_decode_in& in, const bv2_decode_out& out, void* ws, int64_t wsb,
               const bv2_item_controls* ic = nullptr);
int run_flow(bv2_handle* h, hipStream_t s, int B, int Ty, const float* z_p, const int64_t* y_lengths, const float* y_mask,
             const float* g, float* z, void* ws, int64_t wsb, bool forward = false);   // forward: z -> z_p (SynthesizerTrn.forward)
int64_t posterior_workspace_bytes(const Model& m, int B, int Ty);
// enc_q(y, y_lengths, g) (models.py:479-487): y [B][spec][Ty] dense; noise_q null = z = m * mask
int run_posterior_encode(bv2_handle* h, hipStream_t s, int B, int Ty, const float* y, const int64_t* y_lengths, const float* g,
                         const float* noise_q, float noise_scale_q, float* z, float* m_q, float* logs_q, float* y_mask, void* ws, int64_t wsb);
int run_stage_emb_g(bv2_handle* h, hipStream_t s, int B, const int64_t* sid, float* g);
int run_stage_enc_p(bv2_handle* h, hipStream_t s, int B, int T, const int64_t* x, const int64_t* tone, const int64_t* lang,
                    const float* b0, const float* b1, const float* b2, const float* g, const int64_t* x_lengths, float* xout,
                    float* m_p, float* logs_p, float* x_mask, void* ws, int64_t wsb);
int run_stage_sdp(bv2_handle* h, hipStream_t s, int B, int T, const float* x, const float* x_mask, const float* zin,
                  const float* g, float* logw, void* ws, int64_t wsb);
int run_stage_dp(bv2_handle* h, hipStream_t s, int B, int T, const float* x, const float* x_mask, const float* g, float* logw,
                 void* ws, int64_t wsb);
// sdp(x, x_mask, w, g) forward (models.py:206-244): nll_sym [B][T], nll [B]; noise_e [B][2][T] or null with the handle's seeds
int64_t duration_nll_workspace_bytes(const Model& m, int B, int T);
int run_duration_nll(bv2_handle* h, hipStream_t s, int B, int T, const float* x, const float* x_mask, const float* w, const float* g,
                     const float* noise_e, float* nll_sym, float* nll, void* ws, int64_t wsb);
int run_generator(bv2_handle* h, hipStream_t s, int B, int Ty, int L, const float* z, const int64_t* y_lengths,
                  const float* g, float* o, void* ws, int64_t wsb);
// The Generator's ConvTranspose1d launches, built in one place for the executors and for the tests' entry points (bv2_testing.cpp): x =
// ConvTranspose1d(lrelu_0.1(mean of the nsrc sources)) on Lc input columns, `up` samples per latent frame at the input's resolution.
// fp32: U.u polyphase problems of one ConvLaunch writing [B][cout][Lc * u] (omax: the shared max |out| slot or null; ksplit is the caller's).
ConvLaunch ups_conv_launch(const UpW& U, const float* blob, const float* const src[3], int nsrc, float* x, int B, int Lc,
                           const int64_t* lens, int up, unsigned* omax);
// bf16: one channels-last conv over the union tap window writing [B][Lc * u][cout]; phase_taps: each wave multiplies through its phases' taps only
ClLaunch ups_cl_launch(const UpW& U, const float* blob, const uint16_t* const src[3], int nsrc, uint16_t* x, int B, int Lc,
                       const int64_t* lens, int up, bool phase_taps);
// ... and its conv_post + tanh launches (slope 0.01: F.leaky_relu's default, models.py:553); generic: the any-width bf16 kernel also at C = 16
ConvPostArgs conv_post_args(const float* const src[3], int nsrc, const float* w, float* out, int C, int k, int B, int L,
                            const int64_t* lens, int len_mul);
ConvPostClArgs conv_post_cl_args(const uint16_t* const src[3], int nsrc, const float* w, float* out, int C, int k, int B, int L,
                                 const int64_t* lens, int len_mul, bool generic);
// The two launches of an fp32 WN layer (run_wn), built in one place for the executor and for the tests' entry points.  in_layer + g_l + gate:
// `in` has its 2H rows in gate order, gl is the layer's conditioning slice [B][gl_bstride] in the same order, acts gets H rows.
ConvProb wn_in_prob(const ConvW& in, const float* blob, const float* x, float* acts, const float* gl, int gl_bstride, int Ty);
// res_skip: x = (x + res(acts)) * mask in place and outacc (+)= skip(acts) as two problems; res == nullptr is the last layer, whose one
// problem is skip(acts) into outacc, masked.  first: outacc is written, not added to.  ksplit / slab_stride / no_head are the caller's.
ConvLaunch wn_res_skip_launch(const ConvW* res, const ConvW& skip, bool first, const float* blob, const float* acts, float* x, float* outacc,
                              const float* mask, int B, int Ty);
// streamed decode: the flow once (run_stream_begin), the Generator window by window (run_stream_chunk)
int generator_halo(const Model& m);
int64_t stream_plan_bytes(const Model& m, int B, int Ty, int window_frames);            // what a stream itself needs (without phase A)
int64_t stream_workspace_bytes(const Model& m, int B, int T, int Ty, int window_frames);
int run_stream_begin(bv2_handle* h, hipStream_t s, const bv2_decode_in& in, const bv2_decode_out& out, void* ws, int64_t wsb,
                     const bv2_item_controls* ic = nullptr);
int run_stream_chunk(bv2_handle* h, hipStream_t s, const bv2_stream_chunk_args& a, void* ws, int64_t wsb);

}  // namespace bv2
