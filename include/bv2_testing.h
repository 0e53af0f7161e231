/*
 * bv2_testing.h — kernel-level entry points of libbv2.so used ONLY by tests/ and tools/: unit parity of single kernels and of single
 * launches the executors build (the Encoder layer's fused forms, the Generator's ConvTranspose1d / multi-problem / conv_post launches)
 * against torch fp32 and fp64 references, and the host-side packers and number formats on a CPU-only box.  Not part of the drop-in
 * boundary; synchronous where noted.
 */
#ifndef BV2_TESTING_H
#define BV2_TESTING_H
#include <stdint.h>
#include "bv2.h"
#ifdef __cplusplus
extern "C" {
#endif

/* floats of device scratch bv2_test_conv1d needs for the packed weight + bias */
int64_t bv2_test_conv_pack_floats(int cin, int cout, int k);

/* One conv1d problem through the MFMA implicit-GEMM kernels with a forced variant (0 = auto, 1..5 LDS-tiled kernel tile
 * shapes, 6 = split-K kernel; see bv2_kernels.h TILE_*).  With tile 6 and ksplit > 1 the output is `ksplit` partial
 * slabs, `slab_stride` floats apart, whose SUM is the result (bias / residual ride on slab 0).  w_host [cout][cin][k] / bias_host [cout] are HOST pointers (packed + uploaded
 * synchronously into wpack_dev); every other pointer is DEVICE.  x [B][cin][L], out/res [B][cout][L*out_tstride],
 * masks [B][L].  pad_left < 0 means "same" padding ((k-1)/2*dil).  `relu` is the activation code: 0 = none, 1 = ReLU, 2 = the WN gate
 * (ACT_GATE), 3 = exact erf GELU (ACT_GELU); any other value is refused with -1 before anything is packed or launched.  With the gate,
 * weight, bias and bias2 rows are taken as given, in gate order (rows [0,16) of every 32 the tanh rows, [16,32) the sigmoid rows of the
 * same 16 channels), and out has cout / 2 rows per item ([B][cout/2][L]).  The entry itself checks nothing about a gate launch: a K split,
 * a residual, a mask, cout % 32 != 0 or an x6 / x3 tile (>= 8) goes to launch_conv1d as asked, and the -1 that comes back is the
 * launcher's (bv2_kernels.h conv_gate_ok; the weights have been packed and uploaded by then, no conv kernel has run).  With w_host NULL
 * and cin % 32 != 0 the entry makes no device call of its own in front of the launcher's checks. */
int bv2_test_conv1d(void* stream, const float* x, const float* w_host, const float* bias_host, float* out, float* wpack_dev,
                    int B, int cin, int cout, int k, int dil, int pad_left, int L, int tile, float lrelu_slope, int relu,
                    const float* res, int res_mode, const float* in_mask, const float* out_mask, int mask_pre,
                    int mask_post, const float* bias2, int nsrc, const float* x1, const float* x2, float in_scale, int ksplit,
                    int64_t slab_stride);

/* tile 8 = the split-bf16 form of the LDS-tiled kernel with its own tile choice (kernels/conv_x6.hip; cin % 32 == 0, nsrc == 1),
 * 9 / 10 / 11 / 12 = its 128x64 / 128x64-with-loader-waves / 64x128 / 32x256 workgroup tiles forced. */

/* tile 14 = the two-plane fp16 form of the same kernel ("x3", bv2_kernels.h): tile 8's choice with the scaled fp16 planes, max |x|
 * reduced into a slot by a launch in front.  For cin % 32 == 0 and ksplit <= 1 EVERY tile also publishes max |out| (ConvProb::omax)
 * as fp32 bits in a slot (eight words, 32 floats apart: one per XCD — the value is their max) at float offset
 * bv2_test_x3_omax_off(cin, cout, k) of wpack_dev. */
int64_t bv2_test_x3_omax_off(int cin, int cout, int k);

/* v = h[0] + h[1] + h[2] exactly as bf16 bit patterns: the host-side split the packer applies to the x6 weight planes (host only) */
void bv2_test_x6_split(float v, uint16_t* h3);
/* the host number formats of the packer over an array of n elements (host only): kind 0 = fp32 -> bf16 bits, 1 = fp32 -> fp16 bits
 * (both round to nearest even), 2 = fp16 bits -> fp32.  Returns 0, or -1 for a bad argument. */
int bv2_test_convert(int kind, const void* in, void* out, int64_t n);
/* where the packed blob holds x6 weight planes: float offset / float count of every region ([unit][plane 3][64 lanes][8] uint16); returns
 * the number of regions (host only; layout is known after bv2_create) */
int bv2_test_x6_regions(const bv2_handle* h, int64_t* off_floats, int64_t* n_floats, int max_regions);
/* ... and its scaled fp16 planes of the x3 form, in the same conv order: a region = 64 floats (the first = 1 / S_w) followed by
 * [unit][plane 2][64 lanes][8] fp16 — unit / lane / element order as in the x6 region of the same conv */
int bv2_test_x3_regions(const bv2_handle* h, int64_t* off_floats, int64_t* n_floats, int max_regions);

/* fused ResBlock1 pair (kernels/resblock_fused.hip): out = x + conv2(lrelu(conv1(lrelu(x), k, dil) + b1), k, 1) + b2 on
 * [B][C][L]; w*_host [C][C][k], b*_host [C] are HOST pointers; wpack_dev needs 2 * bv2_test_conv_pack_floats(C, C, k) floats */
int bv2_test_resblock_fused(void* stream, const float* x, float* out, const float* w1_host, const float* b1_host,
                            const float* w2_host, const float* b2_host, float* wpack_dev, int B, int C, int k, int dil, int L,
                            float slope);

/* channels-last bf16 conv (kernels/gen_bf16.hip): x* / out / res are DEVICE bf16 [B][L][C] tensors, w_host [cout][cin][k]
 * and bias_host [cout] HOST fp32 (rounded to bf16 / kept fp32 by the packer); wpack_dev needs
 * bv2_test_conv_cl_pack_bytes(cin, cout, k) bytes; the nsrc sources are averaged; pad_left < 0 means "same" padding */
int64_t bv2_test_conv_cl_pack_bytes(int cin, int cout, int k);
int bv2_test_conv_cl_bf16(void* stream, const void* x0, const void* x1, const void* x2, int nsrc, const float* w_host,
                          const float* bias_host, void* wpack_dev, void* out, const void* res, const float* bias2, int B, int cin,
                          int cout, int k, int dil, int pad_left, int L, int pre_lrelu, float slope);

/* a WHOLE ResBlock1 (nd (dilated conv, conv) pairs with their residuals, reference modules.py:296-309) of a narrow Generator stage in one
 * launch, bf16 channels-last: x / out DEVICE bf16 [B][L][C] (out != x), w_host [nd][2][C][C][k] and bias_host [nd][2][C] HOST fp32 (index
 * [d][0] = convs1[d] with dilation dil[d], [d][1] = convs2[d]); variant 0 = kernels/resblock_cl_bf16.hip (v_mfma_f32_32x32x16_bf16, C = 16 /
 * 32), 1 = kernels/resblock_c16_bf16.hip (v_mfma_f32_16x16x32_bf16, C = 16); lens: optional DEVICE int64 [B] valid rows per item;
 * wpack_dev needs bv2_test_resblock_cl_pack_bytes(C, k, nd) bytes.  Returns -2 for an unsupported shape. */
int64_t bv2_test_resblock_cl_pack_bytes(int C, int k, int nd);
int bv2_test_resblock_cl(void* stream, const void* x, void* out, const float* w_host, const float* bias_host, void* wpack_dev, int B,
                         int C, int k, const int* dil, int nd, int L, float slope, int variant, const int64_t* lens);

/* ONE (dilated conv, conv) pair of ResBlock1 with its residual in one launch, bf16 channels-last (kernels/respair_cl_bf16.hip): x / out
 * DEVICE bf16 [B][L][C] (out != x), C = 32 / 64 / 128 / 256; w_host [2][C][C][k] (index 0 = the dilated conv), bias_host [2][C] HOST fp32;
 * form 1 = 64-channel x 128-row wave tiles on the swizzled tile (C >= 64), 0 = 32-channel waves on the padded tile; lens optional DEVICE
 * int64 [B]; wpack_dev needs bv2_test_respair_cl_pack_bytes(C, k) bytes */
int64_t bv2_test_respair_cl_pack_bytes(int C, int k);
int bv2_test_respair_cl(void* stream, const void* x, void* out, const float* w_host, const float* bias_host, void* wpack_dev, int B,
                        int C, int k, int dil, int L, float slope, int form, const int64_t* lens);
/* the same pair in fp32 with both convs on the bf16 matrix core from exact three-way splits (kernels/respair_x6.hip): x / out DEVICE fp32
 * [B][C][L], C = 16 / 32 / 64 / 128; the packer splits w_host into its three bf16 planes (x6_split) */
int64_t bv2_test_respair_x6_pack_bytes(int C, int k);
int bv2_test_respair_x6(void* stream, const float* x, float* out, const float* w_host, const float* bias_host, void* wpack_dev, int B,
                        int C, int k, int dil, int L, float slope, const int64_t* lens);
/* the same pair on the two-plane fp16 form ("x3": scaled fp16 halves, three products, per-workgroup activation scales); same arguments */
int bv2_test_respair_x3(void* stream, const float* x, float* out, const float* w_host, const float* bias_host, void* wpack_dev, int B,
                        int C, int k, int dil, int L, float slope, const int64_t* lens);
/* the flow's coupling boundary in one launch (kernels/flow_boundary.hip): h = LayerNorm_C(sum of nslab slabs a [B][C][T]) * mask;
 * x1 [C/2 rows][T] (inside z, z_bstride floats per item) = (x1 - post(h) - post_b) * mask in place; pre_out [B][C][T] = (pre(x1) + pre_b) *
 * mask unless pre_w_host is NULL.  post_w_host [C/2][C], pre_w_host [C][C/2] HOST fp32; every other pointer DEVICE; wpack_dev needs
 * bv2_test_flow_boundary_pack_floats(C) floats.  C = 192 only (-2 otherwise). */
int64_t bv2_test_flow_boundary_pack_floats(int C);
int bv2_test_flow_boundary(void* stream, const float* a, int nslab, int64_t slab_stride, const float* gamma, const float* beta,
                           const float* mask, float* x1, int64_t z_bstride, const float* post_w_host, const float* post_b_host,
                           const float* pre_w_host, const float* pre_b_host, float* pre_out, float* wpack_dev, int B, int C, int T);

/* fp16 Encoder conv (kernels/enc_f16.hip).  in_ct: x is DEVICE fp32 [B][cin][L] (in_mask [B][L] optional) else fp16 [B][L][cin];
 * out_ct: out is DEVICE fp32 [B][cout][out_rstride] (res like out, res_mode 0/1/2 = none/add/rsub) else fp16 [B][L][cout];
 * w_host [cout][cin][k], bias_host [cout] HOST fp32; wpack_dev needs bv2_test_conv_cl_pack_bytes(cin, cout, k) bytes;
 * "same" padding; act 1 = ReLU; out_mask [B][L] applied before (mask_pre) and/or after (mask_post) the residual op */
int bv2_test_conv_f16(void* stream, const void* x, int in_ct, const float* in_mask, const float* w_host, const float* bias_host,
                      void* wpack_dev, void* out, int out_ct, const float* res, int res_mode, const float* out_mask, int mask_pre,
                      int mask_post, int act, int B, int cin, int cout, int k, int dil, int L, int out_rstride);

/* Decode one Generator conv of a packed HOST blob back to dense form (checks the bf16 packer on a CPU-only box):
 * kind 0 = dec.conv_pre, 1 = dec.ups[i] in its channels-last single-conv form (C_out' = u*C_out), 2 = resblock conv
 * rb[i][j][d][e], 3 = fp16 stream of a transformer-flow Encoder conv (coupling i in application order, layer j, d = 0 fused
 * q/k/v(+relative-key rows) / 1 conv_o / 2 FFN conv_1 / 3 FFN conv_2), 4 = rb[i][j][d][e] read back from the tap-major
 * whole-ResBlock stream (must equal kind 2), 5 = rb[i][j][d][e] (C = 16 stage) read back from the tap-pair stream of
 * kernels/resblock_c16_bf16.hip, bias from its own bias block (must equal kind 2).  dims = {cin, cout, k, pad_left}; w_out [cout][cin][k] (bf16 values widened to fp32) and bias_out [cout]
 * may be NULL to query dims only.  Returns 0, or a negative status. */
int bv2_test_dump_cl_conv(bv2_handle* h, const void* host_blob, int kind, int i, int j, int d, int e, int32_t* dims,
                          float* w_out, float* bias_out);

/* windowed relative-position attention; qkv [B][3*H*D + H*(2W+1)][ld] (q rows pre-divided by sqrt(D); the last H*(2W+1)
 * rows are the relative-key logits q_i·Ek[r]/sqrt(D)), ld % 32 == 0, mask [B][T], erv [2W+1][D], out [B][H*D][T] (all DEVICE) */
int bv2_test_attention(void* stream, const float* qkv, int ld, const float* mask, const float* erv, float* out,
                       int B, int H, int D, int T, int W);
/* the same with QK^T / PV on the fp16 matrix core (bv2_set_flow_dtype(BV2_F16)) */
int bv2_test_attention_f16(void* stream, const float* qkv, int ld, const float* mask, const float* erv, float* out,
                       int B, int H, int D, int T, int W);

/* channel LayerNorm family (see bv2_kernels.h LnArgs); all DEVICE pointers, nullable where optional */
int bv2_test_layernorm(void* stream, const float* a, const float* add, int mode, const float* dww, const float* dwb, int dil,
                       const float* in_mask, const float* gamma, const float* beta, int post_gelu, const float* res,
                       const float* vec, const float* mask, float* out, int B, int C, int T, int nslab, int64_t slab_stride);

/* The Encoder layer's fused launch forms, one field of AttnArgs / LnArgs / HcProb per argument (bv2_kernels.h has their meaning); the
 * kernel launcher's status is returned unchanged (-1 = refused combination, nothing launched).
 *
 * bv2_test_attention_ex: bv2_test_attention plus f16 (0 / 1) and the fp16 K / V hand-over kh [B][ld][H*D] / vh [B][H*D][ld] (DEVICE fp16);
 * the fused conv_o wo_host [Co][H*D] (HOST, packed into wo_pack_dev: round_up(Co, 32) * round_up(H*D, 16) DEVICE floats; NULL = plain
 * output in `out`), bo [Co], res [B][Co][T], partial slabs o_out (slab s at o_out + s * o_slab_stride); the key split ksplit / ml_out
 * [B][H][ksplit][2][T]. */
int bv2_test_attention_ex(void* stream, const float* qkv, int ld, const float* mask, const float* erv, float* out, int B, int H, int D,
                          int T, int W, int f16, const void* kh, const void* vh, const float* wo_host, float* wo_pack_dev,
                          const float* bo, const float* res, float* o_out, int64_t o_slab_stride, int Co, int ksplit, float* ml_out);
/* bv2_test_attention_ex plus the queries per workgroup (AttnArgs::qtile: 0 = picked per shape, 16 — fp32 only — or 32; anything else is
 * refused), and the pick itself: a function of the shape and the dtype alone, no device needed. */
int bv2_test_attention_q(void* stream, const float* qkv, int ld, const float* mask, const float* erv, float* out, int B, int H, int D,
                         int T, int W, int f16, const void* kh, const void* vh, const float* wo_host, float* wo_pack_dev,
                         const float* bo, const float* res, float* o_out, int64_t o_slab_stride, int Co, int ksplit, float* ml_out, int qtile);
int bv2_test_attention_pick_qtile(int B, int H, int T, int D, int ksplit, int f16);
/* bv2_test_layernorm plus the weighted slabs of the key split (ml [B][ml_H][ml_ks][2][T], bias [C]), the second output out2 with vec2
 * [B][C], and the B == 1 weight prefetch (pf_ptr / pf_bytes: DEVICE memory that is only read) */
int bv2_test_layernorm_ex(void* stream, const float* a, const float* add, int mode, const float* dww, const float* dwb, int dil,
                          const float* in_mask, const float* gamma, const float* beta, int post_gelu, const float* res,
                          const float* vec, const float* mask, float* out, int B, int C, int T, int nslab, int64_t slab_stride,
                          const float* ml, int ml_H, int ml_ks, const float* bias, float* out2, const float* vec2,
                          const void* pf_ptr, unsigned pf_bytes);
/* bv2_test_conv_f16 plus: the LayerNorm epilogue (ln_gamma / ln_beta [cout], eps 1e-5, ln_vec [B][cout], ln_mask [B][L]; out may be res);
 * the K / V routing of the q/k/v projection (k16 [B][k16_ld][kv_rows], v16 [B][kv_rows][k16_ld] DEVICE fp16); the gate (act 2: out is fp16
 * [B][L][cout/2]) with its per-batch bias bias2 [B][bias2_bstride]; no_ksplit; and an optional second problem on the same input, masks
 * and activation (p1_w_host / p1_bias_host HOST, p1_out / p1_res DEVICE; p1_w_host NULL = one problem).  wpack_dev needs
 * bv2_test_conv_cl_pack_bytes(cin, cout, k) bytes per problem. */
int bv2_test_conv_f16_ex(void* stream, const void* x, int in_ct, const float* in_mask, const float* w_host, const float* bias_host,
                         void* wpack_dev, void* out, int out_ct, const float* res, int res_mode, const float* out_mask, int mask_pre,
                         int mask_post, int act, int B, int cin, int cout, int k, int dil, int L, int out_rstride,
                         const float* ln_gamma, const float* ln_beta, const float* ln_vec, const float* ln_mask, void* k16, void* v16,
                         int kv_row0, int kv_rows, int k16_ld, const float* bias2, int bias2_bstride, int no_ksplit,
                         const float* p1_w_host, const float* p1_bias_host, void* p1_out, const float* p1_res, int p1_res_mode);

/* ---- the BERT / DeBERTa-v2 feature extractor's own kernels (tests/test_bert_kernels_gpu.py); all DEVICE pointers, the launcher's status
 * returned unchanged (-1 = refused arguments, -2 = a shape the kernel cannot serve; both before any device call).
 *
 * DeBERTa-v2 disentangled attention (kernels/deberta_attn.hip, DebertaAttnArgs): qkv [B][3*H*D][ld] (q rows pre-divided by sqrt(3 D)),
 * mask [B][T], pk / pq [H][D][2*span] (pq pre-divided by sqrt(3 D)), tab [2*P - 1] floats, out [B][H*D][T]. */
int bv2_test_deberta_attn(void* stream, const float* qkv, int ld, const float* mask, const float* pk, const float* pq, const float* tab,
                          float* out, int B, int H, int D, int T, int P, int span);
/* out [B][C][T] = LayerNorm_C(sum of nslab slabs a, slab_stride floats apart; eps) * mask [B][T] (null: none) (kernels/bert.hip,
 * BertLnArgs); pf_ptr / pf_bytes: the B == 1 weight prefetch (DEVICE memory that is only read) */
int bv2_test_bert_ln(void* stream, const float* a, int nslab, int64_t slab_stride, const float* gamma, const float* beta, float eps,
                     const float* mask, float* out, int B, int C, int T, const void* pf_ptr, unsigned pf_bytes);
/* out [B][C][S] = LayerNorm_C(word[id] + type[tt] + pos[s]) (kernels/bert.hip, BertEmbedArgs): input_ids / token_type_ids (null: 0) int64
 * [B][S], word [vocab][C], pos [max_pos][C] and type [type_vocab][C] (either may be null), lengths null or int64 [B] (columns s >=
 * lengths[b] are zeroed) */
int bv2_test_bert_embed_ln(void* stream, const int64_t* input_ids, const int64_t* token_type_ids, const float* word, const float* pos,
                           const float* type, const int64_t* lengths, const float* gamma, const float* beta, float eps, float* out,
                           int B, int S, int C, int vocab, int max_pos, int type_vocab, const void* pf_ptr, unsigned pf_bytes);

/* one fused DDSConv layer (kernels/dds_fused.hip) on x [B][C][T] -> out [B][C][T] (out != x): depthwise k=3 conv (dww_host [C][3],
 * dwb_host [C], dilation dil) + LN1 (g1/b1) + GELU + 1x1 conv (w_host [C][C], bias_host [C]) + LN2 (g2/b2) + GELU + residual,
 * times mask when last_mask.  Optional ConvFlow.pre input transform: pre_w/pre_b HOST [C] with z [B][2][T], z_src and g [B][C][T]
 * (x is ignored then).  Optional post projection post_w_host [post_cout][C] / post_b_host [post_cout]: with post_out
 * [B][post_cout][T] it is written as (W y + b) * mask; with post_out NULL and zio [B][2][T] the 29 rows are the spline
 * parameters applied to zio (z_src / z_dst).  Host arrays are packed into wpack_dev (>= bv2_test_dds_pack_floats(C) floats). */
int64_t bv2_test_dds_pack_floats(int C);
int bv2_test_dds_layer(void* stream, const float* x, const float* pre_w_host, const float* pre_b_host, const float* z, int z_src,
                       const float* g, const float* mask, const float* dww_host, const float* dwb_host, const float* g1_host,
                       const float* b1_host, const float* g2_host, const float* b2_host, const float* w_host,
                       const float* bias_host, float* out, int dil, int last_mask, const float* post_w_host,
                       const float* post_b_host, int post_cout, float* post_out, float* zio, int z_dst, float* wpack_dev,
                       int B, int C, int T);

/* ---- the Generator's stage glue (tests/test_generator_glue_cpu.py, tests/test_generator_glue_fp64_gpu.py).  Conventions as above: HOST
 * weights, DEVICE tensors, packed synchronously into a caller-sized scratch, the launcher's status returned unchanged, -2 = unsupported.
 * lens: optional DEVICE int64 [B] (item b's input is valid on [0, lens[b] * len_mul)).  omax: optional DEVICE slot of 256 zeroed words,
 * 128-byte aligned (ConvProb::omax: max |out| as fp32 bits, one word per XCD 32 words apart — the value is their max).
 * info (optional, HOST int32 [2]) = {placement the launcher took: 0 plain grid / 1 per-XCD column ranges / 2 cost-sorted snake, ksplit}. */

/* The polyphase split of ConvTranspose1d(stride u, kernel k, padding (k - u) / 2) the packer applies to w [cin][cout][k] (host only): the
 * dense phase convs phase_w [u][cout][cin][k/u] with pad_left [u], and the dense channels-last window conv cl_w [u*cout][cin][kk] with
 * cl_dims = {cl_pad_left, kk} and each phase's window offset cl_offs [u].  Any output may be NULL (query cl_dims first: kk <= 7).
 * -2 outside the envelope ((k - u) odd, k % u != 0, k / u > 4, u < 2, u > 8). */
int bv2_test_ups_split(int u, int k, int cin, int cout, const float* w, float* phase_w, int32_t* pad_left, float* cl_w, int32_t* cl_dims,
                       int32_t* cl_offs);

/* One ConvLaunch of 1..8 problems on shared inputs x0 / x1 / x2 [B][cin][L] (nsrc of them are summed and scaled by in_scale, then
 * leaky-ReLU of lrelu_slope unless 0).  Problem i: w_host [cout][cin][k], bias_host [cout] or NULL, pad_left < 0 = "same"; element (b, co,
 * t) of its result goes to out[(b * cout + co) * out_rstride + t * out_tstride + out_toff]; res is indexed like out (res_mode 0 / 1 / 2 =
 * none / add / rsub).  out_mask [B][L] multiplies after the residual op.  tile as in bv2_test_conv1d (tiles >= 8 also pack the x6 planes, 14
 * the x3 planes with max |x0| reduced into each problem's slot; tile 6 with nsrc != 1 is refused); ksplit 0 = the split the executor would take (conv_pick_ksplit), slab s of a split at out +
 * s * slab_stride.  wpack_dev needs bv2_test_conv_multi_pack_floats(cin, cout, k[], nprob) floats. */
typedef struct bv2_test_conv_prob {
  const float* w_host; const float* bias_host;
  int32_t k, dil, pad_left;
  float* out; int32_t out_rstride, out_tstride, out_toff;
  const float* res; int32_t res_mode;
} bv2_test_conv_prob;
int64_t bv2_test_conv_multi_pack_floats(int cin, int cout, const int32_t* k, int nprob);
int bv2_test_conv_multi(void* stream, const bv2_test_conv_prob* probs, int nprob, int cin, int cout, const float* x0, const float* x1,
                        const float* x2, int nsrc, float in_scale, float lrelu_slope, const int64_t* lens, int len_mul, int B, int L,
                        int tile, int ksplit, int64_t slab_stride, const float* out_mask, unsigned* omax, float* wpack_dev, int32_t* info);

/* The fp32 Generator's ConvTranspose1d stage launch, built by the executor's own function (ups_conv_launch): out [B][cout][L * u] =
 * ConvTranspose1d(lrelu_0.1(mean of the nsrc sources [B][cin][L])), w_host [cin][cout][k], bias_host [cout] or NULL.  tile 0 = the
 * product's pick, 1..7 forced; only_phase >= 0 launches that phase alone (it writes out[.., t] with t % u == only_phase and nothing else).
 * wpack_dev needs bv2_test_conv_transpose_pack_floats(u, k, cin, cout) floats. */
int64_t bv2_test_conv_transpose_pack_floats(int u, int k, int cin, int cout);
int bv2_test_conv_transpose(void* stream, const float* w_host, const float* bias_host, int u, int k, int cin, int cout, const float* x0,
                            const float* x1, const float* x2, int nsrc, float* out, const int64_t* lens, int len_mul, int B, int L,
                            int tile, int only_phase, unsigned* omax, float* wpack_dev, int32_t* info);
/* ... and the bf16 path's (ups_cl_launch): sources / out DEVICE bf16 channels-last [B][L][cin] / [B][L * u][cout]; phase_taps 0 = the wave
 * multiplies through the zero taps of the union window (ClProb::ph_cout = 0).  wpack_dev needs bv2_test_conv_transpose_cl_pack_bytes bytes. */
int64_t bv2_test_conv_transpose_cl_pack_bytes(int u, int k, int cin, int cout);
int bv2_test_conv_transpose_cl(void* stream, const float* w_host, const float* bias_host, int u, int k, int cin, int cout, const void* x0,
                               const void* x1, const void* x2, int nsrc, void* out, const int64_t* lens, int len_mul, int B, int L,
                               int phase_taps, void* wpack_dev);

/* conv_post + tanh as the executors launch it (conv_post_args / conv_post_cl_args: leaky-ReLU slope 0.01): out [B][L] = tanh(conv1d(lrelu(
 * mean of the nsrc sources), w [C][k], "same" padding, no bias)); w_host HOST, uploaded into w_dev (C * k DEVICE floats).
 * fp32 (kernels/misc.hip): sources [B][C][L]. */
int bv2_test_conv_post(void* stream, const float* x0, const float* x1, const float* x2, int nsrc, const float* w_host, float* w_dev,
                       float* out, const int64_t* lens, int len_mul, int B, int C, int k, int L);
/* bf16 (kernels/gen_bf16.hip): sources DEVICE bf16 channels-last [B][L][C]; generic 1 = the any-width kernel also at C = 16, k = 7 */
int bv2_test_conv_post_cl(void* stream, const void* x0, const void* x1, const void* x2, int nsrc, const float* w_host, float* w_dev,
                          float* out, const int64_t* lens, int len_mul, int B, int C, int k, int L, int generic);

/* The fp32 WN layer's two launches, built by the executor's own functions (wn_in_prob / wn_res_skip_launch), from weights in the
 * REFERENCE's row order (tests/test_wn_forms_*.py).  H = hidden channels (a multiple of 16), k = 5, tile 0 = the product's pick, 1..7 forced.
 * bv2_test_wn_gate_row (host only): the source row of packed row n of an in_layer / a layer's cond_layer slice (bv2_pack.h wn_gate_row). */
int bv2_test_wn_gate_row(int hid, int n);
/* acts [B][H][L] = tanh(v[:H]) * sigmoid(v[H:]), v = conv1d(x [B][H][L], w_host [2H][H][5]) + bias_host [2H] + gl_host [B][2H] (all three
 * HOST, permuted into gate order by the packer's code); no masks.  wpack_dev needs bv2_test_wn_in_pack_floats(B, H) floats. */
int64_t bv2_test_wn_in_pack_floats(int B, int H);
int bv2_test_wn_in_layer(void* stream, const float* x, const float* w_host, const float* bias_host, const float* gl_host, float* acts,
                         float* wpack_dev, int B, int H, int L, int tile);
/* rs = conv1d(acts [B][H][L], w_host [2H][H][1]) + bias_host [2H] (HOST; [H][H][1] / [H] when last).  Not last: x = (x + rs[:H]) * mask in
 * place and outacc (+)= rs[H:] unmasked, two problems of one launch; last: outacc = (outacc + rs) * mask.  first: outacc is written, not
 * added to.  x / outacc [B][H][L], mask [B][L] DEVICE.  wpack_dev needs bv2_test_wn_res_skip_pack_floats(H) floats. */
int64_t bv2_test_wn_res_skip_pack_floats(int H);
int bv2_test_wn_res_skip(void* stream, const float* acts, const float* w_host, const float* bias_host, float* x, float* outacc,
                         const float* mask, float* wpack_dev, int B, int H, int L, int tile, int first, int last);

/* tuning experiments (tools/kbench.py): force the split-K wave count / C_in chunk / tile-count target of the fp32 conv; 0 = default */
void bv2_test_set_tuning(int splitk_waves, int force_ck, long tile_target);
/* splitk_waves + 100: the split-K kernel's register form (no staged X tile); + 200: the staged form with its row-per-wave staging in the
 * head form too.  bv2_test_splitk_stage: how the last split-K launch staged X: -1 = register form, 0 = row per wave, 16 / 24 = block
 * staging with that many loads per thread */
int bv2_test_splitk_stage(void);
/* ... and the waves per workgroup of the last split-K launch (4 / 8 / 16: which instantiation of the kernel ran) */
int bv2_test_splitk_waves(void);
/* bv2_set_option("kernarg_head") for the launch entries of this header, which have no handle (bv2_test_conv1d, bv2_test_conv_multi,
 * bv2_test_layernorm*, bv2_test_attention*, bv2_test_flow_boundary): 1 (default) = the head form where a launch fits it, 0 = the generic kernels */
void bv2_test_set_kernarg_head(int on);
/* Host only: would a one-problem (nprob = 1) split-K launch with these values take the head form?  1: yes, and out6 = {k, dil, pad_left,
 * ksplit, cin, cin_pad} as the kernel unpacks them from the head's two packed dwords; 0: it falls back to the generic kernel (a value does not
 * fit its packed field — 8 bits for k / dil / pad_left / ksplit, 16 for cin / cin_pad — or B != 1, `lens` set, nprob != 1) */
int bv2_test_splitk_head(int k, int dil, int pad_left, int ksplit, int cin, int cin_pad, int B, int has_lens, int nprob, int32_t* out6);
/* conv_x6.hip: forced tile id (9 / 11, see bv2_kernels.h TILE_X6_*) per C_out class (multiple of 256 / of 128 / other); the last argument is unused */
void bv2_test_set_x6_tuning(int t256, int t128, int t64, int ck);
/* workgroups per CU hipOccupancyMaxActiveBlocksPerMultiprocessor grants the conv_x6 variants {128x64, 128x64 + loader waves, 64x128, 32x256} */
void bv2_test_x6_occupancy(int* out4);
/* bf16 / fp16 conv variants: cl_spec "<nt>:<id>[,...]" forces bf16 variant <id> for launches with <nt> 32-channel tiles ("" = the
 * shipped choice), cl_generic / hc_generic = 1 force the generic GEMM loop instead of the C_in-specialised tap-major one */
void bv2_test_set_variants(const char* cl_spec, int cl_generic, int hc_generic);

/* tools/timeline.py: while dev_buf (capacity_u64 zeroed uint64 on the DEVICE) is set, every fp32 conv launch records 8 uint64 per
 * workgroup {s_memtime at start, after the prologue, after the main loop, at the end, HW_ID, XCC_ID, k or units, valid} into its own
 * slice; bv2_test_conv_timeline_report fills 8 int64 per launch {offset, grid x, y, z, tile (BM*1000+BN), k0|k1<<8|k2<<16, cin, L}. */
void bv2_test_conv_timeline(void* dev_buf, long long capacity_u64);
int bv2_test_conv_timeline_report(long long* meta, int max_launches);

/* inverse RQ spline on channel `dst` of z [B][2][T] with params [B][prow][T] (DEVICE) */
int bv2_test_spline(void* stream, float* z, int src, int dst, const float* params, int prow, const float* mask,
                    float sqrt_fc, float tail, int B, int T);

/* forward RQ spline with linear tails alone (kernels/spline.h rq_spline_forward_one), N elements, all DEVICE: x [N]; uw / uh [N][10]
 * unnormalised widths / heights as the spline takes them (already divided by sqrt(filter_channels)); ud [N][9] raw interior derivatives
 * -> y [N], logabsdet [N] */
int bv2_test_spline_forward(void* stream, const float* x, const float* uw, const float* uh, const float* ud, float tail, long long N,
                            float* y, float* logabsdet);

/* the HOST instantiations of kernels/rng.h (the seeded-noise generator of bv2_set_noise_seeds): Philox4x32-10 itself, and the N(0,1)
 * value at (seed, which, row, t).  The integer core is the device's code; the host value differs from the device's only by the
 * rounding of the host's log / sin / cos. */
void bv2_test_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
float bv2_test_seeded_normal(int64_t seed, int which, int row, int t);

#ifdef __cplusplus
}
#endif
#endif
