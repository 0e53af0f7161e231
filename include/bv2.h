/*
 * bv2.h — C ABI of libbv2.so, the MI355X-native (gfx950) SynthesizerTrn.infer() hot path of Bert-VITS2 v2.3.
 *
 * The reference (fishaudio/Bert-VITS2) is 100 % Python and has NO FFI/operator interface; the only seam is the
 * Python class models.SynthesizerTrn (reference models.py:811-1074).  This header is therefore the boundary a
 * maintainer would bind from the reference's Python (ctypes stub shown in INTEGRATION.md); each entry point names
 * the reference code it replaces.  The stage split mirrors the reference's own ONNX export, which cuts infer() into
 * emb / enc_p / sdp / dp / flow / dec and makes both noise draws explicit inputs
 * (reference onnx_modules/V230/models_onnx.py:896-1063, onnx_modules/V220_OnnxInference/__init__.py:88-117).
 *
 * Conventions
 *  - plain C, no torch types: raw pointers + sizes.  All activations are fp32, layout [B, C, T], T contiguous
 *    (the reference's layout).  Integer inputs are int64 like the reference's LongTensors.
 *  - every DEVICE buffer (inputs, outputs, workspace, packed weights) is allocated and owned by the CALLER
 *    (PyTorch in the shim).  The library never hipMalloc's; it only launches kernels / async copies on the
 *    stream it is handed, so every entry point is hipGraph-capturable.
 *  - status: 0 = ok, negative = error; bv2_last_error(h) holds the message (no exceptions cross the ABI).
 *    The reference raises Python exceptions at the same places (shape asserts infer.py:124, ValueError
 *    transforms.py:113-114); the Python shim turns a non-zero status into RuntimeError.
 *  - one handle per GPU / per caller thread (thread-compatible, like the single-threaded reference).
 */
#ifndef BV2_H
#define BV2_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BV2_ABI_VERSION 3   /* 3: bv2_decode_in.nz_tstride, the six ONNX-seam stage calls, bv2_detach_weights,
                               pack-layout version in the blob header */
#define BV2_PACK_LAYOUT 16   /* bumped whenever bv2_model.cpp changes the order / format of anything inside the packed blob:
                               a blob cached on disk by an older packer is rejected by bv2_attach_weights */
#define BV2_POSTERIOR_LAYOUT 1   /* the same for the posterior encoder's own blob (bv2_posterior_pack) */
#define BV2_SDP_FORWARD_LAYOUT 1 /* ... and for the forward duration predictor's (bv2_sdp_forward_pack) */
#define BV2_MAX_UPS 8
#define BV2_MAX_RESBLOCK_KERNELS 4
#define BV2_MAX_RESBLOCK_DILATIONS 4

typedef struct bv2_handle bv2_handle;
typedef void* bv2_stream; /* hipStream_t */

/* Construction arguments of reference SynthesizerTrn.__init__ (models.py:816-842) that shape the hot path,
 * as infer.get_net_g derives them from configs/config.json (infer.py:95-101). */
typedef struct bv2_config {
  int32_t struct_bytes;            /* = sizeof(bv2_config) */
  int32_t n_vocab, n_tones, n_languages, bert_dim;      /* 112, 12, 3, 1024 (text/symbols.py:167-183) */
  int32_t inter_channels, hidden_channels, filter_channels, n_heads, n_layers, kernel_size;
  int32_t gin_channels, n_speakers;
  int32_t use_transformer_flow, n_flow_layer, n_layers_trans_flow;
  int32_t n_upsamples;
  int32_t upsample_rates[BV2_MAX_UPS];
  int32_t upsample_kernel_sizes[BV2_MAX_UPS];
  int32_t upsample_initial_channel;
  int32_t n_resblock_kernels;
  int32_t resblock_kernel_sizes[BV2_MAX_RESBLOCK_KERNELS];
  int32_t n_resblock_dilations;
  int32_t resblock_dilation_sizes[BV2_MAX_RESBLOCK_KERNELS][BV2_MAX_RESBLOCK_DILATIONS];
  /* appended in round 5 (a caller built against the shorter struct passes its own struct_bytes and gets ResBlock1):
   * 0 / 1 = modules.ResBlock1 (convs1 / convs2 pairs, reference modules.py:239-315), 2 = modules.ResBlock2 (ONE conv per dilation,
   * n_resblock_dilations = 2: `resblock: "2"` of models.py:508, modules.py:318-363) */
  int32_t resblock_type;
  /* appended with the ReferenceEncoder: width of the linear spectrogram the encoder reads (filter_length / 2 + 1; 1025, 513 or 80).  Only
   * read when n_speakers == 0 — the speaker vector g then comes from ref_enc (models.py:1047-1048, bv2_ref_encode below) and the blob holds
   * ref_enc.* instead of emb_g.weight.  A caller built against the shorter struct passes its own struct_bytes: legal with n_speakers >= 1
   * only (the field is ignored there and changes nothing in the blob). */
  int32_t spec_channels;
} bv2_config;

enum { BV2_F32 = 0, BV2_F16 = 1, BV2_BF16 = 2 };

/* ---- lifetime ------------------------------------------------------------------------------------------- */
int bv2_abi_version(void);
/* replaces SynthesizerTrn.__init__ (models.py:816-935). */
int bv2_create(const bv2_config* cfg, bv2_handle** out);
void bv2_destroy(bv2_handle* h);
/* h may be NULL: returns the message of the last failed bv2_create on this thread. */
const char* bv2_last_error(const bv2_handle* h);

/* ---- weights: replaces utils.load_checkpoint (utils.py:65-120) + per-forward weight_norm ---- */
/* Hand over one tensor of the reference state_dict by its reference key.  host_ptr is HOST
 * memory, copied.  Keys outside the inference schema (enc_q.*, sdp.post_*) are accepted and ignored (returns 1).
 * Both weight-norm forms are accepted: <p>.weight_g + <p>.weight_v, or the folded <p>.weight that
 * Generator.remove_weight_norm (models.py:559-564) leaves behind. */
int bv2_load_tensor(bv2_handle* h, const char* ref_key, const void* host_ptr, const int64_t* shape, int ndim, int dtype);
/* Size in bytes of the packed weight blob for this config. */
int64_t bv2_packed_bytes(const bv2_handle* h);
/* Fold weight-norm (w = g*v/||v||, dim 0; C_in for ConvTranspose1d), fold the flows' channel Flips into weight
 * permutations, fuse q/k/v, split ConvTranspose into polyphase taps, pad to MFMA tile multiples, and write the
 * packed blob into host_blob (HOST memory, bv2_packed_bytes large).  Fails listing any missing tensor. */
int bv2_pack_weights(bv2_handle* h, void* host_blob, int64_t bytes);
/* Point the handle at a packed blob resident in DEVICE memory (caller-owned; e.g. uploaded by rank 0 and broadcast
 * to the other GPUs with RCCL).  Verifies the blob header against this handle's config. */
int bv2_attach_weights(bv2_handle* h, const void* dev_blob, int64_t bytes);
/* Forget the attached blob (the caller is about to free or move it): every compute entry point fails with -8 until the
 * next bv2_attach_weights.  Captured graphs that baked the old address in must be destroyed by the caller. */
int bv2_detach_weights(bv2_handle* h);

/* ---- precision (BASELINE config 3: "bf16 weights/activations, fp32 accumulate") ------------------------------- */
/* Arithmetic of the HiFi-GAN Generator (dec, reference models.py:538-557 — 90 % of the path's FLOPs): BV2_F32 (default;
 * v_mfma_f32_32x32x2_f32, exact fp32) or BV2_BF16 (v_mfma_f32_32x32x16_bf16: bf16 weights and channels-last bf16
 * activations, fp32 accumulation / bias / residual, fp32 conv_post + tanh).  The reference's counterpart is running dec
 * under torch.autocast(bfloat16).  Text encoder, duration predictors, length regulation and flow stay fp32 in both modes
 * (durations stay bit-stable).  The packed blob always carries both weight forms, so this is a per-call switch. */
int bv2_set_generator_dtype(bv2_handle* h, int dtype);
/* Arithmetic of the transformer flow's Encoder convolutions (BASELINE config 5 "fp16 flow + fp32 spline"): the fused
 * q/k/v projection, conv_o and the FFN conv_1/conv_2 of TransformerCouplingLayer.enc (reference modules.py:561-580,
 * attentions.py:103-120, 263-266, 438-446) — 95 % of the flow's FLOPs.  BV2_F32 (default) or BV2_F16
 * (v_mfma_f32_32x32x16_f16: fp16 weights and conv inputs, fp32 accumulation; the FFN hidden activation is stored fp16;
 * the attention core's two matrix products QK^T and PV take their operands rounded to fp16 in registers).
 * LayerNorm, logits / softmax / running statistics, the residual stream, pre/post and everything before the flow (text
 * encoder, durations, spline) stay fp32, so durations and the alignment path are unchanged.  The reference's counterpart is running
 * flow under torch.autocast(float16).  Only the transformer flow has an fp16 form (returns -2 otherwise). */
int bv2_set_flow_dtype(bv2_handle* h, int dtype);

/* ---- workspace ------------------------------------------------------------------------------------------- */
/* Bytes of caller-provided DEVICE scratch needed by any stage call with batch B, T symbols, Ty_max frames. */
int64_t bv2_workspace_bytes(const bv2_handle* h, int B, int T, int Ty_max);

/* ---- phase A: models.py:1045-1057 (emb_g, enc_p, sdp, dp, exp/ceil/sum) ------------------------------------- */
typedef struct bv2_encode_in {
  int32_t B, T;
  const int64_t* x;          /* [B,T] symbol ids */
  const int64_t* x_lengths;  /* [B] */
  const int64_t* sid;        /* [B]  (not read by the _g calls when they are given a g) */
  const int64_t* tone;       /* [B,T] */
  const int64_t* language;   /* [B,T] */
  const float* bert;         /* [B,bert_dim,T] */
  const float* ja_bert;      /* [B,bert_dim,T] */
  const float* en_bert;      /* [B,bert_dim,T] */
  const float* noise_w;      /* [B,2,T]  N(0,1): the torch.randn of models.py:248-251, drawn by the caller; may be NULL exactly when the
                              * stochastic predictor is not run (see bv2_encode_out), otherwise NULL is an error (-1) */
  float noise_scale_w, sdp_ratio, length_scale;
  /* Optional WORD-level BERT features.  The reference runs the BERT model, copies hidden_states[-3] to the host,
   * repeats word i's row word2ph[i] times (text/chinese_bert.py:37, 48-58) and uploads [1024, T] again.  With
   * bert_index[f] != NULL feature f (0 = bert, 1 = ja_bert, 2 = en_bert) is handed over as the BERT model emitted it,
   * [B, bert_dim, bert_cols[f]] — one column per word, still on the device — and symbol t of utterance b takes column
   * bert_index[f][b*T + t] (the word2ph repeat as a gather inside the TextEncoder front: the repeated matrix never exists).
   * NULL: the feature is [B, bert_dim, T], one column per symbol, as in the reference. */
  const int32_t* bert_index[3];
  int32_t bert_cols[3];
} bv2_encode_in;

typedef struct bv2_encode_out {   /* all DEVICE, caller-allocated */
  float* g;          /* [B,gin]            emb_g(sid), or a copy of the given g     models.py:1046-1048 */
  float* x;          /* [B,hidden,T]       encoder output                   models.py:1049 */
  float* m_p;        /* [B,inter,T] */
  float* logs_p;     /* [B,inter,T] */
  float* x_mask;     /* [B,T] (1.0 / 0.0)                                  models.py:392-394 */
  float* logw_sdp;   /* [B,T]  sdp(...) before mixing (may be NULL) */
  float* logw_dp;    /* [B,T]  dp(...)  before mixing (may be NULL) */
  /* Only the predictor the mix can see is run.  logw = logw_sdp * r + logw_dp * (1 - r) with r = sdp_ratio, so with
   *   - the scalar bv2_encode_in.sdp_ratio exactly 0.0f (no per-utterance bv2_item_controls.sdp_ratio: those values live on the device),
   *   - logw_sdp == NULL, no tap set (bv2_set_tap) and the option "lean_durations" on (default),
   * the StochasticDurationPredictor is not launched, noise_w is not read and logw = logw_dp * 1.  In the same way sdp_ratio exactly 1.0f
   * with logw_dp == NULL leaves the DurationPredictor out.  Every other request runs both.  The one difference from the reference's
   * `sdp * 0 + dp`: a non-finite value of the skipped predictor cannot reach logw, and a zero in logw may differ in sign; w_ceil,
   * y_lengths and everything downstream are the same. */
  float* logw;       /* [B,T]                                              models.py:1052-1054 */
  float* w_ceil;     /* [B,T]  ceil(exp(logw)*mask*length_scale)           models.py:1055-1056 */
  int64_t* y_lengths;/* [B]    clamp_min(sum(w_ceil),1)                    models.py:1057 */
} bv2_encode_out;

int bv2_encode_durations(bv2_handle* h, bv2_stream stream, const bv2_encode_in* in, const bv2_encode_out* out,
                         void* workspace, int64_t workspace_bytes);

/* ---- phase B: models.py:1058-1073 (sequence_mask, generate_path, expand, z_p, flow reverse, dec) ------------ */
typedef struct bv2_decode_in {
  int32_t B, T;
  int32_t Ty;                /* max(y_lengths), read back by the caller (the reference's one host sync, commons.py:120-122) */
  int32_t max_len;           /* frames fed to dec: (z*y_mask)[:, :, :max_len]; <=0 means all (models.py:1073) */
  const float* m_p;          /* [B,inter,T]  from phase A */
  const float* logs_p;       /* [B,inter,T] */
  const float* x_mask;       /* [B,T] */
  const float* w_ceil;       /* [B,T]  (the caller may substitute durations, as train_ms.evaluate-style tooling does) */
  const int64_t* y_lengths;  /* [B] */
  const float* g;            /* [B,gin] */
  const float* noise_z;      /* N(0,1) for models.py:1071; element (b,c,j) at noise_z[b*nz_bstride + c*nz_cstride + j*nz_tstride].
                                The reference draws it with randn_like on a TRANSPOSED view (strides (C*Ty, 1, C)); passing the
                                strides lets the caller hand that tensor over as it is (the RNG contract). */
  int64_t nz_bstride, nz_cstride, nz_tstride;   /* nz_tstride <= 0 means 1 */
  float noise_scale;
  int32_t exact_lengths;     /* 0: the reference's batch semantics — dec is unmasked, so in a padded batch the activations
                                past an utterance's end bleed into its last ~40 ms (models.py:1073 masks only z).
                                1: every Generator conv treats positions >= y_lengths[b]*(samples per frame at its stage) as
                                zero padding, i.e. each utterance of a ragged batch gets exactly the audio it gets when run
                                alone (what the reference produces, since it only ever infers at batch 1); tiles past an
                                utterance's end are skipped.
                                2: Ty is a BUCKET >= max(y_lengths) (a hipGraph captured once per bucket instead of once per exact
                                T_y — T_y = max(y_lengths) is data-dependent, commons.py:119-123): every Generator conv treats positions
                                >= max_b(y_lengths) * (samples per frame at its stage) as zero padding for EVERY utterance, so the first
                                max(y_lengths) frames of every output are what mode 0 produces at Ty = max(y_lengths); the flow needs
                                nothing (frames past y_lengths[b] are masked in both).  Outputs past that frame are zeros / padding. */
} bv2_decode_in;

typedef struct bv2_decode_out {   /* all DEVICE, caller-allocated; any pointer except o may be NULL */
  float* o;          /* [B,1,S]  S = min(Ty,max_len) * prod(upsample_rates) */
  float* attn;       /* [B,1,Ty,T] one-hot monotone path                   models.py:1061-1062 */
  float* y_mask;     /* [B,1,Ty] */
  float* z;          /* [B,inter,Ty] */
  float* z_p;        /* [B,inter,Ty] */
  float* m_p;        /* [B,inter,Ty] expanded */
  float* logs_p;     /* [B,inter,Ty] expanded */
} bv2_decode_out;

int bv2_decode(bv2_handle* h, bv2_stream stream, const bv2_decode_in* in, const bv2_decode_out* out,
               void* workspace, int64_t workspace_bytes);

/* ---- single stages: the reference's own ONNX cut of infer() --------------------------------------------------------
 * onnx_modules/V230/models_onnx.py:896-1063 exports six graphs (emb_g, enc_p, sdp, dp, flow, dec) and
 * onnx_modules/V230_OnnxInference/__init__.py:44-126 runs them with the numpy glue in between.  The six calls below take
 * the tensors of those graphs under the same names (comments give "onnx name"), so a MoeVS-style consumer can swap the
 * runtime stage by stage; the parity tests tap them against the oracle.  All fp32 [B,C,T] / int64, DEVICE, caller-owned. */
/* emb_g.run({"sid"}) -> g [B,gin]   (models.py:1046; the consumer unsqueezes to [B,gin,1]) */
int bv2_stage_emb_g(bv2_handle* h, bv2_stream stream, int B, const int64_t* sid, float* g);
/* enc.run({"x","t","language","bert_0","bert_1","bert_2","g"}) -> xout, m_p, logs_p, x_mask   (TextEncoder, models.py:377-400).
 * x_lengths may be NULL: every utterance is T symbols long, as in the exported graph (which has no length input). */
int bv2_stage_enc_p(bv2_handle* h, bv2_stream stream, int B, int T, const int64_t* x, const int64_t* t, const int64_t* language,
                    const float* bert_0, const float* bert_1, const float* bert_2, const float* g, const int64_t* x_lengths,
                    float* xout, float* m_p, float* logs_p, float* x_mask, void* workspace, int64_t workspace_bytes);
/* sdp.run({"x","x_mask","zin","g"}) -> logw [B,1,T]: StochasticDurationPredictor reverse (models.py:197-204, 245-256) where
 * zin [B,2,T] is the ALREADY SCALED noise (randn * noise_scale_w), exactly as the exported graph takes it. */
int bv2_stage_sdp(bv2_handle* h, bv2_stream stream, int B, int T, const float* x, const float* x_mask, const float* zin,
                  const float* g, float* logw, void* workspace, int64_t workspace_bytes);
/* dp.run({"x","x_mask","g"}) -> logw [B,1,T]: DurationPredictor (models.py:285-299) */
int bv2_stage_dp(bv2_handle* h, bv2_stream stream, int B, int T, const float* x, const float* x_mask, const float* g,
                 float* logw, void* workspace, int64_t workspace_bytes);
/* flow.run({"z_p","y_mask","g"}) -> z: flow(z_p, y_mask, g, reverse=True), models.py:1072.  The frame mask comes either as
 * y_lengths [B] (int64) or as the graph's y_mask [B,1,Ty] (fp32 0/1) — exactly one of the two is non-NULL.  z_p is not
 * modified; z receives the result. */
int bv2_stage_flow(bv2_handle* h, bv2_stream stream, int B, int Ty, const float* z_p, const int64_t* y_lengths,
                   const float* y_mask, const float* g, float* z, void* workspace, int64_t workspace_bytes);
/* The same flow in its FORWARD direction, z -> z_p: flow(z, y_mask, g=g) as SynthesizerTrn.forward() calls it (models.py:958; no ONNX graph
 * has it).  It maps a posterior latent into the prior's space, which is where the aligner below compares a recording with its text.  Both
 * flow variants; the couplings run first to last with x1 = (x1 + post(h)) * mask and the channel Flips where the reference has them, so
 * bv2_stage_flow(bv2_stage_flow_forward(z)) returns z up to fp32 round-off on the unmasked frames.  Always fp32: bv2_set_flow_dtype does not
 * apply, and the fused coupling boundary ("fused_boundary") is not used in this direction.  Arguments as bv2_stage_flow; z is not modified. */
int bv2_stage_flow_forward(bv2_handle* h, bv2_stream stream, int B, int Ty, const float* z, const int64_t* y_lengths,
                           const float* y_mask, const float* g, float* z_p, void* workspace, int64_t workspace_bytes);
/* dec.run({"z_in","g"}) -> o: Generator.forward models.py:538-557 on z_in[:, :, :L] (z_in has row stride Ty); with y_lengths
 * non-NULL the input is (z*y_mask)[:, :, :L] as at models.py:1073, with NULL it is taken as it is (the exported graph).
 * o is [B,1,L*prod(rates)]. */
int bv2_stage_generator(bv2_handle* h, bv2_stream stream, int B, int Ty, int L, const float* z, const int64_t* y_lengths,
                        const float* g, float* o, void* workspace, int64_t workspace_bytes);

/* ---- one-shot convenience: whole infer() with an internal stream sync between the phases ---------------------- */
/* Outputs must be sized for Ty_cap frames; returns -3 (and sets *Ty_out) if the realised Ty exceeds Ty_cap.
 * Row strides of the [.,.,Ty] outputs are the realised Ty (*Ty_out), tensors are written densely. */
int bv2_infer(bv2_handle* h, bv2_stream stream, const bv2_encode_in* in, const bv2_encode_out* enc_out,
              const float* noise_z, int64_t nz_bstride, int64_t nz_cstride, int64_t nz_tstride, float noise_scale, int32_t max_len,
              int32_t Ty_cap, const bv2_decode_out* dec_out, int32_t* Ty_out, void* workspace, int64_t workspace_bytes);

/* ---- per-utterance synthesis controls --------------------------------------------------------------------------------
 * The reference's infer() takes sdp_ratio, noise_scale, noise_scale_w and length_scale as values torch broadcasts, so a caller
 * may pass one value per utterance as a [B,1,1] tensor (models.py:248-251, 1052-1056, 1071); a serving front end gives every
 * request its own sliders (hiyoriUI /voice: sdp_ratio, noise, noisew, length).  The _ex calls below take such values as DEVICE
 * fp32 arrays of B elements: utterance b then gets exactly what a batch-1 call with those four values as scalars gets (same
 * logw / w_ceil / y_lengths / path bit for bit; sdp_ratio's complement is formed per utterance as (float)(1.0 - (double)r), the
 * rounding of the scalar path).  A NULL member keeps the scalar of bv2_encode_in / bv2_decode_in / bv2_infer; a NULL
 * bv2_item_controls* is the plain call (the five calls without _ex are exactly that).  A captured graph bakes in the four
 * ADDRESSES, not the values: refill the arrays in place before a replay, and one capture per shape serves every control set.
 * struct_bytes must be sizeof(bv2_item_controls), otherwise the call fails (-1, message in bv2_last_error). */
typedef struct bv2_item_controls {
  int32_t struct_bytes;            /* = sizeof(bv2_item_controls) */
  const float* noise_scale_w;      /* [B] DEVICE fp32, or NULL = the scalar in bv2_encode_in */
  const float* sdp_ratio;          /* [B] or NULL */
  const float* length_scale;       /* [B] or NULL */
  const float* noise_scale;        /* [B] or NULL = the scalar in bv2_decode_in / bv2_infer */
} bv2_item_controls;

int bv2_encode_durations_ex(bv2_handle* h, bv2_stream stream, const bv2_encode_in* in, const bv2_encode_out* out,
                            const bv2_item_controls* controls, void* workspace, int64_t workspace_bytes);
int bv2_decode_ex(bv2_handle* h, bv2_stream stream, const bv2_decode_in* in, const bv2_decode_out* out,
                  const bv2_item_controls* controls, void* workspace, int64_t workspace_bytes);
int bv2_infer_ex(bv2_handle* h, bv2_stream stream, const bv2_encode_in* in, const bv2_encode_out* enc_out,
                 const float* noise_z, int64_t nz_bstride, int64_t nz_cstride, int64_t nz_tstride, float noise_scale, int32_t max_len,
                 int32_t Ty_cap, const bv2_decode_out* dec_out, int32_t* Ty_out, const bv2_item_controls* controls, void* workspace,
                 int64_t workspace_bytes);

/* ---- speaker conditioning from a reference spectrogram or a given vector ----------------------------------------------
 * The reference forms the speaker vector g in one of two ways (models.py:1045-1048): emb_g(sid) when the model has a speaker table,
 * ref_enc(y.transpose(1, 2)) when it was trained with n_speakers = 0 (the voice is taken from a reference recording).
 *
 * bv2_ref_encode is that second branch (ReferenceEncoder, models.py:752-808; n_speakers == 0 models only, -2 otherwise): y is the linear
 * spectrogram [B, spec_channels, L] as the reference's infer() takes it, element (b, f, t) at y[b*strides[0] + f*strides[1] + t*strides[2]]
 * (strides NULL = contiguous), g_out [B, gin].  Exact fp32 throughout, eight launches, graph-capturable.  y_lengths [B] (int64, DEVICE; NULL =
 * every item is L frames long, the reference's semantics) makes a padded batch exact: item b's frames >= y_lengths[b] are zero padding in
 * EVERY layer (the length shrinks as n -> (n - 1) / 2 + 1 per conv) and its GRU stops after its own last step, so each item gets bit for
 * bit the g it gets alone.  Values outside [1, L] are clamped.  The workspace is sized by bv2_ref_workspace_bytes (it depends on L, which
 * bv2_workspace_bytes does not know); g is meant to be computed once per voice and cached by the caller.
 *
 * The _g calls are bv2_encode_durations_ex / bv2_infer_ex / bv2_graph_capture_encode_ex with one more argument, g [B, gin] (DEVICE fp32):
 * phase A then conditions on that vector instead of emb_g(sid) — a ref_enc result, a blend of table rows, any vector — through the same
 * kernel code that reads the table row (g = emb_g row s gives bit-identical results to sid = s), and copies it to bv2_encode_out.g, where
 * phase B reads it.  in->sid is not read and may be NULL.  g == NULL is the plain _ex call.  A model with n_speakers == 0 has no table:
 * every phase-A call without g fails (-1, message) and does not read sid.  A captured graph bakes in the ADDRESS of g: refill it in place
 * before a replay, one capture per shape serves every voice. */
int64_t bv2_ref_workspace_bytes(const bv2_handle* h, int B, int L);
int bv2_ref_encode(bv2_handle* h, bv2_stream stream, const float* y, const int64_t* strides, const int64_t* y_lengths, int B, int L,
                   float* g_out, void* workspace, int64_t workspace_bytes);
int bv2_encode_durations_g(bv2_handle* h, bv2_stream stream, const bv2_encode_in* in, const bv2_encode_out* out,
                           const bv2_item_controls* controls, const float* g, void* workspace, int64_t workspace_bytes);
int bv2_infer_g(bv2_handle* h, bv2_stream stream, const bv2_encode_in* in, const bv2_encode_out* enc_out,
                const float* noise_z, int64_t nz_bstride, int64_t nz_cstride, int64_t nz_tstride, float noise_scale, int32_t max_len,
                int32_t Ty_cap, const bv2_decode_out* dec_out, int32_t* Ty_out, const bv2_item_controls* controls, const float* g,
                void* workspace, int64_t workspace_bytes);

/* ---- 16-bit PCM (serving glue; replaces the host-side gradio convert_to_16_bit_wav the reference's callers run after
 * .cpu(): webui.py:86,129, hiyoriUI.py:343) -------------------------------------------------------------------- */
/* pcm[b][i] = (int16) trunc( wave[b][i] / max_j |wave[b][j]| * 32767 ) over the valid samples i, j < y_lengths[b]*hop
 * (capped at S); samples past the utterance are 0; an all-zero utterance stays 0.  wave [B][wave_bstride >= S] fp32,
 * pcm [B][pcm_bstride >= S] int16, peak_scratch [B] uint32 — all DEVICE.  Asynchronous on `stream`, graph-capturable.
 * (Streamed PCM — bv2_stream_chunk / bv2_emit below — has no peak to divide by: it is trunc(clamp(x * gain)) with a fixed gain and differs
 * from this conversion by exactly the factor 1 / max_j |wave[b][j]|.) */
int bv2_pcm16(bv2_stream stream, const float* wave, int64_t wave_bstride, const int64_t* y_lengths, int32_t hop, int32_t B,
              int64_t S, int16_t* pcm, int64_t pcm_bstride, uint32_t* peak_scratch);

/* ---- streamed synthesis: the flow once, the Generator window by window, audio chunk by chunk ---------------------------
 * bv2_decode returns an utterance after the whole Generator has run over all Ty frames, and its workspace holds fourteen
 * [B, C_i * samples-per-frame * Ty] Generator buffers.  The flow needs all of Ty (its attention spans it); the Generator (models.py:538-557)
 * is a stack of convolutions with a finite receptive field, so a window of frames decodes to the same samples as the whole — given a halo.
 *
 * The halo H = bv2_generator_halo(h): latent frames a window carries on each side.  It is the input interval of output samples [a*U, b*U)
 * (U = product of the upsample rates) walked backwards: conv_post (k = 7) +-3 samples; per stage, last to first, the widest ResBlock branch
 * (ResBlock1: sum_d (k-1)/2 * (d+1); ResBlock2: sum_d (k-1)/2 * d) and ConvTranspose1d(k, stride u, p = (k-u)/2): lo -> ceil((lo + p - k + 1) / u),
 * hi -> floor((hi + p) / u); conv_pre (k = 7) +-3 frames.  13 for the v2.3 shapes.  The Generator work of a stream grows by (N + 2H) / N for chunks
 * of N frames.
 *
 * bv2_stream_begin is bv2_decode_ex up to and including the flow (expand, the speaker GEMVs, the flow): z, y_mask and the GEMV results stay in
 * the workspace; out->o is not written (may be NULL), the other outputs are written as bv2_decode writes them; in->max_len and
 * in->exact_lengths are not read (the chunks carry them).  The caller leaves the workspace untouched until the last chunk.
 * bv2_stream_chunk runs the Generator of the handle's dtype on frames [max(0, t0 - H), min(L, t1 + H)) of that z (L = Ty, or max_len) and
 * writes samples [t0*U, t1*U) of every item to dst + b * dst_bstride (fp32) or dst16 + b * dst16_bstride (16-bit PCM): sample 0 of the
 * destination is sample t0*U of the utterance — the caller offsets the pointer.  Samples at or past y_lengths[b]*U are written as zeros in
 * both exact_lengths modes (bv2_decode's mode 0 leaves the padded batch's bleed there).  Chunks may come in any order and any size up to
 * window_frames, on the stream bv2_stream_begin ran on (or one ordered behind it).
 * Numerics: a window is another tiling of the same convolutions, and with "conv_x3" = 1 the layer-wise two-plane fp16 convs take their
 * activation scale from the max |x| of the window's tensor instead of the utterance's — the agreement with bv2_decode is that of two batch
 * shapes of the same audio (fp32 round-off in fp32 mode, bf16 round-off with the bf16 Generator), not bit identity.
 * Streamed PCM is (int16) trunc(clamp(x * pcm_gain, -32768, 32767)) with a FIXED gain (32767 unless the caller wants headroom): a stream cannot
 * know the utterance's peak, and tanh bounds |x| <= 1.  It differs from bv2_pcm16's peak-normalised conversion by exactly the factor
 * 1 / max|x| of the utterance.
 * Every argument is checked before anything touches the device (-1 and a message in bv2_last_error; -5 for a short workspace).
 * Out of scope: capturing chunks in a hipGraph (the window pointer changes per call), taps during a stream (both calls fail while a tap is set)
 * and exact_lengths == 2. */
int bv2_generator_halo(const bv2_handle* h);
/* window_frames: the largest number of kept frames (t1 - t0) of a chunk.  The kept buffers (speaker GEMV results, y_mask, z, z_p, frame
 * indices, x3 slots, length caps, a [B] window-length array) come first; behind them ONE region is shared by the flow's scratch at Ty and the
 * Generator's buffers at min(Ty, window_frames + 2H) frames plus the window's [B, frames * U] output.  Covers phase A at (B, T) as well. */
int64_t bv2_stream_workspace_bytes(const bv2_handle* h, int B, int T, int Ty, int window_frames);
int bv2_stream_begin(bv2_handle* h, bv2_stream stream, const bv2_decode_in* in, const bv2_decode_out* out,
                     const bv2_item_controls* controls, void* workspace, int64_t workspace_bytes);
typedef struct bv2_stream_chunk_args {
  int32_t struct_bytes;            /* = sizeof(bv2_stream_chunk_args) */
  int32_t B, Ty;                   /* as given to bv2_stream_begin */
  int32_t t0, t1;                  /* kept frames: 0 <= t0 < t1 <= L, t1 - t0 <= window_frames */
  const int64_t* y_lengths;        /* [B] DEVICE */
  int32_t exact_lengths;           /* 0 / 1 as in bv2_decode_in: 1 = item b's window is clamp(y_lengths[b] - w0, 1, W) frames long
                                      (w0 = max(0, t0 - H); an item that ended before w0 runs as one masked frame and comes out as zeros) */
  float* dst; int64_t dst_bstride;           /* EITHER fp32 [B][dst_bstride >= (t1 - t0) * U] ... */
  int16_t* dst16; int64_t dst16_bstride;     /* ... OR 16-bit PCM; exactly one of dst / dst16 is non-NULL */
  float pcm_gain;                  /* dst16 only; <= 0 means 32767 */
  int32_t window_frames;           /* as given to bv2_stream_workspace_bytes */
  int32_t max_len;                 /* frames fed to the Generator, L = min(Ty, max_len) (models.py:1073); <= 0 means all */
} bv2_stream_chunk_args;
int bv2_stream_chunk(bv2_handle* h, bv2_stream stream, const bv2_stream_chunk_args* args, void* workspace, int64_t workspace_bytes);
/* The copy at the end of a chunk on its own (handle-free, like bv2_pcm16; kernels/stream.hip): n samples per item from
 * src + b * src_bstride + src_off to dst + b * dst_bstride (fp32, a copy) or dst16 + b * dst_bstride (PCM as above, gain <= 0 means 32767) —
 * exactly one of the two non-NULL; samples i >= y_lengths[b] * hop - start_sample become zero and their source is not used (y_lengths NULL:
 * none).  One pass, 16 bytes per thread on the aligned body of the destination, any alignment of source offset, destination and n. */
int bv2_emit(bv2_stream stream, const float* src, int64_t src_bstride, int64_t src_off, const int64_t* y_lengths, int32_t hop,
             int64_t start_sample, int32_t B, int64_t n, float* dst, int16_t* dst16, int64_t dst_bstride, float gain);

/* ---- from a waveform to the spectrogram bv2_ref_encode reads (handle-free, like bv2_pcm16) -----------------------------
 * The reference turns a recording into y with mel_processing.spectrogram_torch (mel_processing.py:43-78, called from data_utils.py:99-138
 * after audio / max_wav_value): reflect padding by pad = (n_fft - hop) / 2 at both ends, periodic Hann window of `win` samples centred in
 * n_fft, torch.stft(center = False), sqrt(re^2 + im^2 + 1e-6); a model whose spec_channels is a mel width takes mel_spectrogram_torch
 * (:95-142): log(max(M . spec, 1e-5)) with M the Slaney-scale, Slaney-normalised filterbank of librosa.filters.mel.  bv2_spectrogram is that
 * step on the device, as an fp32 FFT (kernels/stft.hip), two launches, asynchronous on `stream`, graph-capturable.
 *
 * Accepted: n_fft 1024 or 2048, 1 <= hop <= n_fft, 1 <= win <= n_fft, n_mels >= 0 (0 = the linear spectrogram, n_fft / 2 + 1 rows).  A
 * failed call returns non-zero (the frame / size queries a negative value) and leaves its message in bv2_last_error(NULL); every argument is
 * checked before anything touches the device.  No file decoding: samples go in, at the model's sampling rate (bv2_resample below brings a
 * recording at another rate there). */
enum { BV2_WAV_F32 = 0, BV2_WAV_I16 = 1 };     /* fp32 in [-1, 1], or 16-bit PCM read as x / 32768 (exact) */
typedef struct bv2_stft_config {
  int32_t struct_bytes;            /* = sizeof(bv2_stft_config) */
  int32_t n_fft, hop, win;
  int32_t n_mels;                  /* 0 = linear */
  int32_t input_format;            /* BV2_WAV_F32 / BV2_WAV_I16 */
} bv2_stft_config;
/* Frames of a waveform of n_samples: 1 + (n_samples + 2 pad - n_fft) / hop.  Negative for n_samples <= pad (reflect padding needs
 * pad < n_samples; the reference refuses such an input too), for n_samples + 2 pad < n_fft (no whole frame: only with hop > n_fft / 3) and
 * for a bad config. */
int64_t bv2_stft_frames(const bv2_stft_config* cfg, int64_t n_samples);
/* HOST: the filterbank [n_mels][n_fft / 2 + 1] of librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) (htk = False, norm = "slaney"), built
 * in fp64; bv2_mel_basis rounds it to fp32 as the reference does, bv2_mel_basis_f64 hands out the fp64 values.  fmax <= 0 means
 * sampling_rate / 2. */
int bv2_mel_basis(const bv2_stft_config* cfg, int32_t sampling_rate, double fmin, double fmax, float* out);
int bv2_mel_basis_f64(const bv2_stft_config* cfg, int32_t sampling_rate, double fmin, double fmax, double* out);
/* Bytes of DEVICE workspace of a call (twiddles, window and the filterbank's row ranges: it does not grow with B or S). */
int64_t bv2_stft_workspace_bytes(const bv2_stft_config* cfg, int32_t B, int64_t S);
/* wav [B][wav_bstride >= S] (fp32 or int16, DEVICE); wav_lengths [B] (int64, DEVICE) or NULL = every item is S samples long.  Item b's
 * frames are cut from ITS samples [0, wav_lengths[b]) reflect-padded at its own two ends — nothing outside that range is read, so the
 * padding of a batch may hold anything.  spec: element (b, f, t) at spec[b*spec_strides[0] + f*spec_strides[1] + t*spec_strides[2]]
 * (NULL = contiguous [B, C, L]), C = n_mels or n_fft / 2 + 1, L = bv2_stft_frames(cfg, S); a frequency stride of 1 ([B, L, C] memory handed
 * to bv2_ref_encode as the transposed view) is the fast store.  Frames t >= L_b of item b are written as zeros; spec_lengths_out [B] (int64,
 * DEVICE, may be NULL) receives L_b in the form bv2_ref_encode takes as y_lengths (0 for an item of wav_lengths[b] <= pad).  mel_basis
 * [n_mels][n_fft / 2 + 1] (fp32, DEVICE) is read when n_mels > 0. */
int bv2_spectrogram(bv2_stream stream, const bv2_stft_config* cfg, const void* wav, int64_t wav_bstride, const int64_t* wav_lengths,
                    int32_t B, int64_t S, const float* mel_basis, float* spec, const int64_t* spec_strides, int64_t* spec_lengths_out,
                    void* workspace, int64_t workspace_bytes);

/* ---- polyphase resampler: a voice recorded at any rate in, audio at any rate out (handle-free; kernels/resample.hip) ----
 * rate_in -> rate_out are positive integers, rate_in != rate_out; g = gcd, L = rate_out / g, M = rate_in / g.  The filter is a Kaiser-windowed
 * sinc with Z = 32 zero crossings per side, beta = 10.0 and rolloff = 0.91: c = rolloff * min(1, L / M), W = Z / c, K = ceil(W), 2K + 1 taps
 * per phase.  Table T[p][jj], p in [0, L), jj in [0, 2K]: t = p / L - (jj - K), T = c sinc(c t) I0(beta sqrt(1 - (t / W)^2)) / I0(beta) for
 * |t| < W, else 0 (sinc(x) = sin(pi x) / (pi x)); every row is then divided by its own sum, so the DC gain is exactly 1 in every phase.  It
 * is built on the host in fp64 (bv2_resample_taps_f64); the device reads its fp32 rounding (bv2_resample_taps).
 * Item b's signal is x_b[k] for 0 <= k < len_b and ZERO elsewhere; it has N_out(b) = ceil(len_b L / M) outputs
 *   y[n] = sum_{jj = 0..2K} x_b[i0 + jj - K] * T[p][jj],   i0 = floor(n M / L),  p = (n M) mod L   (n M in 64 bits),
 * accumulated in fp32 with fp32 coefficients; int16 input is read as x / 32768 (exact).  Two rules are part of the contract:
 *   1. a sample outside [0, len_b) is SELECTED to zero before it is used, never multiplied in from memory: the padding of a batch may hold
 *      anything (NaN included);
 *   2. the order in which an output's 2K + 1 products are summed depends on nothing but the build of the kernel — not on the tile position,
 *      the batch row, the batch size, n0 or how a stream was cut into ranges: a range of outputs is bit-identical to the same outputs of
 *      the whole.
 * Envelope: L <= 1024 and L * (2K + 1) <= 2^20 table entries (4 MB); 44100 -> 48000 is L = 160 with 73 taps, 44100 -> 8000 L = 80 with 389.
 * Outside it (44100 -> 48001: L = 48001), for equal rates, a rate <= 0 or a wrong struct_bytes every call below fails (non-zero, the
 * length queries negative) with a message in bv2_last_error(NULL) that names the limit; every argument is checked before anything touches
 * the device. */
typedef struct bv2_resample_config {
  int32_t struct_bytes;            /* = sizeof(bv2_resample_config) */
  int32_t rate_in, rate_out;
  int32_t input_format;            /* BV2_WAV_F32 / BV2_WAV_I16 */
} bv2_resample_config;
/* HOST: L, M and K of a rate pair (each pointer may be NULL). */
int bv2_resample_plan(const bv2_resample_config* cfg, int32_t* L, int32_t* M, int32_t* K);
/* ceil(n_in L / M): the outputs of an item of n_in samples. */
int64_t bv2_resample_length(const bv2_resample_config* cfg, int64_t n_in);
/* max(0, ceil((available_in - K) L / M)): the number of outputs whose whole support lies in [0, available_in) — what a stream that has
 * produced available_in samples so far may emit. */
int64_t bv2_resample_ready(const bv2_resample_config* cfg, int64_t available_in);
/* HOST: the table [L][2K + 1]; bv2_resample_taps is exactly the fp32 rounding of bv2_resample_taps_f64. */
int bv2_resample_taps(const bv2_resample_config* cfg, float* out);
int bv2_resample_taps_f64(const bv2_resample_config* cfg, double* out);
/* One launch on `stream`, no allocation, no host sync, graph-capturable.  src + b * src_bstride (fp32 or int16, DEVICE) holds samples
 * [src_start, src_start + src_n) of item b; src_lengths [B] (int64, DEVICE) are the ABSOLUTE lengths len_b, NULL = src_start + src_n for
 * every item.  The call writes outputs [n0, n1) of every item to dst + b * dst_bstride — output n0 lands at offset 0 — and zeros for
 * n >= N_out(b); dst_lengths_out [B] (int64, DEVICE, may be NULL; not written by an empty range n0 == n1) receives N_out(b).  taps is the
 * DEVICE copy of bv2_resample_taps.  The caller guarantees two things about the buffer:
 *   lower edge  src_start <= max(0, i0(n0) - K): checked on the host, -1;
 *   upper edge  every index below len_b that [n0, n1) needs is below src_start + src_n.  With src_lengths == NULL that holds by
 *               construction; otherwise the caller limits n1 with bv2_resample_ready.  (An index outside the buffer is never loaded: it
 *               reads as zero.)
 * This range form is the whole streaming primitive: keep the last samples from max(0, i0(n1) - K) on, append the next chunk, call again
 * with n0 = the previous n1. */
int bv2_resample(bv2_stream stream, const bv2_resample_config* cfg, const float* taps, const void* src, int64_t src_bstride,
                 int64_t src_start, int64_t src_n, const int64_t* src_lengths, int32_t B, int64_t n0, int64_t n1, float* dst,
                 int64_t dst_bstride, int64_t* dst_lengths_out);

/* ---- loudness: ITU-R BS.1770-4 meter (mono) and a gain to a target level (handle-free; kernels/loudness.hip) -------------
 * K-weighting at sampling rate fs: two biquads whose coefficients come from the bilinear forms below, in fp64 on the host
 * (bv2_loudness_coeffs; at 48 kHz they are the standard's table to 1e-15).
 *   stage 1, high shelf: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196; K = tan(pi f0 / fs), Vh = 10^(G/20),
 *     Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2; b = [Vh + Vb K/Q + K^2, 2 (K^2 - Vh), Vh - Vb K/Q + K^2] / a0,
 *     a = [1, 2 (K^2 - 1) / a0, (1 - K/Q + K^2) / a0];
 *   stage 2, high pass: f0 = 38.13547087602444, Q = 0.5003270373238773; b = [1, -2, 1], a as above with its own K and a0.
 * Blocks: step = round(fs / 10) samples, block = 4 step; block j of an item covers its samples [j step, j step + block), only whole blocks
 * count, and an item shorter than a block is ONE block of its own length.  z_j = mean square of the K-weighted samples of block j,
 * l_j = -0.691 + 10 log10 z_j.  Gating: the blocks with l_j > -70; of those, the blocks with l_j > -0.691 + 10 log10(mean z) - 10; the
 * integrated loudness is -0.691 + 10 log10(mean z of what is left).  No block above -70: the loudness is -inf and the group is flagged
 * BV2_LOUDNESS_SILENT.  Items that share a group id are the pieces of one programme: their blocks are pooled (blocks never span two items)
 * and the group gets one loudness and one gain.  groups == NULL: every item is its own group (n_groups == B).
 * Gain of a group: 10^((target_lufs - L) / 20); if peak * gain > 10^(peak_ceiling_db / 20), with peak the group's largest |sample|, the gain
 * is ceiling / peak and the group is flagged BV2_LOUDNESS_LIMITED (a static gain: nothing is distorted); a silent group gets gain 1.  The
 * gain is formed in fp64 on the device and rounded once to fp32.
 * Arithmetic: the recurrence and every energy sum are fp64; each sum has one fixed order that depends on the item's own samples only, so an
 * item's block mean squares (and an ungrouped item's lufs and gain) are the same bits alone and in any batch, at any row, batch stride or
 * S, and a group's numbers do not depend on the order of its items.  Samples at or behind lengths[b] are never loaded (the padding of a
 * batch may hold anything); int16 input is read as x / 32768.
 * Envelope: 8000 <= sample_rate <= 192000, 1 <= B <= 4096, 1 <= S < 2^31 - 4096.  Every argument is checked before anything touches the
 * device: -1 with a message in bv2_last_error(NULL) (the size queries a negative value), -5 for a null or short workspace.  The device
 * calls are asynchronous on `stream`, allocate nothing and do not sync (capture in a hipGraph has not been tested). */
enum { BV2_LOUDNESS_SILENT = 1, BV2_LOUDNESS_LIMITED = 2 };
typedef struct bv2_loudness_config {
  int32_t struct_bytes;            /* = sizeof(bv2_loudness_config) */
  int32_t sample_rate;
  int32_t input_format;            /* BV2_WAV_F32 / BV2_WAV_I16 */
} bv2_loudness_config;
/* HOST: step, block and tile (the samples one workgroup owns, counted from the item's first sample); each pointer may be NULL. */
int bv2_loudness_plan(const bv2_loudness_config* cfg, int32_t* step, int32_t* block, int32_t* tile);
/* HOST: b0 b1 b2 a1 a2 of stage 1, then of stage 2 (a0 = 1). */
int bv2_loudness_coeffs(const bv2_loudness_config* cfg, double out[10]);
/* HOST: blocks of an item of n samples: 0 for n = 0, 1 for n < block, else (n - block) / step + 1; negative for a bad config or n < 0. */
int64_t bv2_loudness_blocks(const bv2_loudness_config* cfg, int64_t n);
/* Bytes of DEVICE workspace of bv2_loudness_measure at (B, S); it covers bv2_loudness_gate at B as well. */
int64_t bv2_loudness_workspace_bytes(const bv2_loudness_config* cfg, int32_t B, int64_t S);
/* Four launches.  wav [B][wav_bstride] fp32 or int16 (DEVICE), item b's samples [0, lengths[b]) (lengths int64 [B] DEVICE, clamped to
 * [0, S]; NULL = S); groups int32 [B] DEVICE with values in [0, n_groups) — the CALLER guarantees the range (an item with another id
 * belongs to no group and its outputs are not written) — or NULL with n_groups == B.  Outputs, all DEVICE: lufs fp64 [n_groups], gain fp32
 * [n_groups], peak fp32 [B] (sample peak per item), flags int32 [n_groups], block_ms fp64 [B][bv2_loudness_blocks(S)] or NULL (z_j per
 * item; zeros behind the item's last block).  lufs, gain and flags all NULL: only peak and block_ms are produced (block_ms is then
 * required) — the first half of a measurement whose groups span several calls; bv2_loudness_gate is the second half. */
int bv2_loudness_measure(bv2_stream stream, const bv2_loudness_config* cfg, const void* wav, int64_t wav_bstride, const int64_t* lengths,
                         int32_t B, int64_t S, const int32_t* groups, int32_t n_groups, double target_lufs, double peak_ceiling_db,
                         double* lufs, float* gain, float* peak, int32_t* flags, double* block_ms, void* workspace,
                         int64_t workspace_bytes);
/* One launch: the gates and gains from block mean squares and peaks that bv2_loudness_measure produced, possibly in several calls:
 * block_ms [B][ms_bstride >= bv2_loudness_blocks(S)] and peak [B] are inputs, item b has bv2_loudness_blocks(lengths[b]) blocks. */
int bv2_loudness_gate(bv2_stream stream, const bv2_loudness_config* cfg, const double* block_ms, int64_t ms_bstride, const int64_t* lengths,
                      int32_t B, int64_t S, const float* peak, const int32_t* groups, int32_t n_groups, double target_lufs,
                      double peak_ceiling_db, double* lufs, float* gain, int32_t* flags, void* workspace, int64_t workspace_bytes);
/* One launch: dst[b][i] = src[b][i] * gain[groups ? groups[b] : b] for i < lengths[b] — ONE fp32 multiply — and zeros behind the length up
 * to S.  Exactly one of dst_f32 / dst_i16 is non-NULL; the 16-bit form is (int16) trunc(clamp(v * 32767.0f, -32768, 32767)) of the fp32
 * product v, bv2_emit's rule, no contraction into an FMA: given the gain, numpy reproduces both outputs bit for bit.  gain [n_groups]:
 * n_groups == B when groups is NULL; with groups it is the length of the gain table, which may exceed B (groups that span several calls;
 * an item whose id lies outside the table keeps gain 1).  B <= 65535; cfg gives the input format. */
int bv2_loudness_apply(bv2_stream stream, const bv2_loudness_config* cfg, const void* src, int64_t src_bstride, const int64_t* lengths,
                       int32_t B, int64_t S, const int32_t* groups, int32_t n_groups, const float* gain, float* dst_f32, int16_t* dst_i16,
                       int64_t dst_bstride);

/* ---- true peak (ITU-R BS.1770-4 annex 2; kernels/truepeak.hip) ---------------------------------------------------------------
 * The oversampling factor F follows the sampling rate: F = 4 below 96 000, F = 2 from 96 000 to below 192 000, F = 1 at 192 000 (true peak =
 * sample peak).  For F > 1 the interpolator is the project's own polyphase table for rate -> F rate: L = F, M = 1, c = 0.91, K = 36, 73 taps
 * per phase — bv2_resample_taps at that rate pair.  Item b's true peak is
 *   max( max_k |x_b[k]| , max_n |y_b[n]| ),
 * y_b EXACTLY the outputs bv2_resample produces for that rate pair: every output one fmaf chain over ascending jj from 0.f, fp32 table
 * values, samples outside [0, len_b) selected to zero and never loaded, int16 read as x / 32768 — so |y| here and there are the same bits,
 * alone and in any batch, at any row and batch stride.  The maximum with the sample peak is part of the definition (phase 0 of the table is
 * not the identity: its centre tap is 0.91), so true peak >= sample peak always.  The result is fp32 [B]; an item of length 0 gives 0.  The
 * oversampled signal is never written.
 * Non-finite input, as for the sample peak of bv2_loudness_measure: the maximum skips NaN operands (fmaxf), so a NaN sample and the outputs
 * it reaches do not count; an infinite sample gives +inf.
 * A workgroup owns BV2_TRUE_PEAK_TILE input samples of one item, counted from the item's first sample.  Envelope, argument checks before
 * anything touches the device and error codes are those of the loudness calls (cfg is a bv2_loudness_config); asynchronous on `stream`, no
 * allocation, no host sync, two launches. */
enum { BV2_TRUE_PEAK_TILE = 1024 };
/* HOST: F and K at cfg's sampling rate (K = 0 when F = 1); each pointer may be NULL. */
int bv2_true_peak_plan(const bv2_loudness_config* cfg, int32_t* factor, int32_t* K);
/* Bytes of DEVICE workspace of bv2_true_peak at (B, S): one fp32 per tile. */
int64_t bv2_true_peak_workspace_bytes(const bv2_loudness_config* cfg, int32_t B, int64_t S);
/* wav, wav_bstride, lengths, B, S as in bv2_loudness_measure; taps is the DEVICE copy of bv2_resample_taps(rate, F rate) — NULL when
 * F = 1; peak_out fp32 [B] DEVICE. */
int bv2_true_peak(bv2_stream stream, const bv2_loudness_config* cfg, const float* taps, const void* wav, int64_t wav_bstride,
                  const int64_t* lengths, int32_t B, int64_t S, float* peak_out, void* workspace, int64_t workspace_bytes);

/* ---- look-ahead true-peak limiter (kernels/limiter.hip) ------------------------------------------------------------------------
 * A static gain under a ceiling (bv2_loudness_gate, BV2_LOUDNESS_LIMITED) leaves a programme with one loud crest under its target.  The
 * limiter holds the ceiling with a gain CURVE instead: the item keeps its static gain g and only the crests are turned down.  The
 * definition is such that numpy restates it bit for bit.  All indices count from the item's first sample; nothing at or behind lengths[b]
 * is loaded.  F, K and the interpolation table are those of bv2_true_peak_plan.  Every fp32 operation below is ONE separately rounded
 * operation (multiply, add, subtract, IEEE division; nothing is contracted into an FMA), as in bv2_loudness_apply.
 *   g      the item's static gain, gain[groups ? groups[b] : b] as in bv2_loudness_apply (1 for an id outside the table)
 *   c      (float) 10^(ceiling_db / 20), formed in fp64 on the host and rounded once
 *   H      max(1, floor(lookahead_ms * rate / 2000 + 0.5));   P = max(H, floor(release_ms * rate / 2000 + 0.5))
 *   e[i]   max(|x[i]|, max_p |y[i F + p]|), y EXACTLY bv2_resample's outputs for rate -> F rate (bv2_true_peak's fmaf chains, the same
 *          bits); F = 1: e[i] = |x[i]|.  max_i e[i] is bv2_true_peak to the bit.
 *   r[i]   fminf(1, c / (e[i] * g)); r = 1 outside [0, len); e * g = 0 gives c / 0 = inf, hence 1
 *   m[j]   min r[t] over t in [j - H - 1, j + P + 1]                                       (the hold)
 *   d[j]   1 - m[j], and 0 outside [0, len)
 *   A[i]   sum_{k = -P..H} w[k] * d[i + k], accumulated from 0.f over ascending k, product and sum rounded separately
 *   s[i]   fminf(1 - A[i], fminf(r[i - 1], fminf(r[i], r[i + 1])))                         (the gain curve)
 *   out[i] (x[i] * g) * s[i] — bv2_loudness_apply's product times s — for i < len, zeros behind the length up to S; the 16-bit form is
 *          bv2_loudness_apply's rule applied to out
 * The window (bv2_limiter_window) is a half-Hann on either side of k = 0: u[k] = 0.5 + 0.5 cos(pi k / (H + 1)) for k >= 0,
 * 0.5 + 0.5 cos(pi k / (P + 1)) for k < 0, w = u / sum(u) in fp64, rounded once to fp32.  s[i] depends on r[i - H - P - 1 .. i + H + P + 1]:
 * that is the limiter's reach on either side, and H + P + 1 + K samples is the delay a streaming form would need.
 * What the definition gives:
 *   sample peak   every m[i + k], k in [-P, H], covers r[i - 1], r[i] and r[i + 1], so every d in the window of A[i] is at least
 *                 1 - min(r[i - 1], r[i], r[i + 1]) and, the weights summing to 1, s[i] <= r[i] in exact arithmetic; the last fminf makes it
 *                 hold after rounding too.  |out[i]| = |x g| s <= (e g)(c / (e g)) with three roundings: |out[i]| <= c (1 + 3 * 2^-24),
 *                 derived, not measured.
 *   pass-through  where no r within reach is below 1, d is exactly 0, A is exactly 0 and s is exactly 1.0f: an item that never reaches
 *                 the ceiling leaves as bv2_loudness_apply writes it, bit for bit.
 *   true peak     the output's TRUE peak is not bounded by construction — the gain moves between samples — it is measured
 *                 (docs/MEASUREMENTS.md, "Limiter"): the ceiling times 1.0000043 (0.00004 dB) at most on the inputs tried.
 *   invariance    an item's s and out depend on its own samples, g, c, H and P only: the same bits alone and in any batch, at any row,
 *                 batch stride or S.
 *   non-finite    as bv2_true_peak: the envelope's fmaxf skips a NaN operand; a NaN sample leaves as NaN.
 * Per item the call returns min_gain (fp32, the minimum of s over the item, 1 when nothing was limited) and limited_samples (int64, the
 * count of s < 1), both through integer atomics on slots the call itself initialises; optionally the curve s (fp32 [B][S], 1 behind the
 * length).  A workgroup owns BV2_LIMITER_TILE samples of an item and stages r over tile and reach in LDS: H + P <= BV2_LIMITER_MAX_REACH
 * (the defaults 3 ms / 60 ms at 192 kHz are 288 + 5760).  Envelope: 8000 <= sample_rate <= 192000, lookahead_ms and release_ms finite and
 * not negative, B <= 65535, S as in the loudness calls.  Anything outside is refused before the device is touched: -1 with a message in
 * bv2_last_error(NULL) (the size query a negative value), -5 for a null or short workspace. */
enum { BV2_LIMITER_TILE = 1024, BV2_LIMITER_MAX_REACH = 6144 };
typedef struct bv2_limiter_config {
  int32_t struct_bytes;            /* = sizeof(bv2_limiter_config) */
  int32_t sample_rate;
  int32_t input_format;            /* BV2_WAV_F32 / BV2_WAV_I16 */
  int32_t reserved;                /* 0 */
  double lookahead_ms, release_ms;
} bv2_limiter_config;
/* HOST: H, P, F and K (K = 0 when F = 1); each pointer may be NULL. */
int bv2_limiter_plan(const bv2_limiter_config* cfg, int32_t* H, int32_t* P, int32_t* factor, int32_t* K);
/* HOST: the window, out[k + P] = w[k] for k in [-P, H]: P + H + 1 floats. */
int bv2_limiter_window(const bv2_limiter_config* cfg, float* out);
/* Bytes of DEVICE workspace of bv2_limit at (B, S): r, one fp32 per sample, and one word per tile. */
int64_t bv2_limiter_workspace_bytes(const bv2_limiter_config* cfg, int32_t B, int64_t S);
/* Two launches on `stream`, no allocation, no host sync.  src, src_bstride, lengths, B, S, groups, n_groups, gain, dst_f32 / dst_i16 and
 * dst_bstride as in bv2_loudness_apply; taps is the DEVICE copy of bv2_resample_taps(rate, F rate) (NULL when F = 1) and window the DEVICE
 * copy of bv2_limiter_window.  curve fp32 [B][S] or NULL; min_gain fp32 [B] and limited_samples int64 [B], DEVICE, are required. */
int bv2_limit(bv2_stream stream, const bv2_limiter_config* cfg, const float* taps, const float* window, const void* src,
              int64_t src_bstride, const int64_t* lengths, int32_t B, int64_t S, const int32_t* groups, int32_t n_groups, const float* gain,
              double ceiling_db, float* dst_f32, int16_t* dst_i16, int64_t dst_bstride, float* curve, float* min_gain,
              int64_t* limited_samples, void* workspace, int64_t workspace_bytes);

/* ---- step energies, short-term loudness and loudness range (EBU Tech 3342; kernels/loudness.hip) --------------------------------
 * step_ss[b][k], k < steps(len_b) = len_b / step (whole steps only), is the sum of squares of the K-weighted samples [k step, (k + 1) step)
 * of item b, formed from the tiles' partial sums in tile order — the order the gate uses for a step.  For an item of at least one block,
 *   (((e_j + e_{j+1}) + e_{j+2}) + e_{j+3}) / block   is block_ms[j] BIT FOR BIT: it is the expression the gate evaluates.
 * Short-term block j of an item covers its steps [j, j + 30) (3 s every 100 ms), only whole blocks count: energy s_j = (the 30 step sums
 * added in ascending order) / (30 step), loudness -0.691 + 10 log10 s_j.  Blocks never span two items; a group pools the short-term blocks
 * of its items, as the integrated measurement pools its 400 ms blocks.  Gating (Tech 3342): the blocks above -70 LUFS; of those, the blocks
 * above (-0.691 + 10 log10 of their mean energy) - 20.  Of the n values left, sorted ascending r[0..n): lo = ((n - 1) 10 + 50) / 100,
 * hi = ((n - 1) 95 + 50) / 100 (integer division), LRA = 10 log10(r[hi] / r[lo]).  The selection is exact — r[lo] and r[hi] are the elements
 * a sort would return (a radix select over the bit patterns) — and all of it is fp64.  max_momentary is the maximum over the 400 ms
 * blocks formed from four whole steps.  flags: BV2_RANGE_SHORT when the group has no whole 3 s block, BV2_RANGE_SILENT when no short-term
 * block passes -70; with either, lra = 0 and the four LUFS outputs are -inf. */
enum { BV2_RANGE_SHORT = 1, BV2_RANGE_SILENT = 2 };
/* HOST: whole steps of an item of n samples, n / step; negative for a bad config or n outside [0, 2^31 - 4096]. */
int64_t bv2_loudness_steps_count(const bv2_loudness_config* cfg, int64_t n);
/* The measurement's three tile launches and one more that writes step_ss fp64 [B][ss_bstride >= bv2_loudness_steps_count(S)] (zeros behind
 * an item's whole steps).  peak fp32 [B] and block_ms fp64 [B][bv2_loudness_blocks(S)] may be NULL; if either is given, the launch that forms
 * them in bv2_loudness_measure runs too, and they are what that call returns.  Workspace: bv2_loudness_workspace_bytes(cfg, B, S). */
int bv2_loudness_steps(bv2_stream stream, const bv2_loudness_config* cfg, const void* wav, int64_t wav_bstride, const int64_t* lengths,
                       int32_t B, int64_t S, double* step_ss, int64_t ss_bstride, float* peak, double* block_ms, void* workspace,
                       int64_t workspace_bytes);
/* Bytes of DEVICE workspace of bv2_loudness_range at (B, S): the items' short-term energies. */
int64_t bv2_loudness_range_workspace_bytes(const bv2_loudness_config* cfg, int32_t B, int64_t S);
/* Two launches.  step_ss [B][ss_bstride >= bv2_loudness_steps_count(S)], lengths and groups (as in bv2_loudness_gate) are inputs, possibly
 * gathered from several bv2_loudness_steps calls.  Outputs, all DEVICE [n_groups]: lra, st_low, st_high (LUFS at the two percentiles),
 * max_short_term, max_momentary fp64; flags int32. */
int bv2_loudness_range(bv2_stream stream, const bv2_loudness_config* cfg, const double* step_ss, int64_t ss_bstride, const int64_t* lengths,
                       int32_t B, int64_t S, const int32_t* groups, int32_t n_groups, double* lra, double* st_low, double* st_high,
                       double* max_short_term, double* max_momentary, int32_t* flags, void* workspace, int64_t workspace_bytes);

/* ---- documents: sentences joined on the device with pauses, one buffer per document (handle-free; kernels/assemble.hip) --------
 * What the reference's callers do on the host after synthesis (webui.py tts_split / generate_audio, hiyoriUI.py:319-349): every piece
 * peak-normalised to 16 bit, a pause behind every sentence, a longer one behind every paragraph, everything concatenated.  tts_split
 * normalises each paragraph a second time, in fp64; a non-silent piece already peaks at +-32767, and trunc(k / 32767.0 * 32767.0) == k for
 * every integer k in [-32767, 32767], so that pass is the identity: the reference's document is each piece under its own peak by
 * bv2_pcm16's rule, with zero-filled pauses between (a paragraph of silent pieces only, 0 / 0 there, is zeros here).
 * The timeline is a caller-built table of SEGMENTS, a DEVICE array filled on the host and uploaded.  A segment is a PIECE (src != NULL:
 * the device address of its first fp32 sample; `length` the device address of an int64 counter, `hop` what multiplies it, `samples` the
 * cap — the row's S) or SILENCE (src == NULL: `samples` zeros; length must be NULL).  A piece has min(max(*length, 0) * hop, samples)
 * samples (length == NULL: `samples` of them): the counters are read on the device when the call runs, so a timeline is laid out without
 * the host ever knowing a length.  Every segment carries a level group and a document; document ids are non-decreasing along the table.
 * Three launches on `stream`, no allocation, no host sync:
 *   layout  offsets[i] = the start of segment i inside its document, totals[d] = the document's samples: an exclusive int64 scan per
 *           document, integer arithmetic (the same bits in any order); a document without segments has total 0;
 *   peaks   (the two peak modes only) max|x| per piece, or per level group over that group's pieces wherever they lie, as the bit
 *           pattern of a non-negative float under an integer max: the order of arrival does not matter;
 *   write   the grid runs over tiles of every document's CAPACITY (the host's upper bound: the sum of its caps and silences,
 *           bv2_assemble_plan); a tile at or behind totals[d] returns without storing.  A workgroup finds the first segment that
 *           reaches into its tile by binary search over the ends and walks from there; stores are 16 bytes per thread on the aligned body
 *           of the destination, the source is loaded as 16 bytes where it shares that phase and as dwords otherwise.  Samples at or
 *           behind totals[d] (and anything in front of dst_bases[d]) are NOT written; nor is anything at or behind capacity[d].
 * Value rules, x a piece's sample; each is reproducible in numpy bit for bit (IEEE fp32 division and multiplication, no contraction):
 *   BV2_LEVEL_PIECE_PEAK  pk = the piece's own max|x|:  fp32 x / pk,  16 bit (int16)(int)((x / pk) * 32767.f)       (bv2_pcm16's rule)
 *   BV2_LEVEL_GROUP_PEAK  the same with pk the peak of the piece's group (a paragraph or a document keeps its inner level differences)
 *   BV2_LEVEL_GAIN        v = x * gain[group], ONE fp32 multiply:  fp32 v,  16 bit trunc(clamp(v * 32767.0f, -32768, 32767))
 *                         (bv2_loudness_apply's rule); gain == NULL: gain 1
 *   BV2_LEVEL_NONE        BV2_LEVEL_GAIN with gain 1 (gain must be NULL)
 * A piece or group whose peak is 0 comes out as zeros.  NaN samples: not specified, as in bv2_pcm16.  The value of a sample depends on
 * the sample, its level and nothing else: not on the row, tensor, S or phase it is read from, nor on how groups are numbered.
 * Envelope: 1 <= n_segments <= 1 048 576, 1 <= n_groups <= n_segments, 1 <= n_docs <= 65 535, hop >= 1, 0 <= samples <= 2^40 per
 * segment (a piece: >= 1), a document's capacity <= 2^42; offsets and totals are int64.  Every argument is checked before anything
 * touches the device: -1 with a message in bv2_last_error(NULL), -5 for a null or short workspace.  What lives on the device cannot be
 * checked: the CALLER guarantees that dev_segments holds what bv2_assemble_plan saw and that dst_bases[d] has room for capacity[d] samples
 * of the output format (ids are clamped into range on the device, so a table that differs can misplace samples but not leave the arrays). */
enum { BV2_LEVEL_NONE = 0, BV2_LEVEL_PIECE_PEAK = 1, BV2_LEVEL_GROUP_PEAK = 2, BV2_LEVEL_GAIN = 3 };
typedef struct bv2_assemble_segment {
  const float* src;                /* a piece: DEVICE address of its first sample; NULL: silence */
  const int64_t* length;           /* a piece: DEVICE address of its int64 counter, or NULL (= samples); silence: NULL */
  int64_t samples;                 /* a piece: the cap (>= 1); silence: its length (>= 0) */
  int32_t hop;                     /* >= 1; multiplies the counter */
  int32_t group;                   /* level group, in [0, n_groups) */
  int32_t doc;                     /* document, in [0, n_docs), non-decreasing along the table */
  int32_t reserved;                /* 0 */
} bv2_assemble_segment;
typedef struct bv2_assemble_config {
  int32_t struct_bytes;            /* = sizeof(bv2_assemble_config) */
  int32_t output_format;           /* BV2_WAV_F32 / BV2_WAV_I16 */
  int32_t level;                   /* BV2_LEVEL_* */
  int32_t reserved;                /* 0 */
  int64_t max_capacity;            /* bv2_assemble only: the largest capacity[d] bv2_assemble_plan returned — the HOST's size of the grid */
} bv2_assemble_config;
/* HOST: validates the host copy of the table (ids in range, documents non-decreasing, hop >= 1, samples >= 0, a piece has src and a cap,
 * silence has no counter, reserved 0) and returns capacity[d] = the sum of document d's caps and silences (capacity [n_docs], HOST) and
 * the tile: the destination samples one workgroup owns, counted from the 16-byte boundary at or in front of dst_bases[d].  tile may be NULL. */
int bv2_assemble_plan(const bv2_assemble_config* cfg, const bv2_assemble_segment* host_segments, int32_t n_segments, int32_t n_groups,
                      int32_t n_docs, int64_t* capacity, int32_t* tile);
/* Bytes of DEVICE workspace of bv2_assemble. */
int64_t bv2_assemble_workspace_bytes(const bv2_assemble_config* cfg, int32_t n_segments, int32_t n_groups, int32_t n_docs);
/* dev_segments [n_segments], gain fp32 [n_groups] or NULL, dst_bases [n_docs] (one device pointer per document, fp32 or int16 by
 * cfg->output_format, any alignment of the element size), capacity int64 [n_docs] (the plan's), offsets int64 [n_segments] and totals
 * int64 [n_docs] (outputs): all DEVICE. */
int bv2_assemble(bv2_stream stream, const bv2_assemble_config* cfg, const bv2_assemble_segment* dev_segments, int32_t n_segments,
                 int32_t n_groups, int32_t n_docs, const float* gain, void* const* dst_bases, const int64_t* capacity, int64_t* offsets,
                 int64_t* totals, void* workspace, int64_t workspace_bytes);

/* ---- forced alignment: the reference's own aligner (handle-free; kernels/align.hip) --------------------------------------
 * SynthesizerTrn.forward() aligns a recording to its text with two steps that need no weights (models.py:960-991): the negative
 * cross-entropy between every latent frame z_p[:, y] of the recording and every symbol's prior N(m_p[:, x], exp(logs_p[:, x])), and
 * monotonic_align.maximum_path over that matrix.  The result — frames per symbol — is what bv2_decode_in.w_ceil takes in place of the
 * predicted durations (timing transfer), and a symbol-level time stamp for the recording.  m_p / logs_p / x_lengths come from phase A
 * (bv2_encode_out); z_p is the recording's latent in the prior's space: bv2_stage_flow_forward(bv2_posterior_encode(spectrogram)), both
 * above, or any latent the caller brings.
 *
 * bv2_neg_cent: neg_cent[b, y, x] = sum_d [ -1/2 log 2pi - logs_p[d, x] - 1/2 (z_p[d, y] - m_p[d, x])^2 exp(-2 logs_p[d, x]) ], formed
 * as the reference forms it (one matrix product over K = 2 inter with A rows [-1/2 z_p^2, z_p] and B columns [exp(-2 logs), m exp(-2 logs)]
 * plus two column constants, added in the reference's order) on v_mfma_f32_16x16x4_f32, exact fp32.  z_p [B, inter, Ty], m_p / logs_p
 * [B, inter, T], neg_cent [B, Ty, T], all DEVICE fp32 contiguous; x_lengths / y_lengths [B] int64 DEVICE or NULL (= T / Ty).  Cells outside
 * y < y_lengths[b], x < x_lengths[b] are written as 0 and their inputs are not read.  inter: a multiple of 4, at most 256.  The
 * noise-scaled-MAS perturbation (use_noise_scaled_mas, models.py:976-982; training only) is not implemented.
 *
 * bv2_maximum_path: monotonic_align/core.py maximum_path_jit on the device, one launch, one workgroup per item: the band
 * max(0, t_x + y - t_y) <= x < min(t_x, y + 1), the -1e9 stand-ins (0 for the cell (0, 0)), plain fp32 add and max — bit for bit the fp32
 * dynamic programme, whatever the shape — and the reference's tie rule on the way back (a step to x - 1 only when x == y or the left
 * predecessor is STRICTLY greater).  neg_cent is only read: instead of the cumulative matrix the forward pass records one decision bit
 * per cell in the workspace (bv2_maximum_path_workspace_bytes: Ty * ceil(T / 64) * 8 bytes per item), and the walk back reads those from
 * on-chip memory.  durations [B, T] int64 = frames per symbol (0 at and past x_lengths[b]); attn [B, 1, Ty, T] fp32 one-hot path or NULL;
 * score [B] fp32 = the path's cumulative value or NULL.  T <= 4096.  Precondition: 1 <= x_lengths[b] <= y_lengths[b] (the reference's
 * band is empty otherwise; the values live on the device, so the CALLER checks — out-of-range lengths are clamped to [0, T] / [0, Ty] and
 * cannot make the kernel leave its arrays, but the durations of such an item mean nothing).
 * Both calls: asynchronous on `stream`, no allocation, no host sync, graph-capturable; a failed call returns non-zero (the size query a
 * negative value) with its message in bv2_last_error(NULL), every argument checked before anything touches the device. */
int bv2_neg_cent(bv2_stream stream, int32_t B, int32_t inter, int32_t T, int32_t Ty, const float* z_p, const float* m_p,
                 const float* logs_p, const int64_t* x_lengths, const int64_t* y_lengths, float* neg_cent);
/* bv2_align: the whole aligner in one call — phase A's m_p / logs_p [B, inter, T] and x_lengths (bv2_encode_out; x_lengths as given to
 * phase A) plus the recording's spectrogram y [B, spec_channels, Ty] and y_lengths -> durations [B, T] (attn, score optional as above):
 * bv2_posterior_encode (noise_q NULL = deterministic), bv2_stage_flow_forward, bv2_neg_cent, bv2_maximum_path on one workspace
 * (bv2_align_workspace_bytes).  Needs both blobs attached.  The same preconditions as the four calls. */
int64_t bv2_align_workspace_bytes(const bv2_handle* h, int B, int T, int Ty);
int bv2_align(bv2_handle* h, bv2_stream stream, int B, int T, int Ty, const float* m_p, const float* logs_p, const int64_t* x_lengths,
              const float* y, const int64_t* y_lengths, const float* g, const float* noise_q, int64_t* durations, float* attn,
              float* score, void* workspace, int64_t workspace_bytes);

/* ---- per-utterance noise seeds -----------------------------------------------------------------------------------------------
 * bv2_set_noise_seeds: seeds_dev [B] DEVICE int64, one per batch item; NULL (B ignored) switches it off.  Until switched off every
 * later call on this handle takes its N(0,1) numbers from a counter-based generator instead of a noise tensor — bv2_encode_durations*
 * (noise_w), bv2_decode*, bv2_infer*, bv2_stream_begin (noise_z), bv2_posterior_encode, bv2_align (noise_q) and the graph captures —
 * computed inside the kernels that consume them.  The value at (seed, draw, row, frame) is a pure function of those four numbers
 * (Philox4x32-10 keyed by the seed, counter (frame, row >> 2, draw, 0), Box-Muller; DESIGN.md "Seeded noise"): it does not depend
 * on the batch, the item's row in it, T, T_y, its bucket or the handle.  Frames of the prior draw at or past y_lengths[b] are 0.
 * The noise pointers may then be NULL; a non-NULL noise_w / noise_z / noise_q together with active seeds is an error, and so is a call
 * whose B differs from the seeds' B.  The array is read when a call RUNS: a captured graph reads it at every replay (a moving input,
 * like the bv2_item_controls arrays), and it must stay valid until the work that reads it has finished.  Without seeds every call
 * behaves exactly as before.  The setting belongs to the handle.
 * bv2_seeded_noise: the same values as a tensor — out[b * bstride + r * rstride + t * tstride] = value(seeds[b], which, r, t) for
 * r < rows, t < T; which: 0 = noise_w, 1 = noise_z, 2 = noise_q; lengths_dev [B] or NULL: frames at or past lengths[b] are written
 * as 0.  Asynchronous on `stream`, graph-capturable, no handle (errors: bv2_last_error(NULL)). */
int bv2_set_noise_seeds(bv2_handle* h, const int64_t* seeds_dev, int32_t B);
int bv2_seeded_noise(bv2_stream stream, const int64_t* seeds_dev, int32_t B, int32_t which, int32_t rows, int32_t T,
                     const int64_t* lengths_dev, float* out, int64_t bstride, int64_t rstride, int64_t tstride);

int64_t bv2_maximum_path_workspace_bytes(int32_t B, int32_t T, int32_t Ty);
int bv2_maximum_path(bv2_stream stream, int32_t B, int32_t T, int32_t Ty, const float* neg_cent, const int64_t* x_lengths,
                     const int64_t* y_lengths, int64_t* durations, float* attn, float* score, void* workspace, int64_t workspace_bytes);

/* ---- the posterior encoder enc_q (PosteriorEncoder, models.py:448-487): a recording's spectrogram -> its posterior latent z ----------
 * enc_q is not part of inference, release checkpoints are stripped of it (compress_model.py), and the packed inference blob is pinned by
 * size and hash — so its weights live in a SECOND, optional blob of their own: pre (Conv1d spec_channels -> hidden, k = 1), enc (WN: hidden,
 * k = 5, dilation 1, 16 layers, cond_layer from gin_channels; weight_g / weight_v pairs or folded weights, as everywhere) and proj
 * (hidden -> 2 inter).  bv2_load_tensor keeps ignoring enc_q.* (returns 1); bv2_posterior_load_tensor takes exactly those keys (others: 1).
 * spec_channels is given where the blob is sized, packed and attached — 1025, 513 or 80, also for a model with a speaker table, whose
 * bv2_config does not carry it; bv2_create's validation is untouched.  Pack on the host, upload, attach; bv2_posterior_detach forgets the
 * blob.  Nothing here changes bv2_packed_bytes, the inference blob or its header.
 *
 * bv2_posterior_encode: y [B, spec_channels, Ty] fp32 dense (the linear spectrogram, e.g. bv2_spectrogram's output made contiguous),
 * y_lengths [B] int64, g [B, gin] ->
 *   x = pre(y) * mask;  x = WN(x, mask, g);  stats = proj(x) * mask;  m_q, logs_q = split(stats);
 *   z = (m_q + noise_q * exp(logs_q) * noise_scale_q) * mask                                                    (models.py:479-487)
 * noise_q [B, inter, Ty] is the caller's N(0, 1) draw (the RNG contract of noise_w / noise_z; the reference scales by 1); NULL gives the
 * deterministic z = m_q * mask.  z [B, inter, Ty] is required; m_q, logs_q [B, inter, Ty] and y_mask [B, Ty] may be NULL.  Exact fp32 on
 * the launch forms of the residual flow's WN (in_layer + gate, res_skip) and conv1d_mfma; an odd spec_channels rides on the padded K range
 * of pre (rows >= spec_channels read as zero).  37 launches, asynchronous on `stream`, no allocation; not meant for graph capture.  Fails
 * with -8 and a message naming compress_model.py while no posterior blob is attached.  Workspace: bv2_posterior_workspace_bytes(h, B, Ty). */
int64_t bv2_posterior_packed_bytes(bv2_handle* h, int spec_channels);
int bv2_posterior_load_tensor(bv2_handle* h, const char* ref_key, const void* host_ptr, const int64_t* shape, int ndim, int dtype);
int bv2_posterior_pack(bv2_handle* h, int spec_channels, void* host_blob, int64_t bytes);
int bv2_posterior_attach(bv2_handle* h, int spec_channels, const void* dev_blob, int64_t bytes);
int bv2_posterior_detach(bv2_handle* h);
int64_t bv2_posterior_workspace_bytes(const bv2_handle* h, int B, int Ty);
int bv2_posterior_encode(bv2_handle* h, bv2_stream stream, int B, int Ty, const float* y, const int64_t* y_lengths, const float* g,
                         const float* noise_q, float noise_scale_q, float* z, float* m_q, float* logs_q, float* y_mask,
                         void* workspace, int64_t workspace_bytes);

/* ---- scoring a take against its text: the duration likelihood and the KL term of SynthesizerTrn.forward() -------------------------
 * forward() computes two quantities that say how well the model explains a recording (models.py:993, losses.py:45-61): the negative
 * log-likelihood of the aligned durations under the StochasticDurationPredictor run FORWARD, and the KL between the recording's posterior
 * and the text's prior along the path.  Every term of both is a per-position sum, so both come back decomposed: per symbol and per frame.
 *
 * Weights.  The forward predictor needs what inference drops: sdp.post_pre / post_convs / post_proj / post_flows.* and the ConvFlow
 * sdp.flows.1.  They live in a THIRD, optional blob, handled exactly like the posterior encoder's: bv2_load_tensor keeps ignoring them
 * (returns 1), bv2_sdp_forward_load_tensor takes exactly those keys (others: 1); pack on the host, upload, attach; detach forgets the blob.
 * Nothing here changes bv2_packed_bytes, the inference blob, the posterior blob or their headers.  hidden_channels must be 128, 192 or 256.
 *
 * bv2_duration_nll: x [B, hidden, T] and x_mask [B, T] of phase A (bv2_encode_out), w [B, T] fp32 frames per symbol (bv2_align's durations
 * or a caller's; 0 past x_lengths), g [B, gin] -> nll_sym [B, T], nll [B] = sdp(x, x_mask, w, g) of models.py:197-244, that is nll + logq.
 * nll_sym is the exact decomposition (every term of the reference's sums over [1, 2] at its position; 0 at masked positions), nll[b] the
 * sum of row b in a fixed order (lane l of one wave adds positions l, l + 64, ... in sequence, then a butterfly over xor 32 .. 1; fp64 accumulators, rounded to fp32 once): it
 * depends neither on a tiling nor on the item's batch neighbours, and no floating-point atomic is used.  noise_e [B, 2, T] is the caller's
 * N(0, 1) draw e_q of models.py:214-217; NULL takes it from the seeds of bv2_set_noise_seeds as draw 3 (RNG_NOISE_E; the draws 0-2 and
 * their values are untouched; bv2_seeded_noise keeps offering 0-2 only) and is an error without seeds.  Always fp32.  35 launches (the
 * trunk's five are phase A's), asynchronous on `stream`, no allocation.  -1 for a bad argument, -5 for a null or short workspace
 * (bv2_duration_nll_workspace_bytes), -8 while a blob is missing; every argument is checked before anything touches the device.
 *
 * bv2_kl_path (no handle; errors in bv2_last_error(NULL)): z_p, logs_q [B, inter, Ty], m_p, logs_p [B, inter, T], w_ceil [B, T] fp32
 * frames per symbol, x_lengths / y_lengths [B] int64 DEVICE or NULL (= T / Ty) ->
 *   kl_frame[b, j] = sum_c (logs_p[c, s] - logs_q[c, j] - 0.5 + 0.5 (z_p[c, j] - m_p[c, s])^2 exp(-2 logs_p[c, s]))   for j < y_lengths[b], else 0
 * with s the symbol whose duration interval holds frame j (a gather, as the length regulator's; frames past the durations' sum take the
 * last symbol), channel c added into fp64 accumulator c & 3, and kl[b] the fixed-order sum of row b (as nll).  The reference's kl_loss is
 * sum(kl) / sum(y_lengths), formed by the caller.  T <= 4096.  Two launches. */
int64_t bv2_sdp_forward_packed_bytes(bv2_handle* h);
int bv2_sdp_forward_load_tensor(bv2_handle* h, const char* ref_key, const void* host_ptr, const int64_t* shape, int ndim, int dtype);
int bv2_sdp_forward_pack(bv2_handle* h, void* host_blob, int64_t bytes);
int bv2_sdp_forward_attach(bv2_handle* h, const void* dev_blob, int64_t bytes);
int bv2_sdp_forward_detach(bv2_handle* h);
int64_t bv2_duration_nll_workspace_bytes(const bv2_handle* h, int B, int T);
int bv2_duration_nll(bv2_handle* h, bv2_stream stream, int B, int T, const float* x, const float* x_mask, const float* w, const float* g,
                     const float* noise_e, float* nll_sym, float* nll, void* workspace, int64_t workspace_bytes);
int bv2_kl_path(bv2_stream stream, int32_t B, int32_t inter, int32_t T, int32_t Ty, const float* z_p, const float* logs_q, const float* m_p,
                const float* logs_p, const float* w_ceil, const int64_t* x_lengths, const int64_t* y_lengths, float* kl_frame, float* kl);

/* ---- hipGraph capture (BASELINE config 3: "hipGraph-captured decode") ----------------------------------------- */
/* Both phases are fixed launch sequences on the caller's stream with no allocation, host sync or device->host copy,
 * so they can be recorded once and replayed: bv2_graph_capture_* puts `stream` (which must NOT be the legacy default
 * stream) into capture mode, records the phase exactly as bv2_encode_durations / bv2_decode would launch it, and
 * instantiates an executable graph.  The graph bakes in every pointer and scalar of in/out/workspace: the caller keeps
 * those buffers alive and at the same addresses (refill the inputs in place before each replay) and re-captures when a
 * shape (B, T, Ty, max_len), a scalar argument or a dtype switch changes (per-utterance controls are arrays: _ex below).  bv2_graph_launch replays on any stream.
 * Taps and profiling must be off while capturing. */
typedef struct bv2_graph bv2_graph;
int bv2_graph_capture_encode(bv2_handle* h, bv2_stream stream, const bv2_encode_in* in, const bv2_encode_out* out,
                             void* workspace, int64_t workspace_bytes, bv2_graph** graph);
int bv2_graph_capture_decode(bv2_handle* h, bv2_stream stream, const bv2_decode_in* in, const bv2_decode_out* out,
                             void* workspace, int64_t workspace_bytes, bv2_graph** graph);
/* the same with per-utterance controls (see bv2_item_controls): the graph reads the control arrays at replay time */
int bv2_graph_capture_encode_ex(bv2_handle* h, bv2_stream stream, const bv2_encode_in* in, const bv2_encode_out* out,
                                const bv2_item_controls* controls, void* workspace, int64_t workspace_bytes, bv2_graph** graph);
int bv2_graph_capture_decode_ex(bv2_handle* h, bv2_stream stream, const bv2_decode_in* in, const bv2_decode_out* out,
                                const bv2_item_controls* controls, void* workspace, int64_t workspace_bytes, bv2_graph** graph);
/* phase A on a caller's g (see bv2_encode_durations_g): the graph reads g at replay time */
int bv2_graph_capture_encode_g(bv2_handle* h, bv2_stream stream, const bv2_encode_in* in, const bv2_encode_out* out,
                               const bv2_item_controls* controls, const float* g, void* workspace, int64_t workspace_bytes,
                               bv2_graph** graph);
int bv2_graph_launch(bv2_graph* graph, bv2_stream stream);
int bv2_graph_num_nodes(const bv2_graph* graph);
void bv2_graph_destroy(bv2_graph* graph);

/* ---- debugging / measurement ------------------------------------------------------------------------------ */
/* Kernel-selection switches, for tests that hold the fused kernels to the layer-wise ones (default 1 = fused):
 *   "fused_resblock"  the narrow Generator stages as whole-ResBlock / fused-pair kernels (0: one conv per launch; in bf16 mode this
 *                     also takes the C = 32 stage off the pair kernel, i.e. 0 = every narrow stage layer-wise)
 *   "conv_x6"         the ResBlock convs of the fp32 Generator stages with C >= 32 on the bf16 matrix core: operands split exactly
 *                     into three bf16 planes, six cross products accumulated in fp32 — fp32 accuracy (dropped terms < 2^-23 of a
 *                     product) at 6/16 of the fp32-MFMA time (kernels/conv_x6.hip).  0: v_mfma_f32_32x32x2_f32 (conv_mfma.hip)
 *   "conv_x3"         those convs (layer-wise at C % 128 == 0, and the pair kernel of the narrower stages) on the TWO-plane fp16 form:
 *                     operands scaled by powers of two into fp16's range and split into two fp16 halves, three cross products — the
 *                     same order of error (dropped term <= 2^-24 of a product) at half the matrix work.  The activation scale comes
 *                     from the data: max |x| of the whole input tensor, published by the launch that wrote it (layer-wise form), or of
 *                     the workgroup's own tile (pair kernel), so an element more than 2^15 below that maximum keeps an absolute, not a
 *                     relative, error (2^-40 of the maximum), and a non-finite input leaves the whole tensor non-finite or zero.
 *                     0: the three-plane bf16 form above (exact splits, fp32's exponent range)
 *   "conv_x6_c32"     also the C = 32 stage layer-wise on conv_x6.hip (two launches per ResBlock pair, 44.6 us each at batch 1) instead
 *                     of the fused fp32-MFMA pair kernel (one launch, 110 us); 0: resblock_fused.hip.  Only consulted when the C = 32
 *                     stage is NOT on the split-bf16 pair kernel, i.e. together with "x6_pair" = 0 (the default runs respair_x6.hip there)
 *   "fused_respair"   the wide bf16 Generator stages (C = 64 / 128 / 256) one (dilated conv, conv) ResBlock pair per launch, the
 *                     intermediate in LDS (kernels/respair_cl_bf16.hip; bit-identical to the layer-wise path); 0: one conv per launch
 *   "respair_c32"     1 (default): also the C = 32 stage pair by pair (one wave owns all channels); 0: whole-ResBlock launches
 *   "f16_kv"          1 (default): in the fp16 Encoder stacks the fused q/k/v projection writes K (channels-last) and V (channel-major) as fp16 in the
 *                     layouts the attention kernel's matrix products consume (kernels/attention.hip KV16: 6 loads of 16 B per key tile instead of 48
 *                     dword loads + conversions, 80 fewer registers); 0: fp32 rows, rounded to fp16 in the attention kernel's registers.  Same fp16
 *                     values either way; measured -0.6 us per attention launch at B = 32 and nothing on the projection (profiles/r06_fam_f16_kv.txt)
 *   "f16_wn"          tile tuning of the fp16 Encoder convs (0 = the launcher's choice): waves per workgroup (4 / 6 / 8, taken when it wastes no more wave
 *                     slots than the default).  Measured round 6 (profiles/r06_ab_f16_tiles.txt): four-wave workgroups for the FFN conv_1 at B = 32
 *                     give 14.56 vs 14.62 ms — inside the spread, default unchanged
 *   "f16_ni"          the same for the time steps per workgroup (2 = 64, 4 = 128; 0 = the launcher's choice)
 *   "stage_sum"       0 (default, measured: no gain — what the consumers save the producers lose, see bv2_internal.h); 1: the launch that finishes a bf16 Generator stage's ResBlocks (the last pair launch of the wide stages, the whole-ResBlock
 *                     launch at C = 16) runs the stage's n branches tile by tile in one workgroup and writes ONE tensor — the branch mean of reference
 *                     models.py:545-552 (`xs / self.num_kernels`) — so the next ConvTranspose1d / conv_post reads one tensor instead of n; 0: n
 *                     tensors, the consumer forms the mean.  Same rounding points either way (kernels/cl_bf16.h stage_mean): bit-identical results
 *   "resblock_c16"    1 (default): the C = 16 bf16 stage's whole-ResBlock launch on v_mfma_f32_16x16x32_bf16 (two taps x 16 channels per
 *                     instruction, unpadded 32-byte LDS rows, two workgroups per CU: kernels/resblock_c16_bf16.hip); 0: the 32x32x16
 *                     whole-ResBlock kernel (resblock_cl_bf16.hip), whose MFMA block is half zero padding at this width
 *   "f16_fused_ln"    1 (default): in the fp16 Encoder stacks LayerNorm-1 runs in conv_o's epilogue and every LayerNorm-2 but the stack's last (with the speaker add of the
 *                     conditioning layer where it follows) in the FFN conv_2's — the workgroup owns all 192 channels of
 *                     its columns (kernels/enc_f16.hip); 0: LayerNorm launches of their own (layernorm.hip)
 *   "f16_ksplit"      1 (default): the fp16 Encoder stacks' FFN conv_2 (C_in = 768 -> 192 rows) on 64-column tiles splits K inside the workgroup:
 *                     the whole 768-channel tile staged once, 12 waves = 6 output tiles x 2 channel halves, partial sums merged through LDS
 *                     (kernels/enc_f16.hip); 0: 6 waves over three staged 256-channel chunks.  Same products, another fp32 summation order
 *   "conv_post_rows"  1 (default): the bf16 path's conv_post + tanh at C = 16, k = 7 row-wise (a thread owns one 32-byte input row per branch, K floats
 *                     per thread through LDS); 0: the any-width kernel (C*K scalar LDS reads per output sample).  fp32 arithmetic in both
 *   "ups_phase_taps"  1 (default): a bf16 ConvTranspose1d launch (one conv with C_out' = u*C_out over the union of the phases' tap windows) runs,
 *                     per wave, only the window taps of the phases its output channels belong to — the zero weights that pad the other
 *                     phases' taps are stepped over (1/3 of the matrix work at k = 2u); 0: every tap of the window (same results)
 *   "prefetch"        default 0 (measured: within noise at config 2 — the batch-1 launches do not wait for their weights; the BERT extractor,
 *                     where it is worth 0.6 %, has it on: bv2_bert_set_option).  Batch 1 (small-N regime): bit 0 — a LayerNorm launch carries the NEXT launch's weight stream (FFN conv_1 behind
 *                     LayerNorm-1, the next layer's q/k/v projection behind LayerNorm-2), bit 1 — a split-K conv launch does (conv_2 behind
 *                     conv_1): 128 spare workgroups touch it line by line into the L2 of the XCD whose workgroups will read it
 *                     (bv2_kernels.h Prefetch).  0: every launch fetches its own weights from HBM / the Infinity Cache when it starts
 *   "xcd_affine"      1 (default): in the fp16 Encoder stacks at batch 8, 16, 24 and any batch >= 32 (B >= 8 && (B % 8 == 0 || B >= 32): the batch fills the eight XCDs about evenly), batch item b runs on XCD b % 8 in EVERY kernel of a layer (q/k/v,
 *                     attention, conv_o, LayerNorms, FFN convs), so a layer's tensors are handed on inside one XCD's L2 (the eight L2s are
 *                     not coherent with each other); 0: plain grids
 *   "respair_form"    1 (default): 64-channel x 128-row wave tiles on the XOR-swizzled tile; 0: 32-channel waves on the padded tile
 *   "respair_mix"     1 (default): the k = 11 / 7 / 3 branches of a pair launch interleaved in dispatch order; 0: branch after branch
 *   "fused_dds"       one launch per DDSConv layer incl. the projection / spline that follows (0: 3 launches per layer)
 *   "x6_pair"         fp32 mode, the C = 64 / 32 / 16 Generator stages one (dilated conv, conv) ResBlock pair per launch with both convs on
 *                     the bf16 matrix core and the intermediate planes in LDS (kernels/respair_x6.hip; bit-identical to the two conv_x6
 *                     launches); 0: two launches per pair
 *   "x6_pair_c64"     1 (default); 0: "x6_pair" without the C = 64 stage
 *   "x6_pair_c16"     1 (default); 0: "x6_pair" without the C = 16 stage (back on resblock_fused.hip)
 *   "x6_pair_c128"    0 (default); 1: "x6_pair" also on the C = 128 stage (one 8-wave workgroup per CU: measured, no gain)
 *   "fused_boundary"  transformer flow, small-batch fp32 regime: LayerNorm-2 of a coupling's last Encoder layer, its `post` and the next
 *                     coupling's `pre` in one launch (kernels/flow_boundary.hip); 0: three launches
 *   "fused_attn_o"    MultiHeadAttention.conv_o inside the attention kernel in the small-batch fp32 regime: head h writes partial
 *                     slab h, the LayerNorm sums the slabs (0: conv_o as its own launch)
 *   "attn_ksplit"     -1 (default): the key ranges per (head, query tile) of the fused attention are picked per shape (2 or 4 at batch 1 and long
 *                     sequences: each range's workgroup writes its own partial slab, LayerNorm-1 merges them with the flash-decoding weights);
 *                     0 / 1: no key split; 2 / 4: that many ranges where the slabs allow it
 *   "attn_qtile"      0 (default): the queries per workgroup of the fp32 attention are picked per shape — 16 (the 16x16x4 matrix form) where
 *                     32-query tiles would leave at least half of the compute units without a workgroup, else 32; 16 / 32: that tile for
 *                     every fp32 attention launch (the fp16 forms always use 32)
 *   "overlap_dp"      default 0: 1 runs the DurationPredictor on an internal side stream beside the stochastic one (fork / join
 *                     with events on the caller's stream; measured slower at batch 1, kept for experiments)
 *   "lean_durations"  default 1: phase A runs only the duration predictor the mix can see (bv2_encode_out); 0: both, always
 *   "phase_b_front"   default 1: the head of phase B (length regulation, prior sampling, attn path, speaker GEMVs, the fp32 Generator's
 *                     x3 slot words) is one launch; 0: five launches.  Bit-identical either way
 *   "kernarg_head"    default 1: the launches of the batch-1 chain — one-problem split-K convs, mode-0 LayerNorms, the fp32 attention with the
 *                     fused conv_o, the flow boundary — pass what a workgroup needs for its first global loads as leading scalar kernel
 *                     arguments (preloaded into SGPRs at wave launch) in front of the argument struct; 0: the generic kernels (struct
 *                     first).  Bit-identical either way
 * Captured graphs keep whatever was selected when they were recorded. */
int bv2_set_option(bv2_handle* h, const char* key, int value);

/* Ask the executor to copy a named intermediate (e.g. "dec.ups.0", "dec.stage.2", "flow.3.h", "enc.layer.1")
 * into dev_dst (capacity in floats) the next time it is produced.  name==NULL clears all taps. */
int bv2_set_tap(bv2_handle* h, const char* name, float* dev_dst, int64_t capacity_floats);

/* Per-kernel-family timing with HIP events recorded on the caller's stream (bench.py's roofline leg). */
typedef struct bv2_profile_row {
  char name[96];          /* kernel family, e.g. "conv1d_mfma<128x128>" (mode 3: "site|family shape") */
  int64_t launches;
  double total_ms;        /* sum of event-timed durations */
  double flops;           /* algorithmic FLOPs (2*MAC) over those launches */
  double bytes;           /* algorithmic bytes (inputs read once + outputs written once + weights) */
} bv2_profile_row;
int bv2_profile_enable(bv2_handle* h, int on);          /* 0 off, 1 every MFMA kernel launch, 2 Generator launches only,
                                                            3 every MFMA launch with one row per launch site and shape,
                                                            4 the Generator's ConvTranspose1d ("dec.ups") launches only, one row each */
int bv2_profile_reset(bv2_handle* h);
/* Synchronises the recorded events and aggregates them; returns the number of rows written (<= max_rows). */
int bv2_profile_report(bv2_handle* h, bv2_profile_row* rows, int max_rows);

#ifdef __cplusplus
}
#endif
#endif /* BV2_H */
