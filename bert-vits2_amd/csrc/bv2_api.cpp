// bv2_api.cpp — the extern "C" surface declared in include/bv2.h.
#include <cmath>
#include <cstddef>
#include <cstring>
#include <functional>
#include <new>

#include "bv2_internal.h"
#include "bv2_pack.h"

using namespace bv2;

static thread_local std::string g_create_err;

#define BV2_TRY try {
#define BV2_CATCH(h_)                                                                  \
  } catch (const std::exception& e) {                                                  \
    if (h_) (h_)->err = std::string("exception: ") + e.what();                         \
    return -100;                                                                       \
  } catch (...) {                                                                      \
    if (h_) (h_)->err = "unknown exception";                                           \
    return -100;                                                                       \
  }

extern "C" {

int bv2_abi_version(void) { return BV2_ABI_VERSION; }

int bv2_create(const bv2_config* cfg, bv2_handle** out) {
  if (!cfg || !out) { g_create_err = "bv2_create: null argument"; return -1; }
  bv2_handle* h = nullptr;
  try {
    h = new bv2_handle();
    std::memset(&h->model.cfg, 0, sizeof(bv2_config));
    // the struct grew by one trailing field twice (resblock_type, round 5; spec_channels with the ReferenceEncoder): the shorter forms are
    // still accepted — no resblock_type means ResBlock1, no spec_channels is legal for a model with a speaker table
    const int32_t old_bytes = (int32_t)offsetof(bv2_config, resblock_type), mid_bytes = (int32_t)offsetof(bv2_config, spec_channels);
    if (cfg->struct_bytes != (int32_t)sizeof(bv2_config) && cfg->struct_bytes != mid_bytes && cfg->struct_bytes != old_bytes) {
      g_create_err = "bv2_create: bv2_config.struct_bytes mismatch (ABI drift)";
      delete h;
      return -1;
    }
    std::memcpy(&h->model.cfg, cfg, (size_t)cfg->struct_bytes);
    h->model.cfg.struct_bytes = (int32_t)sizeof(bv2_config);
    if (h->model.cfg.resblock_type == 0) h->model.cfg.resblock_type = 1;
    if (h->model.cfg.n_speakers == 0 && cfg->struct_bytes != (int32_t)sizeof(bv2_config)) {
      g_create_err = "bv2_create: n_speakers == 0 needs bv2_config.spec_channels (this bv2_config is the shorter, older struct)";
      delete h;
      return -1;
    }
    if (h->model.cfg.n_speakers >= 1) h->model.cfg.spec_channels = 0;     // not read: the layout and the blob do not depend on it
    std::string err;
    if (int rc = build_layout(h->model, h->blob[kInference], err)) {
      g_create_err = "bv2_create: " + err;
      delete h;
      return rc;
    }
  } catch (...) {
    delete h;
    g_create_err = "bv2_create: out of memory";
    return -100;
  }
  *out = h;
  return 0;
}

void bv2_destroy(bv2_handle* h) {
  if (!h) return;
  for (auto& r : h->prof_pool) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->side_stream) (void)hipStreamDestroy(h->side_stream);
  delete h;
}

const char* bv2_last_error(const bv2_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

// ---- the packed weight blobs: the inference blob, the posterior encoder's (enc_q.*) and the forward duration predictor's (sdp.post_*,
// sdp.flows.1.*).  Each is its own allocation with its own header; they share one lifecycle — host tensors in, size, pack, attach, detach —
// written once below for a BlobKind (bv2_internal.h kBlobDesc); the exported entry points name the kind and themselves.
// The inference layout is bv2_create's; the posterior's is built once spec_channels is known (and again, dropping the attached blob, when
// it changes), the forward duration predictor's on first use.
static int blob_layout(bv2_handle* h, BlobKind k, int spec_channels, const char* what) {
  WeightBlob& b = h->blob[k];
  std::string e;
  int rc = 0;
  if (k == kPosterior && !(h->post.spec == spec_channels && b.total_floats > 0)) {
    rc = build_posterior_layout(h->model.cfg, spec_channels, h->post, b, e);
    if (!rc) b.dev = nullptr;          // a blob attached for another width no longer fits
  } else if (k == kSdpForward && b.total_floats == 0) {
    rc = build_sdp_forward_layout(h->model.cfg, h->sdpf, b, e);
  }
  if (rc) h->err = std::string(what) + ": " + e;
  return rc;
}

static int blob_load_tensor(bv2_handle* h, BlobKind k, const char* what, const char* key, const void* host_ptr, const int64_t* shape,
                            int ndim, int dtype) {
  if (!h) return -1;
  BV2_TRY
  if (!key || !host_ptr || ndim < 0 || ndim > 8 || (ndim && !shape)) { h->err = std::string(what) + ": bad argument"; return -1; }
  if (!kBlobDesc[k].mine(key)) return 1;           // another blob's tensor (the inference blob: enc_q.*, sdp.post_*, sdp.flows.1.*): ignored
  HostTensor t;
  int64_t n = 1;
  for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= shape[i]; }
  t.data.resize((size_t)n);
  if (dtype == BV2_F32) std::memcpy(t.data.data(), host_ptr, sizeof(float) * (size_t)n);
  else if (dtype == BV2_F16) {             // compress_model.py:49-53 "release" checkpoints are .half()
    const uint16_t* s = static_cast<const uint16_t*>(host_ptr);
    for (int64_t i = 0; i < n; ++i) t.data[(size_t)i] = h2f(s[i]);
  } else if (dtype == BV2_BF16) {
    const uint16_t* s = static_cast<const uint16_t*>(host_ptr);
    for (int64_t i = 0; i < n; ++i) { uint32_t b = (uint32_t)s[i] << 16; std::memcpy(&t.data[(size_t)i], &b, 4); }
  } else { h->err = std::string(what) + ": unknown dtype"; return -1; }
  h->blob[k].tensors[key] = std::move(t);
  return 0;
  BV2_CATCH(h)
}

static int64_t blob_bytes(const bv2_handle* h, BlobKind k) { return h->blob[k].total_floats * (int64_t)sizeof(float); }

static int64_t blob_packed_bytes(bv2_handle* h, BlobKind k, int spec_channels, const char* what) {
  if (!h) return -1;
  BV2_TRY
  if (blob_layout(h, k, spec_channels, what)) return -1;
  return blob_bytes(h, k);
  BV2_CATCH(h)
}

static int blob_pack(bv2_handle* h, BlobKind k, int spec_channels, const char* what, void* host_blob, int64_t bytes) {
  if (!h) return -1;
  BV2_TRY
  if (int rc = blob_layout(h, k, spec_channels, what)) return rc;
  if (!host_blob || bytes < blob_bytes(h, k)) { h->err = std::string(what) + ": buffer too small"; return -1; }
  float* out = static_cast<float*>(host_blob);
  const WeightBlob& b = h->blob[k];
  if (k == kPosterior) return pack_posterior_blob(h->model.cfg, h->post, b, out, h->err);
  if (k == kSdpForward) return pack_sdp_forward_blob(h->model.cfg, h->sdpf, b, out, h->err);
  return pack_blob(h->model, b, out, h->err);
  BV2_CATCH(h)
}

static int blob_attach(bv2_handle* h, BlobKind k, int spec_channels, const char* what, const void* dev_blob, int64_t bytes) {
  if (!h) return -1;
  BV2_TRY
  const std::string w(what);
  if (int rc = blob_layout(h, k, spec_channels, what)) return rc;
  if (!dev_blob || bytes < blob_bytes(h, k)) { h->err = w + ": blob too small for this config"; return -1; }
  uint32_t hdr[8];
  if (hipMemcpy(hdr, dev_blob, sizeof(hdr), hipMemcpyDeviceToHost) != hipSuccess) {
    h->err = w + ": cannot read the blob header (is this a device pointer on the current GPU?)";
    return -6;
  }
  const BlobDesc& d = kBlobDesc[k];
  WeightBlob& b = h->blob[k];
  if (!blob_header_matches(hdr, d.magic, d.layout, b.cfg_hash, b.total_floats)) {
    if (k == kInference && blob_header_matches(hdr, d.magic, hdr[3], b.cfg_hash, b.total_floats))
      h->err = w + ": blob was packed with another pack layout (a cache written by an older library build): repack";
    else
      h->err = w + ": blob header does not match this handle's " + d.noun + " layout (not packed, another kind of blob, or packed for another model)";
    return -7;
  }
  b.dev = static_cast<const float*>(dev_blob);
  return 0;
  BV2_CATCH(h)
}

static int blob_detach(bv2_handle* h, BlobKind k) {
  if (!h) return -1;
  h->blob[k].dev = nullptr;
  return 0;
}

int bv2_load_tensor(bv2_handle* h, const char* key, const void* host_ptr, const int64_t* shape, int ndim, int dtype) {
  return blob_load_tensor(h, kInference, "bv2_load_tensor", key, host_ptr, shape, ndim, dtype);
}
int64_t bv2_packed_bytes(const bv2_handle* h) { return h ? blob_bytes(h, kInference) : -1; }
int bv2_pack_weights(bv2_handle* h, void* host_blob, int64_t bytes) { return blob_pack(h, kInference, 0, "bv2_pack_weights", host_blob, bytes); }
int bv2_attach_weights(bv2_handle* h, const void* dev_blob, int64_t bytes) {
  return blob_attach(h, kInference, 0, "bv2_attach_weights", dev_blob, bytes);
}
int bv2_detach_weights(bv2_handle* h) { return blob_detach(h, kInference); }

int bv2_posterior_load_tensor(bv2_handle* h, const char* key, const void* host_ptr, const int64_t* shape, int ndim, int dtype) {
  return blob_load_tensor(h, kPosterior, "bv2_posterior_load_tensor", key, host_ptr, shape, ndim, dtype);
}
int64_t bv2_posterior_packed_bytes(bv2_handle* h, int spec_channels) {
  return blob_packed_bytes(h, kPosterior, spec_channels, "bv2_posterior_packed_bytes");
}
int bv2_posterior_pack(bv2_handle* h, int spec_channels, void* host_blob, int64_t bytes) {
  return blob_pack(h, kPosterior, spec_channels, "bv2_posterior_pack", host_blob, bytes);
}
int bv2_posterior_attach(bv2_handle* h, int spec_channels, const void* dev_blob, int64_t bytes) {
  return blob_attach(h, kPosterior, spec_channels, "bv2_posterior_attach", dev_blob, bytes);
}
int bv2_posterior_detach(bv2_handle* h) { return blob_detach(h, kPosterior); }

int bv2_sdp_forward_load_tensor(bv2_handle* h, const char* key, const void* host_ptr, const int64_t* shape, int ndim, int dtype) {
  return blob_load_tensor(h, kSdpForward, "bv2_sdp_forward_load_tensor", key, host_ptr, shape, ndim, dtype);
}
int64_t bv2_sdp_forward_packed_bytes(bv2_handle* h) { return blob_packed_bytes(h, kSdpForward, 0, "bv2_sdp_forward_packed_bytes"); }
int bv2_sdp_forward_pack(bv2_handle* h, void* host_blob, int64_t bytes) {
  return blob_pack(h, kSdpForward, 0, "bv2_sdp_forward_pack", host_blob, bytes);
}
int bv2_sdp_forward_attach(bv2_handle* h, const void* dev_blob, int64_t bytes) {
  return blob_attach(h, kSdpForward, 0, "bv2_sdp_forward_attach", dev_blob, bytes);
}
int bv2_sdp_forward_detach(bv2_handle* h) { return blob_detach(h, kSdpForward); }

int64_t bv2_posterior_workspace_bytes(const bv2_handle* h, int B, int Ty) {
  if (!h || B < 1 || Ty < 1) return -1;
  return posterior_workspace_bytes(h->model, B, Ty);
}

int bv2_posterior_encode(bv2_handle* h, bv2_stream stream, int B, int Ty, const float* y, const int64_t* y_lengths, const float* g,
                         const float* noise_q, float noise_scale_q, float* z, float* m_q, float* logs_q, float* y_mask,
                         void* ws, int64_t wsb) {
  if (!h) return -1;
  BV2_TRY
  if (!h->blob[kPosterior].dev) {
    h->err = "bv2_posterior_encode: no posterior weights attached (bv2_posterior_pack + bv2_posterior_attach; release checkpoints "
             "written by compress_model.py are stripped of enc_q.*)";
    return -8;
  }
  if (B < 1 || Ty < 1 || !y || !y_lengths || !g || !z || !ws) { h->err = "bv2_posterior_encode: bad argument"; return -1; }
  return run_posterior_encode(h, static_cast<hipStream_t>(stream), B, Ty, y, y_lengths, g, noise_q, noise_scale_q, z, m_q, logs_q, y_mask,
                              ws, wsb);
  BV2_CATCH(h)
}

int64_t bv2_duration_nll_workspace_bytes(const bv2_handle* h, int B, int T) {
  if (!h || B < 1 || B > 65535 || T < 1) return -1;
  return duration_nll_workspace_bytes(h->model, B, T);
}

int bv2_duration_nll(bv2_handle* h, bv2_stream stream, int B, int T, const float* x, const float* x_mask, const float* w, const float* g,
                     const float* noise_e, float* nll_sym, float* nll, void* ws, int64_t wsb) {
  if (!h) return -1;
  BV2_TRY
  if (B < 1 || B > 65535 || T < 1 || !x || !x_mask || !w || !g || !nll_sym || !nll) {
    h->err = "bv2_duration_nll: bad argument (B in [1, 65535], T >= 1; x, x_mask, w, g, nll_sym and nll must not be null)";
    return -1;
  }
  if ((int64_t)h->model.cfg.hidden_channels * T >= (1ll << 31)) { h->err = "bv2_duration_nll: hidden_channels * T must stay below 2^31"; return -1; }
  if (!ws) { h->err = "bv2_duration_nll: workspace is null"; return -5; }
  if (wsb < duration_nll_workspace_bytes(h->model, B, T)) { h->err = "workspace too small for bv2_duration_nll"; return -5; }
  if (!h->blob[kInference].dev) { h->err = "bv2_duration_nll: no weights attached (call bv2_pack_weights + bv2_attach_weights first)"; return -8; }
  if (!h->blob[kSdpForward].dev) {
    h->err = "bv2_duration_nll: no forward duration predictor weights attached (bv2_sdp_forward_pack + bv2_sdp_forward_attach; release "
             "checkpoints written by compress_model.py are stripped of sdp.post_*)";
    return -8;
  }
  return run_duration_nll(h, static_cast<hipStream_t>(stream), B, T, x, x_mask, w, g, noise_e, nll_sym, nll, ws, wsb);
  BV2_CATCH(h)
}

int bv2_kl_path(bv2_stream stream, int32_t B, int32_t inter, int32_t T, int32_t Ty, const float* z_p, const float* logs_q, const float* m_p,
                const float* logs_p, const float* w_ceil, const int64_t* x_lengths, const int64_t* y_lengths, float* kl_frame, float* kl) {
  auto fail = [&](const std::string& m, int rc) { g_create_err = "bv2_kl_path: " + m; return rc; };
  if (!z_p || !logs_q || !m_p || !logs_p || !w_ceil || !kl_frame || !kl)
    return fail("z_p, logs_q, m_p, logs_p, w_ceil, kl_frame and kl must not be null", -1);
  if (B < 1 || B > 65535) return fail("B must be in [1, 65535]", -1);
  if (inter < 1 || inter > 65535) return fail("inter must be in [1, 65535]", -1);
  if (T < 1 || T > MP_MAX_T) return fail("T must be in [1, " + std::to_string(MP_MAX_T) + "]", -1);
  if (Ty < 1 || (int64_t)inter * Ty >= (1ll << 31)) return fail("Ty must be >= 1 with inter * Ty below 2^31", -1);
  try {
    KlPathArgs a;
    a.z_p = z_p; a.logs_q = logs_q; a.m_p = m_p; a.logs_p = logs_p; a.w_ceil = w_ceil; a.x_lengths = x_lengths; a.y_lengths = y_lengths;
    a.kl_frame = kl_frame; a.kl = kl; a.B = B; a.D = inter; a.T = T; a.Ty = Ty;
    if (launch_kl_path(static_cast<hipStream_t>(stream), a)) return fail("kernel launch failed", -6);
    return 0;
  } catch (...) { return fail("exception", -100); }
}

int bv2_set_generator_dtype(bv2_handle* h, int dtype) {
  if (!h) return -1;
  if (dtype != BV2_F32 && dtype != BV2_BF16) { h->err = "bv2_set_generator_dtype: BV2_F32 or BV2_BF16"; return -1; }
  if (dtype == BV2_BF16) {
    const Model& m = h->model;
    bool ok = m.conv_pre.wb_off >= 0 && m.post_c % 8 == 0 && m.post_c <= 64;
    for (int i = 0; i < m.n_ups && ok; ++i) {
      ok = m.ups[i].cl.wb_off >= 0 && conv_cl_bf16_supported(m.ups[i].cl.cin, m.ups[i].cl.cout, m.ups[i].cl.k, 1);
      for (int j = 0; j < m.n_rbk && ok; ++j)
        for (int d = 0; d < m.n_rbd && ok; ++d)
          ok = m.rb[i][j][d][0].wb_off >= 0 &&
               conv_cl_bf16_supported(m.rb[i][j][d][0].cin, m.rb[i][j][d][0].cout, m.rb[i][j][d][0].k,
                                      m.cfg.resblock_dilation_sizes[j][d]);
    }
    if (!ok) { h->err = "bv2_set_generator_dtype: this Generator configuration has no bf16 kernel (channels must be multiples of 16, tile must fit LDS)"; return -2; }
  }
  h->gen_dtype = dtype;
  return 0;
}

int bv2_set_flow_dtype(bv2_handle* h, int dtype) {
  if (!h) return -1;
  if (dtype != BV2_F32 && dtype != BV2_F16) { h->err = "bv2_set_flow_dtype: BV2_F32 or BV2_F16"; return -1; }
  if (dtype == BV2_F16 && !h->model.cfg.use_transformer_flow) {
    // residual (WN) flow: in_layers (gate epilogue) and res_skip_layers on the fp16 matrix core, reference modules.py:185-210
    const Model& m = h->model;
    bool ok = m.cfg.hidden_channels % 32 == 0;
    for (int a = 0; a < m.n_coupling && ok; ++a)
      for (int i = 0; i < m.coupling[a].wn.layers && ok; ++i) {
        const WnW& K = m.coupling[a].wn;
        const bool last = i + 1 == K.layers;
        ok = K.in[i].wh_off >= 0 && K.skip[i].wh_off >= 0 && (last || K.res[i].wh_off >= 0) &&
             conv_f16_supported(K.in[i].cin, K.in[i].cout, K.in[i].k, 1, true) &&
             conv_f16_supported(K.skip[i].cin, K.skip[i].cout, 1, 1, false);
      }
    if (!ok) { h->err = "bv2_set_flow_dtype: the fp16 WN flow needs hidden_channels % 32 == 0"; return -2; }
  } else if (dtype == BV2_F16) {
    const Model& m = h->model;
    bool ok = m.cfg.use_transformer_flow != 0;
    for (int a = 0; a < m.n_coupling && ok; ++a)
      for (int i = 0; i < m.coupling[a].enc.n_layers && ok; ++i) {
        const EncLayerW& L = m.coupling[a].enc.layer[i];
        ok = L.qkv.wh_off >= 0 && L.o.wh_off >= 0 && L.ffn1.wh_off >= 0 && L.ffn2.wh_off >= 0 &&
             conv_f16_supported(L.qkv.cin, L.qkv.cout, 1, 1, false) && conv_f16_supported(L.o.cin, L.o.cout, 1, 1, false) &&
             conv_f16_supported(L.ffn1.cin, L.ffn1.cout, L.ffn1.k, 1, true) && conv_f16_supported(L.ffn2.cin, L.ffn2.cout, L.ffn2.k, 1, false);
      }
    if (!ok) { h->err = "bv2_set_flow_dtype: fp16 needs the transformer flow with channel counts that are multiples of 16"; return -2; }
  }
  h->flow_dtype = dtype;
  return 0;
}

int64_t bv2_workspace_bytes(const bv2_handle* h, int B, int T, int Ty_max) {
  if (!h || B < 1 || T < 1 || Ty_max < 1) return -1;
  return workspace_bytes(h->model, B, T, Ty_max);
}

static int ready(bv2_handle* h, const void* ws) {
  if (!h) return -1;
  if (!h->blob[kInference].dev) { h->err = "no weights attached (call bv2_pack_weights + bv2_attach_weights first)"; return -8; }
  if (!ws) { h->err = "workspace is null"; return -5; }
  return 0;
}

// a bv2_item_controls the caller built against another layout is refused (NULL = the scalar call)
static int check_controls(bv2_handle* h, const bv2_item_controls* ic, const char* what) {
  if (ic && ic->struct_bytes != (int32_t)sizeof(bv2_item_controls)) {
    h->err = std::string(what) + ": bv2_item_controls.struct_bytes must be sizeof(bv2_item_controls) (" +
             std::to_string(sizeof(bv2_item_controls)) + ")";
    return -1;
  }
  return 0;
}

int bv2_encode_durations(bv2_handle* h, bv2_stream stream, const bv2_encode_in* in, const bv2_encode_out* out,
                         void* ws, int64_t wsb) {
  return bv2_encode_durations_ex(h, stream, in, out, nullptr, ws, wsb);
}

int bv2_encode_durations_ex(bv2_handle* h, bv2_stream stream, const bv2_encode_in* in, const bv2_encode_out* out,
                            const bv2_item_controls* ic, void* ws, int64_t wsb) {
  return bv2_encode_durations_g(h, stream, in, out, ic, nullptr, ws, wsb);
}

// a model without a speaker table (n_speakers == 0) cannot look g up: checked before anything else, sid is never read
static int check_speaker(bv2_handle* h, const float* g, const char* what) {
  if (g || h->model.cfg.n_speakers >= 1) return 0;
  h->err = std::string(what) + ": this model has no speaker table (n_speakers == 0): pass g (bv2_ref_encode's result) through the _g call";
  return -1;
}

// what every phase-A entry point checks; g: the caller's speaker vectors (null: emb_g(in->sid), which needs a speaker table)
static int check_encode(bv2_handle* h, const bv2_encode_in* in, const bv2_encode_out* out, const float* g, const char* what) {
  const std::string w(what);
  if (!in || !out || in->B < 1 || in->T < 1) { h->err = w + ": bad argument"; return -1; }
  if (!in->x || !in->x_lengths || (!g && !in->sid) || !in->tone || !in->language || !in->bert || !in->ja_bert || !in->en_bert ||
      !out->g || !out->x || !out->m_p || !out->logs_p || !out->x_mask || !out->logw || !out->w_ceil ||
      !out->y_lengths) { h->err = w + ": null tensor pointer"; return -1; }
  for (int f = 0; f < 3; ++f)
    if (in->bert_index[f] && (in->bert_cols[f] < 1 || in->bert_cols[f] > in->T)) {
      h->err = w + ": bert_cols must be in [1, T] for a word-level feature"; return -1;
    }
  return 0;
}

int bv2_encode_durations_g(bv2_handle* h, bv2_stream stream, const bv2_encode_in* in, const bv2_encode_out* out,
                           const bv2_item_controls* ic, const float* g, void* ws, int64_t wsb) {
  if (!h) return -1;
  if (int rc = check_controls(h, ic, "bv2_encode_durations")) return rc;
  if (int rc = check_speaker(h, g, "bv2_encode_durations")) return rc;
  if (int rc = ready(h, ws)) return rc;
  BV2_TRY
  if (int rc = check_encode(h, in, out, g, "bv2_encode_durations")) return rc;
  return run_encode(h, static_cast<hipStream_t>(stream), *in, *out, ws, wsb, ic, g);
  BV2_CATCH(h)
}

int64_t bv2_ref_workspace_bytes(const bv2_handle* h, int B, int L) {
  if (!h || B < 1 || L < 1 || !h->model.ref_enc.present) return -1;
  return (int64_t)sizeof(float) * ref_enc_workspace_floats(B, L, h->model.cfg.spec_channels) + 256;
}

int bv2_ref_encode(bv2_handle* h, bv2_stream stream, const float* y, const int64_t* strides, const int64_t* y_lengths, int B, int L,
                   float* g_out, void* ws, int64_t wsb) {
  if (!h) return -1;
  if (!h->model.ref_enc.present) { h->err = "bv2_ref_encode: this model has a speaker table (n_speakers >= 1) and no ReferenceEncoder"; return -2; }
  if (int rc = ready(h, ws)) return rc;
  BV2_TRY
  if (!y || !g_out || B < 1 || B > 65535 || L < 1 || L > (1 << 20)) { h->err = "bv2_ref_encode: bad argument"; return -1; }
  if (strides && (strides[0] < 0 || strides[1] < 0 || strides[2] < 0)) { h->err = "bv2_ref_encode: negative stride"; return -1; }
  return run_ref_encode(h, static_cast<hipStream_t>(stream), y, strides, y_lengths, B, L, g_out, ws, wsb);
  BV2_CATCH(h)
}

int bv2_decode(bv2_handle* h, bv2_stream stream, const bv2_decode_in* in, const bv2_decode_out* out, void* ws, int64_t wsb) {
  return bv2_decode_ex(h, stream, in, out, nullptr, ws, wsb);
}

int bv2_decode_ex(bv2_handle* h, bv2_stream stream, const bv2_decode_in* in, const bv2_decode_out* out,
                  const bv2_item_controls* ic, void* ws, int64_t wsb) {
  if (!h) return -1;
  if (int rc = check_controls(h, ic, "bv2_decode")) return rc;
  if (int rc = ready(h, ws)) return rc;
  BV2_TRY
  if (!in || !out || in->B < 1 || in->T < 1 || in->Ty < 1) { h->err = "bv2_decode: bad argument"; return -1; }
  if (!in->m_p || !in->logs_p || !in->x_mask || !in->w_ceil || !in->y_lengths || !in->g || (!in->noise_z && !h->seeds) || !out->o) {
    h->err = "bv2_decode: null tensor pointer"; return -1;
  }
  return run_decode(h, static_cast<hipStream_t>(stream), *in, *out, ws, wsb, ic);
  BV2_CATCH(h)
}

int bv2_stage_emb_g(bv2_handle* h, bv2_stream stream, int B, const int64_t* sid, float* g) {
  if (!h) return -1;
  if (!h->blob[kInference].dev) { h->err = "no weights attached (call bv2_pack_weights + bv2_attach_weights first)"; return -8; }
  BV2_TRY
  if (B < 1 || !sid || !g) { h->err = "bv2_stage_emb_g: bad argument"; return -1; }
  if (h->model.cfg.n_speakers == 0) { h->err = "bv2_stage_emb_g: this model has no speaker table (n_speakers == 0); g comes from bv2_ref_encode"; return -2; }
  return run_stage_emb_g(h, static_cast<hipStream_t>(stream), B, sid, g);
  BV2_CATCH(h)
}

int bv2_stage_enc_p(bv2_handle* h, bv2_stream stream, int B, int T, const int64_t* x, const int64_t* t, const int64_t* language,
                    const float* bert_0, const float* bert_1, const float* bert_2, const float* g, const int64_t* x_lengths,
                    float* xout, float* m_p, float* logs_p, float* x_mask, void* ws, int64_t wsb) {
  if (int rc = ready(h, ws)) return rc;
  BV2_TRY
  if (B < 1 || T < 1 || !x || !t || !language || !bert_0 || !bert_1 || !bert_2 || !g || !xout || !m_p || !logs_p || !x_mask) {
    h->err = "bv2_stage_enc_p: bad argument"; return -1;
  }
  return run_stage_enc_p(h, static_cast<hipStream_t>(stream), B, T, x, t, language, bert_0, bert_1, bert_2, g, x_lengths, xout,
                         m_p, logs_p, x_mask, ws, wsb);
  BV2_CATCH(h)
}

int bv2_stage_sdp(bv2_handle* h, bv2_stream stream, int B, int T, const float* x, const float* x_mask, const float* zin,
                  const float* g, float* logw, void* ws, int64_t wsb) {
  if (int rc = ready(h, ws)) return rc;
  BV2_TRY
  if (B < 1 || T < 1 || !x || !x_mask || !zin || !g || !logw) { h->err = "bv2_stage_sdp: bad argument"; return -1; }
  return run_stage_sdp(h, static_cast<hipStream_t>(stream), B, T, x, x_mask, zin, g, logw, ws, wsb);
  BV2_CATCH(h)
}

int bv2_stage_dp(bv2_handle* h, bv2_stream stream, int B, int T, const float* x, const float* x_mask, const float* g,
                 float* logw, void* ws, int64_t wsb) {
  if (int rc = ready(h, ws)) return rc;
  BV2_TRY
  if (B < 1 || T < 1 || !x || !x_mask || !g || !logw) { h->err = "bv2_stage_dp: bad argument"; return -1; }
  return run_stage_dp(h, static_cast<hipStream_t>(stream), B, T, x, x_mask, g, logw, ws, wsb);
  BV2_CATCH(h)
}

int bv2_stage_flow(bv2_handle* h, bv2_stream stream, int B, int Ty, const float* z_p, const int64_t* y_lengths,
                   const float* y_mask, const float* g, float* z, void* ws, int64_t wsb) {
  if (int rc = ready(h, ws)) return rc;
  BV2_TRY
  if (B < 1 || Ty < 1 || !z_p || !g || !z || ((y_lengths != nullptr) == (y_mask != nullptr))) {
    h->err = "bv2_stage_flow: bad argument (exactly one of y_lengths / y_mask)"; return -1;
  }
  return run_flow(h, static_cast<hipStream_t>(stream), B, Ty, z_p, y_lengths, y_mask, g, z, ws, wsb, false);
  BV2_CATCH(h)
}

int bv2_stage_flow_forward(bv2_handle* h, bv2_stream stream, int B, int Ty, const float* z, const int64_t* y_lengths,
                           const float* y_mask, const float* g, float* z_p, void* ws, int64_t wsb) {
  if (int rc = ready(h, ws)) return rc;
  BV2_TRY
  if (B < 1 || Ty < 1 || !z || !g || !z_p || ((y_lengths != nullptr) == (y_mask != nullptr))) {
    h->err = "bv2_stage_flow_forward: bad argument (exactly one of y_lengths / y_mask)"; return -1;
  }
  return run_flow(h, static_cast<hipStream_t>(stream), B, Ty, z, y_lengths, y_mask, g, z_p, ws, wsb, true);
  BV2_CATCH(h)
}

int bv2_stage_generator(bv2_handle* h, bv2_stream stream, int B, int Ty, int L, const float* z, const int64_t* y_lengths,
                        const float* g, float* o, void* ws, int64_t wsb) {
  if (int rc = ready(h, ws)) return rc;
  BV2_TRY
  if (B < 1 || Ty < 1 || !z || !g || !o) { h->err = "bv2_stage_generator: bad argument"; return -1; }
  return run_generator(h, static_cast<hipStream_t>(stream), B, Ty, L, z, y_lengths, g, o, ws, wsb);
  BV2_CATCH(h)
}

int bv2_infer(bv2_handle* h, bv2_stream stream, const bv2_encode_in* in, const bv2_encode_out* enc_out,
              const float* noise_z, int64_t nz_bstride, int64_t nz_cstride, int64_t nz_tstride, float noise_scale, int32_t max_len,
              int32_t Ty_cap, const bv2_decode_out* dec_out, int32_t* Ty_out, void* ws, int64_t wsb) {
  return bv2_infer_ex(h, stream, in, enc_out, noise_z, nz_bstride, nz_cstride, nz_tstride, noise_scale, max_len, Ty_cap, dec_out,
                      Ty_out, nullptr, ws, wsb);
}

int bv2_infer_ex(bv2_handle* h, bv2_stream stream, const bv2_encode_in* in, const bv2_encode_out* enc_out,
                 const float* noise_z, int64_t nz_bstride, int64_t nz_cstride, int64_t nz_tstride, float noise_scale, int32_t max_len,
                 int32_t Ty_cap, const bv2_decode_out* dec_out, int32_t* Ty_out, const bv2_item_controls* ic, void* ws,
                 int64_t wsb) {
  return bv2_infer_g(h, stream, in, enc_out, noise_z, nz_bstride, nz_cstride, nz_tstride, noise_scale, max_len, Ty_cap, dec_out,
                     Ty_out, ic, nullptr, ws, wsb);
}

int bv2_infer_g(bv2_handle* h, bv2_stream stream, const bv2_encode_in* in, const bv2_encode_out* enc_out,
                const float* noise_z, int64_t nz_bstride, int64_t nz_cstride, int64_t nz_tstride, float noise_scale, int32_t max_len,
                int32_t Ty_cap, const bv2_decode_out* dec_out, int32_t* Ty_out, const bv2_item_controls* ic, const float* g, void* ws,
                int64_t wsb) {
  if (int rc = bv2_encode_durations_g(h, stream, in, enc_out, ic, g, ws, wsb)) return rc;
  BV2_TRY
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::vector<int64_t> yl((size_t)in->B);
  // the reference's one host sync (commons.py:120-122: length.max() feeds torch.arange)
  if (hipMemcpyAsync(yl.data(), enc_out->y_lengths, sizeof(int64_t) * (size_t)in->B, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) { h->err = "bv2_infer: reading y_lengths failed"; return -6; }
  int64_t Ty = 1;
  for (int64_t v : yl) Ty = v > Ty ? v : Ty;
  if (Ty_out) *Ty_out = (int32_t)Ty;
  if (Ty > Ty_cap) { h->err = "bv2_infer: realised T_y exceeds Ty_cap"; return -3; }
  bv2_decode_in d;
  std::memset(&d, 0, sizeof(d));
  d.B = in->B; d.T = in->T; d.Ty = (int32_t)Ty; d.max_len = max_len;
  d.m_p = enc_out->m_p; d.logs_p = enc_out->logs_p; d.x_mask = enc_out->x_mask; d.w_ceil = enc_out->w_ceil;
  d.y_lengths = enc_out->y_lengths; d.g = enc_out->g;
  d.noise_z = noise_z; d.nz_bstride = nz_bstride; d.nz_cstride = nz_cstride; d.nz_tstride = nz_tstride; d.noise_scale = noise_scale;
  return bv2_decode_ex(h, stream, &d, dec_out, ic, ws, wsb);
  BV2_CATCH(h)
}

int bv2_pcm16(bv2_stream stream, const float* wave, int64_t wave_bstride, const int64_t* y_lengths, int32_t hop, int32_t B,
              int64_t S, int16_t* pcm, int64_t pcm_bstride, uint32_t* peak_scratch) {
  if (!wave || !y_lengths || !pcm || !peak_scratch || wave_bstride < S || pcm_bstride < S) return -1;
  try {
    return launch_pcm16(static_cast<hipStream_t>(stream), wave, wave_bstride, y_lengths, hop, B, S, pcm, pcm_bstride,
                        peak_scratch);
  } catch (...) { return -100; }
}

// ---- streamed synthesis (bv2_exec.cpp run_stream_*, kernels/stream.hip) ------------------------------------------
int bv2_generator_halo(const bv2_handle* h) { return h ? generator_halo(h->model) : -1; }

int64_t bv2_stream_workspace_bytes(const bv2_handle* h, int B, int T, int Ty, int window_frames) {
  if (!h || B < 1 || T < 1 || Ty < 1 || window_frames < 1) return -1;
  return stream_workspace_bytes(h->model, B, T, Ty, window_frames);
}

int bv2_stream_begin(bv2_handle* h, bv2_stream stream, const bv2_decode_in* in, const bv2_decode_out* out,
                     const bv2_item_controls* ic, void* ws, int64_t wsb) {
  if (!h) return -1;
  BV2_TRY
  if (int rc = check_controls(h, ic, "bv2_stream_begin")) return rc;
  if (!in || !out || in->B < 1 || in->T < 1 || in->Ty < 1) { h->err = "bv2_stream_begin: bad argument"; return -1; }
  if (!in->m_p || !in->logs_p || !in->x_mask || !in->w_ceil || !in->y_lengths || !in->g || (!in->noise_z && !h->seeds)) {
    h->err = "bv2_stream_begin: null tensor pointer"; return -1;
  }
  if (!h->taps.empty()) { h->err = "bv2_stream_begin: taps are not supported during a stream (bv2_set_tap(h, NULL, ...) clears them)"; return -1; }
  if (int rc = ready(h, ws)) return rc;
  return run_stream_begin(h, static_cast<hipStream_t>(stream), *in, *out, ws, wsb, ic);
  BV2_CATCH(h)
}

int bv2_stream_chunk(bv2_handle* h, bv2_stream stream, const bv2_stream_chunk_args* a, void* ws, int64_t wsb) {
  if (!h) return -1;
  BV2_TRY
  auto bad = [&](const std::string& m) { h->err = "bv2_stream_chunk: " + m; return -1; };
  if (!a) return bad("args is null");
  if (a->struct_bytes != (int32_t)sizeof(bv2_stream_chunk_args))
    return bad("bv2_stream_chunk_args.struct_bytes must be sizeof(bv2_stream_chunk_args) (" + std::to_string(sizeof(bv2_stream_chunk_args)) + ")");
  if (a->B < 1 || a->B > 65535 || a->Ty < 1) return bad("need 1 <= B <= 65535 and Ty >= 1");
  const int L = (a->max_len > 0 && a->max_len < a->Ty) ? a->max_len : a->Ty;
  if (a->t0 < 0 || a->t0 >= a->t1) return bad("need 0 <= t0 < t1, got t0 = " + std::to_string(a->t0) + ", t1 = " + std::to_string(a->t1));
  if (a->t1 > L) return bad("t1 = " + std::to_string(a->t1) + " is past the last frame (" + std::to_string(L) + ")");
  if (a->window_frames < 1 || a->t1 - a->t0 > a->window_frames)
    return bad("the chunk keeps " + std::to_string(a->t1 - a->t0) + " frames, the workspace was planned for window_frames = " +
               std::to_string(a->window_frames));
  if (!a->y_lengths) return bad("y_lengths is null");
  if (a->exact_lengths != 0 && a->exact_lengths != 1) return bad("exact_lengths must be 0 or 1");
  if ((a->dst != nullptr) == (a->dst16 != nullptr)) return bad("exactly one of dst / dst16 must be given");
  const int64_t n = (int64_t)(a->t1 - a->t0) * h->model.total_up;
  if ((a->dst ? a->dst_bstride : a->dst16_bstride) < n) return bad("the destination's batch stride is shorter than the chunk (" + std::to_string(n) + " samples)");
  if (!h->taps.empty()) return bad("taps are not supported during a stream (bv2_set_tap(h, NULL, ...) clears them)");
  if (!ws || wsb < stream_plan_bytes(h->model, a->B, a->Ty, a->window_frames)) {
    h->err = "bv2_stream_chunk: workspace is null or smaller than bv2_stream_workspace_bytes(h, B, T, Ty, window_frames)"; return -5;
  }
  if (int rc = ready(h, ws)) return rc;
  bv2_stream_chunk_args c = *a;
  if (!(c.pcm_gain > 0.f)) c.pcm_gain = 32767.f;
  return run_stream_chunk(h, static_cast<hipStream_t>(stream), c, ws, wsb);
  BV2_CATCH(h)
}

int bv2_emit(bv2_stream stream, const float* src, int64_t src_bstride, int64_t src_off, const int64_t* y_lengths, int32_t hop,
             int64_t start_sample, int32_t B, int64_t n, float* dst, int16_t* dst16, int64_t dst_bstride, float gain) {
  auto bad = [&](const char* m) { g_create_err = std::string("bv2_emit: ") + m; return -1; };
  try {
    if (!src) return bad("src is null");
    if ((dst != nullptr) == (dst16 != nullptr)) return bad("exactly one of dst / dst16 must be given");
    if (B < 1 || B > 65535 || n < 1 || hop < 1 || src_off < 0 || src_bstride < 0) return bad("need 1 <= B <= 65535, n >= 1, hop >= 1, src_off >= 0, src_bstride >= 0");
    if (dst_bstride < n) return bad("dst_bstride is shorter than n");
    if (launch_stream_emit(static_cast<hipStream_t>(stream), src, src_bstride, src_off, y_lengths, hop, start_sample, B, n, dst, dst16,
                           dst_bstride, gain > 0.f ? gain : 32767.f)) return bad("kernel launch failed");
    return 0;
  } catch (...) { return -100; }
}

// ---- spectrogram of a waveform (kernels/stft.hip) ---------------------------------------------------------------
static int stft_check(const bv2_stft_config* c, const char* what) {
  auto fail = [&](const std::string& m) { g_create_err = std::string(what) + ": " + m; return -1; };
  if (!c) return fail("cfg is null");
  if (c->struct_bytes != (int32_t)sizeof(bv2_stft_config)) return fail("bv2_stft_config.struct_bytes mismatch (ABI drift)");
  if (c->n_fft != 1024 && c->n_fft != 2048) return fail("n_fft must be 1024 or 2048, got " + std::to_string(c->n_fft));
  if (c->hop < 1 || c->hop > c->n_fft) return fail("hop must be in [1, n_fft], got " + std::to_string(c->hop));
  if (c->win < 1 || c->win > c->n_fft) return fail("win must be in [1, n_fft], got " + std::to_string(c->win));
  if (c->n_mels < 0 || c->n_mels > 1024) return fail("n_mels must be in [0, 1024], got " + std::to_string(c->n_mels));
  if (c->input_format != BV2_WAV_F32 && c->input_format != BV2_WAV_I16) return fail("input_format must be BV2_WAV_F32 or BV2_WAV_I16");
  return 0;
}

int64_t bv2_stft_frames(const bv2_stft_config* cfg, int64_t n_samples) {
  if (stft_check(cfg, "bv2_stft_frames")) return -1;
  const int64_t pad = (cfg->n_fft - cfg->hop) / 2;
  if (n_samples <= pad) {
    g_create_err = "bv2_stft_frames: n_samples must be at least pad + 1 = " + std::to_string(pad + 1) + " (reflect padding), got " + std::to_string(n_samples);
    return -1;
  }
  const int64_t n = n_samples + 2 * pad - cfg->n_fft;
  if (n < 0) {
    g_create_err = "bv2_stft_frames: n_samples must be at least n_fft - 2 pad = " + std::to_string(cfg->n_fft - 2 * pad) + " (one whole frame), got " + std::to_string(n_samples);
    return -1;
  }
  return 1 + n / cfg->hop;
}

// librosa.filters.mel (htk = False, norm = "slaney"): the Slaney scale is linear below 1 kHz (200 / 3 Hz per mel) and logarithmic above
static double hz_to_mel(double f) {
  const double f_sp = 200.0 / 3, min_log_hz = 1000.0, logstep = std::log(6.4) / 27.0;
  return f >= min_log_hz ? min_log_hz / f_sp + std::log(f / min_log_hz) / logstep : f / f_sp;
}
static double mel_to_hz(double m) {
  const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
  return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

int bv2_mel_basis_f64(const bv2_stft_config* cfg, int32_t sampling_rate, double fmin, double fmax, double* out) {
  if (int rc = stft_check(cfg, "bv2_mel_basis")) return rc;
  if (!out || cfg->n_mels < 1 || sampling_rate < 1) { g_create_err = "bv2_mel_basis: needs out, n_mels >= 1 and sampling_rate >= 1"; return -1; }
  if (fmax <= 0) fmax = sampling_rate / 2.0;
  if (fmin < 0 || fmin >= fmax) { g_create_err = "bv2_mel_basis: fmin must be in [0, fmax)"; return -1; }
  try {
    const int M = cfg->n_mels, C = cfg->n_fft / 2 + 1;
    std::vector<double> mel_f(M + 2);
    const double m0 = hz_to_mel(fmin), m1 = hz_to_mel(fmax), step = (m1 - m0) / (M + 1);
    for (int i = 0; i < M + 2; ++i) mel_f[i] = mel_to_hz(i == M + 1 ? m1 : m0 + step * i);
    const double fstep = (sampling_rate / 2.0) / (C - 1);
    for (int m = 0; m < M; ++m) {
      const double d0 = mel_f[m + 1] - mel_f[m], d1 = mel_f[m + 2] - mel_f[m + 1], norm = 2.0 / (mel_f[m + 2] - mel_f[m]);
      for (int f = 0; f < C; ++f) {
        const double fr = f == C - 1 ? sampling_rate / 2.0 : fstep * f;
        const double lower = -(mel_f[m] - fr) / d0, upper = (mel_f[m + 2] - fr) / d1;
        out[(size_t)m * C + f] = std::max(0.0, std::min(lower, upper)) * norm;
      }
    }
    return 0;
  } catch (...) { g_create_err = "bv2_mel_basis: out of memory"; return -100; }
}

int bv2_mel_basis(const bv2_stft_config* cfg, int32_t sampling_rate, double fmin, double fmax, float* out) {
  if (int rc = stft_check(cfg, "bv2_mel_basis")) return rc;
  if (!out || cfg->n_mels < 1) { g_create_err = "bv2_mel_basis: needs out and n_mels >= 1"; return -1; }
  try {
    const size_t n = (size_t)cfg->n_mels * (cfg->n_fft / 2 + 1);
    std::vector<double> d(n);
    if (int rc = bv2_mel_basis_f64(cfg, sampling_rate, fmin, fmax, d.data())) return rc;
    for (size_t i = 0; i < n; ++i) out[i] = (float)d[i];
    return 0;
  } catch (...) { g_create_err = "bv2_mel_basis: out of memory"; return -100; }
}

int64_t bv2_stft_workspace_bytes(const bv2_stft_config* cfg, int32_t B, int64_t S) {
  if (stft_check(cfg, "bv2_stft_workspace_bytes")) return -1;
  if (B < 1 || S < 1) { g_create_err = "bv2_stft_workspace_bytes: B and S must be at least 1"; return -1; }
  return stft_workspace_bytes(cfg->n_fft, cfg->n_mels) + 256;
}

int bv2_spectrogram(bv2_stream stream, const bv2_stft_config* cfg, const void* wav, int64_t wav_bstride, const int64_t* wav_lengths,
                    int32_t B, int64_t S, const float* mel_basis, float* spec, const int64_t* spec_strides, int64_t* spec_lengths_out,
                    void* workspace, int64_t workspace_bytes) {
  const char* what = "bv2_spectrogram";
  if (int rc = stft_check(cfg, what)) return rc;
  auto fail = [&](const std::string& m, int rc) { g_create_err = std::string(what) + ": " + m; return rc; };
  if (!wav || !spec) return fail("wav and spec must not be null", -1);
  if (B < 1 || B > 65535) return fail("B must be in [1, 65535]", -1);
  if (S < 1 || S > ((int64_t)1 << 31) - 4096) return fail("S must be in [1, 2^31 - 4096]", -1);
  if (wav_bstride < 0) return fail("wav_bstride must not be negative", -1);
  if (cfg->n_mels > 0 && !mel_basis) return fail("mel_basis must not be null when n_mels > 0", -1);
  const int64_t L = bv2_stft_frames(cfg, S);
  if (L < 1) return -1;                                      // message set by bv2_stft_frames
  if (L > ((int64_t)1 << 30)) return fail("too many frames", -1);
  const int64_t C = cfg->n_mels ? cfg->n_mels : cfg->n_fft / 2 + 1;
  int64_t st[3] = {C * L, L, 1};
  if (spec_strides) {
    for (int i = 0; i < 3; ++i) {
      if (spec_strides[i] < 0) return fail("spec_strides must not be negative", -1);
      st[i] = spec_strides[i];
    }
  }
  const int64_t need = stft_workspace_bytes(cfg->n_fft, cfg->n_mels);
  if (!workspace || workspace_bytes < need) return fail("workspace too small (bv2_stft_workspace_bytes)", -5);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const uintptr_t mis = reinterpret_cast<uintptr_t>(ws) & 7u;
  if (mis) {
    if (workspace_bytes < need + 8) return fail("workspace too small (bv2_stft_workspace_bytes)", -5);
    ws += 8 - mis;
  }
  try {
    StftArgs a;
    a.wav = wav; a.wav_bstride = wav_bstride; a.wav_lengths = wav_lengths; a.B = B; a.S = S;
    a.n_fft = cfg->n_fft; a.hop = cfg->hop; a.win = cfg->win; a.n_mels = cfg->n_mels; a.input_format = cfg->input_format;
    a.L = (int)L; a.mel = cfg->n_mels ? mel_basis : nullptr;
    a.spec = spec; a.sb = st[0]; a.sf = st[1]; a.st = st[2]; a.lengths_out = spec_lengths_out; a.ws = ws;
    if (launch_stft(static_cast<hipStream_t>(stream), a)) return fail("kernel launch failed", -6);
    return 0;
  } catch (...) { return fail("exception", -100); }
}

// ---- polyphase resampler (kernels/resample.hip) -------------------------------------------------------------------
struct ResamplePlan { int L, M, K; };
static const int RS_ZEROS = 32, RS_MAX_L = 1024;
static const int64_t RS_MAX_TABLE = (int64_t)1 << 20, RS_MAX_INDEX = (int64_t)1 << 40;
static const double RS_BETA = 10.0, RS_ROLLOFF = 0.91;

static int resample_plan(const bv2_resample_config* c, const char* what, ResamplePlan* out) {
  auto fail = [&](const std::string& m) { g_create_err = std::string(what) + ": " + m; return -1; };
  if (!c) return fail("cfg is null");
  if (c->struct_bytes != (int32_t)sizeof(bv2_resample_config)) return fail("bv2_resample_config.struct_bytes mismatch (ABI drift)");
  if (c->rate_in <= 0 || c->rate_out <= 0)
    return fail("rates must be positive, got " + std::to_string(c->rate_in) + " -> " + std::to_string(c->rate_out));
  if (c->rate_in == c->rate_out) return fail("rate_in equals rate_out (" + std::to_string(c->rate_in) + "): nothing to resample");
  if (c->input_format != BV2_WAV_F32 && c->input_format != BV2_WAV_I16) return fail("input_format must be BV2_WAV_F32 or BV2_WAV_I16");
  int64_t a = c->rate_in, b = c->rate_out;
  while (b) { const int64_t t = a % b; a = b; b = t; }
  const int64_t L = c->rate_out / a, M = c->rate_in / a;
  if (L > RS_MAX_L)
    return fail("L = rate_out / gcd = " + std::to_string(L) + " exceeds the limit of " + std::to_string(RS_MAX_L) + " phases (" +
                std::to_string(c->rate_in) + " -> " + std::to_string(c->rate_out) + ")");
  const double cut = RS_ROLLOFF * std::min(1.0, (double)L / (double)M);
  const double W = RS_ZEROS / cut;
  const double Kd = std::ceil(W);
  if (Kd * 2 + 1 > (double)RS_MAX_TABLE || L * ((int64_t)Kd * 2 + 1) > RS_MAX_TABLE)
    return fail("L * taps = " + std::to_string(L) + " * " + std::to_string((int64_t)Kd * 2 + 1) + " exceeds the limit of 2^20 = " +
                std::to_string(RS_MAX_TABLE) + " table entries (" + std::to_string(c->rate_in) + " -> " + std::to_string(c->rate_out) + ")");
  out->L = (int)L; out->M = (int)M; out->K = (int)Kd;
  return 0;
}

static double bessel_i0(double x) {                  // sum_k ((x / 2)^k / k!)^2: positive terms, converged to the last bit for x <= beta
  const double q = x * x / 4;
  double term = 1, sum = 1;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * k);
    sum += term;
    if (term < sum * 1e-18) break;
  }
  return sum;
}

int bv2_resample_plan(const bv2_resample_config* cfg, int32_t* L, int32_t* M, int32_t* K) {
  ResamplePlan p;
  if (int rc = resample_plan(cfg, "bv2_resample_plan", &p)) return rc;
  if (L) *L = p.L;
  if (M) *M = p.M;
  if (K) *K = p.K;
  return 0;
}

int64_t bv2_resample_length(const bv2_resample_config* cfg, int64_t n_in) {
  ResamplePlan p;
  if (resample_plan(cfg, "bv2_resample_length", &p)) return -1;
  if (n_in < 0 || n_in >= RS_MAX_INDEX) { g_create_err = "bv2_resample_length: n_in must be in [0, 2^40)"; return -1; }
  return (n_in * p.L + p.M - 1) / p.M;
}

int64_t bv2_resample_ready(const bv2_resample_config* cfg, int64_t available_in) {
  ResamplePlan p;
  if (resample_plan(cfg, "bv2_resample_ready", &p)) return -1;
  if (available_in < 0 || available_in >= RS_MAX_INDEX) { g_create_err = "bv2_resample_ready: available_in must be in [0, 2^40)"; return -1; }
  const int64_t a = available_in - p.K;
  return a <= 0 ? 0 : (a * p.L + p.M - 1) / p.M;
}

int bv2_resample_taps_f64(const bv2_resample_config* cfg, double* out) {
  ResamplePlan p;
  if (int rc = resample_plan(cfg, "bv2_resample_taps", &p)) return rc;
  if (!out) { g_create_err = "bv2_resample_taps: out is null"; return -1; }
  const double pi = 3.14159265358979323846;
  const double cut = RS_ROLLOFF * std::min(1.0, (double)p.L / (double)p.M), W = RS_ZEROS / cut, i0b = bessel_i0(RS_BETA);
  const int taps = 2 * p.K + 1;
  for (int ph = 0; ph < p.L; ++ph) {
    double* row = out + (size_t)ph * taps;
    double sum = 0;
    for (int jj = 0; jj < taps; ++jj) {
      const double t = (double)ph / (double)p.L - (double)(jj - p.K);
      double v = 0;
      if (std::fabs(t) < W) {
        const double x = cut * t, r = t / W;
        const double sinc = x == 0 ? 1.0 : std::sin(pi * x) / (pi * x);
        v = cut * sinc * bessel_i0(RS_BETA * std::sqrt(1 - r * r)) / i0b;
      }
      row[jj] = v;
      sum += v;
    }
    for (int jj = 0; jj < taps; ++jj) row[jj] /= sum;          // DC gain exactly 1 in every phase
  }
  return 0;
}

int bv2_resample_taps(const bv2_resample_config* cfg, float* out) {
  ResamplePlan p;
  if (int rc = resample_plan(cfg, "bv2_resample_taps", &p)) return rc;
  if (!out) { g_create_err = "bv2_resample_taps: out is null"; return -1; }
  try {
    const size_t n = (size_t)p.L * (2 * p.K + 1);
    std::vector<double> d(n);
    if (int rc = bv2_resample_taps_f64(cfg, d.data())) return rc;
    for (size_t i = 0; i < n; ++i) out[i] = (float)d[i];
    return 0;
  } catch (...) { g_create_err = "bv2_resample_taps: out of memory"; return -100; }
}

int bv2_resample(bv2_stream stream, const bv2_resample_config* cfg, const float* taps, const void* src, int64_t src_bstride,
                 int64_t src_start, int64_t src_n, const int64_t* src_lengths, int32_t B, int64_t n0, int64_t n1, float* dst,
                 int64_t dst_bstride, int64_t* dst_lengths_out) {
  const char* what = "bv2_resample";
  ResamplePlan p;
  if (int rc = resample_plan(cfg, what, &p)) return rc;
  auto fail = [&](const std::string& m, int rc) { g_create_err = std::string(what) + ": " + m; return rc; };
  if (!taps) return fail("taps is null (the DEVICE copy of bv2_resample_taps)", -1);
  if (!src) return fail("src is null", -1);
  if (!dst) return fail("dst is null", -1);
  if (B < 1 || B > 65535) return fail("B must be in [1, 65535]", -1);
  if (n0 < 0) return fail("n0 must not be negative", -1);
  if (n1 < n0) return fail("n1 = " + std::to_string(n1) + " is below n0 = " + std::to_string(n0), -1);
  if (n1 >= RS_MAX_INDEX) return fail("n1 must be below 2^40", -1);
  if (src_start < 0 || src_n < 0 || src_start + src_n >= RS_MAX_INDEX || src_n >= RS_MAX_INDEX)
    return fail("src_start and src_n must not be negative and src_start + src_n must be below 2^40", -1);
  if (src_bstride < 0) return fail("src_bstride must not be negative", -1);
  if (dst_bstride < n1 - n0) return fail("dst_bstride is shorter than n1 - n0", -1);
  const int64_t first = (n0 * p.M) / p.L - p.K, lower = first > 0 ? first : 0;
  if (src_start > lower)
    return fail("src_start = " + std::to_string(src_start) + " is above the lower edge max(0, i0(n0) - K) = " + std::to_string(lower) +
                " that output n0 = " + std::to_string(n0) + " reads", -1);
  if (n1 == n0) return 0;
  try {
    ResampleArgs a;
    a.src = src; a.src_bstride = src_bstride; a.src_start = src_start; a.src_n = src_n; a.src_lengths = src_lengths; a.taps = taps;
    a.B = B; a.L = p.L; a.M = p.M; a.K = p.K; a.input_format = cfg->input_format; a.n0 = n0; a.n1 = n1;
    a.dst = dst; a.dst_bstride = dst_bstride; a.dst_lengths_out = dst_lengths_out;
    if (launch_resample(static_cast<hipStream_t>(stream), a)) return fail("kernel launch failed", -6);
    return 0;
  } catch (...) { return fail("exception", -100); }
}

// ---- BS.1770 loudness (kernels/loudness.hip) -------------------------------------------------------------------------
static const int LD_MIN_RATE = 8000, LD_MAX_RATE = 192000, LD_MAX_B = 4096;
static const int64_t LD_MAX_S = ((int64_t)1 << 31) - 4096;

static int loudness_check(const bv2_loudness_config* c, const char* what) {
  auto fail = [&](const std::string& m) { g_create_err = std::string(what) + ": " + m; return -1; };
  if (!c) return fail("cfg is null");
  if (c->struct_bytes != (int32_t)sizeof(bv2_loudness_config)) return fail("bv2_loudness_config.struct_bytes mismatch (ABI drift)");
  if (c->sample_rate < LD_MIN_RATE || c->sample_rate > LD_MAX_RATE)
    return fail("sample_rate must be in [" + std::to_string(LD_MIN_RATE) + ", " + std::to_string(LD_MAX_RATE) + "], got " +
                std::to_string(c->sample_rate));
  if (c->input_format != BV2_WAV_F32 && c->input_format != BV2_WAV_I16) return fail("input_format must be BV2_WAV_F32 or BV2_WAV_I16");
  return 0;
}

static int loudness_step(const bv2_loudness_config* c) { return (c->sample_rate + 5) / 10; }   // round(fs / 10)

static void loudness_coeffs(int rate, double out[10]) {
  const double pi = 3.14159265358979323846;
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = std::tan(pi * f0 / rate), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    out[0] = (Vh + Vb * K / Q + K * K) / a0;
    out[1] = 2.0 * (K * K - Vh) / a0;
    out[2] = (Vh - Vb * K / Q + K * K) / a0;
    out[3] = 2.0 * (K * K - 1.0) / a0;
    out[4] = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = std::tan(pi * f0 / rate), a0 = 1.0 + K / Q + K * K;
    out[5] = 1.0; out[6] = -2.0; out[7] = 1.0;
    out[8] = 2.0 * (K * K - 1.0) / a0;
    out[9] = (1.0 - K / Q + K * K) / a0;
  }
}

// The cascade in transposed direct form II has the state (s1, s2, t1, t2) and, for a zero input, s' = A s.  P, Q, R = A^16, A^256, A^4096
// by repeated squaring in fp64 (the spectral radius is below 1: the powers only shrink).
static void loudness_filter(int rate, LoudnessFilter* f) {
  loudness_coeffs(rate, f->c);
  const double *c = f->c;
  double M[16] = {-c[3], 1, 0, 0,
                  -c[4], 0, 0, 0,
                  c[6] - c[8] * c[5], 0, -c[8], 1,
                  c[7] - c[9] * c[5], 0, -c[9], 0};
  for (int sq = 1; sq <= 12; ++sq) {                                          // M = A^(2^sq)
    double N[16];
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        double s = 0;
        for (int k = 0; k < 4; ++k) s += M[i * 4 + k] * M[k * 4 + j];
        N[i * 4 + j] = s;
      }
    std::memcpy(M, N, sizeof(M));
    if (sq == 4) std::memcpy(f->P, M, sizeof(M));
    if (sq == 8) std::memcpy(f->Q, M, sizeof(M));
    if (sq == 12) std::memcpy(f->R, M, sizeof(M));
  }
  static_assert(LD_SEG == 16 && LD_TILE == 4096, "the powers above are A^LD_SEG, A^(LD_SEG^2) and A^LD_TILE");
}

static int64_t loudness_blocks(int64_t n, int step) {
  const int64_t block = 4 * (int64_t)step;
  return n <= 0 ? 0 : (n < block ? 1 : (n - block) / step + 1);
}

struct LoudnessWs { int64_t tile_z, tile_s, part, item, block_ms, tile_peak, total; };
static LoudnessWs loudness_ws(int step, int64_t B, int64_t S) {
  const int64_t nt = (S + LD_TILE - 1) / LD_TILE;
  LoudnessWs w;
  int64_t o = 0;
  w.tile_z = o; o += B * nt * 4 * 8;
  w.tile_s = o; o += B * nt * 4 * 8;
  w.part = o; o += B * nt * LD_MAX_PARTS * 8;
  w.item = o; o += B * 4 * 8;
  w.block_ms = o; o += B * loudness_blocks(S, step) * 8;
  w.tile_peak = o; o += B * nt * 4;
  w.total = o;
  return w;
}

int bv2_loudness_plan(const bv2_loudness_config* cfg, int32_t* step, int32_t* block, int32_t* tile) {
  if (int rc = loudness_check(cfg, "bv2_loudness_plan")) return rc;
  if (step) *step = loudness_step(cfg);
  if (block) *block = 4 * loudness_step(cfg);
  if (tile) *tile = LD_TILE;
  return 0;
}

int bv2_loudness_coeffs(const bv2_loudness_config* cfg, double out[10]) {
  if (int rc = loudness_check(cfg, "bv2_loudness_coeffs")) return rc;
  if (!out) { g_create_err = "bv2_loudness_coeffs: out is null"; return -1; }
  loudness_coeffs(cfg->sample_rate, out);
  return 0;
}

int64_t bv2_loudness_blocks(const bv2_loudness_config* cfg, int64_t n) {
  if (loudness_check(cfg, "bv2_loudness_blocks")) return -1;
  if (n < 0 || n > LD_MAX_S) { g_create_err = "bv2_loudness_blocks: n must be in [0, 2^31 - 4096]"; return -1; }
  return loudness_blocks(n, loudness_step(cfg));
}

int64_t bv2_loudness_workspace_bytes(const bv2_loudness_config* cfg, int32_t B, int64_t S) {
  if (loudness_check(cfg, "bv2_loudness_workspace_bytes")) return -1;
  if (B < 1 || B > LD_MAX_B || S < 1 || S > LD_MAX_S) {
    g_create_err = "bv2_loudness_workspace_bytes: B must be in [1, " + std::to_string(LD_MAX_B) + "] and S in [1, 2^31 - 4096]";
    return -1;
  }
  return loudness_ws(loudness_step(cfg), B, S).total + 256;
}

// the checks bv2_loudness_measure and bv2_loudness_gate share; returns the 8-byte aligned workspace through *ws
static int loudness_common(const char* what, const bv2_loudness_config* cfg, int32_t B, int64_t S, const int32_t* groups, int32_t n_groups,
                           void* workspace, int64_t workspace_bytes, int64_t need, unsigned char** ws) {
  if (int rc = loudness_check(cfg, what)) return rc;
  auto fail = [&](const std::string& m, int rc) { g_create_err = std::string(what) + ": " + m; return rc; };
  if (B < 1 || B > LD_MAX_B) return fail("B must be in [1, " + std::to_string(LD_MAX_B) + "]", -1);
  if (S < 1 || S > LD_MAX_S) return fail("S must be in [1, 2^31 - 4096]", -1);
  if (groups ? (n_groups < 1 || n_groups > B) : n_groups != B)
    return fail("n_groups must be in [1, B] with groups, and equal to B without", -1);
  if (!workspace || workspace_bytes < need) return fail("workspace too small (bv2_loudness_workspace_bytes)", -5);
  *ws = static_cast<unsigned char*>(workspace);
  const uintptr_t mis = reinterpret_cast<uintptr_t>(*ws) & 7u;
  if (mis) {
    if (workspace_bytes < need + 8) return fail("workspace too small (bv2_loudness_workspace_bytes)", -5);
    *ws += 8 - mis;
  }
  return 0;
}

static void loudness_gate_args(const bv2_loudness_config* cfg, LoudnessGateArgs* g, unsigned char* item_ws, const int64_t* lengths,
                               int32_t B, int64_t S, const int32_t* groups, int32_t n_groups, double target_lufs, double peak_ceiling_db) {
  g->lengths = lengths; g->S = S; g->B = B; g->groups = groups; g->n_groups = n_groups;
  g->step = loudness_step(cfg);
  g->ms_width = loudness_blocks(S, g->step);
  g->abs_ms = std::pow(10.0, (-70.0 + 0.691) / 10.0);
  g->target_lufs = target_lufs;
  g->ceiling = std::pow(10.0, peak_ceiling_db / 20.0);
  g->item_s = reinterpret_cast<double*>(item_ws);
  g->item_c = reinterpret_cast<int64_t*>(item_ws + (size_t)B * 8);
  g->sort_s = reinterpret_cast<double*>(item_ws + (size_t)B * 16);
  g->sort_c = reinterpret_cast<int64_t*>(item_ws + (size_t)B * 24);
}

int bv2_loudness_measure(bv2_stream stream, const bv2_loudness_config* cfg, const void* wav, int64_t wav_bstride, const int64_t* lengths,
                         int32_t B, int64_t S, const int32_t* groups, int32_t n_groups, double target_lufs, double peak_ceiling_db,
                         double* lufs, float* gain, float* peak, int32_t* flags, double* block_ms, void* workspace,
                         int64_t workspace_bytes) {
  const char* what = "bv2_loudness_measure";
  auto fail = [&](const std::string& m, int rc) { g_create_err = std::string(what) + ": " + m; return rc; };
  if (int rc = loudness_check(cfg, what)) return rc;
  if (!wav) return fail("wav is null", -1);
  if (!peak) return fail("peak is null", -1);
  if (wav_bstride < 0) return fail("wav_bstride must not be negative", -1);
  const bool gate = lufs || gain || flags;
  if (gate && (!lufs || !gain || !flags)) return fail("lufs, gain and flags go together: all three, or none (block_ms and peak only)", -1);
  if (!gate && !block_ms) return fail("block_ms is null in a call without lufs, gain and flags: nothing to produce", -1);
  if (!(target_lufs == target_lufs) || !(peak_ceiling_db == peak_ceiling_db) || std::isinf(target_lufs) || std::isinf(peak_ceiling_db))
    return fail("target_lufs and peak_ceiling_db must be finite", -1);
  if (!gate) { groups = nullptr; n_groups = B; }
  unsigned char* ws = nullptr;
  const LoudnessWs lay = (B >= 1 && B <= LD_MAX_B && S >= 1 && S <= LD_MAX_S) ? loudness_ws(loudness_step(cfg), B, S) : LoudnessWs{};
  if (int rc = loudness_common(what, cfg, B, S, groups, n_groups, workspace, workspace_bytes, lay.total ? lay.total : 1, &ws)) return rc;
  try {
    LoudnessArgs a;
    a.wav = wav; a.bstride = wav_bstride; a.lengths = lengths; a.B = B; a.S = S; a.step = loudness_step(cfg);
    a.input_format = cfg->input_format;
    loudness_filter(cfg->sample_rate, &a.filter);
    a.tile_z = reinterpret_cast<double*>(ws + lay.tile_z);
    a.tile_s = reinterpret_cast<double*>(ws + lay.tile_s);
    a.part = reinterpret_cast<double*>(ws + lay.part);
    a.tile_peak = reinterpret_cast<float*>(ws + lay.tile_peak);
    LoudnessGateArgs& g = a.gate;
    loudness_gate_args(cfg, &g, ws + lay.item, lengths, B, S, groups, n_groups, target_lufs, peak_ceiling_db);
    g.part = a.part; g.tile_peak = a.tile_peak; g.nt = (int)((S + LD_TILE - 1) / LD_TILE);
    g.block_ms = block_ms ? block_ms : reinterpret_cast<double*>(ws + lay.block_ms);
    g.ms_bstride = g.ms_width;
    g.gate = gate ? 1 : 0;
    g.lufs = lufs; g.gain = gain; g.peak = peak; g.flags = flags;
    if (launch_loudness_measure(static_cast<hipStream_t>(stream), a)) return fail("kernel launch failed", -6);
    return 0;
  } catch (...) { return fail("exception", -100); }
}

int bv2_loudness_gate(bv2_stream stream, const bv2_loudness_config* cfg, const double* block_ms, int64_t ms_bstride, const int64_t* lengths,
                      int32_t B, int64_t S, const float* peak, const int32_t* groups, int32_t n_groups, double target_lufs,
                      double peak_ceiling_db, double* lufs, float* gain, int32_t* flags, void* workspace, int64_t workspace_bytes) {
  const char* what = "bv2_loudness_gate";
  auto fail = [&](const std::string& m, int rc) { g_create_err = std::string(what) + ": " + m; return rc; };
  if (int rc = loudness_check(cfg, what)) return rc;
  if (!block_ms || !peak || !lufs || !gain || !flags) return fail("block_ms, peak, lufs, gain and flags must not be null", -1);
  if (!(target_lufs == target_lufs) || !(peak_ceiling_db == peak_ceiling_db) || std::isinf(target_lufs) || std::isinf(peak_ceiling_db))
    return fail("target_lufs and peak_ceiling_db must be finite", -1);
  unsigned char* ws = nullptr;
  if (int rc = loudness_common(what, cfg, B, S, groups, n_groups, workspace, workspace_bytes, (int64_t)(B > 0 ? B : 1) * 32, &ws)) return rc;
  if (ms_bstride < loudness_blocks(S, loudness_step(cfg))) return fail("ms_bstride is shorter than bv2_loudness_blocks(S)", -1);
  try {
    LoudnessGateArgs g;
    loudness_gate_args(cfg, &g, ws, lengths, B, S, groups, n_groups, target_lufs, peak_ceiling_db);
    g.part = nullptr; g.tile_peak = nullptr; g.nt = 0;
    g.block_ms = const_cast<double*>(block_ms); g.ms_bstride = ms_bstride;
    g.gate = 1;
    g.lufs = lufs; g.gain = gain; g.peak = const_cast<float*>(peak); g.flags = flags;
    if (launch_loudness_gate(static_cast<hipStream_t>(stream), g)) return fail("kernel launch failed", -6);
    return 0;
  } catch (...) { return fail("exception", -100); }
}

int bv2_loudness_apply(bv2_stream stream, const bv2_loudness_config* cfg, const void* src, int64_t src_bstride, const int64_t* lengths,
                       int32_t B, int64_t S, const int32_t* groups, int32_t n_groups, const float* gain, float* dst_f32, int16_t* dst_i16,
                       int64_t dst_bstride) {
  const char* what = "bv2_loudness_apply";
  auto fail = [&](const std::string& m, int rc) { g_create_err = std::string(what) + ": " + m; return rc; };
  if (int rc = loudness_check(cfg, what)) return rc;
  if (!src) return fail("src is null", -1);
  if (!gain) return fail("gain is null", -1);
  if ((dst_f32 != nullptr) == (dst_i16 != nullptr)) return fail("exactly one of dst_f32 / dst_i16 must be given", -1);
  if (src_bstride < 0) return fail("src_bstride must not be negative", -1);
  if (B < 1 || B > 65535) return fail("B must be in [1, 65535]", -1);
  if (S < 1 || S > LD_MAX_S) return fail("S must be in [1, 2^31 - 4096]", -1);
  if (groups ? n_groups < 1 : n_groups != B)                  // with groups the gain table may be longer than B: groups can span calls
    return fail("n_groups (the length of gain) must be at least 1 with groups, and equal to B without", -1);
  if (dst_bstride < S) return fail("dst_bstride is shorter than S", -1);
  try {
    LoudnessApplyArgs a;
    a.src = src; a.src_bstride = src_bstride; a.lengths = lengths; a.B = B; a.S = S; a.input_format = cfg->input_format;
    a.groups = groups; a.n_gain = n_groups; a.gain = gain; a.dst = dst_f32; a.dst16 = dst_i16; a.dst_bstride = dst_bstride;
    if (launch_loudness_apply(static_cast<hipStream_t>(stream), a)) return fail("kernel launch failed", -6);
    return 0;
  } catch (...) { return fail("exception", -100); }
}

// ---- true peak (kernels/truepeak.hip) ----------------------------------------------------------------------------
static_assert(BV2_TRUE_PEAK_TILE == TP_TILE, "BV2_TRUE_PEAK_TILE and TP_TILE are one number");

static int true_peak_factor(const bv2_loudness_config* c) { return c->sample_rate < 96000 ? 4 : (c->sample_rate < 192000 ? 2 : 1); }

int bv2_true_peak_plan(const bv2_loudness_config* cfg, int32_t* factor, int32_t* K) {
  if (int rc = loudness_check(cfg, "bv2_true_peak_plan")) return rc;
  const int F = true_peak_factor(cfg);
  if (F > 1) {                                                                // the table's K comes from the resampler's own plan
    bv2_resample_config r = {(int32_t)sizeof(bv2_resample_config), cfg->sample_rate, F * cfg->sample_rate, cfg->input_format};
    ResamplePlan p;
    if (int rc = resample_plan(&r, "bv2_true_peak_plan", &p)) return rc;
    if (p.L != F || p.M != 1 || p.K != TP_K) { g_create_err = "bv2_true_peak_plan: the resampler's plan is not (F, 1, 36)"; return -1; }
  }
  if (factor) *factor = F;
  if (K) *K = F > 1 ? TP_K : 0;
  return 0;
}

int64_t bv2_true_peak_workspace_bytes(const bv2_loudness_config* cfg, int32_t B, int64_t S) {
  if (loudness_check(cfg, "bv2_true_peak_workspace_bytes")) return -1;
  if (B < 1 || B > LD_MAX_B || S < 1 || S > LD_MAX_S) {
    g_create_err = "bv2_true_peak_workspace_bytes: B must be in [1, " + std::to_string(LD_MAX_B) + "] and S in [1, 2^31 - 4096]";
    return -1;
  }
  return (int64_t)B * ((S + TP_TILE - 1) / TP_TILE) * 4 + 256;
}

int bv2_true_peak(bv2_stream stream, const bv2_loudness_config* cfg, const float* taps, const void* wav, int64_t wav_bstride,
                  const int64_t* lengths, int32_t B, int64_t S, float* peak_out, void* workspace, int64_t workspace_bytes) {
  const char* what = "bv2_true_peak";
  auto fail = [&](const std::string& m, int rc) { g_create_err = std::string(what) + ": " + m; return rc; };
  int32_t F = 0;
  if (int rc = bv2_true_peak_plan(cfg, &F, nullptr)) { g_create_err = std::string(what) + ": " + g_create_err; return rc; }
  if (!wav) return fail("wav is null", -1);
  if (!peak_out) return fail("peak_out is null", -1);
  if (wav_bstride < 0) return fail("wav_bstride must not be negative", -1);
  if (F > 1 && !taps) return fail("taps is null (the DEVICE copy of bv2_resample_taps(rate, F * rate))", -1);
  const int64_t need = (B >= 1 && B <= LD_MAX_B && S >= 1 && S <= LD_MAX_S) ? (int64_t)B * ((S + TP_TILE - 1) / TP_TILE) * 4 : 1;
  unsigned char* ws = nullptr;
  if (int rc = loudness_common(what, cfg, B, S, nullptr, B, workspace, workspace_bytes, need, &ws)) return rc;
  try {
    TruePeakArgs a;
    a.wav = wav; a.bstride = wav_bstride; a.lengths = lengths; a.B = B; a.S = S; a.input_format = cfg->input_format;
    a.factor = F; a.taps = F > 1 ? taps : nullptr;
    a.tile_peak = reinterpret_cast<float*>(ws); a.peak = peak_out;
    if (launch_true_peak(static_cast<hipStream_t>(stream), a)) return fail("kernel launch failed", -6);
    return 0;
  } catch (...) { return fail("exception", -100); }
}

// ---- look-ahead true-peak limiter (kernels/limiter.hip) ------------------------------------------------------------
static_assert(BV2_LIMITER_TILE == LM_TILE && BV2_LIMITER_MAX_REACH == LM_MAX_REACH, "BV2_LIMITER_* and LM_* are one pair of numbers");

struct LimiterPlan { int H, P, F, K; };

static int limiter_plan(const bv2_limiter_config* c, const char* what, LimiterPlan* out) {
  auto fail = [&](const std::string& m) { g_create_err = std::string(what) + ": " + m; return -1; };
  if (!c) return fail("cfg is null");
  if (c->struct_bytes != (int32_t)sizeof(bv2_limiter_config)) return fail("bv2_limiter_config.struct_bytes mismatch (ABI drift)");
  if (c->reserved != 0) return fail("bv2_limiter_config.reserved must be 0");
  const bv2_loudness_config lc = {(int32_t)sizeof(bv2_loudness_config), c->sample_rate, c->input_format};
  int32_t F = 0, K = 0;
  if (int rc = bv2_true_peak_plan(&lc, &F, &K)) {                             // the rate envelope, the input format, the table's K
    const std::string m = g_create_err;
    const size_t at = m.find(": ");
    fail(at == std::string::npos ? m : m.substr(at + 2));
    return rc;
  }
  if (!(c->lookahead_ms >= 0.0) || !(c->release_ms >= 0.0) || std::isinf(c->lookahead_ms) || std::isinf(c->release_ms))
    return fail("lookahead_ms and release_ms must be finite and not negative");
  const double h = std::floor(c->lookahead_ms * c->sample_rate / 2000.0 + 0.5), p = std::floor(c->release_ms * c->sample_rate / 2000.0 + 0.5);
  const double H = std::max(1.0, h), P = std::max(H, p);
  if (H + P > (double)LM_MAX_REACH)
    return fail("H + P = " + std::to_string((long long)H) + " + " + std::to_string((long long)P) + " exceeds BV2_LIMITER_MAX_REACH = " +
                std::to_string(LM_MAX_REACH) + " samples (lookahead_ms " + std::to_string(c->lookahead_ms) + ", release_ms " +
                std::to_string(c->release_ms) + " at " + std::to_string(c->sample_rate) + " Hz)");
  out->H = (int)H; out->P = (int)P; out->F = F; out->K = K;
  return 0;
}

int bv2_limiter_plan(const bv2_limiter_config* cfg, int32_t* H, int32_t* P, int32_t* factor, int32_t* K) {
  LimiterPlan p;
  if (int rc = limiter_plan(cfg, "bv2_limiter_plan", &p)) return rc;
  if (H) *H = p.H;
  if (P) *P = p.P;
  if (factor) *factor = p.F;
  if (K) *K = p.K;
  return 0;
}

int bv2_limiter_window(const bv2_limiter_config* cfg, float* out) {
  LimiterPlan p;
  if (int rc = limiter_plan(cfg, "bv2_limiter_window", &p)) return rc;
  if (!out) { g_create_err = "bv2_limiter_window: out is null"; return -1; }
  try {
    const double pi = 3.14159265358979323846;
    std::vector<double> u((size_t)p.P + p.H + 1);
    double sum = 0;
    for (int k = -p.P; k <= p.H; ++k) {
      u[(size_t)(k + p.P)] = 0.5 + 0.5 * std::cos(pi * (double)k / (double)((k >= 0 ? p.H : p.P) + 1));
      sum += u[(size_t)(k + p.P)];
    }
    for (size_t i = 0; i < u.size(); ++i) out[i] = (float)(u[i] / sum);
    return 0;
  } catch (...) { g_create_err = "bv2_limiter_window: out of memory"; return -100; }
}

int64_t bv2_limiter_workspace_bytes(const bv2_limiter_config* cfg, int32_t B, int64_t S) {
  LimiterPlan p;
  if (limiter_plan(cfg, "bv2_limiter_workspace_bytes", &p)) return -1;
  if (B < 1 || B > 65535 || S < 1 || S > LD_MAX_S) {
    g_create_err = "bv2_limiter_workspace_bytes: B must be in [1, 65535] and S in [1, 2^31 - 4096]";
    return -1;
  }
  return (int64_t)B * S * 4 + (int64_t)B * ((S + LM_TILE - 1) / LM_TILE) * 4 + 256;
}

int bv2_limit(bv2_stream stream, const bv2_limiter_config* cfg, const float* taps, const float* window, const void* src,
              int64_t src_bstride, const int64_t* lengths, int32_t B, int64_t S, const int32_t* groups, int32_t n_groups, const float* gain,
              double ceiling_db, float* dst_f32, int16_t* dst_i16, int64_t dst_bstride, float* curve, float* min_gain,
              int64_t* limited_samples, void* workspace, int64_t workspace_bytes) {
  const char* what = "bv2_limit";
  auto fail = [&](const std::string& m, int rc) { g_create_err = std::string(what) + ": " + m; return rc; };
  LimiterPlan p;
  if (int rc = limiter_plan(cfg, what, &p)) return rc;
  if (!src) return fail("src is null", -1);
  if (!gain) return fail("gain is null", -1);
  if (p.F > 1 && !taps) return fail("taps is null (the DEVICE copy of bv2_resample_taps(rate, F * rate))", -1);
  if (!window) return fail("window is null (the DEVICE copy of bv2_limiter_window)", -1);
  if (!min_gain || !limited_samples) return fail("min_gain and limited_samples must not be null", -1);
  if ((dst_f32 != nullptr) == (dst_i16 != nullptr)) return fail("exactly one of dst_f32 / dst_i16 must be given", -1);
  if (src_bstride < 0) return fail("src_bstride must not be negative", -1);
  if (B < 1 || B > 65535) return fail("B must be in [1, 65535]", -1);
  if (S < 1 || S > LD_MAX_S) return fail("S must be in [1, 2^31 - 4096]", -1);
  if (groups ? n_groups < 1 : n_groups != B)
    return fail("n_groups (the length of gain) must be at least 1 with groups, and equal to B without", -1);
  if (dst_bstride < S) return fail("dst_bstride is shorter than S", -1);
  if (!(ceiling_db == ceiling_db) || std::isinf(ceiling_db)) return fail("ceiling_db must be finite", -1);
  const float c = (float)std::pow(10.0, ceiling_db / 20.0);
  if (!(c > 0.f) || std::isinf(c)) return fail("10^(ceiling_db / 20) is not a positive finite float", -1);
  const int64_t need = (int64_t)B * S * 4 + (int64_t)B * ((S + LM_TILE - 1) / LM_TILE) * 4;
  if (!workspace || workspace_bytes < need) return fail("workspace too small (bv2_limiter_workspace_bytes)", -5);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const uintptr_t mis = reinterpret_cast<uintptr_t>(ws) & 7u;
  if (mis) {
    if (workspace_bytes < need + 8) return fail("workspace too small (bv2_limiter_workspace_bytes)", -5);
    ws += 8 - mis;
  }
  try {
    LimitArgs a;
    a.src = src; a.src_bstride = src_bstride; a.lengths = lengths; a.B = B; a.S = S; a.input_format = cfg->input_format;
    a.factor = p.F; a.taps = p.F > 1 ? taps : nullptr;
    a.H = p.H; a.P = p.P; a.window = window;
    a.groups = groups; a.n_gain = n_groups; a.gain = gain; a.ceiling = c;
    a.dst = dst_f32; a.dst16 = dst_i16; a.dst_bstride = dst_bstride; a.curve = curve;
    a.min_gain = min_gain; a.limited_samples = limited_samples;
    a.req = reinterpret_cast<float*>(ws);
    a.tile_min = reinterpret_cast<int*>(ws + (size_t)B * S * 4);
    if (launch_limit(static_cast<hipStream_t>(stream), a)) return fail("kernel launch failed", -6);
    return 0;
  } catch (...) { return fail("exception", -100); }
}

// ---- step energies and loudness range (kernels/loudness.hip) -----------------------------------------------------
static_assert(BV2_RANGE_SHORT == LD_RANGE_SHORT && BV2_RANGE_SILENT == LD_RANGE_SILENT, "BV2_RANGE_* and LD_RANGE_* are one numbering");

int64_t bv2_loudness_steps_count(const bv2_loudness_config* cfg, int64_t n) {
  if (loudness_check(cfg, "bv2_loudness_steps_count")) return -1;
  if (n < 0 || n > LD_MAX_S) { g_create_err = "bv2_loudness_steps_count: n must be in [0, 2^31 - 4096]"; return -1; }
  return n / loudness_step(cfg);
}

int bv2_loudness_steps(bv2_stream stream, const bv2_loudness_config* cfg, const void* wav, int64_t wav_bstride, const int64_t* lengths,
                       int32_t B, int64_t S, double* step_ss, int64_t ss_bstride, float* peak, double* block_ms, void* workspace,
                       int64_t workspace_bytes) {
  const char* what = "bv2_loudness_steps";
  auto fail = [&](const std::string& m, int rc) { g_create_err = std::string(what) + ": " + m; return rc; };
  if (int rc = loudness_check(cfg, what)) return rc;
  if (!wav) return fail("wav is null", -1);
  if (!step_ss) return fail("step_ss is null", -1);
  if (wav_bstride < 0) return fail("wav_bstride must not be negative", -1);
  unsigned char* ws = nullptr;
  const LoudnessWs lay = (B >= 1 && B <= LD_MAX_B && S >= 1 && S <= LD_MAX_S) ? loudness_ws(loudness_step(cfg), B, S) : LoudnessWs{};
  if (int rc = loudness_common(what, cfg, B, S, nullptr, B, workspace, workspace_bytes, lay.total ? lay.total : 1, &ws)) return rc;
  if (ss_bstride < S / loudness_step(cfg)) return fail("ss_bstride is shorter than bv2_loudness_steps_count(S)", -1);
  try {
    LoudnessStepsArgs s;
    LoudnessArgs& a = s.m;
    a.wav = wav; a.bstride = wav_bstride; a.lengths = lengths; a.B = B; a.S = S; a.step = loudness_step(cfg);
    a.input_format = cfg->input_format;
    loudness_filter(cfg->sample_rate, &a.filter);
    a.tile_z = reinterpret_cast<double*>(ws + lay.tile_z);
    a.tile_s = reinterpret_cast<double*>(ws + lay.tile_s);
    a.part = reinterpret_cast<double*>(ws + lay.part);
    a.tile_peak = reinterpret_cast<float*>(ws + lay.tile_peak);
    LoudnessGateArgs& g = a.gate;
    loudness_gate_args(cfg, &g, ws + lay.item, lengths, B, S, nullptr, B, 0.0, 0.0);
    g.part = a.part; g.tile_peak = a.tile_peak; g.nt = (int)((S + LD_TILE - 1) / LD_TILE);
    g.block_ms = block_ms ? block_ms : reinterpret_cast<double*>(ws + lay.block_ms);
    g.ms_bstride = g.ms_width;
    g.gate = 0;
    g.lufs = nullptr; g.gain = nullptr; g.flags = nullptr;
    g.peak = peak ? peak : reinterpret_cast<float*>(ws + lay.item);           // the gate's per-item scratch is idle without a gate
    s.want_blocks = (peak || block_ms) ? 1 : 0;
    s.step_ss = step_ss; s.ss_bstride = ss_bstride; s.ss_width = S / a.step;
    if (launch_loudness_steps(static_cast<hipStream_t>(stream), s)) return fail("kernel launch failed", -6);
    return 0;
  } catch (...) { return fail("exception", -100); }
}

int64_t bv2_loudness_range_workspace_bytes(const bv2_loudness_config* cfg, int32_t B, int64_t S) {
  if (loudness_check(cfg, "bv2_loudness_range_workspace_bytes")) return -1;
  if (B < 1 || B > LD_MAX_B || S < 1 || S > LD_MAX_S) {
    g_create_err = "bv2_loudness_range_workspace_bytes: B must be in [1, " + std::to_string(LD_MAX_B) + "] and S in [1, 2^31 - 4096]";
    return -1;
  }
  return (int64_t)B * std::max<int64_t>(S / loudness_step(cfg), 1) * 8 + 256;
}

int bv2_loudness_range(bv2_stream stream, const bv2_loudness_config* cfg, const double* step_ss, int64_t ss_bstride, const int64_t* lengths,
                       int32_t B, int64_t S, const int32_t* groups, int32_t n_groups, double* lra, double* st_low, double* st_high,
                       double* max_short_term, double* max_momentary, int32_t* flags, void* workspace, int64_t workspace_bytes) {
  const char* what = "bv2_loudness_range";
  auto fail = [&](const std::string& m, int rc) { g_create_err = std::string(what) + ": " + m; return rc; };
  if (int rc = loudness_check(cfg, what)) return rc;
  if (!step_ss || !lra || !st_low || !st_high || !max_short_term || !max_momentary || !flags)
    return fail("step_ss, lra, st_low, st_high, max_short_term, max_momentary and flags must not be null", -1);
  const int64_t width = (S >= 1 && S <= LD_MAX_S) ? S / loudness_step(cfg) : 0;
  const int64_t need = (int64_t)(B > 0 && B <= LD_MAX_B ? B : 1) * std::max<int64_t>(width, 1) * 8;
  unsigned char* ws = nullptr;
  if (int rc = loudness_common(what, cfg, B, S, groups, n_groups, workspace, workspace_bytes, need, &ws)) return rc;
  if (ss_bstride < width) return fail("ss_bstride is shorter than bv2_loudness_steps_count(S)", -1);
  try {
    LoudnessRangeArgs a;
    a.step_ss = step_ss; a.ss_bstride = ss_bstride; a.ss_width = width;
    a.lengths = lengths; a.S = S; a.B = B; a.groups = groups; a.n_groups = n_groups;
    a.step = loudness_step(cfg);
    a.abs_ms = std::pow(10.0, (-70.0 + 0.691) / 10.0);
    a.st = reinterpret_cast<double*>(ws);
    a.lra = lra; a.st_low = st_low; a.st_high = st_high; a.max_short_term = max_short_term; a.max_momentary = max_momentary; a.flags = flags;
    if (launch_loudness_range(static_cast<hipStream_t>(stream), a)) return fail("kernel launch failed", -6);
    return 0;
  } catch (...) { return fail("exception", -100); }
}

// ---- documents (kernels/assemble.hip) --------------------------------------------------------------------------
static_assert(sizeof(bv2_assemble_segment) == sizeof(AssembleSegment) && offsetof(bv2_assemble_segment, samples) == offsetof(AssembleSegment, samples) &&
              offsetof(bv2_assemble_segment, hop) == offsetof(AssembleSegment, hop) && offsetof(bv2_assemble_segment, doc) == offsetof(AssembleSegment, doc),
              "bv2_assemble_segment and AssembleSegment are one layout");
static_assert(BV2_LEVEL_NONE == AS_LEVEL_NONE && BV2_LEVEL_PIECE_PEAK == AS_LEVEL_PIECE_PEAK && BV2_LEVEL_GROUP_PEAK == AS_LEVEL_GROUP_PEAK &&
              BV2_LEVEL_GAIN == AS_LEVEL_GAIN, "BV2_LEVEL_* and AS_LEVEL_* are one numbering");

// the checks every bv2_assemble_* call shares: the config and the three counts
static int assemble_check(const char* what, const bv2_assemble_config* c, int32_t n_segments, int32_t n_groups, int32_t n_docs) {
  auto fail = [&](const std::string& m) { g_create_err = std::string(what) + ": " + m; return -1; };
  if (!c) return fail("cfg is null");
  if (c->struct_bytes != (int32_t)sizeof(bv2_assemble_config)) return fail("bv2_assemble_config.struct_bytes mismatch (ABI drift)");
  if (c->output_format != BV2_WAV_F32 && c->output_format != BV2_WAV_I16) return fail("output_format must be BV2_WAV_F32 or BV2_WAV_I16");
  if (c->level < BV2_LEVEL_NONE || c->level > BV2_LEVEL_GAIN) return fail("level must be one of BV2_LEVEL_*");
  if (c->reserved != 0) return fail("bv2_assemble_config.reserved must be 0");
  if (n_segments < 1 || n_segments > AS_MAX_SEGMENTS)
    return fail("n_segments must be in [1, " + std::to_string(AS_MAX_SEGMENTS) + "], got " + std::to_string(n_segments));
  if (n_groups < 1 || n_groups > n_segments) return fail("n_groups must be in [1, n_segments], got " + std::to_string(n_groups));
  if (n_docs < 1 || n_docs > AS_MAX_DOCS) return fail("n_docs must be in [1, " + std::to_string(AS_MAX_DOCS) + "], got " + std::to_string(n_docs));
  return 0;
}

struct AssembleWs { int64_t run, doc_base, doc_seg, peaks, total; };
static AssembleWs assemble_ws(int32_t n_segments, int32_t n_docs) {
  AssembleWs w;
  w.run = 0;
  w.doc_base = w.run + 8 * ((int64_t)n_segments + 1);
  w.doc_seg = w.doc_base + 8 * (int64_t)n_docs;
  w.peaks = w.doc_seg + 4 * (((int64_t)n_docs + 2) & ~(int64_t)1);
  w.total = w.peaks + 4 * (int64_t)n_segments;
  return w;
}

int bv2_assemble_plan(const bv2_assemble_config* cfg, const bv2_assemble_segment* seg, int32_t n_segments, int32_t n_groups, int32_t n_docs,
                      int64_t* capacity, int32_t* tile) {
  const char* what = "bv2_assemble_plan";
  if (int rc = assemble_check(what, cfg, n_segments, n_groups, n_docs)) return rc;
  auto fail = [&](int i, const std::string& m) { g_create_err = std::string(what) + ": segment " + std::to_string(i) + ": " + m; return -1; };
  if (!seg || !capacity) { g_create_err = std::string(what) + ": host_segments and capacity must not be null"; return -1; }
  try {
    std::vector<int64_t> cap((size_t)n_docs, 0);
    for (int i = 0; i < n_segments; ++i) {
      const bv2_assemble_segment& s = seg[i];
      if (s.group < 0 || s.group >= n_groups) return fail(i, "group " + std::to_string(s.group) + " is outside [0, n_groups = " + std::to_string(n_groups) + ")");
      if (s.doc < 0 || s.doc >= n_docs) return fail(i, "doc " + std::to_string(s.doc) + " is outside [0, n_docs = " + std::to_string(n_docs) + ")");
      if (i && s.doc < seg[i - 1].doc) return fail(i, "document ids must be non-decreasing along the table (" + std::to_string(s.doc) + " follows " + std::to_string(seg[i - 1].doc) + ")");
      if (s.hop < 1) return fail(i, "hop must be >= 1, got " + std::to_string(s.hop));
      if (s.samples < 0) return fail(i, "samples must not be negative, got " + std::to_string(s.samples));
      if (s.samples > AS_MAX_SAMPLES) return fail(i, "samples must be at most 2^40");
      if (s.reserved != 0) return fail(i, "reserved must be 0");
      if (s.src && s.samples < 1) return fail(i, "a piece needs a cap: samples >= 1 (the row's S)");
      if (!s.src && s.length) return fail(i, "a length counter without src: a piece needs src, silence takes no counter");
      cap[(size_t)s.doc] += s.samples;
    }
    for (int d = 0; d < n_docs; ++d)
      if (cap[(size_t)d] > AS_MAX_CAPACITY) { g_create_err = std::string(what) + ": document " + std::to_string(d) + " exceeds the capacity of 2^42 samples"; return -1; }
    for (int d = 0; d < n_docs; ++d) capacity[d] = cap[(size_t)d];
    if (tile) *tile = AS_TILE;
    return 0;
  } catch (...) { g_create_err = std::string(what) + ": exception"; return -100; }
}

int64_t bv2_assemble_workspace_bytes(const bv2_assemble_config* cfg, int32_t n_segments, int32_t n_groups, int32_t n_docs) {
  if (assemble_check("bv2_assemble_workspace_bytes", cfg, n_segments, n_groups, n_docs)) return -1;
  return assemble_ws(n_segments, n_docs).total + 8;              // + 8: the call aligns the pointer it is given
}

int bv2_assemble(bv2_stream stream, const bv2_assemble_config* cfg, const bv2_assemble_segment* dev_segments, int32_t n_segments,
                 int32_t n_groups, int32_t n_docs, const float* gain, void* const* dst_bases, const int64_t* capacity, int64_t* offsets,
                 int64_t* totals, void* workspace, int64_t workspace_bytes) {
  const char* what = "bv2_assemble";
  if (int rc = assemble_check(what, cfg, n_segments, n_groups, n_docs)) return rc;
  auto fail = [&](const std::string& m, int rc) { g_create_err = std::string(what) + ": " + m; return rc; };
  if (!dev_segments || !dst_bases || !capacity || !offsets || !totals)
    return fail("dev_segments, dst_bases, capacity, offsets and totals must not be null", -1);
  if (gain && cfg->level != BV2_LEVEL_GAIN) return fail("a gain table goes with BV2_LEVEL_GAIN only", -1);
  if (cfg->max_capacity < 0 || cfg->max_capacity > AS_MAX_CAPACITY)
    return fail("cfg->max_capacity must be the largest capacity of bv2_assemble_plan, in [0, 2^42]", -1);
  const AssembleWs lay = assemble_ws(n_segments, n_docs);
  if (!workspace || workspace_bytes < lay.total) return fail("workspace too small (bv2_assemble_workspace_bytes)", -5);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  if (const uintptr_t mis = reinterpret_cast<uintptr_t>(ws) & 7u) {
    if (workspace_bytes < lay.total + 8) return fail("workspace too small (bv2_assemble_workspace_bytes)", -5);
    ws += 8 - mis;
  }
  try {
    AssembleArgs a;
    a.seg = reinterpret_cast<const AssembleSegment*>(dev_segments);
    a.n_segments = n_segments; a.n_groups = n_groups; a.n_docs = n_docs;
    a.pcm16 = cfg->output_format == BV2_WAV_I16 ? 1 : 0; a.level = cfg->level; a.max_capacity = cfg->max_capacity;
    a.gain = gain; a.dst_bases = dst_bases; a.capacity = capacity; a.offsets = offsets; a.totals = totals;
    a.run = reinterpret_cast<int64_t*>(ws + lay.run); a.doc_base = reinterpret_cast<int64_t*>(ws + lay.doc_base);
    a.doc_seg = reinterpret_cast<int*>(ws + lay.doc_seg); a.peaks = reinterpret_cast<unsigned*>(ws + lay.peaks);
    if (launch_assemble(static_cast<hipStream_t>(stream), a)) return fail("kernel launch failed", -6);
    return 0;
  } catch (...) { return fail("exception", -100); }
}

// ---- forced alignment (kernels/align.hip) ----------------------------------------------------------------------
int bv2_neg_cent(bv2_stream stream, int32_t B, int32_t inter, int32_t T, int32_t Ty, const float* z_p, const float* m_p,
                 const float* logs_p, const int64_t* x_lengths, const int64_t* y_lengths, float* neg_cent) {
  auto fail = [&](const std::string& m, int rc) { g_create_err = "bv2_neg_cent: " + m; return rc; };
  if (!z_p || !m_p || !logs_p || !neg_cent) return fail("z_p, m_p, logs_p and neg_cent must not be null", -1);
  if (B < 1 || B > 65535) return fail("B must be in [1, 65535]", -1);
  if (inter < 4 || inter % 4 || inter > NC_MAX_D) return fail("inter must be a multiple of 4 in [4, " + std::to_string(NC_MAX_D) + "]", -1);
  if (T < 1 || Ty < 1 || Ty > 65535 * 64) return fail("T must be >= 1 and Ty in [1, 4194240]", -1);
  try {
    NegCentArgs a;
    a.z_p = z_p; a.m_p = m_p; a.logs_p = logs_p; a.x_lengths = x_lengths; a.y_lengths = y_lengths; a.out = neg_cent;
    a.B = B; a.D = inter; a.T = T; a.Ty = Ty;
    if (launch_neg_cent(static_cast<hipStream_t>(stream), a)) return fail("kernel launch failed", -6);
    return 0;
  } catch (...) { return fail("exception", -100); }
}

int64_t bv2_maximum_path_workspace_bytes(int32_t B, int32_t T, int32_t Ty) {
  if (B < 1 || B > 65535 || T < 1 || T > MP_MAX_T || Ty < 1) {
    g_create_err = "bv2_maximum_path_workspace_bytes: B must be in [1, 65535], T in [1, " + std::to_string(MP_MAX_T) + "] and Ty >= 1";
    return -1;
  }
  return maximum_path_workspace_bytes(B, T, Ty);
}

int bv2_maximum_path(bv2_stream stream, int32_t B, int32_t T, int32_t Ty, const float* neg_cent, const int64_t* x_lengths,
                     const int64_t* y_lengths, int64_t* durations, float* attn, float* score, void* workspace, int64_t workspace_bytes) {
  auto fail = [&](const std::string& m, int rc) { g_create_err = "bv2_maximum_path: " + m; return rc; };
  if (!neg_cent || !durations) return fail("neg_cent and durations must not be null", -1);
  if (B < 1 || B > 65535) return fail("B must be in [1, 65535]", -1);
  if (T < 1 || T > MP_MAX_T) return fail("T must be in [1, " + std::to_string(MP_MAX_T) + "]", -1);
  if (Ty < 1) return fail("Ty must be >= 1", -1);
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u)) return fail("workspace must be a DEVICE pointer aligned to 8 bytes", -1);
  if (workspace_bytes < maximum_path_workspace_bytes(B, T, Ty)) return fail("workspace too small (bv2_maximum_path_workspace_bytes)", -5);
  try {
    MaxPathArgs a;
    a.neg_cent = neg_cent; a.x_lengths = x_lengths; a.y_lengths = y_lengths; a.durations = durations; a.attn = attn; a.score = score;
    a.bits = static_cast<unsigned long long*>(workspace); a.B = B; a.T = T; a.Ty = Ty;
    if (launch_maximum_path(static_cast<hipStream_t>(stream), a)) return fail("kernel launch failed", -6);
    return 0;
  } catch (...) { return fail("exception", -100); }
}

// spectrogram + phase A's prior -> durations in one call: enc_q, the forward flow, neg_cent, maximum_path on one workspace
namespace {
struct PlanAlign { float *z, *zp, *nc; unsigned long long* bits; void* sub; int64_t sub_bytes; };
PlanAlign plan_align(Arena& A, const Model& m, int B, int T, int Ty) {
  PlanAlign p;
  const int64_t BT = (int64_t)B * Ty;
  p.z = A.get<float>(BT * m.cfg.inter_channels);
  p.zp = A.get<float>(BT * m.cfg.inter_channels);
  p.nc = A.get<float>(BT * T);
  p.bits = A.get<unsigned long long>(maximum_path_workspace_bytes(B, T, Ty) / 8);
  const int64_t a = posterior_workspace_bytes(m, B, Ty), b = workspace_bytes(m, B, 1, Ty);   // enc_q, then the flow, share one region
  p.sub_bytes = a > b ? a : b;
  p.sub = A.get<char>(p.sub_bytes);
  return p;
}
}  // namespace

// ---- per-utterance noise seeds (kernels/rng.h) ---------------------------------------------------------------------
int bv2_set_noise_seeds(bv2_handle* h, const int64_t* seeds_dev, int32_t B) {
  if (!h) return -1;
  BV2_TRY
  if (!seeds_dev) { h->seeds = nullptr; h->seeds_B = 0; return 0; }
  if (B < 1) { h->err = "bv2_set_noise_seeds: B must be at least 1 (NULL seeds switch the seeded noise off)"; return -1; }
  h->seeds = seeds_dev; h->seeds_B = B;
  return 0;
  BV2_CATCH(h)
}

int bv2_seeded_noise(bv2_stream stream, const int64_t* seeds_dev, int32_t B, int32_t which, int32_t rows, int32_t T,
                     const int64_t* lengths_dev, float* out, int64_t bstride, int64_t rstride, int64_t tstride) {
  auto bad = [&](const char* m) { g_create_err = std::string("bv2_seeded_noise: ") + m; return -1; };
  try {
    if (!seeds_dev) return bad("seeds is null");
    if (!out) return bad("out is null");
    if (B < 1 || B > 65535) return bad("need 1 <= B <= 65535");
    if (which < 0 || which > 2) return bad("which is 0 (noise_w), 1 (noise_z) or 2 (noise_q)");
    if (rows < 1 || rows > 65535) return bad("need 1 <= rows <= 65535");
    if (T < 1) return bad("T must be at least 1");
    if (launch_seeded_noise(static_cast<hipStream_t>(stream), seeds_dev, B, which, rows, T, lengths_dev, out, bstride, rstride, tstride))
      return bad("kernel launch failed");
    return 0;
  } catch (...) { return -100; }
}

int64_t bv2_align_workspace_bytes(const bv2_handle* h, int B, int T, int Ty) {
  if (!h || B < 1 || T < 1 || T > MP_MAX_T || Ty < 1) return -1;
  Arena A(nullptr, 0);
  plan_align(A, h->model, B, T, Ty);
  return A.off + 256;
}

int bv2_align(bv2_handle* h, bv2_stream stream, int B, int T, int Ty, const float* m_p, const float* logs_p, const int64_t* x_lengths,
              const float* y, const int64_t* y_lengths, const float* g, const float* noise_q, int64_t* durations, float* attn,
              float* score, void* ws, int64_t wsb) {
  if (int rc = ready(h, ws)) return rc;
  BV2_TRY
  if (!h->blob[kPosterior].dev) {
    h->err = "bv2_align: no posterior weights attached (bv2_posterior_pack + bv2_posterior_attach; release checkpoints written by "
             "compress_model.py are stripped of enc_q.*)";
    return -8;
  }
  if (B < 1 || B > 65535 || T < 1 || T > MP_MAX_T || Ty < 1 || !m_p || !logs_p || !x_lengths || !y || !y_lengths || !g || !durations) {
    h->err = "bv2_align: bad argument (T <= " + std::to_string(MP_MAX_T) + ")";
    return -1;
  }
  const int C = h->model.cfg.inter_channels;
  if (C % 4 || C > NC_MAX_D) { h->err = "bv2_align: inter_channels must be a multiple of 4, at most " + std::to_string(NC_MAX_D); return -1; }
  Arena A(ws, wsb);
  PlanAlign P = plan_align(A, h->model, B, T, Ty);
  if (!A.ok()) { h->err = "workspace too small for bv2_align"; return -5; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = run_posterior_encode(h, s, B, Ty, y, y_lengths, g, noise_q, 1.f, P.z, nullptr, nullptr, nullptr, P.sub, P.sub_bytes)) return rc;
  if (int rc = run_flow(h, s, B, Ty, P.z, y_lengths, nullptr, g, P.zp, P.sub, P.sub_bytes, true)) return rc;
  NegCentArgs n;
  n.z_p = P.zp; n.m_p = m_p; n.logs_p = logs_p; n.x_lengths = x_lengths; n.y_lengths = y_lengths; n.out = P.nc; n.B = B; n.D = C; n.T = T; n.Ty = Ty;
  if (launch_neg_cent(s, n)) { h->err = "bv2_align: neg_cent launch failed"; return -6; }
  MaxPathArgs a;
  a.neg_cent = P.nc; a.x_lengths = x_lengths; a.y_lengths = y_lengths; a.durations = durations; a.attn = attn; a.score = score;
  a.bits = P.bits; a.B = B; a.T = T; a.Ty = Ty;
  if (launch_maximum_path(s, a)) { h->err = "bv2_align: maximum_path launch failed"; return -6; }
  return 0;
  BV2_CATCH(h)
}

// ---- hipGraph capture -----------------------------------------------------------------------------------------
struct bv2_graph {
  hipGraphExec_t exec = nullptr;
  int nodes = 0;
};

static int capture_phase(bv2_handle* h, bv2_stream stream, bv2_graph** graph, const char* what,
                         const std::function<int(hipStream_t)>& run) {
  if (!graph) { h->err = std::string(what) + ": graph is null"; return -1; }
  *graph = nullptr;
  if (!h->blob[kInference].dev) { h->err = std::string(what) + ": no weights attached"; return -4; }
  if (h->prof_on || !h->taps.empty()) { h->err = std::string(what) + ": switch profiling and taps off before capturing"; return -1; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!s) { h->err = std::string(what) + ": capture needs a non-default stream"; return -1; }
  if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    h->err = std::string(what) + ": hipStreamBeginCapture failed";
    return -6;
  }
  const int rc = run(s);
  hipGraph_t g = nullptr;
  const hipError_t e = hipStreamEndCapture(s, &g);
  if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
  if (e != hipSuccess || !g) { (void)hipGetLastError(); h->err = std::string(what) + ": hipStreamEndCapture failed"; return -6; }
  bv2_graph* out = new bv2_graph();
  size_t n = 0;
  if (hipGraphGetNodes(g, nullptr, &n) == hipSuccess) out->nodes = (int)n;
  const hipError_t ei = hipGraphInstantiate(&out->exec, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (ei != hipSuccess) { (void)hipGetLastError(); delete out; h->err = std::string(what) + ": hipGraphInstantiate failed"; return -6; }
  *graph = out;
  return 0;
}

int bv2_graph_capture_encode(bv2_handle* h, bv2_stream stream, const bv2_encode_in* in, const bv2_encode_out* out, void* ws,
                             int64_t wsb, bv2_graph** graph) {
  return bv2_graph_capture_encode_ex(h, stream, in, out, nullptr, ws, wsb, graph);
}

int bv2_graph_capture_encode_ex(bv2_handle* h, bv2_stream stream, const bv2_encode_in* in, const bv2_encode_out* out,
                                const bv2_item_controls* ic, void* ws, int64_t wsb, bv2_graph** graph) {
  return bv2_graph_capture_encode_g(h, stream, in, out, ic, nullptr, ws, wsb, graph);
}

int bv2_graph_capture_encode_g(bv2_handle* h, bv2_stream stream, const bv2_encode_in* in, const bv2_encode_out* out,
                               const bv2_item_controls* ic, const float* g, void* ws, int64_t wsb, bv2_graph** graph) {
  if (!h) return -1;
  if (int rc = check_controls(h, ic, "bv2_graph_capture_encode")) return rc;
  BV2_TRY
  if (!in || !out || in->B < 1 || in->T < 1) { h->err = "bv2_graph_capture_encode: bad argument"; return -1; }
  if (int rc = check_speaker(h, g, "bv2_graph_capture_encode")) return rc;
  return capture_phase(h, stream, graph, "bv2_graph_capture_encode",
                       [&](hipStream_t s) { return run_encode(h, s, *in, *out, ws, wsb, ic, g); });
  BV2_CATCH(h)
}

int bv2_graph_capture_decode(bv2_handle* h, bv2_stream stream, const bv2_decode_in* in, const bv2_decode_out* out, void* ws,
                             int64_t wsb, bv2_graph** graph) {
  return bv2_graph_capture_decode_ex(h, stream, in, out, nullptr, ws, wsb, graph);
}

int bv2_graph_capture_decode_ex(bv2_handle* h, bv2_stream stream, const bv2_decode_in* in, const bv2_decode_out* out,
                                const bv2_item_controls* ic, void* ws, int64_t wsb, bv2_graph** graph) {
  if (!h) return -1;
  if (int rc = check_controls(h, ic, "bv2_graph_capture_decode")) return rc;
  BV2_TRY
  if (!in || !out || in->B < 1 || in->T < 1 || in->Ty < 1 || !out->o) { h->err = "bv2_graph_capture_decode: bad argument"; return -1; }
  return capture_phase(h, stream, graph, "bv2_graph_capture_decode",
                       [&](hipStream_t s) { return run_decode(h, s, *in, *out, ws, wsb, ic); });
  BV2_CATCH(h)
}

int bv2_graph_launch(bv2_graph* g, bv2_stream stream) {
  if (!g || !g->exec) return -1;
  return hipGraphLaunch(g->exec, static_cast<hipStream_t>(stream)) == hipSuccess ? 0 : -6;
}

int bv2_graph_num_nodes(const bv2_graph* g) { return g ? g->nodes : -1; }

void bv2_graph_destroy(bv2_graph* g) {
  if (!g) return;
  if (g->exec) (void)hipGraphExecDestroy(g->exec);
  delete g;
}

int bv2_set_option(bv2_handle* h, const char* key, int value) {
  if (!h) return -1;
  BV2_TRY
  const std::string k = key ? key : "";
  if (k == "fused_resblock") h->no_fused_resblock = value == 0;
  else if (k == "fused_respair") h->no_fused_respair = value == 0;
  else if (k == "fused_boundary") h->no_fused_boundary = value == 0;
  else if (k == "x6_pair") h->no_x6_pair = value == 0;
  else if (k == "x6_pair_c64") h->no_x6_pair_c64 = value == 0;
  else if (k == "x6_pair_c16") h->no_x6_pair_c16 = value == 0;
  else if (k == "x6_pair_c128") h->x6_pair_c128 = value != 0;
  else if (k == "respair_mix") h->respair_problem_major = value == 0;
  else if (k == "respair_form") h->respair_form = value;
  else if (k == "respair_c32") h->no_respair_c32 = value == 0;
  else if (k == "f16_wn") h->f16_wn = value;
  else if (k == "f16_ni") h->f16_ni = value;
  else if (k == "f16_kv") h->no_f16_kv = !value;
  else if (k == "stage_sum") h->no_stage_sum = !value;
  else if (k == "resblock_c16") h->no_resblock_c16 = value == 0;
  else if (k == "f16_fused_ln") h->no_f16_fused_ln = value == 0;
  else if (k == "f16_ksplit") h->no_f16_ksplit = value == 0;
  else if (k == "conv_post_rows") h->no_conv_post_rows = value == 0;
  else if (k == "ups_phase_taps") h->no_ups_phase_taps = value == 0;
  else if (k == "xcd_affine") h->no_xcd_affine = value == 0;
  else if (k == "prefetch") h->prefetch = value & 3;
  else if (k == "conv_x6") h->no_conv_x6 = value == 0;
  else if (k == "conv_x3") h->no_conv_x3 = value == 0;
  else if (k == "conv_x6_c32") h->x6_narrow = value != 0;
  else if (k == "fused_dds") h->no_fused_dds = value == 0;
  else if (k == "fused_attn_o") h->no_fused_attn_o = value == 0;
  else if (k == "attn_ksplit") h->attn_ksplit = value;
  else if (k == "attn_qtile") {
    if (value != 0 && value != 16 && value != 32) { h->err = "bv2_set_option: attn_qtile is 0, 16 or 32"; return -1; }
    h->attn_qtile = value;
  }
  else if (k == "overlap_dp") h->no_overlap_dp = value == 0;
  else if (k == "lean_durations") h->no_lean_durations = value == 0;
  else if (k == "phase_b_front") h->no_phase_b_front = value == 0;
  else if (k == "kernarg_head") h->no_kernarg_head = value == 0;
  else { h->err = "bv2_set_option: unknown key '" + k + "'"; return -1; }
  return 0;
  BV2_CATCH(h)
}

int bv2_set_tap(bv2_handle* h, const char* name, float* dev_dst, int64_t cap) {
  if (!h) return -1;
  BV2_TRY
  if (!name) { h->taps.clear(); return 0; }
  if (!dev_dst || cap <= 0) { h->taps.erase(name); return 0; }
  h->taps[name] = Tap{dev_dst, cap};
  return 0;
  BV2_CATCH(h)
}

int bv2_profile_enable(bv2_handle* h, int on) {
  if (!h) return -1;
  BV2_TRY
  if (on && h->prof_pool.empty()) {
    h->prof_pool.resize(8192);
    for (auto& r : h->prof_pool) {
      if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) {
        h->err = "bv2_profile_enable: hipEventCreate failed";
        return -6;
      }
    }
  }
  h->prof_on = on != 0;
  h->prof_mode = (on >= 2 && on <= 4) ? on : 1;
  return 0;
  BV2_CATCH(h)
}

int bv2_profile_reset(bv2_handle* h) {
  if (!h) return -1;
  h->prof_used = 0;
  return 0;
}

int bv2_profile_report(bv2_handle* h, bv2_profile_row* rows, int max_rows) {
  if (!h || !rows) return -1;
  BV2_TRY
  const int nf = (int)h->prof_names.size();
  std::vector<bv2_profile_row> acc((size_t)nf);
  for (int i = 0; i < nf; ++i) {
    std::memset(&acc[i], 0, sizeof(bv2_profile_row));
    std::strncpy(acc[i].name, h->prof_names[i].c_str(), sizeof(acc[i].name) - 1);
  }
  for (size_t i = 0; i < h->prof_used; ++i) {
    const ProfileRec& r = h->prof_pool[i];
    if (hipEventSynchronize(r.e1) != hipSuccess) continue;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) continue;
    bv2_profile_row& a = acc[(size_t)r.fam];
    a.launches += 1; a.total_ms += ms; a.flops += r.flops; a.bytes += r.bytes;
  }
  int n = 0;
  for (int i = 0; i < nf && n < max_rows; ++i)
    if (acc[i].launches) rows[n++] = acc[i];
  return n;
  BV2_CATCH(h)
}

}  // extern "C"
