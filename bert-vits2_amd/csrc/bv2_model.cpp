// bv2_model.cpp — packed-weight layout and the host-side packer.
//
// What the reference does on EVERY forward and we do ONCE at load:
//   * weight_norm fold  w = g * v / ||v||  over all dims but 0 (dim 0 = C_out for Conv1d, C_in for ConvTranspose1d;
//     reference models.py:513, modules.py:160-182, 226-292) — also accepts already folded `.weight` checkpoints
//     (Generator.remove_weight_norm, models.py:559-564);
// and what only a from-scratch layout can do:
//   * conv weights re-laid as [C_out/32][C_in/8][tap][C_in&1][C_out%32][(C_in%8)/2] = the MFMA A-operand fragment order,
//     one contiguous stream per 32-row output tile (bv2_kernels.h conv_w_index);
//   * conv_q/k/v fused into one projection that also emits, per head, the 2W+1 relative-key logits
//     q_i·Ek[r]/sqrt(d) (they are linear in the layer input: rows Ek·Wq/sqrt(d)); 1/sqrt(d) folded into the q rows;
//   * ConvTranspose1d split into its u polyphase stride-1 convolutions (k/u taps each);
//   * the flows' channel Flip (modules.py:374-381) folded into input/output channel permutations of pre/post,
//     so no flip ever touches HBM;
//   * enc_p.proj split into its m / logs halves (models.py:397-399).
// The layout is a pure function of bv2_config, so every rank derives identical offsets and the blob can be broadcast.
#include <cmath>
#include <cstddef>
#include <cstring>
#include <functional>

#include "bv2_internal.h"
#include "bv2_pack.h"

namespace bv2 {

namespace {

// weight_norm fold w = g * v / ||v|| over all dims but 0: v is [d0][inner], g is [d0]
void fold_weight_norm(const std::vector<float>& v, const std::vector<float>& g, int64_t d0, int64_t inner, std::vector<float>& w) {
  w.resize(v.size());
  for (int64_t a = 0; a < d0; ++a) {
    double ss = 0;
    for (int64_t i = 0; i < inner; ++i) { const double x = v[a * inner + i]; ss += x * x; }
    // torch computes the norm in fp32; a double sqrt rounded to fp32 agrees to <= 1 ulp
    const float nrm = (float)std::sqrt(ss);
    const float sc = g[a] / nrm;
    for (int64_t i = 0; i < inner; ++i) w[a * inner + i] = v[a * inner + i] * sc;
  }
}

struct Packer {
  const std::map<std::string, HostTensor>* T = nullptr;   // null => layout only
  float* blob = nullptr;
  int64_t cursor = kBlobHeaderFloats;
  std::vector<std::string> missing;
  bool emit_bf16 = false;                                  // also write the channels-last bf16 fragment stream (dec.*)
  bool emit_f16 = false;                                   // also write the fp16 fragment stream (flow Encoder convs)
  bool emit_x6 = false;                                    // also write the three-plane bf16 split of the fp32 weights (conv_x6.hip)

  bool fill() const { return blob != nullptr; }
  uint16_t* u16(int64_t off) const { return reinterpret_cast<uint16_t*>(blob + off); }   // a 16-bit stream at a float offset

  int64_t alloc(int64_t n) {
    const int64_t off = cursor;
    cursor += (n + 63) / 64 * 64;                          // 256-byte alignment
    if (fill()) std::memset(blob + off, 0, sizeof(float) * (size_t)((n + 63) / 64 * 64));
    return off;
  }

  const HostTensor* get(const std::string& key, const std::vector<int64_t>& want) {
    if (!fill()) return nullptr;
    auto it = T->find(key);
    if (it == T->end()) { missing.push_back(key); return nullptr; }
    if (it->second.shape != want) {
      std::string s = key + " (shape mismatch: got [";
      for (auto d : it->second.shape) s += std::to_string(d) + ",";
      s += "] want [";
      for (auto d : want) s += std::to_string(d) + ",";
      s += "])";
      missing.push_back(s);
      return nullptr;
    }
    return &it->second;
  }
  bool has(const std::string& key) const { return fill() && T->count(key); }

  // folded weight of a (possibly weight-normed) conv of any rank, shape = [d0][...]; norm over all dims but 0
  bool folded(const std::string& p, const std::vector<int64_t>& shape, std::vector<float>& w) {
    if (!fill()) return false;
    if (has(p + ".weight_v") || !has(p + ".weight")) {
      std::vector<int64_t> gshape(shape.size(), 1);
      gshape[0] = shape[0];
      const HostTensor* v = get(p + ".weight_v", shape);
      const HostTensor* g = get(p + ".weight_g", gshape);
      if (!v || !g) return false;
      fold_weight_norm(v->data, g->data, shape[0], (int64_t)v->data.size() / shape[0], w);
      return true;
    }
    const HostTensor* t = get(p + ".weight", shape);
    if (!t) return false;
    w = t->data;
    return true;
  }
  bool folded(const std::string& p, int d0, int d1, int k, std::vector<float>& w) { return folded(p, {d0, d1, k}, w); }

  VecW vec(const std::string& key, const std::vector<int64_t>& shape) {
    int64_t n = 1;
    for (auto d : shape) n *= d;
    VecW v; v.n = n; v.off = alloc(n);
    if (const HostTensor* t = get(key, shape)) std::memcpy(blob + v.off, t->data.data(), sizeof(float) * (size_t)n);
    return v;
  }

  // generic conv packer: src(co, ci, j) gives the folded weight, bsrc(co) the bias; every stream through its writer in bv2_pack.h
  ConvW conv(int cout, int cin, int k, bool bias, const std::function<float(int, int, int)>& src,
             const std::function<float(int)>& bsrc, bool ok) {
    ConvW c = conv_desc(cin, cout, k);
    c.w_off = alloc(conv_w_floats(c));
    c.b_off = bias ? alloc(c.cout_pad) : -1;
    if (emit_bf16 && cin % 16 == 0) c.wb_off = alloc(cl_w_floats(c));
    if (emit_f16 && cin % 16 == 0) c.wh_off = alloc(cl_w_floats(c));
    if (emit_x6 && cin % 16 == 0) c.wx_off = alloc(x6_w_floats(c));
    // ... and the two scaled fp16 planes of the "x3" form of conv_x6.hip / respair_x6.hip (1 / S_w in front)
    if (emit_x6 && cin % 16 == 0) c.wy_off = alloc(x3_region_floats(c));
    if (fill() && ok) {
      pack_f32(blob + c.w_off, cin, cout, k, src);
      if (bias) pack_bias(blob + c.b_off, cout, bsrc);
      if (c.wb_off >= 0) pack_cl_bf16(u16(c.wb_off), cin, cout, k, src);
      if (c.wx_off >= 0) pack_x6(u16(c.wx_off), cin, cout, k, src);
      if (c.wy_off >= 0) blob[c.wy_off] = pack_x3(u16(c.wy_off + X3_HDR_FLOATS), cin, cout, k, src);
      if (c.wh_off >= 0) pack_cl_f16(u16(c.wh_off), cin, cout, k, src);
    }
    return c;
  }

  // bf16-only conv (no fp32 copy): weights as a channels-last fragment stream + fp32 bias
  ConvW conv_cl(int cout, int cin, int k, const std::function<float(int, int, int)>& src,
                const std::function<float(int)>& bsrc, bool ok) {
    ConvW c = conv_cl_desc(cin, cout, k);
    c.b_off = alloc(c.cout_pad);
    c.wb_off = alloc(cl_w_floats(c));
    if (fill() && ok) {
      pack_cl_bf16(u16(c.wb_off), cin, cout, k, src);
      pack_bias(blob + c.b_off, cout, bsrc);
    }
    return c;
  }

  // plain nn.Conv1d `p` ([cout][cin][k] + bias), optional row range / channel permutations
  ConvW conv1d(const std::string& p, int cout, int cin, int k, bool bias = true, bool wn = false, int row0 = 0,
               int rows = -1, bool rev_in = false, bool rev_out = false, const std::function<int(int)>* rowmap = nullptr) {
    if (rows < 0) rows = cout;
    std::vector<float> w;
    const HostTensor* wt = nullptr;
    bool ok = true;
    if (fill()) {
      if (wn) ok = folded(p, cout, cin, k, w);
      else { wt = get(p + ".weight", {cout, cin, k}); ok = wt != nullptr; }
    }
    const float* wd = wn ? w.data() : (wt ? wt->data.data() : nullptr);
    const HostTensor* bt = bias ? get(p + ".bias", {cout}) : nullptr;
    if (bias && fill() && !bt) ok = false;
    auto src = [&](int co, int ci, int j) {
      const int sco = rowmap ? (*rowmap)(co) : row0 + (rev_out ? rows - 1 - co : co);
      const int sci = rev_in ? cin - 1 - ci : ci;
      return wd[((int64_t)sco * cin + sci) * k + j];
    };
    auto bsrc = [&](int co) { return bt->data[rowmap ? (*rowmap)(co) : row0 + (rev_out ? rows - 1 - co : co)]; };
    return conv(rows, cin, k, bias, src, bsrc, ok);
  }

  GemvW gemv(const std::string& p, int cout, int cin, bool conv_shape, bool wn = false,
             const std::function<int(int)>* rowmap = nullptr) {      // rowmap: packed row r is source row (*rowmap)(r)
    GemvW g; g.cout = cout; g.cin = cin;
    g.w_off = alloc((int64_t)cout * cin);
    g.b_off = alloc(cout);
    if (fill()) {
      std::vector<float> w;
      const float* wd = nullptr;
      if (wn) { if (folded(p, cout, cin, 1, w)) wd = w.data(); }
      else if (conv_shape) { if (auto* t = get(p + ".weight", {cout, cin, 1})) wd = t->data.data(); }
      else { if (auto* t = get(p + ".weight", {cout, cin})) wd = t->data.data(); }
      const HostTensor* b = get(p + ".bias", {cout});
      for (int r = 0; r < cout; ++r) {
        const int sr = rowmap ? (*rowmap)(r) : r;
        if (wd) std::memcpy(blob + g.w_off + (int64_t)r * cin, wd + (int64_t)sr * cin, sizeof(float) * (size_t)cin);
        if (b) blob[g.b_off + r] = b->data[sr];
      }
    }
    return g;
  }
};

EncoderW pack_encoder(Packer& P, const std::string& p, int hidden, int filter, int heads, int layers, int ksize, int gin) {
  EncoderW e;
  e.n_layers = layers; e.ksize = ksize; e.hidden = hidden; e.filter = filter; e.heads = heads;
  const int dk = hidden / heads, nr = 2 * kAttnWindow + 1;
  e.spk = P.gemv(p + ".spk_emb_linear", hidden, gin, /*conv_shape=*/false);
  for (int i = 0; i < layers; ++i) {
    EncLayerW& L = e.layer[i];
    const std::string a = p + ".attn_layers." + std::to_string(i);
    // fused q/k/v projection (reference attentions.py:264-266 runs three 1x1 convs) + relative-key logit rows
    const HostTensor *wq = P.get(a + ".conv_q.weight", {hidden, hidden, 1}), *wk = P.get(a + ".conv_k.weight", {hidden, hidden, 1}),
                     *wv = P.get(a + ".conv_v.weight", {hidden, hidden, 1});
    const HostTensor *bq = P.get(a + ".conv_q.bias", {hidden}), *bk = P.get(a + ".conv_k.bias", {hidden}),
                     *bv = P.get(a + ".conv_v.bias", {hidden});
    const HostTensor* ek = P.get(a + ".emb_rel_k", {1, nr, dk});
    const bool ok = wq && wk && wv && bq && bk && bv && ek;
    const double isq = 1.0 / std::sqrt((double)dk);        // query / sqrt(k_channels), attentions.py:280
    auto wsrc = [&](int co, int ci, int) -> float {
      if (co < hidden) return (float)(wq->data[(int64_t)co * hidden + ci] * isq);
      if (co < 2 * hidden) return wk->data[(int64_t)(co - hidden) * hidden + ci];
      if (co < 3 * hidden) return wv->data[(int64_t)(co - 2 * hidden) * hidden + ci];
      const int hh = (co - 3 * hidden) / nr, r = (co - 3 * hidden) % nr;
      double acc = 0;
      for (int c = 0; c < dk; ++c) acc += (double)ek->data[r * dk + c] * wq->data[(int64_t)(hh * dk + c) * hidden + ci];
      return (float)(acc * isq);
    };
    auto bsrc = [&](int co) -> float {
      if (co < hidden) return (float)(bq->data[co] * isq);
      if (co < 2 * hidden) return bk->data[co - hidden];
      if (co < 3 * hidden) return bv->data[co - 2 * hidden];
      const int hh = (co - 3 * hidden) / nr, r = (co - 3 * hidden) % nr;
      double acc = 0;
      for (int c = 0; c < dk; ++c) acc += (double)ek->data[r * dk + c] * bq->data[hh * dk + c];
      return (float)(acc * isq);
    };
    L.qkv = P.conv(3 * hidden + heads * nr, hidden, 1, true, wsrc, bsrc, ok);
    L.o = P.conv1d(a + ".conv_o", hidden, hidden, 1);
    L.erv = P.vec(a + ".emb_rel_v", {1, nr, dk});
    L.g1 = P.vec(p + ".norm_layers_1." + std::to_string(i) + ".gamma", {hidden});
    L.b1 = P.vec(p + ".norm_layers_1." + std::to_string(i) + ".beta", {hidden});
    const std::string f = p + ".ffn_layers." + std::to_string(i);
    // (Round 5, measured and not kept: these two convs also as the three split-bf16 planes, so that at batch 1 their split-K launches
    // run on the bf16 matrix core — config 2 3.611 / 3.596 -> 3.584 / 3.588 ms for +195 MB of blob: a split-K launch at batch 1 is 10k
    // ticks of prologue (first bytes of x and of the weights), 10k of K loop and 2k of epilogue behind a ~3 us launch gap, and only the
    // loop gets shorter; profiles/r05_ab_splitk_x6_not_kept.txt.  The kernel was deleted in round 6.)
    L.ffn1 = P.conv1d(f + ".conv_1", filter, hidden, ksize);
    L.ffn2 = P.conv1d(f + ".conv_2", hidden, filter, ksize);
    L.g2 = P.vec(p + ".norm_layers_2." + std::to_string(i) + ".gamma", {hidden});
    L.b2 = P.vec(p + ".norm_layers_2." + std::to_string(i) + ".beta", {hidden});
  }
  return e;
}

DDSW pack_dds(Packer& P, const std::string& p, int c) {
  DDSW d;
  int dil = 1;
  for (int i = 0; i < kSdpLayers; ++i) {
    DDSLayerW& L = d.l[i];
    const std::string si = std::to_string(i);
    L.dil = dil; dil *= kSdpKernel;
    L.dww = P.vec(p + ".convs_sep." + si + ".weight", {c, 1, kSdpKernel});
    L.dwb = P.vec(p + ".convs_sep." + si + ".bias", {c});
    L.c1x1 = P.conv1d(p + ".convs_1x1." + si, c, c, 1);
    L.g1 = P.vec(p + ".norms_1." + si + ".gamma", {c});
    L.b1 = P.vec(p + ".norms_1." + si + ".beta", {c});
    L.g2 = P.vec(p + ".norms_2." + si + ".gamma", {c});
    L.b2 = P.vec(p + ".norms_2." + si + ".beta", {c});
  }
  return d;
}

ConvFlowW pack_convflow(Packer& P, const std::string& p, int hid) {
  ConvFlowW f;
  f.pre_w = P.vec(p + ".pre.weight", {hid, 1, 1});
  f.pre_b = P.vec(p + ".pre.bias", {hid});
  f.convs = pack_dds(P, p + ".convs", hid);
  f.proj = P.conv1d(p + ".proj", 3 * kSdpBins - 1, hid, 1);
  return f;
}

// modules.WN `p` (the residual flow's couplings, enc_q.enc).  The gate (commons.py:98-105: tanh(first half) * sigmoid(second half)) is fused
// into in_layer's epilogue (ACT_GATE): rows are packed so that every 32-row tile holds the tanh rows of 16 channels followed by their
// sigmoid rows; the conditioning slice g_l (cond_layer rows [2H*i, 2H*(i+1)), modules.py:189-197) is permuted the same way.
// f16: in_layers / res_skip_layers also as fp16 streams in the same row order ("fp16 flow"); cond_layer never is.
WnW pack_wn(Packer& P, const std::string& p, int hid, int nl, int gin, bool f16) {
  WnW W;
  W.layers = nl;
  const std::function<int(int)> gate_row = [hid](int n) { return wn_gate_row(hid, n); };
  const std::function<int(int)> cond_row = [hid, &gate_row](int n) { return (n / (2 * hid)) * 2 * hid + gate_row(n % (2 * hid)); };
  W.cond = P.gemv(p + ".cond_layer", 2 * hid * nl, gin, true, /*wn=*/true, &cond_row);
  P.emit_f16 = f16;
  for (int i = 0; i < nl; ++i) {
    const std::string rsn = p + ".res_skip_layers." + std::to_string(i);
    W.in[i] = P.conv1d(p + ".in_layers." + std::to_string(i), 2 * hid, hid, kFlowKernel, true, true, 0, -1, false, false, &gate_row);
    // res_skip (modules.py:203-210): rows [0,H) update x, rows [H,2H) accumulate into the output; the last layer has H rows,
    // all of them output.  Two problems of ONE launch, each with its own residual target (no separate res/skip kernel).
    if (i < nl - 1) {
      W.res[i] = P.conv1d(rsn, 2 * hid, hid, 1, true, true, 0, hid);
      W.skip[i] = P.conv1d(rsn, 2 * hid, hid, 1, true, true, hid, hid);
    } else {
      W.skip[i] = P.conv1d(rsn, hid, hid, 1, true, true);
    }
  }
  P.emit_f16 = false;
  return W;
}

uint32_t hash_cfg(const bv2_config& c_in) {
  // A model with a speaker table hashes the struct as it was before spec_channels was appended (the field is not read there), so its blob —
  // header included — is byte for byte what the earlier packer wrote; a ReferenceEncoder model hashes the whole struct.
  bv2_config c = c_in;
  size_t n = sizeof(c);
  if (c.n_speakers >= 1) { n = offsetof(bv2_config, spec_channels); c.struct_bytes = (int32_t)n; }
  const unsigned char* p = reinterpret_cast<const unsigned char*>(&c);
  uint32_t h = 2166136261u;
  for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 16777619u; }
  return h;
}

// ReferenceEncoder (reference models.py:752-808), present iff n_speakers == 0.  Conv2d weights [Cout][Cin][3][3], weight-normed over all
// dims but 0 (both forms accepted, like every other conv); packed for kernels/ref_enc.hip: conv 1 as [tap][32], convs 2-6 as
// [Cout/8][Cin][tap][8] (the 8 weights a wave needs for one (channel, tap) are consecutive).  GRU and proj keep PyTorch's layout.
void pack_ref_enc(Model& m, Packer& P) {
  const bv2_config& c = m.cfg;
  RefEncW& R = m.ref_enc;
  R.present = true;
  const int C[7] = {1, 32, 32, 64, 64, 128, 128};
  int W[7], Hd[7];
  ref_enc_dims(1, c.spec_channels, Hd, W);
  for (int i = 0; i < 6; ++i) {
    const int cin = C[i], cout = C[i + 1];
    const std::string p = "ref_enc.convs." + std::to_string(i);
    R.cw[i].n = (int64_t)cout * cin * 9; R.cw[i].off = P.alloc(R.cw[i].n);
    R.cb[i] = P.vec(p + ".bias", {cout});
    if (!P.fill()) continue;
    std::vector<float> w;
    if (!P.folded(p, {cout, cin, 3, 3}, w)) continue;
    float* dst = P.blob + R.cw[i].off;
    for (int co = 0; co < cout; ++co)
      for (int ci = 0; ci < cin; ++ci)
        for (int t = 0; t < 9; ++t) {
          const float v = w[((int64_t)co * cin + ci) * 9 + t];
          if (i == 0) dst[t * 32 + co] = v;
          else dst[(((int64_t)(co / 8) * cin + ci) * 9 + t) * 8 + co % 8] = v;
        }
  }
  const int K = 128 * W[6];
  R.w_ih = P.vec("ref_enc.gru.weight_ih_l0", {384, K});
  R.w_hh = P.vec("ref_enc.gru.weight_hh_l0", {384, 128});
  R.b_ih = P.vec("ref_enc.gru.bias_ih_l0", {384});
  R.b_hh = P.vec("ref_enc.gru.bias_hh_l0", {384});
  R.pw = P.vec("ref_enc.proj.weight", {c.gin_channels, 128});
  R.pb = P.vec("ref_enc.proj.bias", {c.gin_channels});
}

int pack_all(Model& m, Packer& P) {
  const bv2_config& c = m.cfg;
  const int hid = c.hidden_channels, inter = c.inter_channels, filt = c.filter_channels, gin = c.gin_channels;
  const int half = inter / 2;

  // ---- enc_p (reference models.py:333-400)
  m.emb = P.vec("enc_p.emb.weight", {c.n_vocab, hid});
  m.tone_emb = P.vec("enc_p.tone_emb.weight", {c.n_tones, hid});
  m.lang_emb = P.vec("enc_p.language_emb.weight", {c.n_languages, hid});
  const char* bn[3] = {"enc_p.bert_proj", "enc_p.ja_bert_proj", "enc_p.en_bert_proj"};
  // (Round 5, measured and not kept: these convs also as split-bf16 planes so that at batch >= 16, where they leave the split-K regime,
  // they take conv_x6.hip — config 3 15.12 / 15.08 -> 15.06 / 15.08 ms, nothing, for +42 MB of blob: N = 128 columns per batch item gives
  // the 64x128 / 128x64 tiles one or two column tiles per item; profiles/r05_ab_x6_enc_not_kept.txt.)
  for (int i = 0; i < 3; ++i) m.bert[i] = P.conv1d(bn[i], hid, c.bert_dim, 1);
  m.enc = pack_encoder(P, "enc_p.encoder", hid, filt, c.n_heads, c.n_layers, c.kernel_size, gin);
  m.proj_m = P.conv1d("enc_p.proj", 2 * inter, hid, 1, true, false, 0, inter);
  m.proj_logs = P.conv1d("enc_p.proj", 2 * inter, hid, 1, true, false, inter, inter);

  // ---- sdp (reference models.py:148-204, 245-256)
  m.sdp_pre = P.conv1d("sdp.pre", hid, hid, 1);
  m.sdp_proj = P.conv1d("sdp.proj", hid, hid, 1);
  m.sdp_cond = P.gemv("sdp.cond", hid, gin, true);
  m.sdp_convs = pack_dds(P, "sdp.convs", hid);
  const int cf_idx[kSdpFlowsUsed] = {7, 5, 3};      // reversed(flows) minus the "useless vflow" (models.py:246-247)
  for (int i = 0; i < kSdpFlowsUsed; ++i) m.cf[i] = pack_convflow(P, "sdp.flows." + std::to_string(cf_idx[i]), hid);
  m.ea_m = P.vec("sdp.flows.0.m", {2, 1});
  m.ea_logs = P.vec("sdp.flows.0.logs", {2, 1});

  // ---- dp (reference models.py:259-299)
  m.dp_cond = P.gemv("dp.cond", hid, gin, true);
  m.dp_c1 = P.conv1d("dp.conv_1", kDpFilter, hid, kDpKernel);
  m.dp_g1 = P.vec("dp.norm_1.gamma", {kDpFilter});
  m.dp_b1 = P.vec("dp.norm_1.beta", {kDpFilter});
  m.dp_c2 = P.conv1d("dp.conv_2", kDpFilter, kDpFilter, kDpKernel);
  m.dp_g2 = P.vec("dp.norm_2.gamma", {kDpFilter});
  m.dp_b2 = P.vec("dp.norm_2.beta", {kDpFilter});
  m.dp_proj = P.conv1d("dp.proj", 1, kDpFilter, 1);

  if (c.n_speakers >= 1) m.emb_g = P.vec("emb_g.weight", {c.n_speakers, gin});
  else pack_ref_enc(m, P);                         // models.py:1047-1048: g comes from the ReferenceEncoder, there is no table

  // ---- flow, in APPLICATION order of the reverse pass (reference models.py:143-144 / 443-444)
  m.n_coupling = c.use_transformer_flow ? c.n_flow_layer : 4;
  for (int a = 0; a < m.n_coupling; ++a) {
    CouplingW& C = m.coupling[a];
    const int f = m.n_coupling - 1 - a;
    const std::string p = "flow.flows." + std::to_string(2 * f);
    // a+1 Flips have been applied before coupling a (reverse pass: Flip, C_{n-1}, Flip, ..., C_0).  They are folded into pre's input /
    // post's output channel order instead of moving data — which leaves the tensor un-flipped at the end only if their number n is even.
    // Odd n: the FIRST Flip is real data movement (flow_core, one launch per pass), the remaining n - 1 are folded
    m.flow_flip_first = (m.n_coupling % 2) == 1;
    C.flipped = m.flow_flip_first ? (a % 2) == 1 : (a % 2) == 0;
    C.pre = P.conv1d(p + ".pre", hid, half, 1, true, false, 0, -1, /*rev_in=*/C.flipped, false);
    if (c.use_transformer_flow) {
      P.emit_f16 = true;                           // BASELINE config 5 "fp16 flow": q/k/v/o and FFN convs also as fp16 streams
      C.enc = pack_encoder(P, p + ".enc", hid, filt, c.n_heads, c.n_layers_trans_flow, kFlowKernel, gin);
      P.emit_f16 = false;
    } else {
      C.wn = pack_wn(P, p + ".enc", hid, c.n_flow_layer, gin, /*f16=*/true);
    }
    C.post = P.conv1d(p + ".post", half, hid, 1, true, false, 0, -1, false, /*rev_out=*/C.flipped);
  }

  // ---- dec (reference models.py:490-564)
  const int c0 = c.upsample_initial_channel;
  P.emit_bf16 = true;
  m.conv_pre = P.conv1d("dec.conv_pre", c0, inter, 7);
  m.dec_cond = P.gemv("dec.cond", c0, gin, true);
  m.n_ups = c.n_upsamples; m.n_rbk = c.n_resblock_kernels; m.n_rbd = c.n_resblock_dilations; m.rb_type = c.resblock_type == 2 ? 2 : 1;
  m.total_up = 1;
  int ch = c0;
  for (int i = 0; i < m.n_ups; ++i) {
    UpW& U = m.ups[i];
    U.u = c.upsample_rates[i]; U.k = c.upsample_kernel_sizes[i];
    U.cin = c0 >> i; U.cout = c0 >> (i + 1);
    UpsGeom G;                                     // the polyphase split, bv2_internal.h (validate() has admitted the pair)
    if (!ups_geometry(U.u, U.k, G)) return -1;
    U.ntaps = G.ntaps;
    m.total_up *= U.u;
    std::vector<float> w;                          // folded ConvTranspose1d weight [cin][cout][k]
    const bool ok = P.folded("dec.ups." + std::to_string(i), U.cin, U.cout, U.k, w);
    const HostTensor* bt = P.get("dec.ups." + std::to_string(i) + ".bias", {U.cout});
    P.emit_bf16 = false;                           // the bf16 path uses the single channels-last form below, not the phases
    const int kfull = U.k, cout = U.cout;
    for (int ph = 0; ph < U.u; ++ph) {
      U.pad_left[ph] = G.pad_left[ph];
      U.phase[ph] = P.conv(U.cout, U.cin, G.ntaps, true,
                           [&, ph, kfull, cout](int co, int ci, int j) { return w[((int64_t)ci * cout + co) * kfull + G.tap(ph, j)]; },
                           [&](int co) { return bt->data[co]; }, ok && bt);
    }
    P.emit_bf16 = true;
    // channels-last form: tap window = union over phases; phase ph uses window taps [cl_off, cl_off + ntaps)
    U.cl_pad_left = G.cl_pad_left;
    U.cl = P.conv_cl(U.u * U.cout, U.cin, G.cl_k,
                     [&, kfull, cout](int cop, int ci, int jw) -> float {
                       const int tap = G.cl_tap(cop / cout, jw);
                       return tap < 0 ? 0.f : w[((int64_t)ci * cout + cop % cout) * kfull + tap];
                     },
                     [&, cout](int cop) { return bt->data[cop % cout]; }, ok && bt);
    ch = U.cout;
    for (int j = 0; j < m.n_rbk; ++j) {
      const int k = c.resblock_kernel_sizes[j];
      const std::string rp = "dec.resblocks." + std::to_string(i * m.n_rbk + j);
      // wide stages (the ones the LDS-tiled fp32 conv runs): the weights also as the three bf16 planes of conv_x6.hip
      P.emit_x6 = ch >= 16 && ch % 16 == 0;        // C = 16: the pair kernel only (respair_x6.hip; conv_x6.hip wants whole 32-channel chunks)
      const bool rb2 = c.resblock_type == 2;       // modules.ResBlock2: one weight-normed conv per dilation, `convs.<d>`
      for (int d = 0; d < m.n_rbd; ++d) {
        if (rb2) {
          m.rb[i][j][d][0] = P.conv1d(rp + ".convs." + std::to_string(d), ch, ch, k, true, true);
          m.rb[i][j][d][1] = ConvW();
        } else {
          m.rb[i][j][d][0] = P.conv1d(rp + ".convs1." + std::to_string(d), ch, ch, k, true, true);
          m.rb[i][j][d][1] = P.conv1d(rp + ".convs2." + std::to_string(d), ch, ch, k, true, true);
        }
      }
      P.emit_x6 = false;
      m.rbcl_w_off[i][j] = m.rbcl_b_off[i][j] = m.rb16_w_off[i][j] = m.rb16_b_off[i][j] = -1;
      if (rb2) continue;                           // the fused / whole-ResBlock streams describe (conv, conv) pairs: ResBlock1 only
      // narrow stages: the 2*n_rbd convs of the block once more as ONE contiguous bf16 stream (+ one bias block) for the
      // whole-ResBlock kernel, and at C = 16 as the tap-pair stream of resblock_c16_bf16.hip; both rearranged from the per-conv
      // bf16 streams just written (bv2_pack.h: same bf16 values)
      const bool rbcl = m.n_rbd <= BV2_RBCL_MAX_D && resblock_cl_bf16_supported(ch, k, c.resblock_dilation_sizes[j], m.n_rbd);
      if (rbcl) {
        m.rbcl_w_off[i][j] = P.alloc((rbcl_stream_units(ch, k, m.n_rbd) * 512 + 1) / 2);
        m.rbcl_b_off[i][j] = P.alloc((int64_t)2 * m.n_rbd * kRbclBiasRow);
      }
      const bool rb16 = m.n_rbd <= BV2_RBCL_MAX_D && resblock_c16_bf16_supported(ch, k, c.resblock_dilation_sizes[j], m.n_rbd);
      if (rb16) {
        m.rb16_w_off[i][j] = P.alloc((rb16_stream_units(k, m.n_rbd) * 512 + 1) / 2);
        m.rb16_b_off[i][j] = P.alloc((int64_t)2 * m.n_rbd * kRb16BiasRow);
      }
      if (!P.fill()) continue;
      for (int s = 0; s < 2 * m.n_rbd; ++s) {
        const ConvW& cw = m.rb[i][j][s / 2][s % 2];
        if (rbcl) rbcl_put_conv(P.u16(m.rbcl_w_off[i][j]), P.blob + m.rbcl_b_off[i][j], s, P.u16(cw.wb_off), P.blob + cw.b_off, ch, k);
        if (rb16) rb16_put_conv(P.u16(m.rb16_w_off[i][j]), P.blob + m.rb16_b_off[i][j], s, P.u16(cw.wb_off), P.blob + cw.b_off, k);
      }
    }
  }
  P.emit_bf16 = false;
  m.post_c = ch;
  m.conv_post = P.vec("dec.conv_post.weight", {1, ch, m.post_k});
  P.alloc(2048);                                  // slack: weight prefetch rings run up to 4 units (4 KB) past a stream's end
  return 0;
}

// The accepted hyper-parameter envelope == the tested one (bert_vits2_amd/hparams.py ENVELOPE holds the same numbers; tests/test_envelope_cpu.py
// checks both sides agree and that every bound below rejects).  Its corners are pinned on the GPU against goldens of the real reference
// (oracle/cases.ENVELOPE), its interior against the oracle (cases.random_hparams).  Round 5 accepted far more than anything ran — and an accepted,
// never-run config (odd coupling count) had been wrong for four rounds.
int validate(const bv2_config& c, std::string& err) {
  auto bad = [&](const char* s) { err = s; return -1; };
  auto in = [](int v, int lo, int hi) { return v >= lo && v <= hi; };
  if (c.struct_bytes != (int32_t)sizeof(bv2_config)) return bad("bv2_config.struct_bytes does not match this library");
  if (c.n_vocab < 1 || c.n_tones < 1 || c.n_languages < 1 || c.bert_dim < 8 || c.bert_dim % 8)
    return bad("n_vocab / n_tones / n_languages must be >= 1 and bert_dim a multiple of 8");
  if (c.n_heads < 1 || c.hidden_channels % c.n_heads) return bad("hidden_channels must be divisible by n_heads (attentions.py:223)");
  if (!in(c.hidden_channels, 96, 256) || c.hidden_channels % 32) return bad("hidden_channels must be a multiple of 32 in 96..256");
  const int dk = c.hidden_channels / c.n_heads;
  if (dk % 32 || dk > 128) return bad("head dim (hidden_channels / n_heads) must be 32, 64, 96 or 128");
  if (!in(c.filter_channels, 128, 1024) || c.filter_channels % 64) return bad("filter_channels must be a multiple of 64 in 128..1024");
  if (!in(c.inter_channels, 64, 256) || c.inter_channels % 32) return bad("inter_channels must be a multiple of 32 in 64..256");
  if (c.kernel_size != 1 && c.kernel_size != 3 && c.kernel_size != 5 && c.kernel_size != 7) return bad("FFN kernel_size must be 1, 3, 5 or 7");
  if (!in(c.n_layers, kCondLayer + 1, 8)) return bad("n_layers must be 3..8 (cond_layer_idx = 2 < n_layers, attentions.py:69-75)");
  if (c.use_transformer_flow && !in(c.n_layers_trans_flow, kCondLayer + 1, 8)) return bad("n_layers_trans_flow must be 3..8");
  if (!in(c.n_flow_layer, 1, kMaxFlows)) return bad("n_flow_layer must be 1..8");
  if (c.n_speakers < 0) return bad("n_speakers must be >= 0");
  // n_speakers == 0: g = ref_enc(y) (models.py:1047-1048).  The spectrogram widths pinned against the reference: two odd chains and an even one
  if (c.n_speakers == 0 && c.spec_channels != 1025 && c.spec_channels != 513 && c.spec_channels != 80)
    return bad("spec_channels must be 1025, 513 or 80 when n_speakers == 0 (ReferenceEncoder, models.py:752-808)");
  if (!in(c.gin_channels, 64, 768) || c.gin_channels % 64) return bad("gin_channels must be a multiple of 64 in 64..768");
  if (!in(c.n_upsamples, 2, 5)) return bad("2..5 upsampling stages supported");
  if (!in(c.n_resblock_kernels, 1, 3)) return bad("1..3 resblock kernels supported");
  if (c.resblock_type != 1 && c.resblock_type != 2) return bad("resblock_type must be 1 (ResBlock1) or 2 (ResBlock2)");
  // modules.ResBlock1 reads dilation[0..2], ResBlock2 dilation[0..1] and ignores the rest (modules.py:208-258, 318-346): hand over exactly those
  if (c.resblock_type == 1 && c.n_resblock_dilations != 3) return bad("ResBlock1 has exactly three (dilated conv, conv) pairs: n_resblock_dilations must be 3");
  if (c.resblock_type == 2 && c.n_resblock_dilations != 2) return bad("ResBlock2 has exactly two convs (dilation[0], dilation[1]: modules.py:318-346)");
  for (int i = 0; i < c.n_upsamples; ++i) {
    const int u = c.upsample_rates[i], k = c.upsample_kernel_sizes[i];
    if (!in(u, 2, BV2_MAX_UPS)) return bad("upsample rates must be 2..8");
    if (k < u || k % u || (k - u) % 2 || k / u > 4) return bad("upsample kernel must be 1..4 x its rate with even (kernel - rate)");
  }
  // 512 = the released width; a 1024-channel channels-last bf16 ConvTranspose tile does not fit the 160 KB LDS (gen_bf16.hip conv_cl_bf16_supported)
  if (!in(c.upsample_initial_channel, 64, 512) || c.upsample_initial_channel % (1 << c.n_upsamples))
    return bad("upsample_initial_channel must be 64..512 and divisible by 2^n_upsamples");
  const int fw = c.upsample_initial_channel >> c.n_upsamples;
  if (fw != 16 && fw != 32 && fw != 64) return bad("final Generator width (upsample_initial_channel >> n_upsamples) must be 16, 32 or 64");
  for (int j = 0; j < c.n_resblock_kernels; ++j) {
    if (c.resblock_kernel_sizes[j] % 2 == 0 || !in(c.resblock_kernel_sizes[j], 3, 11)) return bad("resblock kernels must be odd, 3..11");
    for (int d = 0; d < c.n_resblock_dilations; ++d)
      if (!in(c.resblock_dilation_sizes[j][d], 1, 12)) return bad("resblock dilations must be 1..12");
  }
  return 0;
}

// enc_q (models.py:448-487) into its own blob: the WN stack exactly as the residual flow's (without fp16 streams), pre with an odd cin on
// the cin_pad route, proj split into m / logs
void pack_posterior(const bv2_config& c, PosteriorW& W, Packer& P) {
  const int hid = c.hidden_channels, inter = c.inter_channels;
  W.pre = P.conv1d("enc_q.pre", hid, W.spec, 1);
  W.wn = pack_wn(P, "enc_q.enc", hid, kPosteriorLayers, c.gin_channels, /*f16=*/false);
  W.proj_m = P.conv1d("enc_q.proj", 2 * inter, hid, 1, true, false, 0, inter);
  W.proj_logs = P.conv1d("enc_q.proj", 2 * inter, hid, 1, true, false, inter, inter);
  P.alloc(2048);                                  // slack, as the inference blob's
}

// the forward duration predictor's blob: every DDSConv and ConvFlow through pack_dds / pack_convflow, as the inference blob's
void pack_sdp_forward(const bv2_config& c, SdpForwardW& W, Packer& P) {
  const int hid = c.hidden_channels;               // models.py:159: the predictor's filter_channels is its in_channels
  W.post_pre_w = P.vec("sdp.post_pre.weight", {hid, 1, 1});
  W.post_pre_b = P.vec("sdp.post_pre.bias", {hid});
  W.post_convs = pack_dds(P, "sdp.post_convs", hid);
  W.post_proj = P.conv1d("sdp.post_proj", hid, hid, 1);
  W.post_ea_m = P.vec("sdp.post_flows.0.m", {2, 1});
  W.post_ea_logs = P.vec("sdp.post_flows.0.logs", {2, 1});
  for (int i = 0; i < kSdpFlows; ++i) W.post_cf[i] = pack_convflow(P, "sdp.post_flows." + std::to_string(2 * i + 1), hid);
  W.cf_first = pack_convflow(P, "sdp.flows.1", hid);
  P.alloc(2048);                                  // slack, as the inference blob's
}

// The two passes every blob takes.  First: `pack` on a Packer without tensors walks the layout, which gives the blob's length.  Second: the
// same walk with the tensors writes `blob`; what it could not find or fit is reported, and the header goes in last.
template <class Pack>
void lay_out(WeightBlob& b, uint32_t cfg_hash, const Pack& pack) {
  Packer P;
  pack(P);
  b.total_floats = P.cursor;
  b.cfg_hash = cfg_hash;
}
template <class Pack>
int fill_blob(BlobKind kind, const WeightBlob& b, float* blob, std::string& err, const Pack& pack) {
  const BlobDesc& d = kBlobDesc[kind];
  Packer P;
  P.T = &b.tensors;
  P.blob = blob;
  std::memset(blob, 0, sizeof(float) * kBlobHeaderFloats);
  pack(P);
  if (!P.missing.empty()) {
    err = std::string(d.noun) + ": missing/invalid tensors (" + std::to_string(P.missing.size()) + "): ";
    for (size_t i = 0; i < P.missing.size() && i < 12; ++i) err += P.missing[i] + "; ";
    return -2;
  }
  if (P.cursor != b.total_floats) { err = std::string(d.noun) + ": internal: layout drift between passes"; return -4; }
  write_blob_header(blob, d.magic, d.layout, b.cfg_hash, b.total_floats);
  return 0;
}

}  // namespace

bool posterior_key(const std::string& key) { return key.compare(0, 6, "enc_q.") == 0; }
bool sdp_forward_key(const std::string& key) { return key.compare(0, 9, "sdp.post_") == 0 || key.compare(0, 12, "sdp.flows.1.") == 0; }
bool inference_key(const std::string& key) { return !posterior_key(key) && !sdp_forward_key(key); }

int build_layout(Model& m, WeightBlob& b, std::string& err) {
  if (int rc = validate(m.cfg, err)) return rc;
  lay_out(b, hash_cfg(m.cfg), [&](Packer& P) { pack_all(m, P); });
  return 0;
}
int pack_blob(const Model& m_in, const WeightBlob& b, float* blob, std::string& err) {
  Model m = m_in;
  return fill_blob(kInference, b, blob, err, [&](Packer& P) { pack_all(m, P); });
}

int build_posterior_layout(const bv2_config& cfg, int spec_channels, PosteriorW& w, WeightBlob& b, std::string& err) {
  // the widths pinned against the reference (hparams.ENVELOPE["spec_channels"]), for models with a speaker table too
  if (spec_channels != 1025 && spec_channels != 513 && spec_channels != 80) {
    err = "posterior encoder: spec_channels must be 1025, 513 or 80";
    return -1;
  }
  w = PosteriorW();
  w.spec = spec_channels;
  lay_out(b, hash_cfg(cfg) * 16777619u ^ (uint32_t)spec_channels, [&](Packer& P) { pack_posterior(cfg, w, P); });
  return 0;
}
int pack_posterior_blob(const bv2_config& cfg, const PosteriorW& w_in, const WeightBlob& b, float* blob, std::string& err) {
  PosteriorW w = w_in;
  return fill_blob(kPosterior, b, blob, err, [&](Packer& P) { pack_posterior(cfg, w, P); });
}

int build_sdp_forward_layout(const bv2_config& cfg, SdpForwardW& w, WeightBlob& b, std::string& err) {
  if (!dds_fused_supported(cfg.hidden_channels)) {
    err = "forward duration predictor: hidden_channels must be 128, 192 or 256 (the whole-layer DDSConv kernel)";
    return -1;
  }
  w = SdpForwardW();
  lay_out(b, hash_cfg(cfg) * 16777619u ^ kSdpForwardMagic, [&](Packer& P) { pack_sdp_forward(cfg, w, P); });
  return 0;
}
int pack_sdp_forward_blob(const bv2_config& cfg, const SdpForwardW& w_in, const WeightBlob& b, float* blob, std::string& err) {
  SdpForwardW w = w_in;
  return fill_blob(kSdpForward, b, blob, err, [&](Packer& P) { pack_sdp_forward(cfg, w, P); });
}

}  // namespace bv2
