"""CPU: the fp64 references of tests/bert_refs.py proved against HuggingFace's formulation of the disentangled attention, the
sensitivity of every attention case's inputs to the errors the GPU tests must catch (a condition on the inputs, asserted on the
reference alone), and the refusals of the BERT kernels' launchers (they return before any device call).  This proves the references
and the inputs that tests/test_bert_kernels_gpu.py holds the kernels to, not the kernels."""
import ctypes as C

import pytest
import torch

from oracle import deberta_oracle as DO
from tests import bert_refs as R
from tests.encoder_refs import ref_attention

BAR = 2e-5            # the GPU bar of the fp32 attention cases (tests/test_bert_kernels_gpu.py)
BAR_F16 = 4e-3        # ... and of the f16 = 1 form of the W = 0 cases, which run on the same inputs


# ---------------------------------------------------------------------------------------------------------------- HuggingFace's form
def _hf_pairwise(q, k, v, pk, pq, mask, cfg):
    """DisentangledSelfAttention.disentangled_attention_bias the way transformers writes it (models/deberta_v2/modeling_deberta_v2.py),
    in fp64 on [B][H][T][D] tensors: relative_pos = bucket(q_id - k_id); the c2p index is clamp(relative_pos + span), the p2c index
    clamp(-relative_pos + span) gathered on the KEY axis of K.PQ^T and transposed."""
    B, H, T, D = q.shape
    span = DO.att_span(cfg)
    mr = cfg.get("max_relative_positions", -1)
    mr = cfg["max_position_embeddings"] if mr < 1 else mr
    ids = torch.arange(T)
    rel = ids[:, None] - ids[None, :]
    pb = cfg.get("position_buckets", -1)
    if pb > 0:
        rel = DO.log_bucket_position(rel, pb, mr).long()
    c2p_pos = torch.clamp(rel + span, 0, 2 * span - 1)
    p2c_pos = torch.clamp(-rel + span, 0, 2 * span - 1)
    score = q @ k.transpose(-1, -2)
    score = score + torch.gather(q @ pk.transpose(-1, -2), -1, c2p_pos.expand(B, H, T, T))
    score = score + torch.gather(k @ pq.transpose(-1, -2), -1, p2c_pos.expand(B, H, T, T)).transpose(-1, -2)
    pair = (mask[:, None, :, None] * mask[:, None, None, :]).bool()
    score = score.masked_fill(~pair, torch.finfo(score.dtype).min)
    return torch.softmax(score, -1) @ v


HF_CONFIGS = {
    "bucketed": dict(max_position_embeddings=48, position_buckets=8, max_relative_positions=-1),      # midpoint 4, span 8
    "mid_v3": DO.MID_V3,                                                                              # midpoint 16, span 32
    "no_buckets": dict(max_position_embeddings=48, position_buckets=-1, max_relative_positions=16),   # span 16: saturates at |r| >= 16
    "no_buckets_full": dict(max_position_embeddings=48, position_buckets=-1, max_relative_positions=-1),
}


@pytest.mark.parametrize("name,T,lens", [("bucketed", 37, (37, 20)), ("bucketed", 7, (7, 1)), ("mid_v3", 70, (70, 33)),
                                         ("no_buckets", 37, (37, 20)), ("no_buckets_full", 41, (41, 5))])
def test_reference_equals_the_huggingface_formulation(name, T, lens):
    cfg = HF_CONFIGS[name]
    B, H, D = 2, 2, 8
    P, span = cfg["max_position_embeddings"], DO.att_span(cfg)
    g = torch.Generator().manual_seed(T + span)
    q, k, v = (torch.randn(B, H * D, T, generator=g, dtype=torch.float64) for _ in range(3))
    pk, pq = (torch.randn(H, D, 2 * span, generator=g, dtype=torch.float64) for _ in range(2))
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).double()
    tab = DO.relative_index_table(cfg, P)
    got = R.ref_deberta_attention(q, k, v, pk, pq, tab, mask, P)
    hd = lambda t: t.view(B, H, D, T).transpose(2, 3)
    want = _hf_pairwise(hd(q), hd(k), hd(v), pk.transpose(1, 2), pq.transpose(1, 2), mask, cfg).transpose(2, 3).reshape(B, H * D, T)
    err = (got - want).abs().max().item()
    assert err <= 1e-12 * want.abs().max().item(), err
    assert T - 1 > span // 2                    # the sequence crosses the bucket midpoint (half the span for a table without buckets)


def test_linear_table_is_the_oracles_table_without_buckets():
    cfg = dict(max_position_embeddings=64, position_buckets=-1, max_relative_positions=-1)
    assert torch.equal(R.linear_table(64, 64), DO.relative_index_table(cfg, 64))
    cfg8 = dict(max_position_embeddings=64, position_buckets=-1, max_relative_positions=8)
    assert torch.equal(R.linear_table(64, 8), DO.relative_index_table(cfg8, 64))
    t = R.linear_table(64, 8)
    assert t.min() == 0 and t.max() == 15 and (t == 0).sum() > 1 and (t == 15).sum() > 1


def test_real_configuration_reaches_the_log_region_and_both_table_ends():
    tab, P, span, half = R.deberta_table("LARGE_V3")
    assert (P, span, half) == (512, 256, 128)
    r = torch.arange(-(P - 1), P)
    assert torch.equal(tab[r.abs() <= half], (r + span)[r.abs() <= half])          # exact up to the midpoint
    assert (tab[r.abs() > half] != (r + span)[r.abs() > half]).any()                # log-spaced beyond it
    assert (tab[1:] >= tab[:-1]).all() and (tab[1:] - tab[:-1]).max() <= 1          # monotone, slope <= 1: what the kernel's staging relies on
    for name in ("real_config", "large_h1_d128", "large_h4_d32", "t512"):
        assert R.DEBERTA_CASES[name][4] - 1 > half
    for table in ("MID_V3", ("linear", 64, 64), ("linear", 64, 8)):
        t = R.deberta_table(table)[0]
        assert (t[1:] >= t[:-1]).all() and (t[1:] - t[:-1]).max() <= 1


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def _perturbations(c):
    """name -> keyword arguments of ref_deberta_attention that make it wrong in one of the four ways, where the case has a valid pair
    the way can act on.  (a) needs a pair of valid tokens more than `half` apart.  A query with ONE valid key has probability 1 on
    it whatever the score is: a case whose longest item has one token (T = 1) cannot see any score error — it covers the tile
    tails of a one-key launch, and is exempt from all four."""
    T, half = c["T"], c["half"]
    longest = int(c["mask"].sum(1).max().item())
    if longest < 2:
        return {}
    i = torch.arange(T)
    far = ((i[:, None] - i[None, :]).abs() > half).long()
    out = {"b_index_plus_one": dict(index_shift=torch.ones(T, T, dtype=torch.long)),
           "c_no_p2c": dict(drop_p2c=True), "d_no_c2p": dict(drop_c2p=True)}
    if longest - 1 > half:
        out["a_index_plus_one_beyond_half"] = dict(index_shift=far)
    return out


@pytest.mark.parametrize("name", list(R.DEBERTA_CASES))
def test_deberta_case_inputs_expose_index_and_term_errors(name):
    c = R.deberta_case(name)
    pert = _perturbations(c)
    if name == "t1":
        assert pert == {}
        assert torch.equal(c["ref"], c["v"].double())         # out = v: what the GPU case holds the kernel to
        return
    assert {"b_index_plus_one", "c_no_p2c", "d_no_c2p"} <= set(pert)
    if name in ("real_config", "mid_h3_d32", "mid_h1_d96", "mid_h2_d128", "large_h1_d128", "large_h4_d32", "t512", "nobucket_t64",
                "nobucket_t50", "span8", "nobucket_d128"):
        assert "a_index_plus_one_beyond_half" in pert
    for what, kw in pert.items():
        wrong = R.ref_deberta_attention(c["q"], c["k"], c["v"], c["pk"], c["pq"], c["tab"], c["mask"], c["P"], **kw)
        d = R.masked_rel_err(wrong, c["ref"], c["mask"])
        print(f"\n[{name}] {what}: differs by {d:.3f}")
        assert d >= 100 * BAR, (what, d)


@pytest.mark.parametrize("B,T,lens,H,D", R.W0_CASES)
def test_w0_case_inputs_expose_a_dropped_band_logit_and_a_dropped_erv_row(B, T, lens, H, D):
    qkv, erk, erv, mask, ref = R.w0_case(B, T, lens, H, D)
    for what, wrong in (("band logit", ref_attention(qkv, mask, torch.zeros_like(erk), erv, H, 0)),
                        ("erv row", ref_attention(qkv, mask, erk, torch.zeros_like(erv), H, 0))):
        d = R.masked_rel_err(wrong, ref, mask)
        print(f"\n[W = 0, T={T} H={H} D={D}] {what} dropped: differs by {d:.3f}")
        assert d >= 100 * BAR_F16, (what, d)


def test_fp32_restatement_error_leaves_the_bar_a_margin():
    """The same formula in fp32 torch on the CPU against the fp64 reference, on the three cases the bar was argued from: of order 1e-6,
    more than 10 x below the 2e-5 bar."""
    for name in ("large_h4_d32", "large_h1_d128", "mid_h1_d96"):
        c = R.deberta_case(name)
        B, H, D, T = c["B"], c["H"], c["D"], c["T"]
        q, k, v = [t.view(B, H, D, T).transpose(2, 3) for t in (c["q"], c["k"], c["v"])]
        i = torch.arange(T)
        idx = c["tab"][(i[:, None] - i[None, :]) + c["P"] - 1]
        s = q @ k.transpose(-1, -2) + torch.gather(q @ c["pk"], -1, idx.expand(B, H, T, T)) \
            + torch.gather(k @ c["pq"], -1, idx.t().expand(B, H, T, T)).transpose(-1, -2)
        pair = (c["mask"][:, None, :, None] * c["mask"][:, None, None, :]).bool()
        o = (torch.softmax(s.masked_fill(~pair, torch.finfo(torch.float32).min), -1) @ v).transpose(2, 3).reshape(B, H * D, T)
        e = R.masked_rel_err(o, c["ref"], c["mask"])
        print(f"\n[{name}] fp32 restatement error {e:.2e}")
        assert e < BAR / 10


# ---------------------------------------------------------------------------------------------------------------- the other references
def test_ln_and_embedding_references_equal_torch_layer_norm():
    g = torch.Generator().manual_seed(3)
    B, Cc, T = 2, 24, 11
    slabs = torch.randn(3, B, Cc, T, generator=g, dtype=torch.float64)
    gamma, beta = torch.randn(Cc, generator=g, dtype=torch.float64), torch.randn(Cc, generator=g, dtype=torch.float64)
    mask = (torch.arange(T)[None, :] < torch.tensor([T, 4])[:, None]).double()
    want = torch.nn.functional.layer_norm(slabs.sum(0).transpose(1, 2), (Cc,), gamma, beta, 1e-7).transpose(1, 2) * mask[:, None]
    assert (R.ref_bert_ln(slabs, gamma, beta, 1e-7, mask) - want).abs().max().item() < 1e-12
    vocab, max_pos, tv, S = 9, 6, 2, 8
    word, pos, typ = (torch.randn(n, Cc, generator=g, dtype=torch.float64) for n in (vocab, max_pos, tv))
    ids = torch.tensor([[0, 8, -3, vocab + 5, 2, 3, 4, 5], [1, 1, 2, 2, 3, 3, 4, 4]])
    tt = torch.tensor([[0, 1, tv + 1, 0, 1, 0, 1, 0], [0] * 8])
    lens = torch.tensor([S, 3])
    x = word[ids.clamp(0, vocab - 1)] + typ[tt.clamp(0, tv - 1)] + pos[torch.tensor([0, 1, 2, 3, 4, 5, 5, 5])][None]
    want = torch.nn.functional.layer_norm(x, (Cc,), gamma, beta, 1e-12)
    want = (want * (torch.arange(S)[None, :] < lens[:, None])[..., None]).transpose(1, 2)
    assert (R.ref_bert_embed_ln(ids, tt, word, pos, typ, lens, gamma, beta, 1e-12) - want).abs().max().item() < 1e-12
    x0 = word[ids.clamp(0, vocab - 1)]
    want0 = torch.nn.functional.layer_norm(x0, (Cc,), gamma, beta, 1e-12).transpose(1, 2)
    assert (R.ref_bert_embed_ln(ids, None, word, None, None, None, gamma, beta, 1e-12) - want0).abs().max().item() < 1e-12


# ---------------------------------------------------------------------------------------------------------------- launcher refusals
def _lib():
    from bert_vits2_amd import lib as L
    lib = L.load()
    R_ = C.c_void_p
    lib.bv2_test_deberta_attn.restype = C.c_int
    lib.bv2_test_deberta_attn.argtypes = [R_, R_, C.c_int] + [R_] * 5 + [C.c_int] * 6
    lib.bv2_test_bert_ln.restype = C.c_int
    lib.bv2_test_bert_ln.argtypes = [R_, R_, C.c_int, C.c_int64, R_, R_, C.c_float, R_, R_, C.c_int, C.c_int, C.c_int, R_, C.c_uint]
    lib.bv2_test_bert_embed_ln.restype = C.c_int
    lib.bv2_test_bert_embed_ln.argtypes = [R_] * 9 + [C.c_float, R_] + [C.c_int] * 6 + [R_, C.c_uint]
    lib.bv2_test_conv1d.restype = C.c_int
    lib.bv2_test_conv1d.argtypes = ([R_] * 6 + [C.c_int] * 8 + [C.c_float, C.c_int, R_, C.c_int, R_, R_, C.c_int, C.c_int, R_, C.c_int, R_, R_,
                                    C.c_float, C.c_int, C.c_int64])
    return lib


def test_launchers_refuse_before_any_device_call():
    """Every call below must return its refusal from the host-side checks alone: this box has no device, and the pointers are not device
    memory (a launch would be an error of another kind)."""
    lib = _lib()
    buf = torch.zeros(64)                       # stands for every non-null pointer; never dereferenced
    p = C.c_void_p(buf.data_ptr())
    da = lambda **kw: lib.bv2_test_deberta_attn(None, kw.get("qkv", p), kw.get("ld", 64), kw.get("mask", p), kw.get("pk", p),
                                                kw.get("pq", p), kw.get("tab", p), p, 1, 1, kw.get("D", 64), kw.get("T", 40), kw.get("P", 64),
                                                kw.get("span", 8))
    assert da(ld=48) == -1                      # ld % 32
    assert da(ld=32) == -1                      # ld < T
    assert da(P=39) == -1                       # P < T
    assert da(span=0) == -1
    for n in ("qkv", "pk", "pq", "tab", "mask"):
        assert da(**{n: None}) == -1, n
    assert da(D=48) == -2                       # no such head dim
    assert da(D=128, P=4096) == -2              # 16 + 64 + 32 + 66 KB of LDS > 160 KB
    ln = lambda Cc: lib.bv2_test_bert_ln(None, p, 1, 0, p, p, 1e-7, None, p, 1, Cc, 8, None, 0)
    for Cc in (64, 200, 1152):
        assert ln(Cc) == -1, Cc
    assert lib.bv2_test_bert_embed_ln(None, p, None, p, None, None, None, p, p, 1e-7, p, 1, 4, 2049, 8, 8, 1, None, 0) == -1
    # an activation code the conv kernels do not have (2, the WN gate, is one they have: tests/test_wn_forms_cpu.py holds its refusals)
    assert lib.bv2_test_conv1d(None, p, p, None, p, p, 1, 32, 32, 1, 1, -1, 8, 0, 0.0, 4, None, 0, None, None, 0, 0, None, 1, None, None,
                               1.0, 1, 0) == -1
