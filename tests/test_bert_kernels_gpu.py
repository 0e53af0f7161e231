"""GPU: the BERT / DeBERTa-v2 feature extractor's own kernels, one launch at a time through the test entry points of
include/bv2_testing.h, against the fp64 references of tests/bert_refs.py (proved on the CPU by tests/test_bert_refs_cpu.py, which also
proves that every attention case's inputs turn a wrong table index or a dropped score term into an error of order 1):

* kernels/deberta_attn.hip at every head dim (32 / 64 / 96 / 128), the reference's real table (256 buckets, P = 512, span 256) into its
  log region and to both table ends, tables without buckets and with 2 span < 32, T from 1 to P;
* kernels/bert.hip: bert_ln_kernel at every (channels per thread, slab count, token tile) the launcher dispatches, bert_embed_ln_kernel
  from C = 128 to 2048 with its id / type / position clamps, both with the B == 1 prefetch grid;
* kernels/attention.hip with window 0, the form BERT runs;
* the exact-erf GELU epilogue of kernels/conv_mfma.hip (LDS-tiled and split-K kernel), alone and as the ConvLayer's
  gelu(W x + b) * mask + residual.

Bars: attention and convs 2e-5 of the output scale over the valid positions (tests/test_kernels_gpu.py's, same fp32 MFMA arithmetic; an
fp32 torch restatement of the disentangled formula is 0.7e-6 .. 1.3e-6 from fp64); the f16 = 1 attention form that file's 4e-3; LayerNorms
1e-5 (test_layernorm_family's).  Outputs start as NaN, the padding columns of qkv are NaN, every output must be finite."""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import bert_refs as R
from tests import test_kernels_gpu as K
from tests.encoder_refs import ref_attention

pytestmark = pytest.mark.gpu

BAR, BAR_LN = 2e-5, 1e-5
P = K.P
rel_err = K.rel_err


@functools.lru_cache(maxsize=None)
def _lib():
    lib = K._lib()
    V = C.c_void_p
    lib.bv2_test_deberta_attn.restype = C.c_int
    lib.bv2_test_deberta_attn.argtypes = [V, V, C.c_int] + [V] * 5 + [C.c_int] * 6
    lib.bv2_test_bert_ln.restype = C.c_int
    lib.bv2_test_bert_ln.argtypes = [V, V, C.c_int, C.c_int64, V, V, C.c_float, V, V, C.c_int, C.c_int, C.c_int, V, C.c_uint]
    lib.bv2_test_bert_embed_ln.restype = C.c_int
    lib.bv2_test_bert_embed_ln.argtypes = [V] * 9 + [C.c_float, V] + [C.c_int] * 6 + [V, C.c_uint]
    return lib


@functools.lru_cache(maxsize=None)
def _prefetch_target():
    return torch.zeros(1 << 20, device="cuda")          # 4 MB that the spare workgroups only read


# ---------------------------------------------------------------------------------------------------------------- disentangled attention
def _run_deberta(c, ld):
    lib = _lib()
    B, H, D, T = c["B"], c["H"], c["D"], c["T"]
    packed = torch.full((B, 3 * H * D, ld), float("nan"))
    packed[:, :, :T] = torch.cat([c["q"], c["k"], c["v"]], 1)
    dev = [t.cuda() for t in (packed, c["mask"], c["pk"], c["pq"], c["tab"].float())]
    out = torch.full((B, H * D, T), float("nan"), device="cuda")
    rc = lib.bv2_test_deberta_attn(None, P(dev[0]), ld, P(dev[1]), P(dev[2]), P(dev[3]), P(dev[4]), P(out), B, H, D, T, c["P"], c["span"])
    assert rc == 0
    torch.cuda.synchronize()
    return out


# case -> deberta_attn_kernel<D / 32>: <2> real_config, t512, t1, t32, t33_ragged, t129, nobucket_t64, nobucket_t50, span8;
# <1> mid_h3_d32, large_h4_d32; <3> mid_h1_d96; <4> mid_h2_d128, large_h1_d128, nobucket_d128
@pytest.mark.parametrize("name", list(R.DEBERTA_CASES))
def test_deberta_attention(name):
    c = R.deberta_case(name)
    T = c["T"]
    ld = (T + 31) // 32 * 32
    out = _run_deberta(c, ld)
    assert torch.isfinite(out).all()
    err = R.masked_rel_err(out, c["ref"], c["mask"])
    print(f"\n[{name}] error {err:.2e}")
    assert err < BAR
    if name in ("real_config", "t33_ragged"):             # a wide row stride changes addresses only: bit-identical
        assert torch.equal(_run_deberta(c, ld + 32), out)


# ---------------------------------------------------------------------------------------------------------------- bert_ln
@functools.lru_cache(maxsize=None)
def _ln_inputs(Cc, nslab, B, T, offset=False):
    """slabs [nslab][B][C][T]: random parts (the first is `a` minus the others) of rows whose spread falls from 1 to 3e-4 with the token
    index — at a variance of 1e-7 the two eps values of the models (1e-12, 1e-7) give results a factor sqrt(2) apart; gamma, beta, and a
    mask that zeroes a tail."""
    g = torch.Generator().manual_seed(Cc * 31 + nslab * 7 + B * 1000 + T)
    parts = torch.randn(nslab, B, Cc, T, generator=g)
    if nslab > 1:
        parts[0] = torch.randn(B, Cc, T, generator=g) - parts[1:].sum(0)
    if offset:
        parts = parts + (3.0 + torch.randn(B, 1, T, generator=g))
    else:
        parts = parts * torch.tensor([3e-4, 1.0, 1e-1, 1e-2])[torch.arange(T) % 4]      # token 0 (the only one at T = 1) has the small spread
    gamma, beta = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    mask = (torch.arange(T)[None, :] < torch.tensor([max(1, T - 5), T][:B])[:, None]).float()
    return parts, gamma, beta, mask


def _run_ln(slabs_d, gamma_d, beta_d, eps, mask_d, B, Cc, T, pf=None):
    out = torch.full((B, Cc, T), float("nan"), device="cuda")
    rc = _lib().bv2_test_bert_ln(None, P(slabs_d), slabs_d.shape[0], B * Cc * T, P(gamma_d), P(beta_d), eps, P(mask_d), P(out), B, Cc, T,
                                 P(pf), 0 if pf is None else pf.numel() * 4)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    return out


def _ln_case(Cc, nslab, B, T):
    parts, gamma, beta, mask = _ln_inputs(Cc, nslab, B, T)
    sd, gd, bd, md = parts.cuda(), gamma.cuda(), beta.cuda(), mask.cuda()
    for eps in (1e-12, 1e-7):
        for m, m_d in ((None, None), (mask, md)):
            ref = R.ref_bert_ln(parts, gamma, beta, eps, m)
            err = rel_err(_run_ln(sd, gd, bd, eps, m_d, B, Cc, T), ref)
            assert err < BAR_LN, (eps, m is not None, err)
    # the two eps values are told apart by these rows
    assert rel_err(R.ref_bert_ln(parts, gamma, beta, 1e-12), R.ref_bert_ln(parts, gamma, beta, 1e-7)) > 100 * BAR_LN


# B * T = 134 > 128 keeps C = 512 / 1024 on the 8-token form: bert_ln_kernel<C / 128, nslab (0 for 3: the runtime loop), 8>
@pytest.mark.parametrize("nslab", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("Cc", [128, 256, 384, 512, 640, 768, 896, 1024])
def test_bert_ln_wide_form(Cc, nslab):
    _ln_case(Cc, nslab, 2, 67)


# B * T <= 128: bert_ln_kernel<C / 512, nslab, 2>, one token (half a workgroup idle), an odd count, two items
@pytest.mark.parametrize("B,T", [(1, 1), (1, 53), (2, 53)])
@pytest.mark.parametrize("nslab", [1, 2, 4])
@pytest.mark.parametrize("Cc", [512, 1024])
def test_bert_ln_narrow_form(Cc, nslab, B, T):
    _ln_case(Cc, nslab, B, T)


def test_bert_ln_rows_with_a_common_offset():
    """Rows of unit spread on a per-token offset of mean 3 (the mean is no longer small against the spread).  The one measured bar of this
    file: 4 x the error of F.layer_norm in fp32 against fp64 on the same rows, computed here from the reference side alone."""
    B, Cc, T, eps = 2, 768, 67, 1e-7
    parts, gamma, beta, mask = _ln_inputs(Cc, 1, B, T, offset=True)
    ref = R.ref_bert_ln(parts, gamma, beta, eps)
    restated = F.layer_norm(parts[0].transpose(1, 2), (Cc,), gamma, beta, eps).transpose(1, 2)
    bar = 4 * rel_err(restated, ref)
    err = rel_err(_run_ln(parts.cuda(), gamma.cuda(), beta.cuda(), eps, None, B, Cc, T), ref)
    print(f"\n[offset rows] kernel error {err:.2e}, fp32 F.layer_norm error {bar / 4:.2e}, bar {bar:.2e}")
    assert err < bar


@pytest.mark.parametrize("Cc,T,nslab", [(768, 67, 4), (1024, 53, 4), (512, 1, 1)])
def test_bert_ln_prefetch_grid_is_bit_identical(Cc, T, nslab):
    """B == 1 with a prefetch target: token tiles padded to a multiple of 8 workgroups plus the spare ones that only read."""
    parts, gamma, beta, mask = _ln_inputs(Cc, nslab, 1, T)
    sd, gd, bd, md = parts.cuda(), gamma.cuda(), beta.cuda(), mask.cuda()
    plain = _run_ln(sd, gd, bd, 1e-7, md, 1, Cc, T)
    assert torch.equal(_run_ln(sd, gd, bd, 1e-7, md, 1, Cc, T, pf=_prefetch_target()), plain)
    assert rel_err(plain, R.ref_bert_ln(parts, gamma, beta, 1e-7, mask)) < BAR_LN


# ---------------------------------------------------------------------------------------------------------------- bert_embed_ln
VOCAB, TYPE_VOCAB, POS_ROWS = 50, 2, 32


@functools.lru_cache(maxsize=None)
def _embed_tables(Cc):
    g = torch.Generator().manual_seed(Cc)
    word, pos, typ = (torch.randn(n, Cc, generator=g) for n in (VOCAB, POS_ROWS, TYPE_VOCAB))
    return word, pos, typ, torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)


def _run_embed(ids, tt, word, pos, typ, lengths, gamma, beta, eps, Cc, max_pos, pf=None):
    B, S = ids.shape
    d = lambda t: None if t is None else t.cuda()
    a = [d(t) for t in (ids, tt, word, pos, typ, lengths, gamma, beta)]
    out = torch.full((B, Cc, S), float("nan"), device="cuda")
    rc = _lib().bv2_test_bert_embed_ln(None, *[P(t) for t in a], eps, P(out), B, S, Cc, VOCAB, max_pos, TYPE_VOCAB, P(pf),
                                       0 if pf is None else pf.numel() * 4)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    return out


@pytest.mark.parametrize("Cc", [128, 384, 768, 1024, 2048])
def test_bert_embed_ln(Cc):
    """C = 2048: all 8 register slots live; 384 / 768: the last slot partly filled.  S = 19 tokens on a position table cut to 16 rows:
    the last three repeat row 15."""
    word, pos, typ, gamma, beta = _embed_tables(Cc)
    g = torch.Generator().manual_seed(Cc + 1)
    B, S, eps = 2, 19, 1e-12
    ids = torch.randint(0, VOCAB, (B, S), generator=g)
    tt = torch.randint(0, TYPE_VOCAB, (B, S), generator=g)
    bad_ids, bad_tt = ids.clone(), tt.clone()
    bad_ids[0, 3], bad_ids[1, 0], bad_ids[1, 18], bad_tt[0, 5], bad_tt[1, 2] = -3, VOCAB + 5, VOCAB, TYPE_VOCAB + 1, -1
    lengths = torch.tensor([19, 7])
    runs = [
        ("BertEmbeddings", ids, tt, pos, typ, None, POS_ROWS),
        ("position clamp", ids, tt, pos[:16].contiguous(), typ, None, 16),
        ("token types null", ids, None, pos, typ, None, POS_ROWS),
        ("clamped ids and types", bad_ids, bad_tt, pos[:16].contiguous(), typ, lengths, 16),
        ("DebertaV2Embeddings", ids, None, None, None, lengths, POS_ROWS),
        ("DeBERTa, clamped ids", bad_ids, None, None, None, None, POS_ROWS),
    ]
    for what, i_, t_, p_, y_, l_, mp in runs:
        ref = R.ref_bert_embed_ln(i_, t_, word, p_, y_, l_, gamma, beta, eps)
        out = _run_embed(i_, t_, word, p_, y_, l_, gamma, beta, eps, Cc, mp)
        assert rel_err(out, ref) < BAR_LN, what
        if l_ is not None:
            assert (out[1, :, 7:] == 0).all() and (out[1, :, :7] != 0).any(), what
    # the clamped ids are the table's end rows: equal to the run that names them
    named = _run_embed(bad_ids.clamp(0, VOCAB - 1), None, word, None, None, None, gamma, beta, eps, Cc, POS_ROWS)
    assert torch.equal(_run_embed(bad_ids, None, word, None, None, None, gamma, beta, eps, Cc, POS_ROWS), named)


@pytest.mark.parametrize("Cc", [768, 2048])
def test_bert_embed_ln_prefetch_grid_is_bit_identical(Cc):
    """B == 1, S = 19 (not a multiple of 8) with a prefetch target: 24 token workgroups of which 5 idle, then the spare ones."""
    word, pos, typ, gamma, beta = _embed_tables(Cc)
    g = torch.Generator().manual_seed(Cc + 2)
    ids, tt = torch.randint(0, VOCAB, (1, 19), generator=g), torch.randint(0, TYPE_VOCAB, (1, 19), generator=g)
    lengths = torch.tensor([11])
    plain = _run_embed(ids, tt, word, pos, typ, lengths, gamma, beta, 1e-7, Cc, POS_ROWS)
    assert torch.equal(_run_embed(ids, tt, word, pos, typ, lengths, gamma, beta, 1e-7, Cc, POS_ROWS, pf=_prefetch_target()), plain)
    assert rel_err(plain, R.ref_bert_embed_ln(ids, tt, word, pos, typ, lengths, gamma, beta, 1e-7)) < BAR_LN


# ---------------------------------------------------------------------------------------------------------------- plain attention, W = 0
@pytest.mark.parametrize("f16", [0, 1])
@pytest.mark.parametrize("B,T,lens,H,D", R.W0_CASES)
def test_attention_window_0(B, T, lens, H, D, f16):
    """One band logit row per head (the diagonal's) and one erv row, both non-zero (test_bert_refs_cpu.py: dropping either moves the result
    by more than 0.4 of its scale)."""
    K._attention_case(B, T, list(lens), f16, H, D, W=0, inputs=R.w0_case(B, T, lens, H, D))


def test_attention_window_0_without_relative_terms():
    """Band logits and erv row all zero: BERT's plain softmax(Q K^T / sqrt(d)) V, the form bv2_bert.cpp runs."""
    B, T, lens, H, D = 2, 300, (300, 129), 16, 64
    qkv, erk, erv, mask, _ = R.w0_case(B, T, lens, H, D)
    erk, erv = torch.zeros_like(erk), torch.zeros_like(erv)
    q, k, v = [t.view(B, H, D, T).transpose(2, 3).double() for t in qkv.split(H * D, 1)]
    pair = (mask[:, None, :, None] * mask[:, None, None, :]) != 0
    s = (q @ k.transpose(-1, -2) / math.sqrt(D)).masked_fill(~pair, -1e4)
    plain = (torch.softmax(s, -1) @ v).transpose(2, 3).reshape(B, H * D, T)
    ref = ref_attention(qkv, mask, erk, erv, H, 0)
    assert (ref - plain).abs().max().item() < 1e-12
    for f16 in (0, 1):
        K._attention_case(B, T, list(lens), f16, H, D, W=0, inputs=(qkv, erk, erv, mask, ref))


def test_attention_window_1():
    B, T, lens, H, D = 2, 100, (100, 37), 4, 32
    K._attention_case(B, T, list(lens), 0, H, D, W=1, inputs=R.w0_case(B, T, lens, H, D, W=1))


# ---------------------------------------------------------------------------------------------------------------- GELU epilogue
@functools.lru_cache(maxsize=None)
def _gelu_inputs(cin, cout, k, B, L):
    g = torch.Generator().manual_seed(cin + cout + k)
    x = torch.randn(B, cin, L, generator=g)
    w = torch.randn(cout, cin, k, generator=g) / math.sqrt(cin * k) * 1.5      # pre-activations of spread 1.5: both GELU tails and its bend
    bias, res = torch.randn(cout, generator=g), torch.randn(B, cout, L, generator=g)
    mask = (torch.arange(L)[None, :] < torch.tensor([53, 20])[:, None]).float()
    pre = F.conv1d(x.double(), w.double(), bias.double(), padding=(k - 1) // 2)
    y = F.gelu(pre)                                                                          # the erf form
    # the bar tells the erf form from the tanh approximation (up to 5e-4 apart in absolute terms)
    assert rel_err(F.gelu(pre, approximate="tanh"), y) > 2 * BAR
    return x, w, bias, res, mask, y, y * mask[:, None].double() + res.double()


# tile 0: the launcher's pick; 2: the LDS-tiled kernel's 64x128 tile forced; 6: the split-K kernel (one slab)
@pytest.mark.parametrize("tile", [0, 2, 6])
def test_conv_gelu_intermediate_dense(tile):
    """BertIntermediate: gelu(W x + b), k = 1, 256 -> 1024."""
    lib = _lib()
    B, cin, cout, k, L = 2, 256, 1024, 1, 53
    x, w, bias, res, mask, ref, _ = _gelu_inputs(cin, cout, k, B, L)
    xd = x.cuda()
    out = torch.full((B, cout, L), float("nan"), device="cuda")
    wp = torch.empty(lib.bv2_test_conv_pack_floats(cin, cout, k), device="cuda")
    rc = lib.bv2_test_conv1d(None, P(xd), P(w), P(bias), P(out), P(wp), B, cin, cout, k, 1, -1, L, tile, 0.0, 3, None, 0,
                             None, None, 0, 0, None, 1, None, None, 1.0, 1, 0)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert rel_err(out, ref) < BAR


@pytest.mark.parametrize("tile", [0, 2, 6])
def test_conv_gelu_conv_layer(tile):
    """DeBERTa-v2's ConvLayer: gelu(W x + b) * mask + residual, k = 3, 256 -> 256, lengths [53, 20]: the mask acts between the
    activation and the residual (mask_pre with RES_ADD), so the masked columns hold the residual alone."""
    lib = _lib()
    B, cin, cout, k, L = 2, 256, 256, 3, 53
    x, w, bias, res, mask, _, ref = _gelu_inputs(cin, cout, k, B, L)
    xd, rd, md = x.cuda(), res.cuda(), mask.cuda()
    out = torch.full((B, cout, L), float("nan"), device="cuda")
    wp = torch.empty(lib.bv2_test_conv_pack_floats(cin, cout, k), device="cuda")
    rc = lib.bv2_test_conv1d(None, P(xd), P(w), P(bias), P(out), P(wp), B, cin, cout, k, 1, -1, L, tile, 0.0, 3, P(rd), 1,
                             None, P(md), 1, 0, None, 1, None, None, 1.0, 1, 0)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert rel_err(out, ref) < BAR
    assert torch.equal(out[1, :, 20:].cpu(), res[1, :, 20:])
