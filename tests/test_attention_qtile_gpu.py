"""The fp32 attention kernel on 16-query tiles (v_mfma_f32_16x16x4_f32) beside the 32-query control, each forced through
bv2_test_attention_q, against the fp64 references of tests/encoder_refs.py; the merge that runs only the rounds and slots of waves
with a key tile; and the rule that picks the tile (host only).

Every output buffer is NaN before the launch.  The bounds are the ones tests/test_encoder_forms_gpu.py holds for the same
arithmetic (fp32 operands, fp32 MFMA, fp32 softmax): 2e-5 of the output scale for the plain output, for the sum of the fused-conv_o
slabs and for the key-split output after ref_split_merge; 2e-5 of the logit scale for a range's maximum, that plus 1e-5 (relative)
for its sum; the LayerNorm bound of test_key_split_attention_and_layernorm.  Each test prints its figure before it asserts.

Shapes: T in {1, 3, 4} is below window + 1; the last query tile holds 1 / 15 / 16 valid queries at T = 17 / 31, 47 / 16, 33 (16-query
tiles) and the last key tile one key at T = 33, 65; every case is ragged (lengths T, T - 13 and 1 in one launch), so queries and keys
are masked inside a tile."""
import ctypes as C
import functools
import math

import pytest
import torch

from tests import encoder_refs as R
from tests import test_encoder_forms_gpu as F

gpu = pytest.mark.gpu

W = R.WINDOW
_ATTNQ = F._ATTN + [("qtile", C.c_int)]
TAILS = [1, 3, 4, 15, 16, 17, 31, 33, 47, 65]
TILES = [16, 32]


@functools.lru_cache(maxsize=None)
def _lib():
    lib = F._lib()
    lib.bv2_test_attention_q.restype = C.c_int
    lib.bv2_test_attention_q.argtypes = [t for _, t in _ATTNQ]
    lib.bv2_test_attention_pick_qtile.restype = C.c_int
    lib.bv2_test_attention_pick_qtile.argtypes = [C.c_int] * 6
    return lib


def attention_q(**kw):
    _lib()
    return F._call("bv2_test_attention_q", _ATTNQ, **kw)


def _ragged(T):
    return (T, max(1, T - 13), 1)


def _inputs(c, H, D, T):
    HD = H * D
    packed, ld = F.pack_qkv(c["qkv"][:, :HD] / math.sqrt(D), c["qkv"][:, HD:], c["erk"], H, D, T)
    return dict(qkv=packed, ld=ld, mask=c["mask"].cuda(), erv=c["erv"].cuda(), H=H, D=D, T=T, W=W)


def _launch_fused(c, B, T, H, D, Co, wo, qt, bo=None, res=None, ks=1):
    slabs, out = F.nanf(H * ks, B, Co, T), F.nanf(B, H * D, T)
    ml = F.nanf(B, H, ks, 2, T) if ks > 1 else None
    wp = torch.empty(F.r32(Co) * ((H * D + 15) // 16 * 16), device="cuda")
    dev = lambda t: None if t is None else t.cuda()
    bo_d, res_d = dev(bo), dev(res)
    rc = attention_q(out=out, B=B, wo_host=wo, wo_pack_dev=wp, bo=bo_d, res=res_d, o_out=slabs, o_slab_stride=B * Co * T, Co=Co,
                     ksplit=ks, ml_out=ml, qtile=qt, **_inputs(c, H, D, T))
    assert torch.isnan(out).all()                          # the plain output is not written by the fused form
    return rc, slabs.cpu().double(), None if ml is None else ml.cpu().double()


# ------------------------------------------------------------------------------------------------------------------
# tails, tiny and ragged sequences: plain output and fused conv_o

@gpu
@pytest.mark.parametrize("qt", TILES)
@pytest.mark.parametrize("H,D", [(2, 96), (4, 32), (2, 64), (4, 64)])
@pytest.mark.parametrize("T", TAILS)
def test_plain_output(T, H, D, qt):
    B, lens = 3, _ragged(T)
    c = F._case(B, T, lens, H, D, 3.0)
    out = F.nanf(B, H * D, T)
    assert attention_q(out=out, B=B, qtile=qt, **_inputs(c, H, D, T)) == 0
    got, ref = out.cpu().double(), c["att"]
    assert torch.isfinite(got).all()                       # masked queries too: every column below T is written
    valid = c["mask"][:, None, :].bool().expand_as(ref)
    err, bound = (got - ref).abs()[valid].max().item(), 2e-5 * ref.abs().max().item()
    print(f"\n[plain q{qt} T={T} H={H} D={D}] max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound


@gpu
@pytest.mark.parametrize("qt", TILES)
@pytest.mark.parametrize("H,D,Co", [(2, 96, 192), (4, 32, 168), (2, 64, 72)])   # 168, 72: a last row block of 8 rows (not a multiple of 16 or 32); 72 <= 128: four waves
@pytest.mark.parametrize("T", TAILS)
def test_fused_conv_o(T, H, D, Co, qt):
    """The sum of the H head slabs is conv_o(attention) + bias + residual, bias and residual on slab 0 alone."""
    B, lens = 3, _ragged(T)
    c = F._case(B, T, lens, H, D, 3.0)
    wo, bo, res = R.conv_o_weights(H, D, Co, B, T)
    ref = R.ref_conv_o(c["att"], wo, bo, res)
    rc, slabs, _ = _launch_fused(c, B, T, H, D, Co, wo, qt, bo, res)
    assert rc == 0
    assert torch.isfinite(slabs).all()
    valid = c["mask"][:, None, :].bool().expand_as(ref)
    err, bound = (slabs.sum(0) - ref).abs()[valid].max().item(), 2e-5 * ref.abs().max().item()
    print(f"\n[fused q{qt} T={T} H={H} D={D} Co={Co}] slab sum: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    head1 = R.ref_conv_o(c["att"][:, D:2 * D], wo[:, D:2 * D])
    err1, bound1 = (slabs[1] - head1).abs()[valid].max().item(), 2e-5 * head1.abs().max().item()
    print(f"[fused] slab 1 against head 1's projection: max err {err1:.3e} (bound {bound1:.3e})")
    assert err1 <= bound1


# ------------------------------------------------------------------------------------------------------------------
# key split: 5, 5 and 12 key tiles over 2 and 4 ranges (8 waves: three to seven of them without a key tile), q x 12

def _split(B, T, lens, H, D, ks, qt, qmul=12.0, Co=192):
    c = F._case(B, T, lens, H, D, qmul)
    wo, bo, res = R.conv_o_weights(H, D, Co, B, T)
    rc, slabs, ml = _launch_fused(c, B, T, H, D, Co, wo, qt, ks=ks)
    assert rc == 0
    assert torch.isfinite(slabs).all() and torch.isfinite(ml).all()
    return c, wo, bo, res, slabs.view(H, ks, B, Co, T), ml


def _check_split(c, wo, bo, res, slabs, ml, B, T, H, ks, tag):
    ref = R.ref_conv_o(c["att"], wo, bo, res)
    got = R.ref_split_merge(slabs, ml[:, :, :, 0], ml[:, :, :, 1]) + bo.double()[None, :, None] + res.double()
    valid = c["mask"][:, None, :].bool().expand_as(ref)
    assert torch.isfinite(got).all()
    err, bound = (got - ref).abs()[valid].max().item(), 2e-5 * ref.abs().max().item()
    print(f"\n[{tag}] merged in fp64: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    logits = R.ref_logits(c["qkv"], c["mask"], c["erk"], H, W)
    smax = logits[logits > -9999.0].abs().max().item()
    vq = c["mask"][:, None, :].bool().expand(B, H, T)
    for r, (k0, k1) in enumerate(R.key_ranges(T, ks)):
        s = logits[..., k0:k1]
        m_ref = s.max(-1).values
        l_ref = torch.exp(s - m_ref[..., None]).sum(-1)
        m, l = ml[:, :, r, 0], ml[:, :, r, 1]
        em = (m - m_ref).abs()[vq].max().item()
        el = ((l * torch.exp(m - m_ref) - l_ref).abs() / l_ref)[vq].max().item()
        print(f"[{tag}] range {r} keys [{k0}, {k1}): max |m - ref| {em:.3e} (bound {2e-5 * smax:.3e}), max rel err of l {el:.3e} "
              f"(bound {2e-5 * smax + 1e-5:.3e})")
        assert em <= 2e-5 * smax
        assert el <= 2e-5 * smax + 1e-5


@gpu
@pytest.mark.parametrize("qt", TILES)
@pytest.mark.parametrize("ks", [2, 4])
@pytest.mark.parametrize("T", [130, 160, 384])
def test_key_split(T, ks, qt):
    """Slabs and (max, sum) pairs merged in fp64 are the unsplit fp64 result; the pairs are each range's own.  For the 32-query form
    this is also the check of the merge that skips the rounds of waves without a key tile (ks = 4 at T = 384: three key tiles on eight
    waves, five empty): what the parent computed is, to the bound, the fp64 reference."""
    B, H, D = 1, 2, 96
    c, wo, bo, res, slabs, ml = _split(B, T, (T,), H, D, ks, qt)
    _check_split(c, wo, bo, res, slabs, ml, B, T, H, ks, f"split q{qt} T={T} ks={ks}")


@gpu
@pytest.mark.parametrize("qt", TILES)
def test_key_split_ranges_without_a_valid_key(qt):
    """B = 2, lengths (160, 1), four ranges: item 1's only valid query sees no valid key in ranges 1 to 3.  Such a range is not empty
    for the kernel — its keys exist and are masked, every logit is the reference's -1e4 — so its pair is exactly (-1e4, number of keys)
    and its slab is the finite projection of the mean value; what is an exact zero is its weight in the merge, e^{-1e4 - M}, and with
    it the range's contribution to the output.  (A range with no key at all cannot be launched: ks > key tiles is refused.)"""
    B, T, H, D, ks = 2, 160, 2, 96, 4
    c, wo, bo, res, slabs, ml = _split(B, T, (160, 1), H, D, ks, qt)
    _check_split(c, wo, bo, res, slabs, ml, B, T, H, ks, f"masked ranges q{qt}")
    nkeys = [k1 - k0 for k0, k1 in R.key_ranges(T, ks)]
    for r in (1, 2, 3):
        assert (ml[1, :, r, 0, 0] == -1e4).all() and (ml[1, :, r, 1, 0] == float(nkeys[r])).all()
        w = ml[1, :, r, 1, 0].float() * torch.exp((ml[1, :, r, 0, 0] - ml[1, :, 0, 0, 0]).float())
        assert (w == 0).all()
        assert ((w[:, None].double() * slabs[:, r, 1, :, 0]) == 0).all()


@gpu
def test_key_split_and_layernorm():
    """16-query kernel + LayerNorm-1 (the merge, conv_o's bias and the residual in the LayerNorm) against fp64
    LN(x + conv_o(attention) + b_o): the LayerNorm's input carries the attention's error d <= 2e-5 max|pre-LN|, passed on times
    rstd * gamma at most; its own bar is 1e-5 of the output scale."""
    B, T, H, D, ks, Co = 1, 160, 2, 96, 4, 192
    c, wo, bo, res, slabs, ml = _split(B, T, (T,), H, D, ks, 16)
    g = torch.Generator().manual_seed(T + ks)
    gamma, beta = torch.randn(Co, generator=g), torch.randn(Co, generator=g)
    pre = R.ref_conv_o(c["att"], wo, bo, res)
    ref, rstd = R.ref_layer_norm(pre, gamma, beta, with_rstd=True)
    out = F.nanf(B, Co, T)
    t = [x.cuda() for x in (slabs.float(), ml.float(), res, bo, gamma, beta)]
    assert F.layernorm_ex(a=t[0], add=t[2], gamma=t[4], beta=t[5], out=out, B=B, C=Co, T=T, nslab=H * ks, slab_stride=B * Co * T,
                          ml=t[1], ml_H=H, ml_ks=ks, bias=t[3]) == 0
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    bound = 1e-5 * ref.abs().max().item() + 2e-5 * pre.abs().max().item() * rstd.max().item() * gamma.abs().max().item()
    err = (got - ref).abs().max().item()
    print(f"\n[split + LN q16] max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound


# ------------------------------------------------------------------------------------------------------------------
# the launcher's contract and the tile rule

@gpu
def test_tile_contract():
    """16 queries with the fp16 products, or a tile that is neither 0, 16 nor 32: refused, nothing launched."""
    B, T, H, D = 1, 33, 2, 96
    c = F._case(B, T, (33,), H, D, 3.0)
    out = F.nanf(B, H * D, T)
    base = _inputs(c, H, D, T)
    assert attention_q(out=out, B=B, f16=1, qtile=16, **base) == -1
    assert attention_q(out=out, B=B, qtile=8, **base) == -1
    assert attention_q(out=out, B=B, qtile=64, **base) == -1
    assert torch.isnan(out).all()
    assert attention_q(out=out, B=B, f16=1, qtile=32, **base) == 0
    assert torch.isfinite(out).all()


def test_tile_rule():
    """Host only.  16 queries where 32-query tiles leave at least half of the 256 compute units without a workgroup, fp32 only; a
    function of (B, H, T, D, ks) and the dtype — the export takes nothing else."""
    pick = _lib().bv2_test_attention_pick_qtile
    assert pick(1, 2, 384, 96, 4, 0) == 16                 # the flow at batch 1: 96 workgroups of 32 queries
    assert pick(1, 2, 384, 96, 2, 0) == 16
    assert pick(1, 2, 128, 96, 1, 0) == 16                 # the text encoder: 8
    assert pick(32, 2, 384, 96, 1, 0) == 32                # 768
    assert pick(1, 2, 384, 96, 4, 1) == 32                 # fp16: always 32
    assert pick(1, 2, 128, 80, 1, 0) == 32                 # a head dim the kernel has no form for
    for D in (32, 64, 96, 128):
        assert pick(1, 2, 2048, D, 1, 0) == 16             # 2 * 64 = 128 workgroups: exactly half
        assert pick(1, 2, 2049, D, 1, 0) == 32             # 130
        assert pick(1, 2, 1024, D, 2, 0) == 16 and pick(1, 2, 1056, D, 2, 0) == 32
    assert pick(1, 2, 384, 96, 0, 0) == pick(1, 2, 384, 96, 1, 0)   # 0 and 1: no split
