"""CPU: the fp64 references of tests/encoder_refs.py proved against the oracle (oracle/bv2_oracle.py, itself verified against the
reference project) and against each other.  This proves the references that tests/test_encoder_forms_gpu.py holds the kernels to,
not the kernels."""
import math

import pytest
import torch

from oracle import bv2_oracle as O
from tests import encoder_refs as R


def _tiny_sd(C, H, g):
    d = C // H
    sd = {}
    for n in "qkvo":
        sd[f"a.conv_{n}.weight"] = torch.randn(C, C, 1, generator=g, dtype=torch.float64) / math.sqrt(C)
        sd[f"a.conv_{n}.bias"] = torch.randn(C, generator=g, dtype=torch.float64)
    sd["a.emb_rel_k"] = torch.randn(1, 2 * O.WINDOW + 1, d, generator=g, dtype=torch.float64) * d ** -0.5
    sd["a.emb_rel_v"] = torch.randn(1, 2 * O.WINDOW + 1, d, generator=g, dtype=torch.float64) * d ** -0.5
    return sd


@pytest.mark.parametrize("B,T,lens,C,H", [(2, 37, [37, 9], 24, 2), (1, 70, [70], 32, 4), (3, 5, [5, 1, 3], 16, 1)])
def test_references_equal_the_oracle(B, T, lens, C, H):
    """ref_attention -> ref_conv_o -> ref_layer_norm is the oracle's rel_attention + channel_layer_norm, to 1e-12 in fp64."""
    assert R.WINDOW == O.WINDOW
    g = torch.Generator().manual_seed(C + T)
    sd = _tiny_sd(C, H, g)
    x = torch.randn(B, C, T, generator=g, dtype=torch.float64)
    gamma, beta = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).double()
    want = O.channel_layer_norm(x + O.rel_attention(sd, "a", x, mask, H), gamma, beta)
    qkv = torch.cat([torch.einsum("oc,bct->bot", sd[f"a.conv_{n}.weight"][:, :, 0], x) + sd[f"a.conv_{n}.bias"][None, :, None]
                     for n in "qkv"], 1)
    att = R.ref_attention(qkv, mask, sd["a.emb_rel_k"][0], sd["a.emb_rel_v"][0], H, O.WINDOW)
    got = R.ref_layer_norm(R.ref_conv_o(att, sd["a.conv_o.weight"][:, :, 0], sd["a.conv_o.bias"], x), gamma, beta)
    err = (got - want).abs().max().item()
    assert err <= 1e-12 * max(1.0, want.abs().max().item()), err
    # (LN + vec) * mask
    vec = torch.randn(B, C, generator=g, dtype=torch.float64)
    want2 = (want + vec[:, :, None]) * mask[:, None, :]
    got2 = R.ref_ln_vec_mask(R.ref_conv_o(att, sd["a.conv_o.weight"][:, :, 0], sd["a.conv_o.bias"], x), gamma, beta, vec, mask)
    assert (got2 - want2).abs().max().item() <= 1e-12 * max(1.0, want2.abs().max().item())


def test_key_ranges_rule():
    assert R.key_ranges(65, 2) == [(0, 32), (32, 65)]
    assert R.key_ranges(160, 4) == [(0, 32), (32, 64), (64, 96), (96, 160)]
    assert R.key_ranges(600, 2) == [(0, 288), (288, 600)]
    assert R.key_ranges(256, 4) == [(0, 64), (64, 128), (128, 192), (192, 256)]


@pytest.mark.parametrize("B,T,lens,H,D,ks,qmul", R.SPLIT_CASES)
def test_split_ranges_merge_to_the_unsplit_result(B, T, lens, H, D, ks, qmul):
    """Per-range softmax (tiles [n r / ks, n (r + 1) / ks) of 32 keys) pushed through conv_o and merged by ref_split_merge is the
    unsplit attention + conv_o, to 1e-12: for every (T, lens, ks) the GPU tests use (and for ks = 2 and 4 at each of them)."""
    qkv, erk, erv, mask = R.attention_inputs(B, T, lens, H, D, qmul)
    Co = 48                                        # the merge is per column and head: the width of conv_o plays no part
    wo, bo, res = R.conv_o_weights(H, D, Co, B, T)
    want = R.ref_conv_o(R.ref_attention(qkv, mask, erk, erv, H, R.WINDOW), wo, bo, res)
    valid = mask[:, None, :].bool().expand_as(want)
    logits = R.ref_logits(qkv, mask, erk, H, R.WINDOW)
    for k in sorted({ks, 2, 4}):
        if k > (T + 31) // 32:                     # more ranges than key tiles: the launcher refuses it
            continue
        slabs = torch.zeros(H, k, B, Co, T, dtype=torch.float64)
        m, l = torch.zeros(B, H, k, T, dtype=torch.float64), torch.zeros(B, H, k, T, dtype=torch.float64)
        for r, (k0, k1) in enumerate(R.key_ranges(T, k)):
            o, m[:, :, r], l[:, :, r] = R.ref_attention_range(qkv, erv, H, R.WINDOW, k0, k1, logits)
            for h in range(H):
                slabs[h, r] = R.ref_conv_o(o[:, h * D:(h + 1) * D], wo[:, h * D:(h + 1) * D])
        got = R.ref_split_merge(slabs, m, l) + bo.double()[None, :, None] + res.double()
        err = (got - want).abs()[valid].max().item()
        assert err <= 1e-12 * want.abs().max().item(), (k, err)
        spread = (m.max(2).values - m.min(2).values)[mask[:, None, :].bool().expand(B, H, T)].max().item()
        print(f"\n[T={T} lens={lens} H={H} D={D} ks={k} q x{qmul}] merge error {err:.2e}, largest spread of the range maxima {spread:.1f}")


def test_split_merge_weights():
    """ref_split_merge on hand-made numbers: equal (m, l) average the slabs; a range 800 below the maximum weighs exactly 0 even in
    fp64; l scales the weight linearly."""
    slabs = torch.tensor([1.0, 3.0], dtype=torch.float64).view(1, 2, 1, 1, 1)
    mk = lambda a, b: torch.tensor([a, b], dtype=torch.float64).view(1, 1, 2, 1)
    assert R.ref_split_merge(slabs, mk(-1e4, -1e4), mk(32, 32)).item() == 2.0
    assert R.ref_split_merge(slabs, mk(0.0, -800.0), mk(1, 64)).item() == 1.0
    assert abs(R.ref_split_merge(slabs, mk(2.0, 2.0), mk(1, 3)).item() - 2.5) < 1e-15
    assert abs(R.ref_split_merge(slabs, mk(0.0, math.log(3.0)), mk(1, 1)).item() - 2.5) < 1e-15
