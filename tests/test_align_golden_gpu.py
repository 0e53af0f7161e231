"""GPU: the forward flow and the aligner against the REAL reference (tests/golden/align_*.npz, tools/gen_align_golden.py): the reference's
``flow(z, y_mask, g=g)`` in fp32 and fp64, its ``neg_cent`` (models.py:962-975) and the dynamic programme's path on that matrix.

Error bars.  A device tensor is held to the fixture's fp64 value with at most 4 x the reference's own fp32 error against the same fp64
value, tensor by tensor (the margin the ReferenceEncoder was given for a changed summation order).  The reference's errors here are
small — 2 to 3 ulp of the tensors' largest values for z_p — but the bar still separates: the measured ratios (printed by the tests,
recorded in docs/MEASUREMENTS.md) are 0.55-0.92 for the flow and 1.12-1.17 for the matrix, so no fallback to a relative bar is taken."""
import numpy as np
import pytest
import torch

from bert_vits2_amd import align, models
from oracle import cases
from tests import posterior_oracle as PO
from tests.helpers import cached_state_dict, load_golden

pytestmark = pytest.mark.gpu
CASES = ["narrow_b2_t18", "mix_b2_ragged", "wn_b1_t16"]      # transformer flow with 3 couplings (odd), with 4 (the v2.3 widths), WN flow
_M, _G = {}, {}


def _setup(name):
    if name not in _M:
        hp, seed, batch, nw, nz, kw = cases.build_case(name)
        m = models.from_hparams(hp)
        m.load_state_dict(cached_state_dict(hp, seed), strict=False)
        _M[name] = (m.to("cuda").eval(), hp, batch, nw, kw)
        _G[name] = load_golden("align_" + name)
    return _M[name] + _G[name]


def _ulp(v):
    return float(np.spacing(np.float32(v)))


def _held(name, what, dev, ref64, ref_err):
    """The bar of the module docstring; the figures are printed before the assertion."""
    err = float((dev.double().cpu() - ref64).abs().max())
    top = float(ref64.abs().max())
    print(f"{name} {what}: device max err {err:.3e}, reference fp32 err {ref_err:.3e} (ratio {err / max(ref_err, 1e-30):.2f}), "
          f"|ref| max {top:.3f} (ulp {_ulp(top):.2e}), maxrel {err / top:.2e}")
    assert err <= 4 * ref_err
    return err


@pytest.mark.parametrize("name", CASES)
def test_flow_forward_against_the_reference_and_round_trip(name):
    m, hp, batch, nw, kw, meta, G = _setup(name)
    g = m.stage_emb_g(batch["sid"])
    z, yl = G["z"], G["y_lengths"]
    z_p = m.stage_flow_forward(z, yl, g)
    assert z_p.shape == z.shape and z_p.dtype == torch.float32
    for b in range(z.shape[0]):
        assert not z_p[b, :, int(yl[b]):].any()                               # masked frames stay zero
    _held(name, "z_p", z_p, G["z_p64"], meta["ref_err_z_p"])
    # the frame mask as a tensor is the same call
    ym = (torch.arange(z.shape[2])[None, :] < yl[:, None]).float()[:, None, :]
    assert torch.equal(m.stage_flow_forward(z, None, g, y_mask=ym), z_p)
    # the flow's fp16 switch does not reach this direction
    m.set_flow_dtype(torch.float16)
    try:
        assert torch.equal(m.stage_flow_forward(z, yl, g), z_p)
    finally:
        m.set_flow_dtype(torch.float32)
    # round trip: the reverse flow undoes it, within the same bar
    back = m.stage_flow(z_p, yl, g)
    _held(name, "stage_flow(stage_flow_forward(z))", back, z.double(), meta["ref_err_z_p"])
    with pytest.raises(ValueError):
        m.stage_flow_forward(z, yl, g, y_mask=ym)


@pytest.mark.parametrize("name", CASES)
def test_neg_cent_and_path_on_the_reference_tensors(name):
    m, hp, batch, nw, kw, meta, G = _setup(name)
    xl, yl = G["x_lengths"], G["y_lengths"]
    nc = align.neg_cent(G["z_p"].cuda(), G["m_p"].cuda(), G["logs_p"].cuda(), xl.cuda(), yl.cuda())
    nc64 = torch.from_numpy(PO.neg_cent_f64(G["z_p"].numpy(), G["m_p"].numpy(), G["logs_p"].numpy(), xl.tolist(), yl.tolist()))
    err = float((nc.double().cpu() - nc64).abs().max())
    print(f"{name} neg_cent: device max err {err:.3e}, reference fp32 err {meta['ref_err_neg_cent']:.3e} "
          f"(ratio {err / meta['ref_err_neg_cent']:.2f}), |neg_cent| max {meta['neg_cent_absmax']:.1f}")
    assert err <= 4 * meta["ref_err_neg_cent"]
    # the dynamic programme on the reference's own matrix: bit for bit the fixture's path and score
    out = align.maximum_path(G["neg_cent"].cuda(), xl.tolist(), yl.tolist(), want_attn=True)
    assert torch.equal(out["durations"].cpu(), G["durations"])
    assert np.array_equal(out["score"].cpu().numpy().view(np.uint32), G["score"].numpy().view(np.uint32))
    for b in range(len(xl)):
        assert np.array_equal(out["attn"][b, 0, :int(yl[b]), :int(xl[b])].cpu().numpy(),
                              PO.path_from_durations(G["durations"][b, :int(xl[b])].numpy(), int(yl[b]), int(xl[b])))


@pytest.mark.parametrize("name", CASES)
def test_text_and_latent_to_durations_end_to_end(name):
    """Phase A, the forward flow, neg_cent and the path, all on the device, from the fixture's inputs.  Round-off in neg_cent may move
    the path at a near tie, so the condition is optimality: the device path, scored in fp64 on the FIXTURE's matrix, is within
    2 Ty eps of the fixture's optimum (eps = max |neg_cent_device - neg_cent_fixture|; both paths sum Ty cells); where eps = 0 the
    durations are the fixture's."""
    m, hp, batch, nw, kw, meta, G = _setup(name)
    dev = lambda k: batch[k].cuda()
    enc = m.encode_durations(dev("x"), dev("x_lengths"), dev("sid"), dev("tone"), dev("language"), dev("bert"), dev("ja_bert"),
                             dev("en_bert"), nw, sdp_ratio=0.0, lean=True)
    xl, yl = G["x_lengths"].tolist(), G["y_lengths"].tolist()
    z_p = m.stage_flow_forward(G["z"], G["y_lengths"], enc["g"])
    out = m.align_latent(enc, z_p, yl, want_attn=True, x_lengths=xl)
    d = out["durations"].cpu().numpy()
    gold = G["neg_cent"].double().numpy()
    eps = float(np.abs(out["neg_cent"].cpu().double().numpy() - gold).max())
    print(f"{name} end to end: eps {eps:.3e}, durations equal: {np.array_equal(d, G['durations'].numpy())}")
    for b in range(len(xl)):
        assert d[b, :xl[b]].min() >= 1 and d[b].sum() == yl[b] and not d[b, xl[b]:].any()
        got, best = PO.path_score(gold[b], d[b]), PO.path_score(gold[b], G["durations"][b].numpy())
        assert got >= best - 2 * yl[b] * eps
    if eps == 0:
        assert np.array_equal(d, G["durations"].numpy())
    # timing transfer on the reference's path: decode walks it
    enc2 = models.with_durations(enc, G["durations"])
    Ty = max(yl)
    nz = torch.zeros(len(xl), hp.inter_channels, Ty, device="cuda")
    dec = m.decode(enc2, nz, Ty)
    assert dec["y_mask"].sum([1, 2]).long().tolist() == yl
    for b in range(len(xl)):
        assert np.array_equal(dec["attn"][b, 0, :yl[b], :xl[b]].cpu().numpy(),
                              PO.path_from_durations(G["durations"][b, :xl[b]].numpy(), yl[b], xl[b]))
