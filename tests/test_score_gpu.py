"""GPU: scoring a take against its text — the forward spline alone, ``duration_nll`` against the REAL reference's
``net.sdp(x, x_mask, w, g=g)`` (tests/golden/score_*.npz, tools/gen_score_golden.py), ``kl_path`` against its ``kl_loss`` on the
``posterior_*`` fixtures, and ``score`` / ``serving.score`` end to end.

Error bars.  Every device number is held to the fixture's fp64 value with at most 4 x the fp32 error of the reference itself (``ref_err_*``
in the fixtures: max |fp32 - fp64| of the reference's own run; for the per-symbol decomposition and the spline, of the restatement
tests/score_oracle.py run in fp32) — the margin tests/test_posterior_gpu.py gives a different but equally valid fp32 order of operations.
The figures are printed before each assertion and recorded in docs/MEASUREMENTS.md."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from bert_vits2_amd import align, hparams as H, lib as L, models, serving, synth
from oracle import cases
from tests import score_oracle as SO
from tests.helpers import cached_state_dict, load_golden

pytestmark = pytest.mark.gpu
NLL_CASES = ["t1", "t3", "t17", "t18", "b2_ragged", "zero_dur", "narrow_b2_t18"]
KL_CASES = ["narrow_b2_t18", "mix_b2_ragged", "wn_b1_t16"]
_M = {}


def _model(hp_over, seed=0, spec=None):
    """One model per width, with the forward duration predictor loaded (and refused before it is)."""
    tup = lambda v: tuple(tup(i) for i in v) if isinstance(v, (list, tuple)) else v       # a fixture's JSON turned the tuples into lists
    hp_over = {k: tup(v) for k, v in hp_over.items()}
    key = (repr(sorted(hp_over.items())), spec)
    if key not in _M:
        hp = H.default_v23(**dict(hp_over, **({} if spec is None else dict(spec_channels=spec))))
        m = models.from_hparams(hp)
        m.load_state_dict(cached_state_dict(hp, seed), strict=False)
        m = m.to("cuda").eval()
        assert not m.has_sdp_forward
        enc = dict(x=torch.zeros(1, hp.hidden_channels, 4), x_mask=torch.ones(1, 4), g=torch.zeros(1, hp.gin_channels))
        with pytest.raises(RuntimeError, match=r"load_sdp_forward\(checkpoint\).*compress_model.py"):
            m.duration_nll(enc, torch.ones(1, 4))
        m.load_sdp_forward(synth.synthetic_sdp_forward_state_dict(hp, seed))
        assert m.has_sdp_forward
        _M[key] = (m, hp)
    return _M[key]


def fixed_order_sum(row):
    """The library's row sum: lane l adds positions l, l + 64, ... in sequence, a butterfly over xor 32 .. 1, fp64, rounded once."""
    lanes = np.zeros(64, dtype=np.float64)
    for t, v in enumerate(np.asarray(row, dtype=np.float32)):
        lanes[t % 64] += np.float64(v)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[np.arange(64) ^ off]
    return np.float32(lanes[0])


# ---------------------------------------------------------------------------------------------------------------- the forward spline
def _spline_inputs():
    """Parameter sets x probe points: both tails and exactly +-tail, every bin's middle, each interior knot -+ 1e-6; the last sets carry
    large positive and negative derivative parameters (slopes up to e^8 and down to the 1e-3 floor)."""
    g = torch.Generator().manual_seed(97)
    S = 48
    uw, uh, ud = torch.randn(S, 10, generator=g), torch.randn(S, 10, generator=g), torch.randn(S, 9, generator=g) * 2
    ud[-8:-4] = 8.0 + torch.rand(4, 9, generator=g)
    ud[-4:] = -8.0 - torch.rand(4, 9, generator=g)
    ud[-10:-8, ::2], ud[-10:-8, 1::2] = 7.0, -7.0
    w = 1e-3 + (1 - 1e-2) * torch.softmax(uw.double(), -1)
    kn = torch.cumsum(w, -1) * 10 - 5                                                   # knots 1 .. 10 (the last is +tail)
    lo = torch.cat([torch.full((S, 1), -5.0, dtype=torch.float64), kn[:, :-1]], 1)
    mids = (lo + kn) / 2
    inner = kn[:, :-1]
    fixed = torch.tensor([-7.0, -5.001, -5.0, 5.0, 5.001, 7.0], dtype=torch.float64).expand(S, 6)
    x = torch.cat([fixed, mids, inner - 1e-6, inner + 1e-6, inner], 1).float()          # [S, 6 + 10 + 27]
    P = x.shape[1]
    rep = lambda t: t[:, None, :].expand(S, P, t.shape[1]).reshape(S * P, -1).contiguous()
    return x.reshape(-1).contiguous(), rep(uw), rep(uh), rep(ud)


def test_forward_spline_against_the_restatement_and_the_inverse():
    lib = L.load()
    lib.bv2_test_spline_forward.restype = C.c_int
    lib.bv2_test_spline_forward.argtypes = [C.c_void_p] * 5 + [C.c_float, C.c_longlong, C.c_void_p, C.c_void_p]
    lib.bv2_test_spline.restype = C.c_int
    lib.bv2_test_spline.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_int]
    x, uw, uh, ud = _spline_inputs()
    N = x.numel()
    d = lambda t: t.double()
    y64, l64 = SO.rq_spline_forward(d(x), d(uw), d(uh), d(ud))
    y32, l32 = SO.rq_spline_forward(x, uw, uh, ud)
    bins = ((d(x)[:, None] >= (torch.cumsum(1e-3 + 0.99 * torch.softmax(d(uw), -1), -1) * 10 - 5)).sum(-1)).clamp(0, 9)
    assert set(bins[(x.abs() <= 5)].tolist()) == set(range(10))                          # every bin is probed
    assert float(l64.max()) > 3 and float(l64.min()) < -5                                # slopes far from 1 on both sides (> 20, < 1 / 150)
    P = lambda t: C.c_void_p(t.data_ptr())
    xd, wd, hd, dd = x.cuda(), uw.cuda(), uh.cuda(), ud.cuda()
    y, lad = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    assert lib.bv2_test_spline_forward(None, P(xd), P(wd), P(hd), P(dd), 5.0, N, P(y), P(lad)) == 0
    torch.cuda.synchronize()
    out = x.abs() > 5
    assert torch.equal(y.cpu()[out], x[out]) and not lad.cpu()[out].any()                # the identity, log-determinant 0
    for what, dev, r32, r64 in (("y", y, y32, y64), ("logabsdet", lad, l32, l64)):
        ref_err = float((d(r32) - r64).abs().max())
        err = float((d(dev.cpu()) - r64).abs().max())
        print(f"forward spline {what}: device max err {err:.3e}, restatement fp32 err {ref_err:.3e} (ratio {err / ref_err:.2f}), N = {N}")
        assert err <= 4 * ref_err
    # inverse(forward(x)) with the existing inverse kernel: z [1][2][N], the 29 parameter rows as [1][32][N] (sqrt_fc 1: already divided)
    z = torch.zeros(1, 2, N, device="cuda")
    z[0, 1] = y
    prm = torch.zeros(1, 32, N, device="cuda")
    prm[0, :10], prm[0, 10:20], prm[0, 20:29] = wd.t(), hd.t(), dd.t()
    mask = torch.ones(1, N, device="cuda")
    assert lib.bv2_test_spline(None, P(z), 0, 1, P(prm.contiguous()), 32, P(mask), 1.0, 5.0, 1, N) == 0
    torch.cuda.synchronize()
    back32 = SO.rq_spline_inverse(y32, uw, uh, ud)
    ref_err = float((d(back32) - d(x)).abs().max())
    err = float((d(z[0, 1].cpu()) - d(x)).abs().max())
    print(f"inverse(forward(x)) - x: device max {err:.3e}, restatement fp32 {ref_err:.3e} (ratio {err / ref_err:.2f})")
    assert err <= 4 * ref_err


# ---------------------------------------------------------------------------------------------------------------- duration_nll
def _nll(m, G, rows=None, T=None):
    s = slice(None) if rows is None else rows
    t = slice(None) if T is None else slice(0, T)
    enc = dict(x=G["x"][s, :, t], x_mask=G["x_mask"][s, 0, t], g=G["g"][s, :, 0])
    return m.duration_nll(enc, G["w"][s, 0, t], noise_e=G["noise_e"][s, :, t])


@pytest.mark.parametrize("name", NLL_CASES)
def test_duration_nll_against_the_reference(name):
    meta, G = load_golden("score_" + name)
    m, hp = _model(meta["hp"], meta["seed"])
    out = _nll(m, G)
    torch.cuda.synchronize()
    nll, sym = out["nll"].cpu(), out["nll_sym"].cpu()
    B, T = sym.shape
    assert nll.shape == (B,) and (B, T) == tuple(G["w"][:, 0].shape)
    err = float((nll.double() - G["nll64"]).abs().max())
    print(f"{name} nll: device max err {err:.3e}, reference fp32 err {meta['ref_err_nll']:.3e} (ratio {err / meta['ref_err_nll']:.2f}), "
          f"|nll| max {float(G['nll64'].abs().max()):.2f}")
    assert err <= 4 * meta["ref_err_nll"]
    err = float((sym.double() - G["nll_sym64"]).abs().max())
    print(f"{name} nll_sym: device max err {err:.3e}, restatement fp32 err {meta['ref_err_nll_sym']:.3e} "
          f"(ratio {err / meta['ref_err_nll_sym']:.2f})")
    assert err <= 4 * meta["ref_err_nll_sym"]
    for b in range(B):
        assert nll[b].numpy() == fixed_order_sum(sym[b].numpy())                         # bit for bit
    masked = G["x_mask"][:, 0] == 0
    assert torch.equal(sym[masked], torch.zeros(int(masked.sum()))) and sym[~masked].abs().min() > 0


def test_a_ragged_batch_gives_each_item_what_it_gets_alone_bit_for_bit():
    for name in ("b2_ragged", "narrow_b2_t18"):
        meta, G = load_golden("score_" + name)
        m, hp = _model(meta["hp"], meta["seed"])
        both = _nll(m, G)
        for b, n in enumerate(meta["lengths"]):
            alone = _nll(m, G, rows=slice(b, b + 1), T=n)
            assert torch.equal(alone["nll"][0], both["nll"][b]), (name, b)
            assert torch.equal(alone["nll_sym"][0], both["nll_sym"][b, :n]), (name, b)


def test_duration_nll_seeded_draw_and_argument_rules():
    meta, G = load_golden("score_b2_ragged")
    m, hp = _model(meta["hp"], meta["seed"])
    enc = dict(x=G["x"], x_mask=G["x_mask"][:, 0], g=G["g"][:, :, 0])
    w = G["w"][:, 0]
    a = m.duration_nll(enc, w, seeds=[5, 6])
    assert torch.equal(a["nll"], m.duration_nll(enc, w, seeds=[5, 6])["nll"])
    swap = dict(x=G["x"].flip(0), x_mask=G["x_mask"][:, 0].flip(0), g=G["g"][:, :, 0].flip(0))
    b = m.duration_nll(swap, w.flip(0), seeds=[6, 5])
    assert torch.equal(b["nll"].flip(0), a["nll"]) and torch.equal(b["nll_sym"].flip(0), a["nll_sym"])   # another batch position
    assert not torch.equal(a["nll"], m.duration_nll(enc, w, seeds=[5, 7])["nll"])
    assert torch.isfinite(m.duration_nll(enc, w)["nll"]).all()                           # neither: drawn like draw_noise_w
    with pytest.raises(ValueError, match="exclude"):
        m.duration_nll(enc, w, noise_e=G["noise_e"], seeds=[1, 2])
    with pytest.raises(ValueError, match="noise_e must be"):
        m.duration_nll(enc, w, noise_e=G["noise_e"][:, :1])
    with pytest.raises(ValueError, match="durations must be"):
        m.duration_nll(enc, w[:, :-1])


# ---------------------------------------------------------------------------------------------------------------- kl_path
def _kl_inputs(name):
    _pm, P = load_golden("posterior_" + name)
    return P["z_p"], P["logs_q64"].float(), P["m_p"], P["logs_p"], P["durations"], P["x_lengths"], P["y_lengths"]


@pytest.mark.parametrize("name", KL_CASES)
def test_kl_path_against_the_reference(name):
    meta, G = load_golden("score_kl_" + name)
    z_p, logs_q, m_p, logs_p, dur, xl, yl = _kl_inputs(name)
    dev = lambda t: t.cuda()
    out = align.kl_path(dev(z_p), dev(logs_q), dev(m_p), dev(logs_p), dev(dur), xl, yl)
    kl, frame = out["kl"].cpu(), out["kl_frame"].cpu()
    err = float((kl.double() - G["kl64"]).abs().max())
    print(f"{name} kl: device max err {err:.3e}, reference fp32 err {meta['ref_err_kl']:.3e} (ratio {err / meta['ref_err_kl']:.2f}), "
          f"|kl| max {float(G['kl64'].abs().max()):.1f}")
    assert err <= 4 * meta["ref_err_kl"]
    # per frame: fp32 terms (a handful of roundings each) summed in fp64 — 1e-5 of the largest frame is twenty times that, and far
    # below what a frame read from the wrong symbol differs by
    assert float((frame.double() - G["kl_frame64"]).abs().max()) <= 1e-5 * float(G["kl_frame64"].abs().max())
    for b, n in enumerate(yl.tolist()):
        assert torch.equal(frame[b, n:], torch.zeros(frame.shape[1] - n))
        assert kl[b].numpy() == fixed_order_sum(frame[b].numpy())


def test_kl_path_ragged_equals_alone_bit_for_bit():
    z_p, logs_q, m_p, logs_p, dur, xl, yl = _kl_inputs("narrow_b2_t18")
    dev = lambda t: t.cuda().contiguous()
    both = align.kl_path(dev(z_p), dev(logs_q), dev(m_p), dev(logs_p), dev(dur), xl, yl)
    for b in range(2):
        n, tx = int(yl[b]), int(xl[b])
        alone = align.kl_path(dev(z_p[b:b + 1, :, :n]), dev(logs_q[b:b + 1, :, :n]), dev(m_p[b:b + 1, :, :tx]), dev(logs_p[b:b + 1, :, :tx]),
                              dev(dur[b:b + 1, :tx]))
        assert torch.equal(alone["kl_frame"][0], both["kl_frame"][b, :n]) and torch.equal(alone["kl"][0], both["kl"][b])


# ---------------------------------------------------------------------------------------------------------------- score, end to end
def _score_setup():
    name = "narrow_b2_t18"
    meta, G = load_golden("posterior_" + name)
    base = cases.CASES[name]
    m, hp = _model(base["hp"], base["seed"], spec=meta["spec_channels"])
    if not m.has_posterior:
        m.load_posterior(synth.synthetic_posterior_state_dict(hp, base["seed"]))
    batch = synth.synthetic_batch(base["lengths"], base["languages"], base["sids"])
    frames = meta["frames"]
    y = torch.zeros(len(frames), hp.spec_channels, max(frames))
    for b, n in enumerate(frames):
        y[b, :, :n] = synth.synthetic_reference_spec(hp.spec_channels, n, b)
    return m, hp, batch, y, G


def _args(batch, rows=None):
    s = slice(None) if rows is None else rows
    return tuple(batch[k][s].cuda() for k in ("x", "x_lengths", "sid", "tone", "language", "bert", "ja_bert", "en_bert"))


def test_score_end_to_end_equals_its_stages():
    m, hp, batch, y, G = _score_setup()
    xl, yl = G["x_lengths"].tolist(), G["y_lengths"].tolist()
    a = list(_args(batch))
    a[1] = xl
    ne = torch.randn(2, 2, batch["x"].shape[1], generator=torch.Generator().manual_seed(3))
    out = m.score(*a, y, yl, noise_q=G["noise_q"], noise_e=ne)
    al = m.align(*a, y, yl, noise_q=G["noise_q"])
    assert torch.equal(out["durations"], al["durations"]) and torch.equal(out["score"], al["score"])
    assert out["y_lengths"].tolist() == yl and out["durations"].sum(1).tolist() == yl
    nll = m.duration_nll(out["enc"], out["durations"], noise_e=ne)
    kl = align.kl_path(out["z_p"], out["posterior"]["logs_q"], out["enc"]["m_p"], out["enc"]["logs_p"], out["durations"], xl, yl)
    assert torch.equal(nll["nll"], out["nll"]) and torch.equal(nll["nll_sym"], out["nll_sym"])
    assert torch.equal(kl["kl"], out["kl"]) and torch.equal(kl["kl_frame"], out["kl_frame"])
    assert out["nll_sym"].shape == (2, 18) and out["kl_frame"].shape == (2, max(yl))
    for k in ("l_length_dp", "l_length_sdp_mse"):
        assert out[k].shape == (2,) and torch.isfinite(out[k]).all() and (out[k] >= 0).all()
    mask = out["enc"]["x_mask"].reshape(2, -1)
    logw_ = torch.log(out["durations"].float() + 1e-6) * mask
    want = ((out["enc"]["logw_dp"].reshape(2, -1) - logw_) ** 2).sum(1) / mask.sum(1)
    assert torch.allclose(out["l_length_dp"], want)
    # given durations are scored as they are: no aligner, the same numbers
    given = m.score(*a, y, yl, noise_q=G["noise_q"], noise_e=ne, durations=out["durations"])
    assert given["score"] is None and torch.equal(given["nll"], out["nll"]) and torch.equal(given["kl"], out["kl"])


def test_seeded_score_does_not_depend_on_the_batch_position_and_serving_score_equals_it():
    m, hp, batch, y, G = _score_setup()
    xl, yl = G["x_lengths"].tolist(), G["y_lengths"].tolist()
    a = list(_args(batch))
    a[1] = xl
    out = m.score(*a, y, yl, seeds=[41, 42])
    flip = lambda t: t.flip(0)
    f = [flip(v) if isinstance(v, torch.Tensor) else v[::-1] for v in a]
    swapped = m.score(*f, flip(y), yl[::-1], seeds=[42, 41])
    for k in ("nll", "nll_sym", "kl", "kl_frame", "durations"):
        assert torch.equal(flip(swapped[k]), out[k]), k
    utts, specs = [], []
    for b, n in enumerate(xl):
        utts.append(serving.Utterance(batch["x"][b, :n], batch["tone"][b, :n], batch["language"][b, :n], batch["bert"][b, :, :n],
                                      batch["ja_bert"][b, :, :n], batch["en_bert"][b, :, :n], int(batch["sid"][b]), seed=41 + b))
        specs.append(y[b, :, :yl[b]])
    res = serving.score(m, utts, specs, max_batch=4, max_pad_ratio=2.0)
    for b, r in enumerate(res):
        n, ny = xl[b], yl[b]
        assert r["nll_sym"].shape == (n,) and r["kl_frame"].shape == (ny,) and r["durations"].dtype == np.int64
        assert r["nll"] == out["nll"][b].item() and r["kl"] == out["kl"][b].item()
        assert np.array_equal(r["nll_sym"], out["nll_sym"][b, :n].cpu().numpy())
        assert np.array_equal(r["kl_frame"], out["kl_frame"][b, :ny].cpu().numpy())
        assert np.array_equal(r["durations"], out["durations"][b, :n].cpu().numpy()) and r["score"] == out["score"][b].item()
    # a timing transfer judged before it is spoken: the same durations, given, score the same; the aligner does not run
    timed = [serving.Utterance(u.phones, u.tones, u.lang_ids, u.bert, u.ja_bert, u.en_bert, u.sid, durations=r["durations"], seed=u.seed)
             for u, r in zip(utts, res)]
    for r, g in zip(res, serving.score(m, timed, specs, use_durations=True, max_batch=4, max_pad_ratio=2.0)):
        assert "score" not in g and g["nll"] == r["nll"] and g["kl"] == r["kl"] and np.array_equal(g["durations"], r["durations"])
    with pytest.raises(ValueError, match="use_durations needs"):
        serving.score(m, utts, specs, use_durations=True)
    with pytest.raises(ValueError, match="one recording per utterance"):
        serving.score(m, utts, specs[:1])
