"""GPU: forced alignment (kernels/align.hip).  ``bv2_neg_cent`` against its fp64 definition at the shapes where the tiling can go wrong,
``bv2_maximum_path`` bit for bit against the numpy restatement of the dynamic programme (tests/posterior_oracle.py), and the paths
from there into synthesis: ``decode(with_durations(enc, d))``, ``serving.Utterance(durations=d)`` and ``serving.align``."""
import numpy as np
import pytest
import torch

from bert_vits2_amd import align, models, serving, synth
from oracle import cases
from tests import posterior_oracle as PO
from tests.helpers import cached_state_dict

pytestmark = pytest.mark.gpu
_M = {}


def _model(name="narrow_b2_t18"):
    if name not in _M:
        hp, seed, batch, nw, nz, kw = cases.build_case(name)
        m = models.from_hparams(hp)
        m.load_state_dict(cached_state_dict(hp, seed), strict=False)
        _M[name] = (m.to("cuda").eval(), hp, batch, nw, nz, kw)
    return _M[name]


def _latents(B, D, T, Ty, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, D, Ty, generator=g)
    m = torch.randn(B, D, T, generator=g)
    ls = torch.randn(B, D, T, generator=g) * 0.4 - 0.3                       # exp(-2 logs) between about 0.3 and 8: the prior's usual range
    return z, m, ls


def _neg_cent_bound(z, m, ls):
    """A-priori fp32 bound per cell: the device sums 2 D products and 2 D constants in fp32, in some order.  With S the sum of the
    ABSOLUTE values of all terms of a cell, any order of n additions errs by at most (n - 1) u S (u = 2^-24), every product and its
    operands (z^2, m r, -1/2 ., expf to 2 ulp) add a few u of their own term: (4 D + 12) u S covers it with room."""
    z, m, ls = z.double().numpy(), m.double().numpy(), ls.double().numpy()
    r = np.exp(-2 * ls)
    D = z.shape[1]
    S = (np.abs(-0.5 * np.log(2 * np.pi) - ls).sum(1)[:, None, :] + (0.5 * m * m * r).sum(1)[:, None, :]
         + np.einsum("bdy,bdx->byx", 0.5 * z * z, r) + np.einsum("bdy,bdx->byx", np.abs(z), np.abs(m) * r))
    return (4 * D + 12) * 2.0 ** -24 * S


def _neg_cent_torch_f32(z, m, ls):
    """The four-term fp32 form a PyTorch user would write from the definition (CPU): its error is printed beside the device's."""
    r = torch.exp(-2 * ls)
    c1 = torch.sum(-0.5 * np.log(2 * np.pi) - ls, [1], keepdim=True)
    c4 = torch.sum(-0.5 * (m ** 2) * r, [1], keepdim=True)
    return c1 + torch.matmul(-0.5 * (z ** 2).transpose(1, 2), r) + torch.matmul(z.transpose(1, 2), m * r) + c4


@pytest.mark.parametrize("B,D,T,Ty,xl,yl", [
    (1, 192, 17, 33, None, None),            # neither a multiple of 16; a second frame tile is absent, a partial symbol tile present
    (1, 192, 1, 9, None, None),              # one symbol
    (2, 64, 40, 70, None, None),             # inter 64, two frame tiles
    (1, 256, 18, 65, None, None),            # inter 256 (the LDS limit), one frame into the second tile
    (3, 128, 37, 131, [37, 5, 16], [131, 64, 17]),   # ragged: padded cells are zeros, and the padding is never read
])
def test_neg_cent_against_fp64(B, D, T, Ty, xl, yl):
    z, m, ls = _latents(B, D, T, Ty, seed=B * 1000 + D + T)
    ref = PO.neg_cent_f64(z, m, ls, xl, yl)
    bound = _neg_cent_bound(z, m, ls)
    zd, md, lsd = z.cuda(), m.cuda(), ls.cuda()
    if xl is not None:                       # poison what lies outside the lengths: it must not reach a valid cell (selected, never multiplied in)
        for b in range(B):
            zd[b, :, yl[b]:] = float("nan")
            md[b, :, xl[b]:] = float("nan")
            lsd[b, :, xl[b]:] = float("inf")
    lens = (None, None) if xl is None else (torch.tensor(xl).cuda(), torch.tensor(yl).cuda())
    out = align.neg_cent(zd, md, lsd, *lens)
    assert out.shape == (B, Ty, T) and out.dtype == torch.float32
    out = out.cpu().double().numpy()
    assert np.isfinite(out).all()
    err = np.abs(out - ref)
    err32 = np.abs(_neg_cent_torch_f32(z, m, ls).double().numpy() - PO.neg_cent_f64(z, m, ls))
    print(f"neg_cent B{B} D{D} T{T} Ty{Ty}: device max err {err.max():.3e} (bound/err min {np.min(bound / np.maximum(err, 1e-30)):.1f}), "
          f"torch fp32 max err {err32.max():.3e}, |ref| max {np.abs(ref).max():.1f}")
    assert (err <= bound).all()
    if xl is not None:
        for b in range(B):
            assert not out[b, yl[b]:, :].any() and not out[b, :, xl[b]:].any()
            assert out[b, :yl[b], :xl[b]].all()


def _check_path(val, xl, yl):
    """Device result bit for bit against the restatement; invariants of a monotone alignment."""
    B, Ty, T = val.shape
    d_ref, a_ref, s_ref = PO.maximum_path(val.numpy(), xl, yl)
    dev = val.cuda()
    keep = dev.clone()
    out = align.maximum_path(dev, xl, yl, want_attn=True)
    assert torch.equal(dev, keep), "neg_cent is a const input"
    d, a, s = out["durations"].cpu().numpy(), out["attn"].cpu().numpy(), out["score"].cpu().numpy()
    assert d.dtype == np.int64 and d.shape == (B, T) and a.shape == (B, 1, Ty, T) and s.dtype == np.float32
    assert np.array_equal(d, d_ref)
    assert np.array_equal(a[:, 0], a_ref)
    assert np.array_equal(s.view(np.uint32), s_ref.view(np.uint32))
    for b in range(B):
        assert d[b, :xl[b]].min() >= 1 and d[b, :xl[b]].sum() == yl[b] and not d[b, xl[b]:].any()
    lean = align.maximum_path(dev, xl, yl)
    assert lean["attn"] is None and torch.equal(lean["durations"], out["durations"])
    return d


@pytest.mark.parametrize("T,Ty", [(1, 1), (1, 9), (7, 7), (65, 130), (130, 300)])
def test_maximum_path_bit_exact_on_random_matrices(T, Ty):
    g = torch.Generator().manual_seed(100 * T + Ty)
    val = torch.randn(1, Ty, T, generator=g) * 50 - 200                      # the scale of a neg_cent matrix at inter = 192
    d = _check_path(val, [T], [Ty])
    if T == Ty:
        assert d[0].tolist() == [1] * T                                        # the forced diagonal


def test_maximum_path_ragged_batch_in_one_padded_tensor():
    g = torch.Generator().manual_seed(7)
    xl, yl = [70, 3, 33], [97, 150, 33]
    val = torch.randn(3, 150, 70, generator=g) * 50 - 200
    for b in range(3):                                                         # what lies outside an item's lengths must not matter
        val[b, yl[b]:, :] = float("nan")
        val[b, :, xl[b]:] = float("nan")
    out = align.maximum_path(val.cuda(), xl, yl, want_attn=True)
    clean = torch.nan_to_num(val, nan=0.0)
    d_ref, a_ref, s_ref = PO.maximum_path(clean.numpy(), xl, yl)
    assert np.array_equal(out["durations"].cpu().numpy(), d_ref)
    assert np.array_equal(out["attn"].cpu().numpy()[:, 0], a_ref)
    assert np.array_equal(out["score"].cpu().numpy().view(np.uint32), s_ref.view(np.uint32))
    # each item alone, cut to its own size: the same path
    for b in range(3):
        alone = align.maximum_path(clean[b:b + 1, :yl[b], :xl[b]].contiguous().cuda(), [xl[b]], [yl[b]])
        assert np.array_equal(alone["durations"].cpu().numpy()[0], d_ref[b, :xl[b]])


def test_maximum_path_wide_text_uses_several_symbols_per_thread():
    """T > 1024: a thread owns more than one symbol and a wave writes more than one ballot word per row."""
    g = torch.Generator().manual_seed(9)
    T, Ty = 1100, 1203
    val = torch.randn(1, Ty, T, generator=g) * 50 - 200
    out = align.maximum_path(val.cuda(), [T], [Ty])
    d_ref, _, s_ref = PO.maximum_path(val.numpy(), [T], [Ty])
    assert np.array_equal(out["durations"].cpu().numpy(), d_ref)
    assert np.array_equal(out["score"].cpu().numpy().view(np.uint32), s_ref.view(np.uint32))


def test_maximum_path_tie_rule_on_integer_matrices():
    rng = np.random.RandomState(3)
    val = torch.from_numpy(rng.randint(-1, 2, size=(4, 40, 13)).astype(np.float32))
    _check_path(val, [13, 13, 5, 1], [40, 13, 39, 40])
    d = _check_path(torch.zeros(1, 7, 3), [3], [7])
    assert d[0].tolist() == [1, 1, 5]                                          # every path ties: spare frames go to the last symbol
    # the small exhaustive shapes of the CPU test, on the device: THE optimal path the rule selects
    for tx in range(1, 5):
        for ty in range(tx, 8):
            m = rng.randint(-1, 2, size=(1, ty, tx)).astype(np.float32)
            best, arg = PO.brute_force_path(m[0], tx, ty)
            out = align.maximum_path(torch.from_numpy(m).cuda(), [tx], [ty])
            assert tuple(out["durations"].cpu().numpy()[0]) == max(arg, key=lambda t: t[::-1]) and float(out["score"].cpu()[0]) == best


def _encode(m, batch, nw, kw):
    dev = lambda k: batch[k].cuda()
    return m.encode_durations(dev("x"), dev("x_lengths"), dev("sid"), dev("tone"), dev("language"), dev("bert"), dev("ja_bert"),
                              dev("en_bert"), nw, noise_scale_w=kw["noise_scale_w"], sdp_ratio=kw["sdp_ratio"],
                              length_scale=kw["length_scale"])


def test_align_latent_is_optimal_and_timing_transfer_decodes_its_path():
    """A latent against the narrow model's prior: the device path, scored in fp64 on the fp64 matrix, is within 2 Ty eps of the optimum
    (eps = max |neg_cent_device - neg_cent_fp64|: both paths sum Ty cells); then ``decode(with_durations(enc, d))`` walks exactly that
    path and y_lengths = sum d."""
    m, hp, batch, nw, nz, kw = _model()
    enc = _encode(m, batch, nw, kw)
    B, T = batch["x"].shape
    xl, yl = batch["x_lengths"].tolist(), [61, 40]
    Ty = max(yl)
    g = torch.Generator().manual_seed(21)
    z_p = torch.randn(B, hp.inter_channels, Ty, generator=g)
    out = m.align_latent(enc, z_p.cuda(), yl, want_attn=True, x_lengths=xl)
    d = out["durations"].cpu().numpy()
    nc64 = PO.neg_cent_f64(z_p, enc["m_p"].cpu(), enc["logs_p"].cpu(), xl, yl)
    eps = np.abs(out["neg_cent"].cpu().double().numpy() - nc64).max()
    d64, _, _ = PO.maximum_path(nc64, xl, yl, dtype=np.float64)
    for b in range(B):
        assert d[b, :xl[b]].min() >= 1 and d[b].sum() == yl[b] and not d[b, xl[b]:].any()
        got, best = PO.path_score(nc64[b], d[b]), PO.path_score(nc64[b], d64[b])
        # Why a second term beside the 2 Ty eps of the fixture tests: there the reference path comes from the SAME fp32 programme, so its
        # round-off cancels; here the optimum is the fp64 programme's, and the device's fp32 additions (Ty of them, on partial sums up to
        # Ty max|nc|, for each of the two paths compared) may legitimately prefer a path that is worse by that much (test_align_cpu.py)
        fp32_dp = 2 * yl[b] * yl[b] * np.abs(nc64[b]).max() * 2.0 ** -24
        assert got >= best - 2 * yl[b] * eps - fp32_dp, (b, got, best, eps)
    assert out["y_lengths"].tolist() == yl and out["attn"].shape == (B, 1, Ty, T)
    with pytest.raises(ValueError, match="must not exceed y_lengths"):
        m.align_latent(enc, z_p[:, :, :10].cuda(), [10, 10], x_lengths=xl)
    # timing transfer
    enc2 = models.with_durations(enc, out["durations"])
    assert enc2["y_lengths"].tolist() == yl
    dec = m.decode(enc2, nz.cuda(), Ty, noise_scale=kw["noise_scale"])
    assert torch.equal(dec["attn"], out["attn"])
    assert dec["y_mask"].sum([1, 2]).long().tolist() == yl and dec["o"].shape[2] == Ty * hp.total_upsample
    assert torch.isfinite(dec["o"]).all()


def _utts(lengths, durations=None):
    out = []
    for i, T in enumerate(lengths):
        b = synth.synthetic_batch([T], languages=[i % 3], sids=[i * 7 % 50], first_index=i)
        out.append(serving.Utterance(b["x"][0], b["tone"][0], b["language"][0], b["bert"][0], b["ja_bert"][0], b["en_bert"][0],
                                     int(b["sid"][0]), durations=None if durations is None else durations[i]))
    return out


def test_serving_align_and_given_durations():
    """``serving.align`` on a ragged set, then ``Utterance(durations=d)``: audio of exactly sum(d) * hop samples, also in a bucket shared
    with an utterance that keeps its predicted durations, and under graph replay."""
    m, hp, *_ = _model()
    hop = hp.total_upsample
    lengths, frames = [12, 9, 14], [40, 33, 14]
    g = torch.Generator().manual_seed(4)
    lat = [torch.randn(hp.inter_channels, n, generator=g) for n in frames]
    plain = _utts(lengths)
    durs = serving.align(m, plain, latents=lat, max_batch=4, max_pad_ratio=2.0)
    for d, T, n in zip(durs, lengths, frames):
        assert d.dtype == np.int64 and d.shape == (T,) and d.min() >= 1 and d.sum() == n
    assert durs[2].tolist() == [1] * 14                                        # as many frames as phones: the diagonal
    with pytest.raises(ValueError, match="cannot be aligned"):
        serving.align(m, plain[:1], latents=[lat[0][:, :5]])
    timed = _utts(lengths, [durs[0], None, durs[2]])
    noise = [(torch.randn(2, T, generator=g), torch.randn(hp.inter_channels, 16 * T, generator=g)) for T in lengths]
    kw = dict(sdp_ratio=0.5, noise_scale=0.6, noise_scale_w=0.9, length_scale=1.0, noise=noise, max_batch=4, max_pad_ratio=2.0)
    base = serving.synthesize(m, plain, **kw)
    out = serving.synthesize(m, timed, **kw)
    assert out[0].shape == (frames[0] * hop,) and out[2].shape == (frames[2] * hop,)
    assert out[1].shape == base[1].shape                                       # the utterance without durations keeps its own timing
    rel = np.sqrt(np.mean((out[1] - base[1]) ** 2)) / max(np.sqrt(np.mean(base[1] ** 2)), 1e-3)
    assert rel <= 1e-5                                                         # the same bucket shape either way: fp32 round-off at most
    assert all(np.isfinite(o).all() and np.abs(o).max() > 0 for o in out)
    m.enable_graphs(True)
    try:
        again = serving.synthesize(m, timed, **kw)
    finally:
        m.enable_graphs(False)
    assert [a.shape for a in again] == [o.shape for o in out]
    streamed = {}
    for i, start, piece in serving.synthesize_stream(m, timed, chunk_frames=16, **kw):
        streamed[i] = streamed.get(i, 0) + piece.shape[0]
    assert streamed[0] == frames[0] * hop and streamed[2] == frames[2] * hop
