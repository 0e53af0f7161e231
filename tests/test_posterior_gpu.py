"""GPU: the posterior encoder and the one-call aligner against the REAL reference's ``forward()`` (tests/golden/posterior_*.npz,
tools/gen_posterior_golden.py): its own ``enc_q`` on a spectrogram with an injected ``noise_q``, its forward flow, ``neg_cent`` and path.

Error bars: each device tensor (``m_q``, ``logs_q``, ``z``, ``z_p``) is held to the fixture's fp64 value with at most 4 x the reference's
own fp32 error against that value, tensor by tensor — the margin the ReferenceEncoder was given for a changed summation order.  ``z_p`` is
computed from the DEVICE ``z`` (the chain the reference's error also covers).  The figures are printed before each assertion and recorded
in docs/MEASUREMENTS.md."""
import numpy as np
import pytest
import torch

from bert_vits2_amd import hparams as H, models, serving, synth
from oracle import cases
from tests import posterior_oracle as PO
from tests.helpers import cached_state_dict, load_golden

pytestmark = pytest.mark.gpu
CASES = ["narrow_b2_t18", "mix_b2_ragged", "wn_b1_t16"]      # spec 80 / 3 couplings; v2.3 widths, spec 1025, transformer flow; WN flow
_M = {}


def _setup(name):
    if name not in _M:
        meta, G = load_golden("posterior_" + name)
        base = cases.CASES[name]
        hp = H.default_v23(**dict(base["hp"], spec_channels=meta["spec_channels"]))
        m = models.from_hparams(hp)
        m.load_state_dict(cached_state_dict(hp, base["seed"]), strict=False)
        m = m.to("cuda").eval()
        assert not m.has_posterior
        m.load_posterior(synth.synthetic_posterior_state_dict(hp, base["seed"]))
        assert m.has_posterior
        batch = synth.synthetic_batch(base["lengths"], base["languages"], base["sids"])
        frames = meta["frames"]
        y = torch.zeros(len(frames), hp.spec_channels, max(frames))
        for b, L in enumerate(frames):
            y[b, :, :L] = synth.synthetic_reference_spec(hp.spec_channels, L, b)
        _M[name] = (m, hp, batch, y, meta, G)
    return _M[name]


def _held(name, what, dev, ref64, ref_err):
    err = float((dev.double().cpu() - ref64).abs().max())
    print(f"{name} {what}: device max err {err:.3e}, reference fp32 err {ref_err:.3e} (ratio {err / ref_err:.2f}), |ref| max {float(ref64.abs().max()):.3f}")
    assert err <= 4 * ref_err


@pytest.mark.parametrize("name", CASES)
def test_posterior_encode_and_forward_flow_against_the_reference(name):
    m, hp, batch, y, meta, G = _setup(name)
    yl = G["y_lengths"]
    g = m.stage_emb_g(batch["sid"])
    out = m.posterior_encode(y, yl, g=g, noise_q=G["noise_q"])
    assert out["z"].shape == (len(yl), hp.inter_channels, y.shape[2]) and out["y_mask"].shape == (len(yl), 1, y.shape[2])
    assert out["y_mask"].sum([1, 2]).long().tolist() == yl.tolist()
    _held(name, "m_q", out["m_q"], G["m_q64"], meta["ref_err_m_q"])
    _held(name, "logs_q", out["logs_q"], G["logs_q64"], meta["ref_err_logs_q"])
    _held(name, "z", out["z"], G["z64"], meta["ref_err_z"])
    z_p = m.stage_flow_forward(out["z"], yl, g)
    _held(name, "z_p", z_p, G["z_p64"], meta["ref_err_z_p"])
    for b in range(len(yl)):
        assert not out["z"][b, :, int(yl[b]):].any() and not out["m_q"][b, :, int(yl[b]):].any()
    # sid instead of g is the same call; no noise is the deterministic latent, exactly m_q (already masked)
    by_sid = m.posterior_encode(y, yl, sid=batch["sid"], noise_q=G["noise_q"])
    assert torch.equal(by_sid["z"], out["z"])
    det = m.posterior_encode(y, yl, g=g)
    assert torch.equal(det["z"], det["m_q"]) and torch.equal(det["m_q"], out["m_q"])
    # round trip through the flow, same bar as z_p
    _held(name, "stage_flow(stage_flow_forward(z))", m.stage_flow(z_p, yl, g), out["z"].double().cpu(), meta["ref_err_z_p"])
    with pytest.raises(ValueError, match="y must be"):
        m.posterior_encode(y[:, :-1], yl, g=g)


def test_a_ragged_batch_gives_each_item_what_it_gets_alone():
    m, hp, batch, y, meta, G = _setup("narrow_b2_t18")
    yl = G["y_lengths"]
    g = m.stage_emb_g(batch["sid"])
    both = m.posterior_encode(y, yl, g=g)
    b, n = 1, int(yl[1])
    alone = m.posterior_encode(y[b:b + 1, :, :n].contiguous(), yl[b:b + 1], g=g[b:b + 1])
    ref = both["m_q"][b, :, :n]
    assert float((alone["m_q"][0] - ref).abs().max()) <= 1e-5 * float(ref.abs().max())   # another tiling of the same sums; padding never read in


@pytest.mark.parametrize("name", CASES)
def test_align_end_to_end_from_the_spectrogram(name):
    """``align`` on the fixture's inputs.  The device path, scored in fp64 on the FIXTURE's neg_cent, is within 2 Ty eps of the fixture's
    optimum (eps = max |neg_cent_device - neg_cent_fixture|; both paths sum Ty cells); where eps = 0 the durations are the fixture's.
    Then timing transfer: ``decode(with_durations(enc, d))`` walks the path's one-hot matrix and y_lengths = sum d."""
    m, hp, batch, y, meta, G = _setup(name)
    xl, yl = G["x_lengths"].tolist(), G["y_lengths"].tolist()
    dev = lambda k: batch[k].cuda()
    out = m.align(dev("x"), xl, dev("sid"), dev("tone"), dev("language"), dev("bert"), dev("ja_bert"), dev("en_bert"), y, yl,
                  noise_q=G["noise_q"], want_attn=True)
    d = out["durations"].cpu().numpy()
    gold = G["neg_cent"].double().numpy()
    eps = float(np.abs(out["neg_cent"].cpu().double().numpy() - gold).max())
    print(f"{name} align: eps {eps:.3e}, durations equal the fixture's: {np.array_equal(d, G['durations'].numpy())}")
    for b in range(len(xl)):
        assert d[b, :xl[b]].min() >= 1 and d[b].sum() == yl[b] and not d[b, xl[b]:].any()
        got, best = PO.path_score(gold[b], d[b]), PO.path_score(gold[b], G["durations"][b].numpy())
        assert got >= best - 2 * yl[b] * eps
    if eps == 0:
        assert np.array_equal(d, G["durations"].numpy())
    assert out["y_lengths"].tolist() == yl and set(out["posterior"]) >= {"z", "m_q", "logs_q", "y_mask"}
    # the one-call form (bv2_align) runs the same launches on one workspace: the same path, bit for bit
    one = m.align(dev("x"), xl, dev("sid"), dev("tone"), dev("language"), dev("bert"), dev("ja_bert"), dev("en_bert"), y, yl,
                  noise_q=G["noise_q"], want_attn=True, one_call=True)
    assert torch.equal(one["durations"], out["durations"]) and torch.equal(one["attn"], out["attn"]) and torch.equal(one["score"], out["score"])
    enc2 = models.with_durations(out["enc"], out["durations"])
    Ty = max(yl)
    dec = m.decode(enc2, torch.zeros(len(xl), hp.inter_channels, Ty, device="cuda"), Ty)
    assert torch.equal(dec["attn"], out["attn"]) and dec["y_mask"].sum([1, 2]).long().tolist() == yl
    with pytest.raises(ValueError, match="must not exceed y_lengths"):
        m.align(dev("x"), xl, dev("sid"), dev("tone"), dev("language"), dev("bert"), dev("ja_bert"), dev("en_bert"), y[:, :, :5], [5] * len(xl))


def test_serving_align_from_spectrograms_and_timing_transfer():
    m, hp, batch, y, meta, G = _setup("narrow_b2_t18")
    hop = hp.total_upsample
    lengths, frames = [12, 9], [40, 33]
    utts = []
    for i, T in enumerate(lengths):
        b = synth.synthetic_batch([T], languages=[i % 3], sids=[i * 7 % 50], first_index=i)
        utts.append(serving.Utterance(b["x"][0], b["tone"][0], b["language"][0], b["bert"][0], b["ja_bert"][0], b["en_bert"][0], int(b["sid"][0])))
    specs = [synth.synthetic_reference_spec(hp.spec_channels, n, i) for i, n in enumerate(frames)]
    durs = serving.align(m, utts, specs, max_batch=4, max_pad_ratio=2.0)
    for d, T, n in zip(durs, lengths, frames):
        assert d.dtype == np.int64 and d.shape == (T,) and d.min() >= 1 and d.sum() == n
    timed = [serving.Utterance(u.phones, u.tones, u.lang_ids, u.bert, u.ja_bert, u.en_bert, u.sid, durations=d) for u, d in zip(utts, durs)]
    out = serving.synthesize(m, timed, max_batch=4, max_pad_ratio=2.0)
    assert [o.shape for o in out] == [(n * hop,) for n in frames]
    with pytest.raises(ValueError, match="exactly one"):
        serving.align(m, utts, specs, latents=specs)
