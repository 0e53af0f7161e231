"""GPU: per-utterance synthesis controls (include/bv2.h bv2_item_controls).  Utterance b of a batch with per-item controls gets what a
batch-1 call with its own values as scalars gets; tensor controls reproduce the real reference run with [B,1,1] tensors
(tests/golden/item_controls_*.npz); one value for every item is the scalar call bit for bit; with graphs on, one capture per shape
serves every control set; the serving glue takes per-utterance sliders."""
import numpy as np
import pytest
import torch

from bert_vits2_amd import hparams as H, models, serving, synth
from oracle import bv2_oracle as O, cases
from tests.helpers import cached_state_dict, load_golden, rms, valid_wave_mask

pytestmark = pytest.mark.gpu

ORDER = ("noise_scale_w", "sdp_ratio", "length_scale", "noise_scale")
ARGS = ("x", "x_lengths", "sid", "tone", "language", "bert", "ja_bert", "en_bert")
NARROW = cases.CASES["narrow_b2_t18"]["hp"]


def _model(hp, seed=0):
    m = models.from_hparams(hp)
    m.load_state_dict(cached_state_dict(hp, seed), strict=False)
    return m.to("cuda").eval()


@pytest.fixture(scope="module")
def v23():
    return _model(H.default_v23())


def _inputs(hp, lengths, seed=4321):
    B = len(lengths)
    batch = synth.synthetic_batch(lengths, [i % 3 for i in range(B)], [(7 * i + 2) % 50 for i in range(B)])
    nw, nz = synth.synthetic_noise(B, max(lengths), cases.T_Y_CAP, hp.inter_channels, seed=seed)
    return batch, nw, nz


def _alone(batch, nw, nz, b, n):
    one = {k: v[b:b + 1] for k, v in batch.items()}
    for k in ("x", "tone", "language"):
        one[k] = one[k][:, :n]
    for k in ("bert", "ja_bert", "en_bert"):
        one[k] = one[k][:, :, :n]
    return one, nw[b:b + 1, :, :n], nz[b:b + 1]


def _infer(m, batch, nw, nz, **kw):
    o, attn, ym, _ = m.infer(*[batch[k].cuda() for k in ARGS], noise_w=nw, noise_z=nz.cuda(), **kw)
    return o, attn, ym, {k: v.clone() for k, v in m.last_encode.items()}


# five utterances, four (or five) distinct values per control
LENGTHS = [17, 24, 9, 22, 13]
CTL = dict(sdp_ratio=[0.2, 0.8, 0.5, 1.0, 0.0], noise_scale=[0.3, 0.9, 0.6, 0.667, 0.45],
           noise_scale_w=[0.5, 1.1, 0.8, 0.9, 0.3], length_scale=[0.8, 1.3, 1.0, 1.15, 0.9])


@pytest.mark.parametrize("mode", ["fp32", "bf16+f16"])
def test_per_item_batch_equals_each_utterance_alone(v23, mode):
    m, hp = v23, v23.hp
    if mode != "fp32":
        m.set_generator_dtype(torch.bfloat16)
        m.set_flow_dtype(torch.float16)
    try:
        batch, nw, nz = _inputs(hp, LENGTHS)
        B = len(LENGTHS)
        shapes = [(B,), (B, 1), (B, 1, 1), (B, 1, 1)]               # the reference's broadcast form and the flat ones
        kw = {k: torch.tensor(CTL[k]).view(*sh) for k, sh in zip(ORDER, shapes)}
        o, attn, ym, enc = _infer(m, batch, nw, nz, exact_lengths=True, **kw)
        for b, n in enumerate(LENGTHS):
            one, w1, z1 = _alone(batch, nw, nz, b, n)
            o1, attn1, ym1, enc1 = _infer(m, one, w1, z1, exact_lengths=True, **{k: float(CTL[k][b]) for k in ORDER})
            ty = int(enc1["y_lengths"][0])
            assert int(enc["y_lengths"][b]) == ty, b
            assert torch.equal(enc["w_ceil"][b, :n], enc1["w_ceil"][0]), b
            assert torch.equal(attn[b, :, :ty, :n], attn1[0]) and attn[b].sum().item() == ty, b
            d = (enc["logw"][b, :n] - enc1["logw"][0]).abs().max().item()
            assert d <= 1e-5, (b, d)
            S = ty * hp.total_upsample
            a, r = o[b, 0, :S].cpu().numpy(), o1[0, 0].cpu().numpy()
            assert r.shape == (S,)
            tol = 1e-5 if mode == "fp32" else 2e-2                  # the bars of test_serving_gpu's batched-versus-alone test
            assert np.sqrt(np.mean((a - r) ** 2)) <= tol * max(np.sqrt(np.mean(r ** 2)), 1e-3), b
    finally:
        m.set_generator_dtype(torch.float32)
        m.set_flow_dtype(torch.float32)


@pytest.mark.parametrize("name", ["item_controls_narrow_b3", "item_controls_narrow_b2"])
def test_tensor_controls_match_reference_golden(name):
    """The reference's batch semantics (exact_lengths=False): durations exact, waveform at the parity bars of test_parity_gpu."""
    meta, gold = load_golden(name)
    hp = H.default_v23(**NARROW)
    assert meta["model_case"] == "narrow_b2_t18"
    m = _model(hp, cases.CASES["narrow_b2_t18"]["seed"])
    batch = synth.synthetic_batch(meta["lengths"], meta["languages"], meta["sids"])
    B, T = batch["x"].shape
    nw, nz = synth.synthetic_noise(B, T, cases.T_Y_CAP, hp.inter_channels)
    kw = {k: gold["controls"][r].view(B, 1, 1) for r, k in enumerate(meta["control_order"])}
    o, attn, ym, enc = _infer(m, batch, nw, nz, **kw)
    assert torch.equal(enc["w_ceil"].cpu(), gold["w_ceil"][:, 0])
    assert torch.equal(enc["y_lengths"].cpu(), gold["y_lengths"])
    assert torch.equal(attn.cpu(), gold["attn"]) and torch.equal(ym.cpu(), gold["y_mask"])
    d = (enc["logw"].cpu() - gold["logw"][:, 0]).abs().max().item()
    assert d < 3e-4 * max(1.0, gold["logw"].abs().max().item()), d
    assert o.shape == gold["o"].shape
    vm = valid_wave_mask(gold["y_lengths"], hp.total_upsample, gold["o"].shape[2])
    err = rms((o.cpu() - gold["o"])[vm])
    assert err <= 1e-3 and err <= 5e-5, err
    print(f"[{name}] wave RMS err vs reference with [B,1,1] controls = {err:.3e}")


def test_uniform_tensor_controls_are_the_scalar_call(v23):
    m, hp = v23, v23.hp
    batch, nw, nz = _inputs(hp, LENGTHS)
    B = len(LENGTHS)
    sc = dict(sdp_ratio=0.5, noise_scale=0.6, noise_scale_w=0.9, length_scale=1.1)
    ref = _infer(m, batch, nw, nz, **sc)
    got = _infer(m, batch, nw, nz, **{k: torch.full((B, 1, 1), v) for k, v in sc.items()})
    for a, b in zip(ref[:3], got[:3]):
        assert torch.equal(a, b)
    for k in ("logw", "logw_sdp", "logw_dp", "w_ceil", "y_lengths", "m_p", "logs_p"):
        assert torch.equal(ref[3][k], got[3][k]), k


def test_graphs_one_capture_serves_every_control_set(v23):
    m, hp = v23, v23.hp
    batch, nw, nz = _inputs(hp, LENGTHS)
    B = len(LENGTHS)
    g = torch.Generator().manual_seed(3)
    cands = []
    for _ in range(6):
        c = {k: torch.tensor(CTL[k]) for k in ORDER}
        c["noise_scale"] = torch.rand(B, generator=g) * 0.8 + 0.1
        c["noise_scale_w"] = torch.rand(B, generator=g) * 0.8 + 0.3
        c["sdp_ratio"] = (c["sdp_ratio"] + torch.rand(B, generator=g) * 0.1 - 0.05).clamp(0, 1)
        cands.append(c)
    tys = [int(_infer(m, batch, nw, nz, **c)[2].shape[2]) for c in cands]
    sets = [c for c, t in zip(cands, tys) if (t + 31) // 32 == (tys[0] + 31) // 32][:3]
    assert len(sets) == 3, tys                                       # three control sets inside one 32-frame T_y bucket
    eager = [_infer(m, batch, nw, nz, ty_bucket=32, **c) for c in sets]   # the eager launch sequence at the bucket
    m.enable_graphs(True)
    try:
        got = [_infer(m, batch, nw, nz, **c) for c in sets]
        torch.cuda.synchronize()
        assert m.graph_stats["captures"] == 2, m.graph_stats           # one encode + one decode capture for all three sets
        assert m.graph_stats["replays"] == 4, m.graph_stats
        for e, r in zip(eager, got):
            for a, b in zip(e[:3], r[:3]):
                assert a.shape == b.shape and torch.equal(a, b)
            for k in ("logw", "w_ceil", "y_lengths"):
                assert torch.equal(e[3][k], r[3][k]), k
    finally:
        m.enable_graphs(False)


def test_serving_with_per_utterance_controls_matches_the_oracle():
    hp = H.default_v23(**NARROW)
    seed = cases.CASES["narrow_b2_t18"]["seed"]
    m = _model(hp, seed)
    sd = cached_state_dict(hp, seed)
    lengths = [14, 9, 17, 11]
    vals = [dict(sdp_ratio=0.2, noise_scale=0.3, noise_scale_w=0.5, length_scale=0.8),
            dict(sdp_ratio=0.8, noise_scale=None, noise_scale_w=1.1, length_scale=1.3),
            dict(sdp_ratio=None, noise_scale=0.9, noise_scale_w=None, length_scale=1.0),
            dict(sdp_ratio=1.0, noise_scale=0.667, noise_scale_w=0.8, length_scale=None)]
    call = dict(sdp_ratio=0.5, noise_scale=0.6, noise_scale_w=0.9, length_scale=1.15)
    utts, noise = [], []
    g = torch.Generator().manual_seed(9)
    for i, (T, v) in enumerate(zip(lengths, vals)):
        b = synth.synthetic_batch([T], languages=[i % 3], sids=[3 * i + 1], first_index=i)
        utts.append(serving.Utterance(b["x"][0], b["tone"][0], b["language"][0], b["bert"][0], b["ja_bert"][0], b["en_bert"][0],
                                      int(b["sid"][0]), **v))
        noise.append((torch.randn(2, T, generator=g), torch.randn(hp.inter_channels, 64 * T, generator=g)))
    out = serving.synthesize(m, utts, noise=noise, max_batch=2, max_pad_ratio=2.0, **call)
    for i, (u, v) in enumerate(zip(utts, vals)):
        kw = {k: call[k] if v[k] is None else v[k] for k in call}
        b = synth.synthetic_batch([lengths[i]], languages=[i % 3], sids=[3 * i + 1], first_index=i)
        ref = O.infer(sd, hp, b["x"], b["x_lengths"], b["sid"], b["tone"], b["language"], b["bert"], b["ja_bert"], b["en_bert"],
                      noise_w=noise[i][0][None], noise_z=noise[i][1][None], **kw)
        r = ref["o"][0, 0].numpy()
        assert out[i].shape == r.shape, (i, out[i].shape, r.shape)       # same durations
        err = float(np.sqrt(np.mean((out[i] - r) ** 2)))
        assert err <= 1e-3 and err <= 5e-5, (i, err)
    again = serving.synthesize(m, utts, noise=noise, max_batch=2, max_pad_ratio=2.0, requests_in_flight=2, **call)
    assert all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(out, again))
