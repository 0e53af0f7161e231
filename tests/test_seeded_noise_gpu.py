"""GPU: per-utterance noise seeds (include/bv2.h bv2_set_noise_seeds, csrc/kernels/rng.h).  The fill kernel against the fp64 restatement
(tests/seeded_noise_ref.py); purity of the value in (seed, draw, row, frame); the fused consumers against the same values injected as
tensors, bit for bit, eager and replayed; batch independence, streaming, posterior / alignment, the serving glue, and the errors."""
import ctypes as C

import numpy as np
import pytest
import torch

from bert_vits2_amd import hparams as H, lib as L, models, serving, synth
from oracle import cases
from tests import seeded_noise_ref as R
from tests.helpers import cached_state_dict

pytestmark = pytest.mark.gpu

ARGS = ("x", "x_lengths", "sid", "tone", "language", "bert", "ja_bert", "en_bert")
ORDER = ("noise_scale_w", "sdp_ratio", "length_scale", "noise_scale")
NARROW = cases.CASES["narrow_b2_t18"]["hp"]
_M = {}


def _model(name):
    if name not in _M:
        hp = H.default_v23() if name == "v23" else H.default_v23(**NARROW)
        seed = 0 if name == "v23" else cases.CASES["narrow_b2_t18"]["seed"]
        m = models.from_hparams(hp)
        m.load_state_dict(cached_state_dict(hp, seed), strict=False)
        _M[name] = m.to("cuda").eval()
    return _M[name]


def _batch(lengths):
    B = len(lengths)
    b = synth.synthetic_batch(lengths, [i % 3 for i in range(B)], [(7 * i + 2) % 50 for i in range(B)])
    return {k: b[k].cuda() for k in ARGS}


def _infer(m, batch, **kw):
    o, attn, ym, (z, z_p, m_p, logs_p) = m.infer(*[batch[k] for k in ARGS], **kw)
    enc = {k: v.clone() for k, v in m.last_encode.items()}
    return dict(o=o, z_p=z_p, w_ceil=enc["w_ceil"], logw=enc["logw"], y_lengths=enc["y_lengths"], attn=attn)


def _rel_rms(a, r):
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    return float(np.sqrt(np.mean((a - r) ** 2)) / max(np.sqrt(np.mean(r ** 2)), 1e-3))


# ---------------------------------------------------------------------------------------------------------------- 1. the fill kernel
@pytest.mark.parametrize("rows,T", [(2, 1), (2, 257), (6, 255), (192, 64)])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_fill_against_fp64(which, rows, T):
    """|device - fp64| <= 4e-6: logf and sqrtf are documented at 1 ulp and sincospif at <= 2 ulp, with one rounded product <= 4 ulp of a
    result of at most 5.77 = 1.4e-6; the bar leaves about 3x over that."""
    seeds, lengths = [0, -1, 12345], [T, 1, T - 1]
    ref = R.fill(seeds, which, rows, T, lengths)
    for transposed in (False, True):
        out = models.seeded_noise(seeds, which, rows, T, lengths=lengths, transposed=transposed)
        assert out.shape == (3, rows, T) and out.dtype == torch.float32
        assert out.stride() == ((T * rows, 1, rows) if transposed else (rows * T, T, 1))
        got = out.cpu().double().numpy()
        err = float(np.abs(got - ref).max())
        print(f"fill which={which} rows={rows} T={T} transposed={transposed}: max |device - fp64| = {err:.3e}, max |value| = {np.abs(got).max():.3f}")
        assert err <= 4e-6
        for b, n in enumerate(lengths):
            assert not got[b, :, n:].any()                      # exactly 0 at and past the length
            assert got[b, :, :n].all() or n == 0
    assert np.abs(ref).max() <= np.sqrt(48 * np.log(2)) + 1e-9


# ---------------------------------------------------------------------------------------------------------------- 2. purity
def test_value_is_a_pure_function_of_seed_draw_row_frame():
    seeds = [7, -3, 2 ** 62]
    long = models.seeded_noise(seeds, 1, 8, 1000)
    assert torch.equal(models.seeded_noise(seeds, 1, 8, 300), long[:, :, :300])
    for b, s in enumerate(seeds):
        assert torch.equal(models.seeded_noise([s], 1, 8, 1000)[0], long[b])
    assert torch.equal(models.seeded_noise(seeds, 1, 192, 300)[:, :8], long[:, :, :300])
    assert not torch.equal(models.seeded_noise(seeds, 2, 8, 300), long[:, :, :300])
    assert not torch.equal(long[0], long[1])


# ---------------------------------------------------------------------------------------------------------------- 3. fused == injected
LENGTHS = [17, 24, 9]
KW = dict(sdp_ratio=0.5, noise_scale=0.6, noise_scale_w=0.9, length_scale=1.0, exact_lengths=True)


def _injected(m, batch, seeds, ref, **kw):
    """The same call with the seeded values handed over as tensors (ref: the seeded run, for T_y and y_lengths)."""
    T = batch["x"].shape[1]
    Ty = int(ref["y_lengths"].max())
    nw = models.seeded_noise(seeds, models.NOISE_W, 2, T)
    nz = models.seeded_noise(seeds, models.NOISE_Z, m.hp.inter_channels, Ty, lengths=ref["y_lengths"])
    return _infer(m, batch, noise_w=nw, noise_z=nz, **kw)


def _same(a, b, what):
    for k in ("o", "z_p", "w_ceil", "logw"):
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("sdp_ratio", [0.5, 0.0])
def test_fused_equals_injected(sdp_ratio):
    """At sdp_ratio 0 the stochastic predictor is skipped and noise_w is never read."""
    m, batch = _model("v23"), _batch(LENGTHS)
    seeds = [11, -5, 2 ** 40 + 3]
    kw = dict(KW, sdp_ratio=sdp_ratio)
    got = _infer(m, batch, seeds=seeds, **kw)
    _same(got, _injected(m, batch, seeds, got, **kw), f"sdp_ratio={sdp_ratio}")
    other = _infer(m, batch, seeds=[12, -5, 2 ** 40 + 3], **kw)
    assert not torch.equal(other["z_p"][0], got["z_p"][0])            # item 0 has another seed ...
    n = int(min(got["y_lengths"][1], other["y_lengths"][1]))
    if sdp_ratio == 0.0:                                              # ... item 1 does not (durations are the same without the SDP)
        assert torch.equal(other["z_p"][1, :, :n], got["z_p"][1, :, :n])


def test_fused_equals_injected_half_precision():
    m, batch = _model("v23"), _batch(LENGTHS)
    m.set_generator_dtype(torch.bfloat16)
    m.set_flow_dtype(torch.float16)
    try:
        seeds = [11, -5, 2 ** 40 + 3]
        got = _infer(m, batch, seeds=seeds, **KW)
        _same(got, _injected(m, batch, seeds, got, **KW), "bf16+f16")
    finally:
        m.set_generator_dtype(torch.float32)
        m.set_flow_dtype(torch.float32)


def test_graph_replay_reads_the_seeds_at_replay_time():
    """Replays with seeds s, then s': each equals the eager run of its own seeds at the same bucket and the injected run through the
    graph — a seed pointer or value baked into the capture would fail the second."""
    m, batch = _model("v23"), _batch(LENGTHS)
    cands = [[11, -5, 2 ** 40 + 3], [1, 2, 3], [-9, 77, 5], [2 ** 63 - 1, 0, -2 ** 63]]
    eager = [_infer(m, batch, seeds=s, ty_bucket=32, **KW) for s in cands]
    bucket = [(int(e["y_lengths"].max()) + 31) // 32 for e in eager]
    pair = next(((i, j) for i in range(4) for j in range(i + 1, 4) if bucket[i] == bucket[j]), (0, 1))
    m.enable_graphs(True, ty_bucket=32)
    try:
        for n, i in enumerate(pair):
            got = _infer(m, batch, seeds=cands[i], **KW)
            _same(got, eager[i], f"replay {n} vs eager")
        torch.cuda.synchronize()
        stats = dict(m.graph_stats)
        assert stats["captures"] == (2 if bucket[pair[0]] == bucket[pair[1]] else 3), (stats, bucket)   # phase A once, phase B once per bucket
        assert all("noise_z" not in e["sin"] for k, e in m._graphs.items() if k[0] == "B")               # a seeded entry owns no noise buffer
        inj = _injected(m, batch, cands[pair[1]], eager[pair[1]], **KW)                                  # injected, through the (unseeded) graphs
        _same(inj, eager[pair[1]], "injected replay vs seeded eager")
    finally:
        m.enable_graphs(False)


# ---------------------------------------------------------------------------------------------------------------- 4. batch independence
LENGTHS5 = [17, 24, 9, 22, 13]                  # the utterances, controls and bars of test_item_controls_gpu's batch-versus-alone test
CTL = dict(sdp_ratio=[0.2, 0.8, 0.5, 1.0, 0.0], noise_scale=[0.3, 0.9, 0.6, 0.667, 0.45],
           noise_scale_w=[0.5, 1.1, 0.8, 0.9, 0.3], length_scale=[0.8, 1.3, 1.0, 1.15, 0.9])
SEEDS5 = [101, -202, 303, 2 ** 50, -7]


def test_an_utterance_sounds_the_same_whatever_it_is_batched_with():
    m, hp = _model("v23"), _model("v23").hp
    batch = _batch(LENGTHS5)
    B = len(LENGTHS5)
    alone = []
    for b, n in enumerate(LENGTHS5):
        one = {k: v[b:b + 1] for k, v in batch.items()}
        for k in ("x", "tone", "language"):
            one[k] = one[k][:, :n]
        for k in ("bert", "ja_bert", "en_bert"):
            one[k] = one[k][:, :, :n]
        alone.append(_infer(m, one, seeds=[SEEDS5[b]], exact_lengths=True, **{k: float(CTL[k][b]) for k in ORDER}))
    for order in (list(range(B)), list(range(B))[::-1]):
        ix = torch.tensor(order).cuda()
        bb = {k: v[ix] for k, v in batch.items()}
        got = _infer(m, bb, seeds=[SEEDS5[i] for i in order], exact_lengths=True,
                     **{k: torch.tensor([CTL[k][i] for i in order]) for k in ORDER})
        for r, i in enumerate(order):
            n, ref = LENGTHS5[i], alone[i]
            ty = int(ref["y_lengths"][0])
            assert int(got["y_lengths"][r]) == ty, (order, i)
            assert torch.equal(got["w_ceil"][r, :n], ref["w_ceil"][0]), (order, i)
            d = (got["logw"][r, :n] - ref["logw"][0]).abs().max().item()
            assert d <= 1e-5, (order, i, d)
            S = ty * hp.total_upsample
            rr = _rel_rms(got["o"][r, 0, :S].cpu().numpy(), ref["o"][0, 0].cpu().numpy())
            assert ref["o"].shape[2] == S and rr <= 1e-5, (order, i, rr)


# ---------------------------------------------------------------------------------------------------------------- 5. streaming
def test_stream_equals_whole_and_z_p_does_not_depend_on_the_chunking():
    m, batch = _model("v23"), _batch(LENGTHS)
    U = m.hp.total_upsample
    seeds = [5, 6, -7]
    whole = _infer(m, batch, seeds=seeds, **KW)
    zps = []
    for chunk in (16, 23):
        st = m.infer_stream(*[batch[k] for k in ARGS], seeds=seeds, chunk_frames=chunk, **KW)
        zps.append(st.aux["z_p"].clone())
        cat = torch.cat([a for _, a in st], dim=1).cpu().numpy()
        for b, n in enumerate(st.y_lengths_host):
            r = _rel_rms(cat[b, :n * U], whole["o"][b, 0, :n * U].cpu().numpy())
            assert r <= 1e-5, (chunk, b, r)                      # the fp32 bar of tests/test_stream_gpu.py, streamed versus whole
    assert torch.equal(zps[0], zps[1]) and torch.equal(zps[0], whole["z_p"])
    with pytest.raises(ValueError, match="seeds"):
        m.infer_stream(*[batch[k] for k in ARGS], seeds=seeds, noise_w=torch.zeros(3, 2, 24), **KW)


# ---------------------------------------------------------------------------------------------------------------- 6. posterior, alignment
def test_posterior_and_align_take_seeds():
    from tests.test_posterior_gpu import _setup
    m, hp, batch, y, meta, G = _setup("narrow_b2_t18")
    yl = G["y_lengths"]
    B, Ty = y.shape[0], y.shape[2]
    seeds = [31, -32][:B]
    g = m.stage_emb_g(batch["sid"])
    got = m.posterior_encode(y, yl, g=g, seeds=seeds)
    ref = m.posterior_encode(y, yl, g=g, noise_q=models.seeded_noise(seeds, models.NOISE_Q, hp.inter_channels, Ty))
    assert torch.equal(got["z"], ref["z"]) and not torch.equal(got["z"], got["m_q"])
    with pytest.raises(ValueError, match="seeds"):
        m.posterior_encode(y, yl, g=g, seeds=seeds, noise_q=G["noise_q"])
    dev = lambda k: batch[k].cuda()
    xl = G["x_lengths"].tolist()
    args = (dev("x"), xl, dev("sid"), dev("tone"), dev("language"), dev("bert"), dev("ja_bert"), dev("en_bert"), y, yl.tolist())
    a = m.align(*args, seeds=seeds)
    b = m.align(*args, seeds=seeds)
    c = m.align(*args, seeds=seeds, one_call=True)
    assert torch.equal(a["durations"], b["durations"]) and torch.equal(a["durations"], c["durations"])
    assert torch.equal(a["posterior"]["z"], got["z"])
    assert a["durations"].sum(1).tolist() == yl.tolist()


# ---------------------------------------------------------------------------------------------------------------- 7. serving
def _utts(lengths, seeds):
    out = []
    for i, (T, s) in enumerate(zip(lengths, seeds)):
        b = synth.synthetic_batch([T], languages=[i % 3], sids=[3 * i + 1], first_index=i)
        out.append(serving.Utterance(b["x"][0], b["tone"][0], b["language"][0], b["bert"][0], b["ja_bert"][0], b["en_bert"][0],
                                     int(b["sid"][0]), seed=s))
    return out


def test_serving_requests_are_reproducible():
    m = _model("narrow")
    hp = m.hp
    call = dict(sdp_ratio=0.5, noise_scale=0.6, noise_scale_w=0.9, length_scale=1.0)
    utts = _utts([14, 9, 17], [1001, -1002, 1003])
    kw = dict(call, max_batch=2, max_pad_ratio=3.0)                      # two buckets
    first = serving.synthesize(m, utts, **kw)
    again = serving.synthesize(m, utts, **kw)
    lanes = serving.synthesize(m, utts, requests_in_flight=2, **kw)
    for a, b, c in zip(first, again, lanes):
        assert a.size > 0 and np.array_equal(a, b) and np.array_equal(a, c)
    # a fourth, longer utterance joins the bucket: the three keep their audio (the bar of the batch-independence test above)
    three = serving.synthesize(m, utts, max_batch=32, max_pad_ratio=3.0, **call)
    four = serving.synthesize(m, utts + _utts([20], [None]), max_batch=32, max_pad_ratio=3.0, **call)
    assert len(four) == 4 and four[3].size > 0
    for i in range(3):
        assert four[i].shape == three[i].shape, i
        assert _rel_rms(four[i], three[i]) <= 1e-5, i
    with pytest.raises(ValueError, match="seed"):
        serving.synthesize(m, utts, noise=[(torch.zeros(2, u.length), torch.zeros(hp.inter_channels, 64 * u.length)) for u in utts], **call)


def test_serving_without_seeds_is_the_drawn_path():
    """No utterance has a seed: torch.manual_seed governs the call exactly as before (draw_noise_w on the CPU generator, draw_noise_z on the
    device's, in the reference's order)."""
    m = _model("narrow")
    hp = m.hp
    call = dict(sdp_ratio=0.5, noise_scale=0.6, noise_scale_w=0.9, length_scale=1.0)
    utts = _utts([14, 9, 17], [None, None, None])
    torch.manual_seed(7)
    out = serving.synthesize(m, utts, max_batch=32, max_pad_ratio=3.0, **call)
    (idx,) = serving.plan_batches([u.length for u in utts], 32, 3.0)
    batch = serving.collate([utts[i] for i in idx], m.device)
    B, T = batch["x"].shape
    torch.manual_seed(7)
    enc = m.encode_durations(*[batch[k] for k in ARGS], models.draw_noise_w(B, T, None), noise_scale_w=0.9, sdp_ratio=0.5, length_scale=1.0,
                             lean=True)
    Ty = int(enc["y_lengths"].max())
    dec = m.decode(enc, models.draw_noise_z(B, hp.inter_channels, Ty, m.device), Ty, noise_scale=0.6, want_attn=False, exact_lengths=True)
    for r, i in enumerate(idx):
        n = int(enc["y_lengths"][r]) * hp.total_upsample
        assert np.array_equal(out[i], dec["o"][r, 0, :n].cpu().numpy()), i


# ---------------------------------------------------------------------------------------------------------------- 8. errors
def _raw_decode(m, enc, Ty, noise_z):
    """bv2_decode as a C caller makes it: (rc, message)."""
    B, _, T = enc["x"].shape
    hp = m.hp
    p = models._ptr
    o = torch.empty(B, 1, Ty * hp.total_upsample, device=m.device)
    din = L.DecodeIn(B, T, int(Ty), int(Ty), p(enc["m_p"]), p(enc["logs_p"]), p(enc["x_mask"]), p(enc["w_ceil"]), p(enc["y_lengths"]),
                     p(enc["g"]), p(noise_z), *((0, 0, 0) if noise_z is None else noise_z.stride()), 0.6, 0)
    dout = L.DecodeOut(p(o), None, None, None, None, None, None)
    ws = m._workspace(B, T, Ty)
    with torch.cuda.device(m.device):
        rc = m._lib.bv2_decode(m._handle, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(din), C.byref(dout),
                               C.c_void_p(ws.data_ptr()), ws.numel())
    torch.cuda.synchronize()
    return rc, m._lib.bv2_last_error(m._handle).decode()


def test_seed_errors():
    m = _model("narrow")
    hp = m.hp
    batch = _batch([9, 7])
    enc = m.encode_durations(*[batch[k] for k in ARGS], seeds=[1, 2], sdp_ratio=0.5)
    Ty = int(enc["y_lengths"].max())
    nz = torch.zeros(2, hp.inter_channels, Ty, device="cuda")
    s3 = torch.tensor([1, 2, 3], dtype=torch.int64, device="cuda")
    s2 = torch.tensor([1, 2], dtype=torch.int64, device="cuda")
    lib, h = m._lib, m._handle
    try:
        assert lib.bv2_set_noise_seeds(h, C.c_void_p(s3.data_ptr()), 3) == 0
        rc, msg = _raw_decode(m, enc, Ty, None)                      # B = 2 against three seeds
        assert rc != 0 and "bv2_set_noise_seeds" in msg and "B = 2" in msg, msg
        with pytest.raises(RuntimeError, match="bv2_set_noise_seeds"):
            m.encode_durations(*[batch[k] for k in ARGS], models.draw_noise_w(2, 9, None), sdp_ratio=0.5)
        assert lib.bv2_set_noise_seeds(h, C.c_void_p(s2.data_ptr()), 2) == 0
        rc, msg = _raw_decode(m, enc, Ty, nz)                        # a noise tensor together with active seeds
        assert rc != 0 and "noise_z" in msg and "seeds" in msg, msg
        rc, msg = _raw_decode(m, enc, Ty, None)                      # NULL noise with seeds: runs
        assert rc == 0, msg
    finally:
        assert lib.bv2_set_noise_seeds(h, None, 0) == 0
    rc, msg = _raw_decode(m, enc, Ty, None)                          # switched off: NULL noise fails as it always did
    assert rc != 0 and msg == "bv2_decode: null tensor pointer", msg
    rc, msg = _raw_decode(m, enc, Ty, nz)
    assert rc == 0, msg
    with pytest.raises(ValueError, match="seeds"):
        m.infer(*[batch[k] for k in ARGS], seeds=[1, 2], noise_w=torch.zeros(2, 2, 9))
    with pytest.raises(ValueError, match="seeds"):
        m.infer(*[batch[k] for k in ARGS], seeds=[1, 2, 3])
