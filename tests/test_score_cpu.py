"""CPU: scoring a take against its text — the fp64 restatement (tests/score_oracle.py) against the REAL reference's numbers
(tests/golden/score_*.npz, tools/gen_score_golden.py), the forward duration predictor's own weight blob, what a stripped checkpoint and an
unloaded model answer, the argument checks of the two new library calls, and the seeded ``e_q`` draw on the host."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest
import torch

from bert_vits2_amd import hparams as H, lib as L, models, schema, serving, synth
from oracle import cases
from tests import score_oracle as SO
from tests import seeded_noise_ref as R
from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLL_CASES = ["t1", "t3", "t17", "t18", "b2_ragged", "zero_dur", "narrow_b2_t18"]
KL_CASES = ["narrow_b2_t18", "mix_b2_ragged", "wn_b1_t16"]
EXPORTS = ("bv2_sdp_forward_load_tensor", "bv2_sdp_forward_packed_bytes", "bv2_sdp_forward_pack", "bv2_sdp_forward_attach",
           "bv2_sdp_forward_detach", "bv2_duration_nll", "bv2_duration_nll_workspace_bytes", "bv2_kl_path")


def narrow_hp():
    return H.default_v23(**cases.CASES["narrow_b2_t18"]["hp"])


def _model(hp):
    m = models.from_hparams(hp)
    m.load_state_dict(synth.synthetic_state_dict(hp, 0), strict=False)
    return m


def test_acceptance_the_score_surface_exists():
    """Fails on the parent: no bv2_duration_nll symbol, no net_g.duration_nll."""
    hdr = open(os.path.join(ROOT, "include", "bv2.h")).read()
    assert re.search(r"#define BV2_ABI_VERSION 3\b", hdr) and re.search(r"#define BV2_PACK_LAYOUT 16\b", hdr)
    assert re.search(r"#define BV2_POSTERIOR_LAYOUT 1\b", hdr)
    lib = L.load()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert getattr(lib, name) is not None and name in {s[0] for s in L.SYMBOLS}
    for attr in ("load_sdp_forward", "has_sdp_forward", "duration_nll", "score"):
        assert hasattr(models.SynthesizerTrn, attr), attr
    assert hasattr(serving, "score") and models.NOISE_E == 3 and (models.NOISE_W, models.NOISE_Z, models.NOISE_Q) == (0, 1, 2)
    with pytest.raises(NotImplementedError):
        _model(narrow_hp()).forward()                                        # training stays with the reference


@pytest.mark.parametrize("name", NLL_CASES)
def test_restatement_reproduces_the_reference_duration_likelihood(name):
    meta, G = load_golden("score_" + name)
    hp = H.default_v23(**meta["hp"])
    sd = synth.synthetic_state_dict(hp, meta["seed"])
    sd.update(synth.synthetic_sdp_forward_state_dict(hp, meta["seed"]))
    assert cases.weight_checksums(sd) == meta["checksums"]
    sd64 = {k: v.double() for k, v in sd.items() if k.startswith("sdp.")}
    d = lambda k: G[k].double()
    nll, sym = SO.sdp_forward(sd64, d("x"), d("x_mask"), d("w"), d("g"), d("noise_e"))
    rel = float(((nll - G["nll64"]).abs() / G["nll64"].abs()).max())
    print(f"{name}: restatement vs the reference's fp64 nll, relative {rel:.2e}")
    assert rel <= 1e-9
    assert float((sym - G["nll_sym64"]).abs().max()) <= 1e-9 * float(G["nll_sym64"].abs().max())
    assert float((sym.sum(1) - nll).abs().max()) <= 1e-9 * float(nll.abs().max())          # the decomposition is exact
    assert not sym[G["x_mask"][:, 0] == 0].any()
    if meta["zero"]:
        for b, t in meta["zero"]:
            assert float(G["w"][b, 0, t]) == 0.0


@pytest.mark.parametrize("name", KL_CASES)
def test_restatement_reproduces_the_reference_kl(name):
    meta, G = load_golden("score_kl_" + name)
    _pm, P = load_golden("posterior_" + name)
    d = lambda t: t.double()
    kl, frame = SO.kl_frames(d(P["z_p"]), d(P["logs_q64"].float()), d(P["m_p"]), d(P["logs_p"]), P["durations"], P["x_lengths"].tolist(),
                             P["y_lengths"].tolist())
    rel = float(((kl - G["kl64"]).abs() / G["kl64"].abs()).max())
    print(f"{name}: restatement vs the reference's fp64 kl, relative {rel:.2e}")
    assert rel <= 1e-9 and torch.equal(frame, G["kl_frame64"])
    for b, n in enumerate(P["y_lengths"].tolist()):
        assert not frame[b, n:].any()


def test_forward_spline_restatement_is_the_inverse_of_the_inverse():
    g = torch.Generator().manual_seed(5)
    n = 4096
    x = (torch.rand(n, generator=g, dtype=torch.float64) * 12 - 6)
    uw, uh, ud = (torch.randn(n, k, generator=g, dtype=torch.float64) for k in (10, 10, 9))
    y, lad = SO.rq_spline_forward(x, uw, uh, ud)
    out = x.abs() > 5
    assert torch.equal(y[out], x[out]) and not lad[out].any()
    assert float((SO.rq_spline_inverse(y, uw, uh, ud) - x).abs().max()) <= 1e-9
    eps = 1e-6                                                                             # logabsdet is log of the slope
    inner = x.abs() < 4.99
    y2, _ = SO.rq_spline_forward(x + eps, uw, uh, ud)
    slope = (y2 - y) / eps
    assert float((torch.log(slope[inner]) - lad[inner]).abs().max()) <= 1e-3


def test_sdp_forward_schema_and_blob_round_trip():
    hp = narrow_hp()
    shapes = schema.sdp_forward_param_shapes(hp)
    assert all(k.startswith("sdp.post_") for k in shapes) and not any(k.startswith("sdp.post_") for k in schema.param_shapes(hp))
    sd = synth.synthetic_sdp_forward_state_dict(hp, 0)
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(shapes)
    assert all(torch.equal(a, b) for a, b in zip(sd.values(), synth.synthetic_sdp_forward_state_dict(hp, 0).values()))
    m = _model(hp)
    before = m.pack_host_blob()
    b1 = m.pack_sdp_forward_host_blob(sd)
    assert not m.has_sdp_forward                                                 # packed on the host, nothing attached
    assert b1.dtype == torch.uint8 and b1.numel() == m._lib.bv2_sdp_forward_packed_bytes(m._handle) > 0
    assert torch.equal(b1, m.pack_sdp_forward_host_blob(sd))                     # a pure function of the tensors
    hdr = np.frombuffer(b1[:32].numpy().tobytes(), dtype=np.uint32)
    assert hdr[0] == 0x66765642 and hdr[1] == 3 and hdr[3] == 1
    assert int(np.frombuffer(b1[16:24].numpy().tobytes(), dtype=np.int64)[0]) * 4 == b1.numel()
    # every weight landed exactly once (padding is zeros): the blob's sum of squares is the tensors' — post_* and the model's own flows.1
    own = {k: v for k, v in m.state_dict().items() if k.startswith("sdp.flows.1.")}
    assert len(own) == len([k for k in schema.param_shapes(hp) if k.startswith("sdp.flows.1.")]) > 0
    want = sum(float(v.double().pow(2).sum()) for v in list(sd.values()) + list(own.values()))
    got = float(b1[256:].view(torch.float32).double().pow(2).sum())
    assert abs(got - want) <= 1e-9 * want
    # a checkpoint's own flows.1 takes the place of the model's
    other = dict(sd)
    other.update({k: v + 1.0 for k, v in own.items()})
    assert not torch.equal(b1, _model(hp).pack_sdp_forward_host_blob(other))
    assert not torch.equal(b1, _model(hp).pack_sdp_forward_host_blob(synth.synthetic_sdp_forward_state_dict(hp, 1)))
    short = {k: v for k, v in sd.items() if k != "sdp.post_flows.5.convs.norms_2.1.beta"}
    with pytest.raises(RuntimeError, match=r"sdp\.post_flows\.5\.convs\.norms_2\.1\.beta"):
        _model(hp).pack_sdp_forward_host_blob(short)
    bad = dict(sd)
    bad["sdp.post_pre.weight"] = torch.zeros(hp.hidden_channels, 2, 1)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        _model(hp).pack_sdp_forward_host_blob(bad)
    # the inference blob, its size and the shim's state_dict did not move
    after = m.pack_host_blob()
    assert hashlib.sha256(before.numpy().tobytes()).hexdigest() == hashlib.sha256(after.numpy().tobytes()).hexdigest()
    assert {k for k, _ in m.named_parameters()} == set(schema.param_shapes(hp))
    t = torch.zeros(4)
    shape = (C.c_int64 * 1)(4)
    P = lambda v: C.c_void_p(v.data_ptr())
    assert m._lib.bv2_load_tensor(m._handle, b"sdp.post_pre.bias", P(t), shape, 1, L.F32) == 1
    assert m._lib.bv2_sdp_forward_load_tensor(m._handle, b"sdp.flows.3.pre.bias", P(t), shape, 1, L.F32) == 1
    assert m._lib.bv2_sdp_forward_load_tensor(m._handle, b"enc_q.pre.bias", P(t), shape, 1, L.F32) == 1
    assert m._lib.bv2_sdp_forward_load_tensor(m._handle, b"sdp.flows.1.pre.bias", P(t), shape, 1, L.F32) == 0
    assert m._lib.bv2_sdp_forward_detach(m._handle) == 0


def test_stripped_checkpoint_and_calls_without_the_blob_raise_with_the_hint(tmp_path):
    hp = narrow_hp()
    m = _model(hp)
    stripped = synth.synthetic_state_dict(hp, 0)                                 # what compress_model.py leaves: no sdp.post_*
    with pytest.raises(ValueError, match="compress_model.py"):
        m.load_sdp_forward(stripped)
    path = tmp_path / "G_0.pth"
    torch.save({"model": stripped, "iteration": 0, "optimizer": None, "learning_rate": 1e-4}, path)
    with pytest.raises(ValueError, match="compress_model.py"):
        m.load_sdp_forward(str(path))
    assert not m.has_sdp_forward
    enc = dict(x=torch.zeros(1, hp.hidden_channels, 4), x_mask=torch.ones(1, 4), g=torch.zeros(1, hp.gin_channels))
    with pytest.raises(RuntimeError, match=r"load_sdp_forward\(checkpoint\).*compress_model.py"):
        m.duration_nll(enc, torch.ones(1, 4))


def test_duration_nll_checks_every_argument_before_the_device():
    m = _model(narrow_hp())
    lib = m._ensure_handle()
    one = C.c_void_p(8)
    n = lib.bv2_duration_nll_workspace_bytes(m._handle, 2, 18)
    assert n > 0 and lib.bv2_duration_nll_workspace_bytes(m._handle, 2, 36) > n
    for B, T in ((0, 18), (2, 0), (70000, 18)):
        assert lib.bv2_duration_nll_workspace_bytes(m._handle, B, T) < 0
    ok = dict(B=2, T=18, x=one, x_mask=one, w=one, g=one, noise_e=one, nll_sym=one, nll=one, ws=one, wsb=n)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.bv2_duration_nll(m._handle, None, a["B"], a["T"], a["x"], a["x_mask"], a["w"], a["g"], a["noise_e"], a["nll_sym"],
                                    a["nll"], a["ws"], a["wsb"])

    for kw in (dict(B=0), dict(T=0), dict(B=65536), dict(x=None), dict(x_mask=None), dict(w=None), dict(g=None), dict(nll_sym=None),
               dict(nll=None)):
        assert call(**kw) == -1 and b"bv2_duration_nll" in lib.bv2_last_error(m._handle), kw
    assert call(ws=None) == -5 and b"workspace" in lib.bv2_last_error(m._handle)
    assert call(wsb=n - 1) == -5 and b"workspace too small" in lib.bv2_last_error(m._handle)
    # well-formed, but nothing is attached: named, and still nothing touched the device
    assert call() == -8 and b"attached" in lib.bv2_last_error(m._handle)
    assert lib.bv2_duration_nll(None, None, 2, 18, one, one, one, one, one, one, one, one, n) == -1


def test_kl_path_checks_every_argument_before_the_device():
    lib = L.load()
    one = C.c_void_p(8)
    ok = dict(B=2, D=128, T=18, Ty=52, z_p=one, logs_q=one, m_p=one, logs_p=one, w=one, kl_frame=one, kl=one)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.bv2_kl_path(None, a["B"], a["D"], a["T"], a["Ty"], a["z_p"], a["logs_q"], a["m_p"], a["logs_p"], a["w"], None, None,
                               a["kl_frame"], a["kl"])

    for kw, word in ((dict(B=0), b"B"), (dict(B=65536), b"B"), (dict(D=0), b"inter"), (dict(T=0), b"T"), (dict(T=4097), b"T"),
                     (dict(Ty=0), b"Ty"), (dict(D=65535, Ty=1 << 20), b"2^31"), (dict(z_p=None), b"null"), (dict(logs_q=None), b"null"),
                     (dict(m_p=None), b"null"), (dict(logs_p=None), b"null"), (dict(w=None), b"null"), (dict(kl_frame=None), b"null"),
                     (dict(kl=None), b"null")):
        assert call(**kw) == -1, kw
        msg = lib.bv2_last_error(None)
        assert msg.startswith(b"bv2_kl_path") and word in msg, (kw, msg)


def test_the_seeded_e_q_draw_is_a_fourth_draw_and_the_first_three_did_not_move():
    lib = L.load()
    lib.bv2_test_seeded_normal.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int]
    lib.bv2_test_seeded_normal.restype = C.c_float
    rows, ts = [0, 1], [0, 1, 17, 255, 4096]
    for seed in (0, 1, -1, 2 ** 63 - 1):
        draw = {w: np.array([[lib.bv2_test_seeded_normal(seed, w, r, t) for t in ts] for r in rows]) for w in range(4)}
        for w in range(4):                                                        # 0-2 as pinned; 3 is the same generator at which = 3
            ref = R.seeded_normal(seed, w, np.array(rows)[:, None], np.array(ts)[None, :])
            assert np.abs(draw[w] - ref).max() <= 4e-6, (seed, w)
        for w in range(3):
            assert np.abs(draw[3] - draw[w]).min() > 0, (seed, w)                 # no value of the new draw repeats one of the old
    # bv2_seeded_noise keeps offering the three tensor draws only
    assert lib.bv2_seeded_noise(None, C.c_void_p(8), 1, 3, 2, 4, None, C.c_void_p(8), 8, 4, 1) == -1
