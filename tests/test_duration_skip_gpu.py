"""GPU: phase A runs only the duration predictor the mix can see (include/bv2.h, ``bv2_encode_out``).

``logw = logw_sdp * r + logw_dp * (1 - r)``: at a host-known ``sdp_ratio`` of exactly 0 the StochasticDurationPredictor's launches (and
at exactly 1 the DurationPredictor's) compute a value that is multiplied by 0.0f.  The lean request (``encode_durations(lean=True)``,
what ``infer`` asks for) leaves them out; everything the request does return is what the full request returns."""
import pytest
import torch

from oracle import cases
from tests.helpers import cached_state_dict

pytestmark = pytest.mark.gpu

NAMES = ["zh_b1_t24", "mix_b2_ragged", "short_b3"]
SHARED = ("g", "x", "m_p", "logs_p", "x_mask", "w_ceil", "y_lengths")      # torch.equal between the two forms; logw: equal by value
ARGS = ("x", "x_lengths", "sid", "tone", "language", "bert", "ja_bert", "en_bert")

_MODELS = {}


def _model(name):
    """One model per case for the whole module (same default hyper-parameters: one checkpoint), with every switch at its default."""
    from bert_vits2_amd import models
    hp, seed, batch, nw, nz, kw = cases.build_case(name)
    if "m" not in _MODELS:
        m = models.from_hparams(hp)
        m.load_state_dict(cached_state_dict(hp, seed), strict=False)
        _MODELS["m"] = m.to("cuda").eval()
    m = _MODELS["m"]
    m.enable_graphs(False)
    m.set_tap(None)
    m.set_option("lean_durations", 1)
    return m, [batch[k].cuda() for k in ARGS], nw, nz, kw


def _encode(m, args, nw, kw, ratio, **extra):
    out = m.encode_durations(*args, nw, noise_scale_w=kw["noise_scale_w"], sdp_ratio=ratio, length_scale=kw["length_scale"], **extra)
    torch.cuda.synchronize()
    return out


def _poison_workspace(m, B, T):
    """Phase A's workspace full of NaN: a skipped predictor's buffers (the SDP's z, logw_dp) hold it when the durations kernel runs."""
    ws = m._workspace(B, T, 1)
    ws[: ws.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
    torch.cuda.synchronize()


def _nodes(m, args, nw, kw, ratio, **extra):
    """Kernel nodes of the captured phase-A graph of this request."""
    m.enable_graphs(True)
    out = _encode(m, args, nw, kw, ratio, **extra)
    ent = [e for k, e in m._graphs.items() if k[0] == "A"]
    assert len(ent) == 1
    n = m._lib.bv2_graph_num_nodes(ent[0]["graph"])
    m.enable_graphs(False)
    return n, {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("ratio", [0.0, 1.0])
@pytest.mark.parametrize("name", NAMES)
def test_lean_equals_full_and_the_skipped_side_is_not_read(name, ratio):
    m, args, nw, nz, kw = _model(name)
    B, T = args[0].shape
    full = _encode(m, args, nw, kw, ratio)
    assert set(full) == set(SHARED) | {"logw", "logw_sdp", "logw_dp"}
    # ratio 0: the stochastic predictor's input is never read — NaN in its place (on the host: it is not uploaded either), NaN in the
    # workspace where its state would be.  ratio 1: the workspace's logw_dp holds NaN in the same way.
    nw_in = torch.full_like(nw, float("nan")) if ratio == 0.0 else nw
    _poison_workspace(m, B, T)
    lean = _encode(m, args, nw_in, kw, ratio, lean=True)
    seen, unseen = ("logw_dp", "logw_sdp") if ratio == 0.0 else ("logw_sdp", "logw_dp")
    assert set(lean) == set(SHARED) | {"logw", seen}
    for k in SHARED + (seen,):
        assert torch.equal(lean[k], full[k]), k
    assert torch.isfinite(lean["logw"]).all()
    assert bool((lean["logw"] == full["logw"]).all())                  # by value: a zero may differ in sign
    assert torch.equal(lean["logw"], full["logw_dp" if ratio == 0.0 else "logw_sdp"])
    # infer() asks for the lean form: its audio is decode() of the full encode
    kw_i = dict(kw, sdp_ratio=ratio)
    _poison_workspace(m, B, T)
    o = m.infer(*args, noise_w=nw_in, noise_z=nz.cuda(), **kw_i)[0]
    assert set(m.last_encode) == set(SHARED) | {"logw", seen}
    if ratio == 1.0:        # a reader of last_encode still gets the skipped predictor's output: computed on first access (stage_dp)
        assert torch.equal(m.last_encode[unseen], full[unseen])
    Ty = int(full["y_lengths"].max().item())
    dec = m.decode(full, nz.cuda(), Ty, noise_scale=kw["noise_scale"])
    torch.cuda.synchronize()
    assert torch.equal(o, dec["o"])


@pytest.mark.parametrize("name", NAMES)
def test_both_predictors_run_when_the_mix_sees_both(name):
    m, args, nw, nz, kw = _model(name)
    B, T = args[0].shape
    full = _encode(m, args, nw, kw, 0.5)
    lean = _encode(m, args, nw, kw, 0.5, lean=True)
    assert set(lean) == set(full)
    for k in full:
        assert torch.equal(lean[k], full[k]), k                        # nothing is skipped: bit for bit
    # per-utterance ratios live on the device: the host cannot see that they are all zero, so both predictors run (the same launch
    # count as a mixed request) and the result is the scalar-0 one
    scalar0 = _encode(m, args, nw, kw, 0.0, lean=True)
    n_full, _ = _nodes(m, args, nw, kw, 0.5)
    n_item, item0 = _nodes(m, args, nw, kw, torch.zeros(B), lean=True)
    assert n_item == n_full
    for k in SHARED + ("logw",):
        assert torch.equal(item0[k], scalar0[k]), k


def test_a_tap_keeps_the_stochastic_predictor():
    m, args, nw, nz, kw = _model("mix_b2_ragged")
    B, T = args[0].shape
    full = _encode(m, args, nw, kw, 0.0)
    taps = {"sdp.x": torch.zeros(B, m.hp.hidden_channels, T, device="cuda"), "sdp.z.2": torch.zeros(B, 2, T, device="cuda")}
    for k, t in taps.items():
        m.set_tap(k, t)
    lean = _encode(m, args, nw, kw, 0.0, lean=True)
    m.set_tap(None)
    assert all(float(t.abs().sum()) > 0 for t in taps.values())         # the tapped intermediates were produced
    for k in SHARED + ("logw",):
        assert torch.equal(lean[k], full[k]), k


def test_graph_node_counts_and_the_option_switch():
    m, args, nw, nz, kw = _model("zh_b1_t24")
    count = {}
    for ratio in (0.0, 0.5, 1.0):
        for lean in (False, True):
            count[ratio, lean], out = _nodes(m, args, nw, kw, ratio, lean=lean)
            if lean:
                ref = _encode(m, args, nw, kw, ratio)
                for k in SHARED:
                    assert torch.equal(out[k], ref[k]), (ratio, k)     # the replayed lean graph gives the eager full result
    assert count[0.0, False] == count[0.5, False] == count[1.0, False]
    assert count[0.0, True] < count[0.0, False]
    assert count[1.0, True] < count[1.0, False]
    assert count[0.5, True] == count[0.5, False]
    assert count[0.0, True] < count[1.0, True]                          # the stochastic predictor is the longer chain
    # "lean_durations" = 0: the full launch sequence again, for every request
    m.set_option("lean_durations", 0)
    try:
        for ratio in (0.0, 1.0):
            n, out = _nodes(m, args, nw, kw, ratio, lean=True)
            assert n == count[ratio, False]
            ref = _encode(m, args, nw, kw, ratio)
            for k in SHARED + ("logw",):
                assert torch.equal(out[k], ref[k]), (ratio, k)
    finally:
        m.set_option("lean_durations", 1)


def test_null_noise_is_refused_when_it_would_be_read():
    """noise_w may be NULL exactly when the rule says it is not read: a mixed request without it is an argument error, not a fault."""
    import ctypes as C
    from bert_vits2_amd import lib as L
    from bert_vits2_amd.models import _ptr
    m, args, nw, nz, kw = _model("zh_b1_t24")
    B, T = args[0].shape
    out = _encode(m, args, nw, kw, 0.5)
    okeys = ("g", "x", "m_p", "logs_p", "x_mask", "logw_sdp", "logw_dp", "logw", "w_ceil", "y_lengths")
    ws = m._workspace(B, T, 1)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(ratio, keys):
        ein = L.EncodeIn(B, T, *[_ptr(a) for a in args], None, float(kw["noise_scale_w"]), float(ratio), float(kw["length_scale"]))
        eout = L.EncodeOut(*[_ptr(out[k]) if k in keys else None for k in okeys])
        rc = m._lib.bv2_encode_durations(m._handle, stream, C.byref(ein), C.byref(eout), C.c_void_p(ws.data_ptr()), ws.numel())
        torch.cuda.synchronize()
        return rc
    lean_keys = [k for k in okeys if k not in ("logw_sdp", "logw_dp")]
    assert call(0.5, lean_keys) == -1                                    # both run
    assert call(0.0, okeys) == -1                                        # logw_sdp is asked for
    assert call(0.0, lean_keys) == 0
