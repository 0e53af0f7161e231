"""GPU: the head of phase B as ONE launch (``phase_b_front``: length regulation, prior sampling, attn path, the speaker GEMVs and the
fp32 Generator's x3 slot words) gives bit for bit what the five launches it replaces give (``set_option("phase_b_front", 0)``)."""
import pytest
import torch

from bert_vits2_amd import hparams as H, synth
from tests.helpers import cached_state_dict

pytestmark = pytest.mark.gpu

KW = dict(noise_scale_w=0.9, sdp_ratio=0.5, length_scale=1.0)
_STATE = {}


def _model():
    from bert_vits2_amd import models
    if "m" not in _STATE:
        hp = H.default_v23()
        m = models.from_hparams(hp)
        m.load_state_dict(cached_state_dict(hp, 0), strict=False)
        _STATE["m"] = m.to("cuda").eval()
    m = _STATE["m"]
    m.enable_graphs(False)
    m.set_generator_dtype(torch.float32)
    m.set_option("phase_b_front", 1)
    return m


def _encoded(m, lengths, durations):
    """Phase A of a synthetic batch (cached), with the durations replaced as ``infer(w_ceil=...)`` does: a fixed pseudo-random pattern of
    0 .. 3 frames per symbol (symbols without a frame included) when ``durations`` is None, else that many frames for every symbol."""
    key = (tuple(lengths), durations)
    if key not in _STATE:
        B, T = len(lengths), max(lengths)
        batch = synth.synthetic_batch(lengths, [i % 3 for i in range(B)], [3 + 7 * i for i in range(B)])
        nw, nz = synth.synthetic_noise(B, T, 3 * T + 8, m.hp.inter_channels)
        enc = m.encode_durations(*[batch[k].cuda() for k in ("x", "x_lengths", "sid", "tone", "language", "bert", "ja_bert", "en_bert")],
                                 nw, **KW)
        g = torch.Generator().manual_seed(5)
        wc = torch.randint(0, 4, (B, T), generator=g).float() if durations is None else torch.full((B, T), float(durations))
        wc = (wc.cuda() * enc["x_mask"]).contiguous()
        enc["w_ceil"] = wc
        enc["y_lengths"] = torch.clamp_min(wc.sum(1), 1).long()
        _STATE[key] = (enc, nz.cuda())
    return _STATE[key]


def _both(m, run):
    """run() with the fused head and with the five launches; outputs cloned."""
    res = []
    for v in (1, 0):
        m.set_option("phase_b_front", v)
        out = run()
        torch.cuda.synchronize()
        res.append({k: (None if t is None else t.clone()) for k, t in out.items()})
    m.set_option("phase_b_front", 1)
    return res


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), k
            assert torch.isfinite(a[k]).all(), k


# lengths, durations, decode kwargs.  Frames: T = 5 -> a handful; ragged B = 3 with one-symbol and zero-frame items; T = 300 crosses the
# 256-symbol scan chunk, with T_y ~ 450 (random) and exactly 600 (2 per symbol): more than one 256-frame chunk, not a multiple of 256.
CASES = {
    "b1_t5": ([5], None, {}),
    "b3_ragged": ([3, 9, 1], None, {}),
    "b3_ragged_noattn": ([3, 9, 1], None, dict(want_attn=False)),
    "t300": ([300], None, dict(max_len=40)),
    "t300_b2_two_per_symbol": ([300, 257], 2, dict(max_len=24)),
    "t300_noattn": ([300], None, dict(max_len=40, want_attn=False)),
    "bucket_exact2": ([20, 13], None, dict(ty_bucket=128)),            # exact_lengths = 2: the bucket is longer than every utterance
    "bucket_exact1": ([20, 13], None, dict(ty_bucket=128, exact_lengths=True)),
    "item_noise_scale": ([20, 13, 7], None, dict(noise_scale=torch.tensor([0.3, 0.667, 1.1]))),
}


@pytest.mark.parametrize("gen", ["fp32", "bf16"])                      # fp32: the launch also zeroes the x3 slot words; bf16: it has none
@pytest.mark.parametrize("strides", ["reference", "contiguous"])
@pytest.mark.parametrize("case", list(CASES))
def test_fused_head_equals_the_five_launches(case, strides, gen):
    lengths, durations, kw = CASES[case]
    m = _model()
    enc, nz = _encoded(m, lengths, durations)
    if gen == "bf16":
        m.set_generator_dtype(torch.bfloat16)
    Ty = int(enc["y_lengths"].max().item())
    if case.startswith("t300"):
        assert Ty > 256 and Ty % 256 != 0 and enc["x"].shape[2] > 256
    if strides == "reference":                                          # randn_like(m_p) of a transposed view: strides (C*Ty, 1, C)
        nz = nz[:, :, :Ty].transpose(1, 2).contiguous().transpose(1, 2)
        assert nz.stride(1) == 1
    kw = dict(dict(noise_scale=0.6), **kw)
    fused, old = _both(m, lambda: m.decode(enc, nz, Ty, **kw))
    _same(fused, old)
    # twice in a row: nothing the launch leaves behind (the slot words) leaks into the next decode
    again = m.decode(enc, nz, Ty, **kw)
    torch.cuda.synchronize()
    assert torch.equal(again["o"], old["o"])
    assert int(fused["y_mask"].sum().item()) == int(enc["y_lengths"].sum().item())
    if fused["attn"] is not None:                                       # a frame belongs to at most one symbol, and only a valid frame does
        assert bool((fused["attn"].sum(-1)[:, 0] <= fused["y_mask"][:, 0]).all())


def test_graph_replay_of_the_fused_head():
    m = _model()
    enc, nz = _encoded(m, [20, 13], None)
    Ty = int(enc["y_lengths"].max().item())
    eager = m.decode(enc, nz, Ty, noise_scale=0.6)
    n = {}
    for v in (1, 0):
        m.set_option("phase_b_front", v)
        m.enable_graphs(True, ty_bucket=1)
        for _ in range(3):                                              # capture, then replays on the state the last one left
            out = m.decode(enc, nz, Ty, noise_scale=0.6)
            torch.cuda.synchronize()
            _same(out, eager)
        n[v] = [m._lib.bv2_graph_num_nodes(e["graph"]) for k, e in m._graphs.items() if k[0] == "B"][0]
        m.enable_graphs(False)
    m.set_option("phase_b_front", 1)
    assert n[1] == n[0] - 4                                             # five launches became one


def test_stage_flow_and_stream_are_unchanged():
    m = _model()
    enc, nz = _encoded(m, [20, 13], None)
    Ty = int(enc["y_lengths"].max().item())
    dec = m.decode(enc, nz, Ty, noise_scale=0.6)
    flow = _both(m, lambda: dict(z=m.stage_flow(dec["z_p"], enc["y_lengths"], enc["g"])))
    _same(*flow)
    batch = synth.synthetic_batch([20, 13], [0, 1], [3, 10])
    args = [batch[k].cuda() for k in ("x", "x_lengths", "sid", "tone", "language", "bert", "ja_bert", "en_bert")]
    nw, nzs = synth.synthetic_noise(2, 20, 1024, m.hp.inter_channels)

    def stream():
        st = m.infer_stream(*args, noise_w=nw, noise_z=nzs.cuda(), noise_scale=0.6, chunk_frames=16, **KW)
        audio = torch.cat([a for _, a in st], dim=1)
        return dict(audio=audio, **{k: v for k, v in st.aux.items()})
    s_fused, s_old = _both(m, stream)
    _same(s_fused, s_old)
