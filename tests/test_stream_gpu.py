"""GPU: streamed synthesis — the flow once, the Generator window by window (bv2_stream_begin / bv2_stream_chunk, kernels/stream.hip).
The chunks of ``infer_stream`` concatenated are the audio of ``infer`` of the same call; ``bv2_emit`` alone is bit-exact against numpy;
``serving.synthesize_stream`` hands every utterance its own pieces in order.

The two bars (relative RMS <= 1e-5 in fp32, <= 2e-2 with the bf16 Generator + fp16 flow) are those tests/test_serving_gpu.py holds "the same
audio from another batch shape" to, for the same reasons: a window is another tiling of the same convolutions, and the two-plane fp16 convs
take their activation scale from the max |x| of another tensor."""
import ctypes as C

import numpy as np
import pytest
import torch

from bert_vits2_amd import hparams as H, lib as L, serving, synth
from oracle import cases
from tests.helpers import cached_state_dict

pytestmark = pytest.mark.gpu

KW = dict(sdp_ratio=0.5, noise_scale=0.6, noise_scale_w=0.9, length_scale=1.0)
_MODELS = {}


def _model(name="default"):
    """One model per config for the whole module (packing the weights is most of a test's time)."""
    if name not in _MODELS:
        from bert_vits2_amd import models
        hp = H.default_v23() if name == "default" else H.default_v23(**cases.ENVELOPE[name]["hp"])
        m = models.from_hparams(hp)
        m.load_state_dict(cached_state_dict(hp, 0), strict=False)
        _MODELS[name] = m.to("cuda").eval()
    m = _MODELS[name]
    if m.generator_dtype != torch.float32:
        m.set_generator_dtype(torch.float32)
    if m.flow_dtype != torch.float32:
        m.set_flow_dtype(torch.float32)
    return m


def _inputs(hp, lengths):
    b = synth.synthetic_batch(lengths, languages=[i % 3 for i in range(len(lengths))], sids=[3 + 5 * i for i in range(len(lengths))])
    nw, nz = synth.synthetic_noise(len(lengths), max(lengths), 16 * max(lengths), hp.inter_channels)
    args = [b[k].cuda() for k in ("x", "x_lengths", "sid", "tone", "language", "bert", "ja_bert", "en_bert")]
    return args, dict(noise_w=nw.cuda(), noise_z=nz.cuda())


def _rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-3))


def _stream_vs_whole(m, lengths, tol, exact, chunk, first=None, expect_ragged_cases=False):
    hp = m.hp
    U = hp.total_upsample
    args, noise = _inputs(hp, lengths)
    o, attn, y_mask, (z, z_p, m_p, logs_p) = m.infer(*args, exact_lengths=exact, **noise, **KW)
    st = m.infer_stream(*args, exact_lengths=exact, chunk_frames=chunk, first_chunk_frames=first, **noise, **KW)
    assert st.halo == H.generator_halo(hp) and st.Ty == o.shape[2] // U and st.total_samples == o.shape[2]
    y_len = [int(v) for v in st.y_lengths.cpu()]
    assert y_len == st.y_lengths_host and max(y_len) == st.Ty
    # the secondary outputs are those of infer, bit for bit (the same launches in the same order)
    for k, ref in (("attn", attn), ("y_mask", y_mask), ("z", z), ("z_p", z_p), ("m_p", m_p), ("logs_p", logs_p)):
        assert torch.equal(st.aux[k], ref), k
    chunks = list(st)
    # the chunks tile [0, Ty * U) exactly and in order
    want, t = [], 0
    while t < st.Ty:
        t1 = min(st.Ty, t + ((first or chunk) if t == 0 else chunk))
        want.append((t * U, (t1 - t) * U))
        t = t1
    assert [(start, a.shape[1]) for start, a in chunks] == want and len(st) == len(want)
    assert all(a.shape[0] == len(lengths) and a.dtype == torch.float32 for _, a in chunks)
    if expect_ragged_cases:
        Hh = st.halo
        starts = [s // U for s, _ in chunks]
        assert len(chunks) >= 4 and (chunks[-1][1].shape[1] // U) < chunk                # interior windows and a last short chunk
        assert any(t0 < n < t0 + chunk for n in y_len for t0 in starts[1:])                # an item ends inside a window
        assert any(n <= starts[-1] - Hh for n in y_len)                                    # an item finished before a window began (runs as one masked frame)
    cat = torch.cat([a for _, a in chunks], dim=1).cpu().numpy()
    whole = o[:, 0].cpu().numpy()
    for b, n in enumerate(y_len):
        r = _rel_rms(cat[b, :n * U], whole[b, :n * U])
        print(f"item {b} ({n} frames of {st.Ty}): relative RMS stream vs whole = {r:.3e}, bit-identical = {np.array_equal(cat[b, :n * U], whole[b, :n * U])}")
        assert r <= tol, (b, r)
        assert not cat[b, n * U:].any()                  # exactly zero past the item's end
    return cat, y_len


@pytest.mark.parametrize("mode", ["fp32", "bf16+f16"])
def test_chunks_equal_the_whole_decode(mode):
    m = _model()
    if mode != "fp32":
        m.set_generator_dtype(torch.bfloat16)
        m.set_flow_dtype(torch.float16)
    _stream_vs_whole(m, [24, 9, 17], 1e-5 if mode == "fp32" else 2e-2, True, 8, 5, expect_ragged_cases=True)


@pytest.mark.parametrize("name,lengths,exact,chunk", [("hp04_tf5_h192x6", [11, 5, 3], True, 3), ("hp10_wn2_h128x4_rb2", [5, 10], True, 4),
                                                      ("hp01_tf3_h128x4", [9], False, 5)])
def test_other_models(name, lengths, exact, chunk):
    """Odd rates (5 * 5 * 4 = 100 samples per frame, halo 26), ResBlock2 (halo 7), and the unmasked Generator at batch 1."""
    _stream_vs_whole(_model(name), lengths, 1e-5, exact, chunk)


def _emit(src, src_bstride, src_off, y_len, hop, start, B, n, dst, dst_off, dst_bstride, gain):
    lib = L.load()
    yl = None if y_len is None else torch.tensor(y_len, dtype=torch.int64, device="cuda")
    p = dst.data_ptr() + dst_off * dst.element_size()
    is16 = dst.dtype == torch.int16
    rc = lib.bv2_emit(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(src.data_ptr()), src_bstride, src_off,
                      None if yl is None else C.c_void_p(yl.data_ptr()), hop, start, B, n, None if is16 else C.c_void_p(p),
                      C.c_void_p(p) if is16 else None, dst_bstride, gain)
    assert rc == 0, lib.bv2_last_error(None)
    torch.cuda.synchronize()


@pytest.mark.parametrize("src_off", [1, 7])
@pytest.mark.parametrize("dst_off", [1, 3])
def test_emit_alone_bit_exact_against_numpy(src_off, dst_off):
    """bv2_emit with every alignment of source offset and destination: odd hop (125), the mask ending inside / before the chunk, and
    values at +-1.0 where the PCM clamp and the truncation meet."""
    B, hop, n, start = 3, 125, 3 * 125, 125
    y_len = [3, 1, 0]                                    # valid samples from `start`: 250 (inside the chunk), 0, 0 (negative before the clamp)
    src_bstride = n + 16
    g = torch.Generator().manual_seed(src_off * 10 + dst_off)
    src = torch.rand(B, src_bstride, generator=g) * 2.2 - 1.1
    src[0, src_off + 3], src[0, src_off + 4], src[0, src_off + 5], src[0, src_off + 6] = 1.0, -1.0, 0.99999, -0.99999
    src[1] = float("nan")                                # a finished item's window output is stale memory: never used
    src = src.cuda()
    x = src.cpu().numpy()[:, src_off:src_off + n]
    valid = [max(0, min(n, y * hop - start)) for y in y_len]
    dst_bstride = n + 24
    for gain in (None, 32767.0, 12000.0):
        is16 = gain is not None
        dst = torch.full((B * dst_bstride + 8,), 77, dtype=torch.int16 if is16 else torch.float32, device="cuda")
        _emit(src, src_bstride, src_off, y_len, hop, start, B, n, dst, dst_off, dst_bstride, gain or 0.0)
        got = dst.cpu().numpy()
        for b in range(B):
            row = got[dst_off + b * dst_bstride:dst_off + b * dst_bstride + n]
            if is16:
                ref = np.clip(x[b] * np.float32(gain), np.float32(-32768), np.float32(32767))
                ref = np.where(np.arange(n) < valid[b], np.nan_to_num(ref), 0).astype(np.int16)       # astype truncates toward zero
            else:
                ref = np.where(np.arange(n) < valid[b], x[b], np.float32(0)).astype(np.float32)
            assert np.array_equal(row, ref), (gain, b, int(np.flatnonzero(row != ref)[0]))
            # nothing outside [0, n) of the item's row is written
            gap = got[dst_off + b * dst_bstride + n:dst_off + (b + 1) * dst_bstride] if b + 1 < B else got[dst_off + b * dst_bstride + n:]
            assert (gap == 77).all() and (got[:dst_off] == 77).all()
    # no lengths: nothing is masked
    dst = torch.zeros(B * dst_bstride + 8, dtype=torch.float32, device="cuda")
    _emit(src, src_bstride, src_off, None, hop, start, B, n, dst, dst_off, dst_bstride, 0.0)
    assert np.array_equal(dst.cpu().numpy()[dst_off:dst_off + n], x[0])


def test_pcm_stream_is_the_truncated_fp32_stream():
    m = _model()
    args, noise = _inputs(m.hp, [12, 7])
    kw = dict(exact_lengths=True, chunk_frames=16, first_chunk_frames=6, **noise, **KW)
    f32 = list(m.infer_stream(*args, **kw))
    pcm = list(m.infer_stream(*args, as_pcm16=True, **kw))
    quiet = list(m.infer_stream(*args, as_pcm16=True, pcm_gain=12000.0, **kw))
    assert len(f32) == len(pcm) == len(quiet) >= 2
    for (s0, a), (s1, p), (s2, q) in zip(f32, pcm, quiet):
        assert s0 == s1 == s2 and p.dtype == torch.int16 and p.shape == a.shape
        x = a.cpu().numpy()
        assert np.array_equal(p.cpu().numpy(), np.clip(x * np.float32(32767), -32768, 32767).astype(np.int16))
        assert np.array_equal(q.cpu().numpy(), (x * np.float32(12000)).astype(np.int16))
    assert max(int(p.abs().max()) for _, p in pcm) > 1000


def _utts(lengths):
    out = []
    for i, T in enumerate(lengths):
        b = synth.synthetic_batch([T], languages=[i % 3], sids=[i * 7 % 50], first_index=i)
        out.append(serving.Utterance(b["x"][0], b["tone"][0], b["language"][0], b["bert"][0], b["ja_bert"][0], b["en_bert"][0],
                                     int(b["sid"][0])))
    return out


@pytest.mark.parametrize("mode", ["fp32", "bf16+f16"])
def test_synthesize_stream_hands_every_utterance_its_pieces_in_order(mode):
    m = _model()
    if mode != "fp32":
        m.set_generator_dtype(torch.bfloat16)
        m.set_flow_dtype(torch.float16)
    lengths = [17, 24, 9, 22, 40, 20]
    utts = _utts(lengths)
    g = torch.Generator().manual_seed(5)
    noise = [(torch.randn(2, T, generator=g), torch.randn(m.hp.inter_channels, 16 * T, generator=g)) for T in lengths]
    kw = dict(noise=noise, max_batch=4, max_pad_ratio=1.5, **KW)
    whole = serving.synthesize(m, utts, **kw)
    got = [[] for _ in utts]
    for i, start, piece in serving.synthesize_stream(m, utts, chunk_frames=16, **kw):
        assert piece.dtype == np.float32 and piece.ndim == 1 and piece.size > 0
        assert start == sum(p.size for p in got[i])                  # in order, contiguous offsets
        got[i].append(piece)
    tol = 1e-5 if mode == "fp32" else 2e-2
    for i, ref in enumerate(whole):
        cat = np.concatenate(got[i])
        assert cat.shape == ref.shape and len(got[i]) == -(-ref.size // (16 * m.hp.total_upsample))   # nothing past its own length
        r = _rel_rms(cat, ref)
        print(f"utterance {i}: {len(got[i])} pieces, relative RMS vs synthesize = {r:.3e}")
        assert r <= tol, (i, r)
    if mode == "fp32":
        pcm = list(serving.synthesize_stream(m, utts[:2], chunk_frames=16, first_chunk_frames=4, as_pcm16=True, **dict(kw, noise=noise[:2])))
        assert pcm and all(p.dtype == np.int16 for _, _, p in pcm)
        assert sum(p.size for i, _, p in pcm if i == 0) == whole[0].size


def test_infer_stream_refuses_graphs_and_taps():
    m = _model()
    args, noise = _inputs(m.hp, [6])
    m.enable_graphs(True)
    try:
        with pytest.raises(RuntimeError, match="graph"):
            m.infer_stream(*args, **noise, **KW)
    finally:
        m.enable_graphs(False)
    tap = torch.zeros(16, device="cuda")
    m.set_tap("dec.pre", tap)
    try:
        with pytest.raises(RuntimeError, match="tap"):
            m.infer_stream(*args, **noise, **KW)
    finally:
        m.set_tap(None)
    with pytest.raises(ValueError):
        m.infer_stream(*args, chunk_frames=0, **noise, **KW)
