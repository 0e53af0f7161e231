"""GPU: from a waveform to the ReferenceEncoder's spectrogram and on to g (kernels/stft.hip, bv2_spectrogram, audio.spectrogram).

 * linear and mel spectrograms against the REAL reference's mel_processing (tests/golden/stft_n2048.npz, stft_n1024.npz):
   max|spec_gpu - ref_fp64| <= 4 * ref_err per case, ref_err the reference's own fp32 error against its fp64 evaluation.  4 is twice the worst
   ratio a plain radix-2 fp32 FFT showed on the CPU over these shapes (0.99-1.99 linear, 0.45-1.51 mel): a proxy for a kernel of another
   radix and order, so the ratios are printed and recorded in docs/MEASUREMENTS.md.
 * g from a waveform (tests/golden/stft_ref_enc_wav_g.npz): max|g_gpu - g_fp64| <= 4 * ref_err of the reference's waveform -> spectrogram ->
   ReferenceEncoder chain, the rule of tests/test_ref_enc_gpu.py.
 * everything else is exact (torch.equal): a ragged batch equals each waveform alone, garbage or NaN in the padding changes no bit, int16
   equals fp32 of x / 32768, a strided batch equals the contiguous one, a side stream equals the default stream,
   reference_embedding_from_wav is spectrogram + reference_embedding, and serving shares one encoding between utterances that share a
   reference_spectrogram.
"""
import numpy as np
import pytest
import torch

from bert_vits2_amd import audio, hparams as H, models, serving, synth
from oracle import cases
from tests.helpers import cached_state_dict, load_golden

pytestmark = pytest.mark.gpu

CASE = cases.CASES["narrow_b2_t18"]
RAGGED = [769, 12345, 5000, 2100]

_MODELS = {}


def ref_model(spec=1025):
    """The narrow model of tests/test_ref_enc_gpu.py, without a speaker table."""
    if spec not in _MODELS:
        hp = H.default_v23(**dict(CASE["hp"], n_speakers=0, spec_channels=spec))
        m = models.from_hparams(hp)
        m.load_state_dict(cached_state_dict(hp, CASE["seed"]), strict=False)
        _MODELS[spec] = m.to("cuda").eval()
    return _MODELS[spec]


def _ragged_batch(lens, fill=0):
    wavs = [synth.synthetic_reference_wav(n, i) for i, n in enumerate(lens)]
    w = torch.full((len(lens), max(lens)), fill, dtype=torch.int16)
    for i, x in enumerate(wavs):
        w[i, :lens[i]] = x
    return wavs, w


@pytest.mark.parametrize("fixture", ["stft_n2048", "stft_n1024"])
def test_spectrogram_matches_the_reference_within_four_times_its_own_fp32_error(fixture):
    """Measured on MI355X (docs/MEASUREMENTS.md, Spectrogram): the largest ratio max|spec_gpu - ref_fp64| / ref_err is 2.47 over the six linear
    cases (2.47 at n_fft 2048 — the one-frame case, one ulp of its peak — and 1.65 at 1024) and 1.34 over the six mel cases (1.34 at 2048, 0.94 at
    1024); the bar is 4."""
    meta, gold = load_golden(fixture)
    worst, bad = {}, []
    for name, c in sorted(meta["cases"].items()):
        p = audio.StftParams(meta["n_fft"], meta["hop"], meta["win"], c["n_mels"], meta["sampling_rate"], meta["fmin"], meta["fmax"])
        spec, n = audio.spectrogram(gold[f"wav_s{c['S']}"], params=p)
        want = gold[name + "_spec64"]
        assert spec.shape == (1,) + tuple(want.shape) and n.tolist() == [c["frames"]] and torch.isfinite(spec).all()
        err = float((spec[0].cpu().double() - want).abs().max())
        ratio = err / c["ref_err"]
        kind = "mel" if c["n_mels"] else "lin"
        worst[kind] = max(worst.get(kind, 0.0), ratio)
        print(f"[{fixture} {name}] max|spec_gpu - ref_fp64| = {err:.3e}  ref_err = {c['ref_err']:.3e}  ratio = {ratio:.2f}  peak = {c['peak']:.1f}")
        if err > 4 * c["ref_err"]:
            bad.append((name, err, c["ref_err"], ratio))
    print(f"[{fixture}] largest ratio: linear {worst['lin']:.2f}  mel {worst['mel']:.2f}")
    assert not bad, bad


def test_g_from_a_waveform_matches_the_reference_chain_within_four_times_its_own_fp32_error():
    """Measured on MI355X (docs/MEASUREMENTS.md, Spectrogram): ratios max|g_gpu - g_fp64| / ref_err of 0.68 (1025), 0.72 (513) and 0.71 (80):
    the ReferenceEncoder does not amplify the spectrogram's error beyond the reference's own; the bar is 4."""
    meta, gold = load_golden("stft_ref_enc_wav_g")
    bad = []
    for name, c in sorted(meta["cases"].items()):
        m = ref_model(c["spec_channels"])
        assert m.stft_params == audio.StftParams(**c["stft"])
        g = m.reference_embedding_from_wav(gold[name + "_wav"]).cpu()
        assert g.shape == (1, m.hp.gin_channels) and torch.isfinite(g).all()
        err = float((g[0].double() - gold[name + "_g64"]).abs().max())
        ratio = err / c["ref_err"]
        print(f"[ref_enc_wav_g {name}] max|g_gpu - g_fp64| = {err:.3e}  ref_err = {c['ref_err']:.3e}  ratio = {ratio:.2f}  rms(g) = {c['rms']:.3f}")
        if err > 4 * c["ref_err"]:
            bad.append((name, err, c["ref_err"], ratio))
    assert not bad, bad


@pytest.mark.parametrize("params", [audio.StftParams(2048, 512, 2048), audio.StftParams(1024, 256, 1024), audio.StftParams(1024, 512, 1024),
                                    audio.StftParams(2048, 512, 2048, 80), audio.StftParams(2048, 300, 1200)],
                         ids=["n2048", "n1024", "n1024_hop512", "mel80", "n2048_hop300_win1200"])
def test_ragged_batch_equals_each_waveform_alone_bit_for_bit(params):
    p = params
    lens = RAGGED if p.pad < 769 else [769 + p.pad, 12345, 5000, 2100 + p.pad]
    wavs, w = _ragged_batch(lens)
    spec, n = audio.spectrogram(w, lens, p)
    frames = [p.frames(k) for k in lens]
    assert n.tolist() == frames and spec.shape == (len(lens), p.channels, max(frames))
    if p == audio.StftParams(2048, 512, 2048):
        assert frames == [1, 24, 9, 4]
    for i, x in enumerate(wavs):
        alone, na = audio.spectrogram(x, params=p)
        assert na.tolist() == [frames[i]]
        assert torch.equal(spec[i, :, :frames[i]], alone[0]), (i, (spec[i, :, :frames[i]] - alone[0]).abs().max())
        assert not spec[i, :, frames[i]:].any()                                       # zeros beyond
    # 7.0 (as int16: full scale) or NaN in the batch's padding changes no bit: it is never read
    _, wg = _ragged_batch(lens, fill=32767)
    assert torch.equal(audio.spectrogram(wg, lens, p)[0], spec)
    wf = w.float() / 32768
    sf, nf = audio.spectrogram(wf, lens, p)
    assert torch.equal(sf, spec) and torch.equal(nf, n)                               # int16 input == fp32 input of x / 32768
    for junk in (7.0, float("nan")):
        wj = wf.clone()
        for i, k in enumerate(lens):
            wj[i, k:] = junk
        assert torch.equal(audio.spectrogram(wj, lens, p)[0], spec), junk
    # lengths that live on the device are not read back; the result is the same
    sd, nd = audio.spectrogram(w.cuda(), torch.tensor(lens).cuda(), p)
    assert torch.equal(sd, spec) and torch.equal(nd, n)
    # every second row of a [2B, S] tensor
    w2 = torch.full((2 * len(lens), max(lens)), -5, dtype=torch.int16)
    w2[::2] = w
    strided = w2.cuda()[::2]
    assert not strided.is_contiguous() and torch.equal(audio.spectrogram(strided, lens, p)[0], spec)
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ss, ns = audio.spectrogram(w.cuda(), lens, p)
    side.synchronize()
    assert torch.equal(ss, spec) and torch.equal(ns, n)


def test_an_item_too_short_for_a_frame_gets_length_zero_and_zero_rows():
    """Only reachable with lengths that live on the device (host lengths are refused before the call)."""
    p = audio.StftParams(2048, 512, 2048)
    wavs, w = _ragged_batch([5000, 768, 12345, 1])
    spec, n = audio.spectrogram(w.cuda(), torch.tensor([5000, 768, 12345, 1]).cuda(), p)
    assert n.tolist() == [9, 0, 24, 0] and not spec[1].any() and not spec[3].any()
    assert torch.equal(spec[0, :, :9], audio.spectrogram(wavs[0], params=p)[0][0])
    assert torch.equal(spec[2], audio.spectrogram(wavs[2], params=p)[0][0])


def test_both_store_layouts_hold_the_same_values():
    """audio.spectrogram hands out the [B, C, L] view of [B, L, C] memory; the C call writes any strides."""
    import ctypes as C
    from bert_vits2_amd import lib as L
    p = audio.StftParams(2048, 512, 2048)
    lens = RAGGED
    _, w = _ragged_batch(lens)
    spec, n = audio.spectrogram(w, lens, p)
    assert spec.stride(1) == 1 and not spec.is_contiguous()
    lib, cfg = L.load(), p.config(L.WAV_I16)
    wd, wl = w.cuda(), torch.tensor(lens).cuda()
    out = torch.full((len(lens), p.channels, 24), -1.0, device="cuda")
    ws = torch.empty(lib.bv2_stft_workspace_bytes(C.byref(cfg), len(lens), w.shape[1]), dtype=torch.uint8, device="cuda")
    n2 = torch.empty(len(lens), dtype=torch.int64, device="cuda")
    rc = lib.bv2_spectrogram(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(cfg), C.c_void_p(wd.data_ptr()), wd.stride(0),
                             C.c_void_p(wl.data_ptr()), len(lens), w.shape[1], None, C.c_void_p(out.data_ptr()), None,
                             C.c_void_p(n2.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel())
    assert rc == 0, lib.bv2_last_error(None).decode()
    assert torch.equal(out, spec) and torch.equal(n2, n)


def test_reference_embedding_from_wav_is_spectrogram_then_reference_embedding():
    for spec_channels in (1025, 80):
        m = ref_model(spec_channels)
        _, w = _ragged_batch(RAGGED)
        calls = m.ref_encode_calls
        g = m.reference_embedding_from_wav(w, RAGGED)
        assert m.ref_encode_calls == calls + 1 and g.shape == (4, m.hp.gin_channels)
        assert torch.equal(g, m.reference_embedding(*audio.spectrogram(w, RAGGED, m.stft_params)))
        alone = torch.cat([m.reference_embedding_from_wav(w[i, :k]) for i, k in enumerate(RAGGED)])
        assert torch.equal(g, alone)                                                   # ragged is exact through both steps
        assert len({tuple(r.tolist()) for r in g}) == 4


def _utts(lengths, **kw):
    out = []
    for i, T in enumerate(lengths):
        b = synth.synthetic_batch([T], languages=[i % 3], sids=[0], first_index=i)
        out.append(serving.Utterance(b["x"][0], b["tone"][0], b["language"][0], b["bert"][0], b["ja_bert"][0], b["en_bert"][0],
                                     int(b["sid"][0]), **{k: v[i] for k, v in kw.items()}))
    return out


def _close(a, b):
    """The bar of tests/test_ref_enc_gpu.py:214-215."""
    return a.shape == b.shape and a.size > 0 and np.sqrt(np.mean((a - b) ** 2)) <= 1e-5 * max(np.sqrt(np.mean(a ** 2)), 1e-3)


def test_serving_shares_one_encoding_between_utterances_that_share_a_reference_spectrogram():
    m = ref_model(1025)
    lengths = [17, 24, 9]
    gen = torch.Generator().manual_seed(7)
    kw = dict(sdp_ratio=0.5, noise_scale=0.6, noise_scale_w=0.9, length_scale=1.0)
    noise = [(torch.randn(2, T, generator=gen), torch.randn(m.hp.inter_channels, 16 * T, generator=gen)) for T in lengths]
    ra = serving.reference_spectrogram(m, synth.synthetic_reference_wav(12345, 0))
    rb = serving.reference_spectrogram(m, synth.synthetic_reference_wav(5000, 1)[None])
    assert ra.shape == (1025, 24) and rb.shape == (1025, 9) and ra.device == m.device
    assert torch.equal(ra, audio.spectrogram(synth.synthetic_reference_wav(12345, 0), params=m.stft_params)[0][0])
    utts = _utts(lengths, ref_spec=[ra, rb, ra])
    single = [serving.synthesize(m, [u], noise=[n], **kw)[0] for u, n in zip(utts, noise)]
    calls = m.ref_encode_calls
    batched = serving.synthesize(m, utts, noise=noise, max_batch=4, max_pad_ratio=3.0, **kw)
    assert m.ref_encode_calls == calls + 1                                             # three utterances, two objects, ONE ragged call
    assert all(_close(a, b) for a, b in zip(single, batched))
