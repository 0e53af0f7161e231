"""GPU: the polyphase resampler (kernels/resample.hip, bv2_resample, audio.resample) and what is built on it — reference voices recorded at
any rate, ``synthesize(output_rate=...)`` and streams that leave at another rate.

 * impulses pin every tap, every phase and both edges bit for bit against the C-provided fp32 table;
 * accuracy: max|y_gpu - y64| <= 4 * e32, y64 the fp64 evaluation with the fp64 table, e32 the error of the plain fp32 evaluation (fp32 table,
   ascending taps, product and sum each rounded) — the factor of the STFT and ReferenceEncoder tests;
 * everything else is exact (torch.equal): a ragged batch equals each waveform alone, junk or NaN in the padding changes no bit, int16 equals
   fp32 of x / 32768, strided batches, device lengths, side streams, ranges of outputs, graph replay, and a stream's pieces against the
   one-shot resampling of the same audio — an output's sum does not depend on where it is computed (include/bv2.h, rule 2).
"""
import numpy as np
import pytest
import torch

from bert_vits2_amd import audio, hparams as H, models, serving, synth
from oracle import cases
from tests.helpers import cached_state_dict
from tests.test_resample_cpu import PAIRS, resample_ref

pytestmark = pytest.mark.gpu

# beyond the issue's seven: a 441 : 1 decimation (one output per workgroup, the tap loop staged in 16 passes) and its inverse
EXTREME = [(44100, 100), (100, 44100)]
CASE = cases.CASES["narrow_b2_t18"]
KW = dict(sdp_ratio=0.5, noise_scale=0.6, noise_scale_w=0.9, length_scale=1.0)
_MODELS = {}


def _ceil_div(a, b):
    return -((-a) // b)


def narrow_model(n_speakers=None):
    """The narrow model of tests/test_stft_gpu.py: with its speaker table, or (n_speakers = 0) with the ReferenceEncoder."""
    if n_speakers not in _MODELS:
        extra = {} if n_speakers is None else dict(n_speakers=0, spec_channels=1025)
        hp = H.default_v23(**dict(CASE["hp"], **extra))
        m = models.from_hparams(hp)
        m.load_state_dict(cached_state_dict(hp, CASE["seed"]), strict=False)
        _MODELS[n_speakers] = m.to("cuda").eval()
    return _MODELS[n_speakers]


# ---- 1. impulses ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate_in,rate_out", PAIRS + EXTREME)
def test_impulses_read_back_the_table_bit_for_bit(rate_in, rate_out):
    Lr, M, K = audio.resample_plan(rate_in, rate_out)
    T32 = torch.from_numpy(audio.resample_taps(rate_in, rate_out))
    N = 2368
    k0s = [0, N // 2, N - 1]
    n = torch.arange(_ceil_div(N * Lr, M), dtype=torch.int64)
    i0, p = (n * M) // Lr, (n * M) % Lr
    for dtype, one, scale in ((torch.float32, 1.0, 1.0), (torch.int16, 16384, 0.5)):
        x = torch.zeros(len(k0s), N, dtype=dtype)
        for r, k0 in enumerate(k0s):
            x[r, k0] = one
        y, lens = audio.resample(x, None, rate_in, rate_out)
        assert y.shape == (len(k0s), len(n)) and lens.tolist() == [len(n)] * len(k0s)
        for r, k0 in enumerate(k0s):
            jj = k0 - i0 + K
            ok = (jj >= 0) & (jj <= 2 * K)
            want = torch.where(ok, T32[p, jj.clamp(0, 2 * K)] * scale, torch.zeros(()))
            assert torch.equal(y[r].cpu(), want), (dtype, k0, int((y[r].cpu() != want).sum()))
        assert y.abs().max() > 0.05 * scale * min(1.0, Lr / M)


# ---- 2. accuracy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate_in,rate_out", PAIRS)
def test_accuracy_within_four_times_the_plain_fp32_evaluation(rate_in, rate_out):
    """Measured on MI355X (docs/MEASUREMENTS.md, Resampler): the ratios max|y_gpu - y64| / e32 are printed per case; the bar is 4."""
    Lr, M, K = audio.resample_plan(rate_in, rate_out)
    T64, T32 = audio.resample_taps(rate_in, rate_out, np.float64), audio.resample_taps(rate_in, rate_out)
    N = 12345
    rng = np.random.default_rng(11)
    inputs = {"noise": torch.from_numpy(rng.integers(-32768, 32768, N).astype(np.int16)), "voice": synth.synthetic_reference_wav(N, 3)}
    for name, pcm in inputs.items():
        x = pcm.numpy().astype(np.float64) / 32768
        y64 = resample_ref(x, T64, Lr, M, K)
        e32 = np.abs(resample_ref(x.astype(np.float32), T32, Lr, M, K, dtype=np.float32).astype(np.float64) - y64).max()
        y, _ = audio.resample(pcm, None, rate_in, rate_out)
        err = np.abs(y[0].cpu().numpy().astype(np.float64) - y64).max()
        print(f"[resample {rate_in}->{rate_out} {name}] max|y_gpu - y64| = {err:.3e}  e32 = {e32:.3e}  ratio = {err / e32:.2f}")
        assert y.shape[1] == len(y64) and e32 > 0 and err <= 4 * e32


# ---- 3. ragged batches and input forms -----------------------------------------------------------------------------------------------
RAGGED = [1, 2, 769, 5000, 12345]


def _ragged(lens, fill=0):
    wavs = [synth.synthetic_reference_wav(n, i) for i, n in enumerate(lens)]
    w = torch.full((len(lens), max(lens)), fill, dtype=torch.int16)
    for i, x in enumerate(wavs):
        w[i, :lens[i]] = x
    return wavs, w


@pytest.mark.parametrize("rate_in,rate_out", PAIRS + EXTREME[:1])
def test_ragged_batch_and_input_forms_are_exact(rate_in, rate_out):
    Lr, M, _ = audio.resample_plan(rate_in, rate_out)
    lens = RAGGED
    wavs, w = _ragged(lens)
    out, n = audio.resample(w, lens, rate_in, rate_out)
    want = [_ceil_div(k * Lr, M) for k in lens]
    assert n.tolist() == want and out.shape == (len(lens), _ceil_div(max(lens) * Lr, M)) and out.dtype == torch.float32
    for i, x in enumerate(wavs):
        alone, na = audio.resample(x, None, rate_in, rate_out)
        assert na.tolist() == [want[i]] and torch.equal(out[i, :want[i]], alone[0]), i
        assert not out[i, want[i]:].any()                                             # zeros beyond N_out(b)
    assert out[4].abs().max() > 1e-3                                                  # (a voice decimated to 100 Hz keeps little)
    _, wg = _ragged(lens, fill=32767)
    assert torch.equal(audio.resample(wg, lens, rate_in, rate_out)[0], out)           # full scale in the padding: never read
    wf = w.float() / 32768
    of, nf = audio.resample(wf, lens, rate_in, rate_out)
    assert torch.equal(of, out) and torch.equal(nf, n)                                # int16 input == fp32 input of x / 32768
    for junk in (7.0, float("nan")):
        wj = wf.clone()
        for i, k in enumerate(lens):
            wj[i, k:] = junk
        assert torch.equal(audio.resample(wj, lens, rate_in, rate_out)[0], out), junk
    od, nd = audio.resample(w.cuda(), torch.tensor(lens).cuda(), rate_in, rate_out)   # lengths on the device
    assert torch.equal(od, out) and torch.equal(nd, n)
    w2 = torch.full((2 * len(lens), max(lens)), -5, dtype=torch.int16)                # every second row of a [2B, S] tensor
    w2[::2] = w
    strided = w2.cuda()[::2]
    assert not strided.is_contiguous() and torch.equal(audio.resample(strided, lens, rate_in, rate_out)[0], out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        os_, ns = audio.resample(w.cuda(), lens, rate_in, rate_out)
    side.synchronize()
    assert torch.equal(os_, out) and torch.equal(ns, n)


def test_an_item_of_length_zero_gets_length_zero_and_a_zero_row():
    """Only reachable with lengths that live on the device (host lengths are refused before the call)."""
    wavs, w = _ragged([5000, 1, 777])
    with pytest.raises(ValueError, match="outside"):
        audio.resample(w, [5000, 0, 777], 44100, 48000)
    out, n = audio.resample(w.cuda(), torch.tensor([5000, 0, 777]).cuda(), 44100, 48000)
    assert n.tolist() == [_ceil_div(5000 * 160, 147), 0, _ceil_div(777 * 160, 147)] and not out[1].any()
    assert torch.equal(out[0, :n[0]], audio.resample(wavs[0], None, 44100, 48000)[0][0])
    assert torch.equal(out[2, :n[2]], audio.resample(wavs[2], None, 44100, 48000)[0][0])


def test_equal_rates_return_the_input_without_a_launch():
    w = synth.synthetic_reference_wav(1000, 0)
    out, n = audio.resample(w, None, 44100, 44100)
    assert out.is_cuda and out.dtype == torch.float32 and n.tolist() == [1000] and torch.equal(out[0].cpu(), w.float() / 32768)
    with pytest.raises(ValueError, match="1024"):
        audio.resample(w, None, 44100, 48001)


# ---- 4. the range form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate_in,rate_out", PAIRS + EXTREME[:1])
def test_a_range_of_outputs_equals_the_slice_of_the_whole(rate_in, rate_out):
    Lr, M, K = audio.resample_plan(rate_in, rate_out)
    lens = [12345, 7001]
    _, w = _ragged(lens)
    wd, ld = w.cuda(), torch.tensor(lens).cuda()
    whole, n = audio.resample(wd, ld, rate_in, rate_out)
    N = whole.shape[1]
    cuts = sorted({c for c in (1, 1000, N - 1) if 0 < c < N})
    n_low = next(c for c in range(1, N) if (c * M) // Lr - K < 0) if K > 0 else 1     # an n0 whose support starts in front of sample 0
    bounds = [0] + cuts + [N]
    for n0, n1 in list(zip(bounds[:-1], bounds[1:])) + [(n_low, min(N, n_low + 300)), (cuts[-1] // 2, cuts[-1] // 2 + 1)]:
        start = max(0, (n0 * M) // Lr - K)
        buf = wd[:, start:]                                                           # sample `start` at offset 0, rows max(lens) apart
        got = audio.resample_range(buf, start, ld, rate_in, rate_out, n0, n1)
        assert got.shape == (2, n1 - n0) and torch.equal(got, whole[:, n0:n1]), (n0, n1)
        # an odd destination offset: the 16-byte body starts elsewhere, the sums are the same
        wide = torch.full((2, n1 - n0 + 3), -1.0, device="cuda")
        audio.resample_range(buf, start, ld, rate_in, rate_out, n0, n1, wide[:, 3:])
        assert torch.equal(wide[:, 3:], whole[:, n0:n1]) and (wide[:, :3] == -1).all(), (n0, n1)


# ---- 5. graph capture ----------------------------------------------------------------------------------------------------------------
def test_a_captured_call_replays_on_refilled_input():
    rate_in, rate_out = 44100, 16000
    lens = [9000, 4001]
    N = _ceil_div(max(lens) * 160, 441)
    src = torch.zeros(2, max(lens), dtype=torch.float32, device="cuda")
    ld = torch.tensor(lens).cuda()
    dst, nl = torch.zeros(2, N, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
    audio.device_taps(rate_in, rate_out, "cuda")                                      # built before the capture: no allocation inside
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        audio.resample_range(src, 0, ld, rate_in, rate_out, 0, N, dst, nl)
    for seed in (1, 2):
        x = torch.rand(2, max(lens), generator=torch.Generator().manual_seed(seed)) * 2 - 1
        src.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        eager, ne = audio.resample(x, lens, rate_in, rate_out)
        assert torch.equal(dst, eager) and torch.equal(nl, ne) and dst.abs().max() > 0.1, seed


# ---- 6. voices -----------------------------------------------------------------------------------------------------------------------
def test_a_reference_voice_at_another_rate_is_resampled_first():
    m = narrow_model(0)
    lens48 = [40000, 13000, 21000]
    _, w48 = _ragged(lens48)
    g = m.reference_embedding_from_wav(w48, lens48, sampling_rate=48000)
    assert g.shape == (3, m.hp.gin_channels) and len({tuple(r.tolist()) for r in g}) == 3
    assert torch.equal(g, m.reference_embedding_from_wav(*audio.resample(w48, lens48, 48000, 44100)))
    gd = m.reference_embedding_from_wav(w48.cuda(), torch.tensor(lens48).cuda(), sampling_rate=48000)     # lengths stay on the device
    assert torch.equal(gd, g)
    with pytest.raises(ValueError, match="at least"):                                 # 800 samples at 48 kHz are 735 at 44.1: below pad + 1 = 769
        m.reference_embedding_from_wav(w48, [40000, 800, 21000], sampling_rate=48000)
    w16 = synth.synthetic_reference_wav(6000, 2)
    r16 = serving.reference_spectrogram(m, w16, sampling_rate=16000)
    res, _ = audio.resample(w16, None, 16000, 44100)
    assert torch.equal(r16, audio.spectrogram(res, params=m.stft_params)[0][0]) and r16.shape == (1025, m.stft_params.frames(res.shape[1]))
    # the model's own rate, named or not, is today's path
    w = synth.synthetic_reference_wav(12345, 0)
    g0 = m.reference_embedding(*audio.spectrogram(w, params=m.stft_params))
    assert torch.equal(m.reference_embedding_from_wav(w), g0)
    assert torch.equal(m.reference_embedding_from_wav(w, sampling_rate=None), g0)
    assert torch.equal(m.reference_embedding_from_wav(w, sampling_rate=m.hp.sampling_rate), g0)
    s0 = audio.spectrogram(w, params=m.stft_params)[0][0]
    assert torch.equal(serving.reference_spectrogram(m, w), s0)
    assert torch.equal(serving.reference_spectrogram(m, w, sampling_rate=44100), s0)


# ---- 7. synthesize(output_rate) ------------------------------------------------------------------------------------------------------
def _utts(lengths):
    out = []
    for i, T in enumerate(lengths):
        b = synth.synthetic_batch([T], languages=[i % 3], sids=[i * 7 % 50], first_index=i)
        out.append(serving.Utterance(b["x"][0], b["tone"][0], b["language"][0], b["bert"][0], b["ja_bert"][0], b["en_bert"][0],
                                     int(b["sid"][0])))
    return out


def _close(a, b):
    """The bar of tests/test_stft_gpu.py (_close)."""
    return a.shape == b.shape and a.size > 0 and np.sqrt(np.mean((a - b) ** 2)) <= 1e-5 * max(np.sqrt(np.mean(a ** 2)), 1e-3)


def _synth_case():
    m = narrow_model()
    lengths = [17, 24, 9]
    gen = torch.Generator().manual_seed(7)
    noise = [(torch.randn(2, T, generator=gen), torch.randn(m.hp.inter_channels, 16 * T, generator=gen)) for T in lengths]
    return m, _utts(lengths), dict(noise=noise, max_batch=4, max_pad_ratio=3.0, **KW)


@pytest.mark.parametrize("rate", [48000, 16000])
def test_synthesize_at_another_rate(rate):
    m, utts, kw = _synth_case()
    Lr, M, _ = audio.resample_plan(m.hp.sampling_rate, rate)
    plain = serving.synthesize(m, utts, **kw)
    got = serving.synthesize(m, utts, output_rate=rate, **kw)
    for a, b in zip(plain, got):
        want = audio.resample(torch.from_numpy(a), None, m.hp.sampling_rate, rate)[0][0].cpu().numpy()
        assert b.dtype == np.float32 and b.shape == (_ceil_div(a.size * Lr, M),) and _close(want, b)
    # PCM: the peak is that of the resampled samples (bv2_pcm16 on resampled lengths, hop = 1), bit-exact against the host formula
    o = serving.synthesize(m, utts[:1], **dict(kw, noise=kw["noise"][:1]), output_rate=rate)[0]
    p = serving.synthesize(m, utts[:1], **dict(kw, noise=kw["noise"][:1]), output_rate=rate, as_pcm16=True)[0]
    assert p.dtype == np.int16 and p.shape == o.shape
    assert np.array_equal(p, np.trunc(o / np.abs(o).max() * np.float32(32767)).astype(np.int16))
    # the model's own rate is today's path
    same = serving.synthesize(m, utts, output_rate=m.hp.sampling_rate, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(plain, same))


# ---- 8. streams ----------------------------------------------------------------------------------------------------------------------
def _stream_inputs(hp, lengths):
    b = synth.synthetic_batch(lengths, languages=[i % 3 for i in range(len(lengths))], sids=[3 + 5 * i for i in range(len(lengths))])
    nw, nz = synth.synthetic_noise(len(lengths), max(lengths), 16 * max(lengths), hp.inter_channels)
    args = [b[k].cuda() for k in ("x", "x_lengths", "sid", "tone", "language", "bert", "ja_bert", "en_bert")]
    return args, dict(noise_w=nw.cuda(), noise_z=nz.cuda())


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("rate", [48000, 8000])
def test_a_stream_at_another_rate_is_the_one_shot_resampling_of_its_audio(rate, exact):
    m = narrow_model()
    U, sr = m.hp.total_upsample, m.hp.sampling_rate
    Lr, M, K = audio.resample_plan(sr, rate)
    args, noise = _stream_inputs(m.hp, [18, 11])
    kw = dict(exact_lengths=exact, chunk_frames=8, first_chunk_frames=3, **noise, **KW)
    plain = m.infer_stream(*args, **kw)
    total_in = plain.total_samples
    base = list(plain)
    model_rate = torch.cat([a for _, a in base], dim=1)
    assert model_rate.shape[1] == total_in and len(base) >= 4
    st = m.infer_stream(*args, output_rate=rate, **kw)
    total = _ceil_div(total_in * Lr, M)
    assert st.total_samples == total and st.y_lengths_host == plain.y_lengths_host
    pieces, at = [], 0
    for start, a in st:
        assert start == at and a.shape[1] > 0 and a.dtype == torch.float32 and a.shape[1] <= st.max_chunk_samples
        pieces.append(a)
        at += a.shape[1]
    assert at == total                                                                # contiguous from 0, nothing past the end
    if rate == 8000:
        assert 3 * U < K and len(pieces) < len(base)                                  # the first chunk completes no output: nothing is yielded
    lens = plain.y_lengths.cpu() * U if exact else torch.full((2,), total_in, dtype=torch.int64)
    want, wl = audio.resample(model_rate, lens.cuda(), sr, rate)
    cat = torch.cat(pieces, dim=1)
    assert torch.equal(cat, want), int((cat != want).sum())
    assert cat.abs().max() > 1e-3
    if exact:
        short = int(wl.min())
        assert short < total and not cat[int(wl.argmin()), short:].any()
    # PCM: the fixed gain on the resampled samples
    pcm = torch.cat([a for _, a in m.infer_stream(*args, output_rate=rate, as_pcm16=True, **kw)], dim=1)
    assert pcm.dtype == torch.int16
    assert np.array_equal(pcm.cpu().numpy(), np.clip(cat.cpu().numpy() * np.float32(32767), -32768, 32767).astype(np.int16))


def test_a_stream_at_the_models_rate_is_todays_stream():
    m = narrow_model()
    args, noise = _stream_inputs(m.hp, [18, 11])
    kw = dict(exact_lengths=True, chunk_frames=8, first_chunk_frames=3, **noise, **KW)
    a = list(m.infer_stream(*args, **kw))
    b = list(m.infer_stream(*args, output_rate=None, **kw))
    c = list(m.infer_stream(*args, output_rate=m.hp.sampling_rate, **kw))
    U = m.hp.total_upsample
    assert len(a) == len(b) == len(c) >= 4 and a[0][1].shape[1] == 3 * U and a[1][1].shape[1] == 8 * U
    for (s0, x0), (s1, x1), (s2, x2) in zip(a, b, c):
        assert s0 == s1 == s2 and torch.equal(x0, x1) and torch.equal(x0, x2)
    assert [s for s, _ in a] == [0] + [3 * U + 8 * U * i for i in range(len(a) - 1)]


@pytest.mark.parametrize("rate", [48000, 8000])
def test_synthesize_stream_at_another_rate(rate):
    m, utts, kw = _synth_case()
    sr = m.hp.sampling_rate
    Lr, M, _ = audio.resample_plan(sr, rate)
    skw = dict(chunk_frames=8, first_chunk_frames=3, **kw)
    base = [[] for _ in utts]
    for i, start, piece in serving.synthesize_stream(m, utts, **skw):
        base[i].append(piece)
    for as_pcm in (False, True):
        got = [[] for _ in utts]
        for i, start, piece in serving.synthesize_stream(m, utts, output_rate=rate, as_pcm16=as_pcm, **skw):
            assert piece.ndim == 1 and piece.size > 0 and start == sum(p.size for p in got[i])      # in order, contiguous offsets
            got[i].append(piece)
        for i in range(len(utts)):
            x = np.concatenate(base[i])
            want = audio.resample(torch.from_numpy(x), None, sr, rate)[0][0].cpu().numpy()
            cat = np.concatenate(got[i])
            assert cat.shape == (_ceil_div(x.size * Lr, M),)                                          # cut at its own resampled length
            if as_pcm:
                want = np.clip(want * np.float32(32767), -32768, 32767).astype(np.int16)
            assert cat.dtype == want.dtype and np.array_equal(cat, want), i
