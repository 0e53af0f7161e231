"""CPU: the host side of the polyphase resampler (include/bv2.h bv2_resample_*): the integer plan, the fp64 / fp32 filter table against the
numpy form of its definition, the filter's spectral quality evaluated in fp64 from the C-provided table, the streaming arithmetic
(bv2_resample_ready + the history rule reproduce the one-shot result bit for bit) and the refusals.  No launch: there is no GPU here."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from bert_vits2_amd import audio, lib as L
from tests.helpers import ROOT

PAIRS = [(44100, 48000), (48000, 44100), (44100, 22050), (22050, 44100), (44100, 16000), (16000, 44100), (44100, 8000)]
SPECTRAL_PAIRS = PAIRS + [(44100, 24000), (32000, 44100)]
Z, BETA, ROLLOFF = 32, 10.0, 0.91


def plan_ref(rate_in, rate_out):
    g = math.gcd(rate_in, rate_out)
    Lr, M = rate_out // g, rate_in // g
    c = ROLLOFF * min(1, Lr / M)
    W = Z / c
    return Lr, M, int(math.ceil(W)), c, W


def taps_ref(rate_in, rate_out):
    """The definition, in numpy fp64."""
    Lr, M, K, c, W = plan_ref(rate_in, rate_out)
    p = np.arange(Lr, dtype=np.float64)[:, None]
    jj = np.arange(2 * K + 1)[None, :]
    t = p / Lr - (jj - K)
    inside = np.abs(t) < W
    T = c * np.sinc(c * t) * np.i0(BETA * np.sqrt(np.where(inside, 1 - (t / W) ** 2, 0.0))) / np.i0(BETA)
    T = np.where(inside, T, 0.0)
    return T / T.sum(1, keepdims=True)


def resample_ref(x, T, Lr, M, K, n0=0, n1=None, length=None, dtype=np.float64):
    """y[n] = sum_jj x[i0 + jj - K] T[p][jj] for n in [n0, n1), x zero outside [0, length); one tap after another in ascending jj,
    product and sum each rounded to `dtype`."""
    length = len(x) if length is None else length
    n_out = -((-length * Lr) // M)
    n1 = n_out if n1 is None else n1
    n = np.arange(n0, n1, dtype=np.int64)
    i0, p = (n * M) // Lr, (n * M) % Lr
    xp = np.concatenate([np.zeros(K, dtype), np.asarray(x[:length], dtype), np.zeros(K + M + 2, dtype)])
    Tt = T.astype(dtype)
    y = np.zeros(len(n), dtype)
    for jj in range(2 * K + 1):
        idx = np.minimum(i0 + jj, len(xp) - 1)                  # index i0 + jj - K of x, shifted by the K zeros in front
        y = (y + (xp[idx] * Tt[p, jj]).astype(dtype)).astype(dtype)
    y[n >= n_out] = 0
    return y


def cfg_of(rate_in, rate_out, fmt=L.WAV_F32):
    return audio.resample_config(rate_in, rate_out, fmt)


def err():
    return L.load().bv2_last_error(None).decode()


@pytest.mark.parametrize("rate_in,rate_out", SPECTRAL_PAIRS + [(44100, 100), (100, 44100), (3, 2)])
def test_plan_length_ready_are_the_integer_formulas(rate_in, rate_out):
    lib = L.load()
    Lr, M, K, _, _ = plan_ref(rate_in, rate_out)
    assert audio.resample_plan(rate_in, rate_out) == (Lr, M, K)
    cfg = cfg_of(rate_in, rate_out)
    for n in (0, 1, K - 1, K, K + 1, 12345):
        assert lib.bv2_resample_length(C.byref(cfg), n) == -((-n * Lr) // M) == audio.resample_length(rate_in, rate_out, n)
        assert lib.bv2_resample_ready(C.byref(cfg), n) == max(0, -((-(n - K) * Lr) // M))
        if n <= K:
            assert lib.bv2_resample_ready(C.byref(cfg), n) == 0
    # ready(A) is the number of outputs whose whole support [i0 - K, i0 + K] lies in [0, A)
    for A in (K + 1, K + 7, 3 * K + 11):
        r = lib.bv2_resample_ready(C.byref(cfg), A)
        assert r >= 1 and ((r - 1) * M) // Lr + K <= A - 1 < (r * M) // Lr + K


def test_the_table_of_the_issue():
    assert [audio.resample_plan(a, b)[0::2] for a, b in ((44100, 48000), (44100, 16000), (44100, 8000), (16000, 44100), (32000, 44100))] == \
        [(160, 36), (160, 97), (80, 194), (441, 36), (441, 36)]


@pytest.mark.parametrize("rate_in,rate_out", PAIRS)
def test_taps_are_the_definition(rate_in, rate_out):
    T64 = audio.resample_taps(rate_in, rate_out, np.float64)
    ref = taps_ref(rate_in, rate_out)
    assert T64.shape == ref.shape
    d = np.abs(T64 - ref).max()
    print(f"{rate_in}->{rate_out}: max |T - numpy| = {d:.3e}")
    assert d <= 1e-12
    assert np.abs(T64.sum(1) - 1).max() <= 1e-14
    T32 = audio.resample_taps(rate_in, rate_out, np.float32)
    assert T32.dtype == np.float32 and np.array_equal(T32, T64.astype(np.float32))


@pytest.mark.parametrize("rate_in,rate_out", SPECTRAL_PAIRS)
def test_spectral_quality_of_the_c_table(rate_in, rate_out):
    """20 000-sample tones, the middle 60 % of the output judged, all in fp64 from the C-provided table."""
    Lr, M, K, _, _ = plan_ref(rate_in, rate_out)
    T = audio.resample_taps(rate_in, rate_out, np.float64)
    nyq = min(rate_in, rate_out) / 2
    N = 20000
    k = np.arange(N)
    for rel, kind, bound in ((0.5, "pass", 2e-5), (0.8, "pass", 2e-5), (1.0001, "stop", 3.2e-5), (1.1, "stop", 1e-5), (1.5, "stop", 1e-5)):
        f = rel * nyq
        if f >= rate_in / 2:                                     # not representable at the input rate (an upsampling's stop band tones)
            continue
        x = np.sin(2 * np.pi * f * k / rate_in + 0.3)
        y = resample_ref(x, T, Lr, M, K)
        a, b = int(0.2 * len(y)), int(0.8 * len(y))
        mid = y[a:b]
        if kind == "pass":
            want = np.sin(2 * np.pi * f * np.arange(a, b) / rate_out + 0.3)
            e = np.abs(mid - want).max()
        else:
            e = np.abs(mid).max()
        print(f"{rate_in}->{rate_out} {rel} nyq ({kind}): {e:.3e}  (bound {bound:.1e})")
        assert e <= bound


def test_round_trip():
    """44.1 -> 48 -> 44.1 kHz of a 12-harmonic 170 Hz signal returns it (4.8e-6 on the prototype) in the interior."""
    k = np.arange(20000)
    x = sum(np.sin(2 * np.pi * 170 * h * k / 44100 + h) / (12 * h ** 0.5) for h in range(1, 13))
    up = resample_ref(x, audio.resample_taps(44100, 48000, np.float64), *plan_ref(44100, 48000)[:3])
    back = resample_ref(up, audio.resample_taps(48000, 44100, np.float64), *plan_ref(48000, 44100)[:3])
    a, b = 4000, 16000
    e = np.abs(back[a:b] - x[a:b]).max()
    print(f"round trip: {e:.3e}")
    assert len(back) in (len(x), len(x) + 1) and e <= 4e-5                    # two passes, each inside the pass-band bound of 2e-5


@pytest.mark.parametrize("chunks", [[3 * 64, 8 * 64, 8 * 64, 8 * 64, 8 * 64, 2 * 64], [1, 700, 5, 64, 1301, 2, 199, 97]],
                         ids=["3_8_8_8_8_2_x64", "uneven"])
@pytest.mark.parametrize("rate_in,rate_out", [(44100, 48000), (44100, 8000), (16000, 44100)])
def test_a_chunk_walk_reproduces_the_one_shot_result(rate_in, rate_out, chunks):
    """The streaming rule in numpy fp32: after the chunk that ends at E emit [done, min(ready(E), N_total)) (everything at the last
    chunk) from a buffer that keeps only the samples from max(0, i0(done) - K) on."""
    lib = L.load()
    cfg = cfg_of(rate_in, rate_out)
    Lr, M, K, _, _ = plan_ref(rate_in, rate_out)
    T = audio.resample_taps(rate_in, rate_out)
    rng = np.random.default_rng(5)
    total = sum(chunks)
    x = rng.uniform(-1, 1, total).astype(np.float32)
    whole = resample_ref(x, T, Lr, M, K, dtype=np.float32)
    n_total = lib.bv2_resample_length(C.byref(cfg), total)
    assert len(whole) == n_total
    buf, start, done, E, pieces, longest = np.zeros(0, np.float32), 0, 0, 0, [], 0
    for ci, n in enumerate(chunks):
        buf = np.concatenate([buf, x[E:E + n]])
        E += n
        r = n_total if ci == len(chunks) - 1 else min(lib.bv2_resample_ready(C.byref(cfg), E), n_total)
        if r <= done:
            continue
        assert start <= max(0, (done * M) // Lr - K)                            # the lower edge bv2_resample checks
        # the buffer stands for the signal: samples in front of `start` are not needed, samples from E on are not yet known
        sig = np.concatenate([np.full(start, np.nan, np.float32), buf])
        n = np.arange(done, r)
        assert ((n * M) // Lr - K).min() >= start or start == 0
        if ci < len(chunks) - 1:
            assert ((n * M) // Lr + K).max() < E
        pieces.append(resample_ref(np.nan_to_num(sig), T, Lr, M, K, done, r, length=total if ci == len(chunks) - 1 else E,
                                   dtype=np.float32))
        done = r
        keep = max(start, max(0, (done * M) // Lr - K))
        buf, start = buf[keep - start:], keep
        longest = max(longest, len(buf))
    assert done == n_total and np.array_equal(np.concatenate(pieces), whole)
    assert longest <= 2 * K + M / Lr + 2


def test_refusals_carry_their_message():
    lib = L.load()
    L_, M_, K_ = (C.c_int32(), C.c_int32(), C.c_int32())
    plan = lambda c: lib.bv2_resample_plan(C.byref(c), C.byref(L_), C.byref(M_), C.byref(K_))
    assert plan(cfg_of(44100, 44100)) != 0 and "equals rate_out" in err()
    assert plan(cfg_of(0, 44100)) != 0 and "positive" in err()
    assert plan(cfg_of(44100, -8000)) != 0 and "positive" in err()
    assert plan(cfg_of(44100, 48001)) != 0 and "1024" in err() and "48001" in err()
    assert plan(cfg_of(44100, 2)) != 0 and "2^20" in err()                      # L = 1, but 2K + 1 = 1 550 771 taps
    bad = cfg_of(44100, 48000)
    bad.struct_bytes = 12
    assert plan(bad) != 0 and "struct_bytes" in err()
    assert lib.bv2_resample_length(C.byref(bad), 10) < 0 and lib.bv2_resample_ready(C.byref(bad), 10) < 0
    assert lib.bv2_resample_taps(C.byref(bad), C.c_void_p(8)) != 0 and lib.bv2_resample_taps_f64(C.byref(bad), C.c_void_p(8)) != 0
    assert lib.bv2_resample_taps(C.byref(cfg_of(44100, 48000)), None) != 0 and "out is null" in err()
    bad = cfg_of(44100, 48000, 7)
    assert plan(bad) != 0 and "input_format" in err()
    with pytest.raises(ValueError, match="1024"):
        audio.resample_plan(44100, 48001)

    # bv2_resample checks every argument before anything touches the device: made-up non-null pointers are never followed
    cfg = cfg_of(44100, 48000)
    p = C.c_void_p(4096)

    def call(cfg=cfg, taps=p, src=p, src_start=0, src_n=1000, n0=0, n1=100, dst=p, dst_bstride=100, B=1):
        return lib.bv2_resample(None, C.byref(cfg), taps, src, 1000, src_start, src_n, None, B, n0, n1, dst, dst_bstride, None)

    for kw, msg in ((dict(cfg=cfg_of(44100, 44100)), "equals rate_out"), (dict(cfg=cfg_of(44100, 48001)), "1024"),
                    (dict(cfg=cfg_of(-1, 48000)), "positive"), (dict(taps=None), "taps is null"), (dict(src=None), "src is null"),
                    (dict(dst=None), "dst is null"), (dict(n0=10, n1=9), "below n0"), (dict(n0=-1), "n0 must not be negative"),
                    (dict(dst_bstride=99), "dst_bstride"), (dict(B=0), "B must be"), (dict(src_n=-1), "src_n"),
                    (dict(src_start=1), "lower edge"),                                    # output 0 reads from sample 0 on
                    (dict(n0=1000, n1=1100, src_start=883), "lower edge")):               # i0(1000) - K = 918 - 36 = 882
        assert call(**kw) == -1, kw
        assert msg in err(), (kw, err())
    assert call(n0=50, n1=50) == 0                                                        # an empty range is legal and launches nothing


def test_abi_version_and_exports():
    lib = L.load()
    assert lib.bv2_abi_version() == 3 == L.ABI_VERSION
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bv2.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bv2_[a-z0-9_]+)\s*\(", src))
    for name in ("bv2_resample_plan", "bv2_resample_length", "bv2_resample_ready", "bv2_resample_taps", "bv2_resample_taps_f64",
                 "bv2_resample"):
        assert name in declared and hasattr(lib, name) and name in [s[0] for s in L.SYMBOLS]
    assert C.sizeof(L.ResampleConfig) == 16
