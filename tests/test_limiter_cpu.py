"""CPU: the host side of the look-ahead true-peak limiter (include/bv2.h bv2_limiter_*, bv2_limit) and its numpy oracle
(tests/limiter_oracle.py): plan and window against the numpy definition, every refusal — made before the device is touched, so it runs
here without one — the oracle's own guarantees (sample bound, exact pass-through, invariance to the buffer around the item), and the input
choices of tests/test_limiter_gpu.py, verified in numpy."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from bert_vits2_amd import audio, build, lib as L
from tests import limiter_oracle as M, loudness_oracle as O, r128_oracle as R
from tests.helpers import ROOT

RATES = (8000, 44100, 48000, 96000, 192000)


def err():
    return L.load().bv2_last_error(None).decode()


# ---- 1. plan and window ----------------------------------------------------------------------------------------------------------------
def test_plan_against_the_definition():
    lib = L.load()
    for rate, want in ((8000, (12, 240, 4, 36)), (44100, (66, 1323, 4, 36)), (48000, (72, 1440, 4, 36)), (96000, (144, 2880, 2, 36)),
                       (192000, (288, 5760, 1, 0))):
        v = [C.c_int32() for _ in range(4)]
        assert lib.bv2_limiter_plan(C.byref(audio.limiter_config(rate)), *[C.byref(x) for x in v]) == 0, err()
        assert tuple(x.value for x in v) == want == audio.limiter_plan(rate), rate
        assert M.plan(rate) == want[:2] and R.factor(rate) == want[2]
    for rate in RATES:                                            # other times: H >= 1, P >= H, halves round up
        for la, rel in ((0.0, 0.0), (0.01, 0.02), (1.5, 1.0), (0.125, 7.3), (2.0, 20.0)):
            H, P = M.plan(rate, la, rel)
            assert audio.limiter_plan(rate, la, rel)[:2] == (H, P) and 1 <= H <= P, (rate, la, rel)
    assert audio.limiter_plan(8000, 0.25, 0.0)[:2] == (1, 1)
    assert lib.bv2_limiter_plan(C.byref(audio.limiter_config(48000)), None, None, None, None) == 0
    assert (L.LIMITER_TILE, L.LIMITER_MAX_REACH) == (1024, 6144)


@pytest.mark.parametrize("rate", RATES)
def test_window_against_the_definition(rate):
    for la, rel in ((3.0, 60.0), (0.0, 0.0), (1.5, 5.0)):
        H, P = M.plan(rate, la, rel)
        w = audio.limiter_window(rate, la, rel)
        want = M.window64(H, P)
        assert w.dtype == np.float32 and w.shape == (P + H + 1,)
        # the library's cos and numpy's may differ in the last bit of fp64: at most one fp32 ulp of the value after the one rounding
        assert np.all(np.abs(w.astype(np.float64) - want) <= 2.0 ** -23 * want + 1e-300), (rate, la, rel)
        assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 2.0 ** -22
        assert np.all(w > 0) and int(np.argmax(w)) == P
        assert np.all(np.diff(w[:P + 1]) >= 0) and np.all(np.diff(w[P:]) <= 0)     # rising up to k = 0, falling behind it


def test_exports_and_sources():
    lib = L.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bv2.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bv2_[a-z0-9_]+)\s*\(", src))
    for name in ("bv2_limiter_plan", "bv2_limiter_window", "bv2_limiter_workspace_bytes", "bv2_limit"):
        assert name in declared and hasattr(lib, name) and name in [s[0] for s in L.SYMBOLS]
    assert "kernels/limiter.hip" in build.SOURCES and "kernels/truepeak_taps.h" in build.HEADERS
    assert re.search(r"BV2_LIMITER_TILE\s*=\s*1024,\s*BV2_LIMITER_MAX_REACH\s*=\s*6144", src)
    assert C.sizeof(L.LimiterConfig) == 32


# ---- 2. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_the_device():
    """Made-up non-null pointers are never followed: every argument is checked first."""
    lib = L.load()
    p = C.c_void_p(4096)
    good = audio.limiter_config(44100)
    bad_bytes = audio.limiter_config(44100)
    bad_bytes.struct_bytes = 8
    reserved = audio.limiter_config(44100)
    reserved.reserved = 1
    S = 100000
    cfgs = ((audio.limiter_config(7999), "sample_rate"), (audio.limiter_config(192001), "sample_rate"), (bad_bytes, "struct_bytes"),
            (reserved, "reserved"), (audio.limiter_config(44100, input_format=5), "input_format"),
            (audio.limiter_config(44100, -1.0), "finite and not negative"), (audio.limiter_config(44100, 3.0, math.nan), "finite and not negative"),
            (audio.limiter_config(44100, math.inf), "finite and not negative"),
            (audio.limiter_config(44100, 3.0, 280.0), "BV2_LIMITER_MAX_REACH"), (audio.limiter_config(192000, 3.0, 61.1), "BV2_LIMITER_MAX_REACH"))
    for c, msg in cfgs:
        assert lib.bv2_limiter_plan(C.byref(c), None, None, None, None) == -1 and msg in err(), (msg, err())
        assert lib.bv2_limiter_window(C.byref(c), p) == -1 and msg in err()
        assert lib.bv2_limiter_workspace_bytes(C.byref(c), 1, S) < 0 and msg in err()
    assert lib.bv2_limiter_plan(None, None, None, None, None) == -1 and "cfg is null" in err()
    assert lib.bv2_limiter_window(C.byref(good), None) == -1 and "out is null" in err()
    assert lib.bv2_limiter_plan(C.byref(audio.limiter_config(192000, 3.0, 60.0)), None, None, None, None) == 0      # the defaults fit everywhere
    for B, s in ((0, S), (65536, S), (1, 0), (1, 2 ** 31)):
        assert lib.bv2_limiter_workspace_bytes(C.byref(good), B, s) < 0 and "B must be" in err()
    need = lib.bv2_limiter_workspace_bytes(C.byref(good), 2, S)
    assert need >= 2 * S * 4

    def lim(cfg=good, taps=p, window=p, src=p, bstride=S, B=2, S=S, groups=None, n_groups=2, gain=p, ceiling=-1.0, f32=p, i16=None,
            dstride=S, curve=None, mg=p, ls=p, ws=p, nbytes=need):
        return lib.bv2_limit(None, C.byref(cfg), taps, window, src, bstride, None, B, S, groups, n_groups, gain, ceiling, f32, i16, dstride,
                             curve, mg, ls, ws, nbytes)

    cases = [(dict(cfg=c), -1, msg) for c, msg in cfgs] + [
        (dict(src=None), -1, "src is null"), (dict(gain=None), -1, "gain is null"), (dict(taps=None), -1, "taps is null"),
        (dict(window=None), -1, "window is null"), (dict(mg=None), -1, "min_gain and limited_samples"),
        (dict(ls=None), -1, "min_gain and limited_samples"), (dict(f32=None), -1, "exactly one of"), (dict(i16=p), -1, "exactly one of"),
        (dict(bstride=-1), -1, "src_bstride"), (dict(B=0), -1, "B must be"), (dict(B=65536), -1, "B must be"), (dict(S=0), -1, "S must be"),
        (dict(n_groups=1), -1, "n_groups"), (dict(groups=p, n_groups=0), -1, "n_groups"), (dict(dstride=S - 1), -1, "dst_bstride"),
        (dict(ceiling=math.nan), -1, "ceiling_db must be finite"), (dict(ceiling=math.inf), -1, "ceiling_db must be finite"),
        (dict(ceiling=-2000.0), -1, "positive finite float"), (dict(ceiling=2000.0), -1, "positive finite float"),
        (dict(ws=None), -5, "workspace"), (dict(nbytes=need - 257), -5, "workspace")]
    for kw, rc, msg in cases:
        assert lim(**kw) == rc, kw
        assert msg in err() and err().startswith("bv2_limit: "), (kw, err())


def test_python_wrappers_refuse_before_any_device_call():
    x = torch.zeros(2, 20000)
    with pytest.raises(ValueError, match="sampling rate"):
        audio.limit(x)
    with pytest.raises(ValueError, match="sample_rate"):
        audio.limit(x, rate=7000)
    with pytest.raises(ValueError, match="float32"):
        audio.limit(x.double(), rate=44100)
    with pytest.raises(ValueError, match="outside"):
        audio.limit(x, [5, 20001], rate=44100)
    with pytest.raises(ValueError, match="BV2_LIMITER_MAX_REACH"):
        audio.limit(x, rate=44100, release_ms=300.0)
    with pytest.raises(ValueError, match="not negative"):
        audio.limit(x, rate=44100, lookahead_ms=-1.0)
    with pytest.raises(ValueError, match="ceiling_db"):
        audio.limit(x, rate=44100, ceiling_db=math.inf)
    with pytest.raises(ValueError, match="makeup_passes"):
        audio.normalize_loudness(x, rate=44100, limiter=True, makeup_passes=4)
    with pytest.raises(ValueError, match="makeup_passes"):
        audio.normalize_loudness(x, rate=44100, limiter=True, makeup_passes=-1)
    with pytest.raises(ValueError, match="BV2_LIMITER_MAX_REACH"):
        audio.normalize_loudness(x, rate=44100, limiter=True, release_ms=300.0)


# ---- 3. the oracle's own guarantees ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def taps(rate, dtype):
    F = R.factor(rate)
    return audio.resample_taps(rate, F * rate, np.float64 if dtype == "f64" else np.float32) if F > 1 else None


def restated(x, rate, la, rel, g, ceiling_db=-1.0):
    """limit32 on the fp32 rounding of the fp64 envelope (the device's envelope is the resampler's own; here only the form matters)."""
    H, P = M.plan(rate, la, rel)
    e = M.envelope64(M.as_f32(x), taps(rate, "f32")).astype(np.float32)
    return M.limit32(M.as_f32(x), e, g, M.ceiling(ceiling_db), H, P, M.window32(H, P))


@pytest.mark.parametrize("rate", (8000, 44100, 96000))
def test_oracle_sample_bound_and_pass_through(rate):
    la, rel = M.GPU_TIMES[rate]
    H, P = M.plan(rate, la, rel)
    n = 3 * M.TILE + 17
    x = M.crest_signal(n, M.crests(n, P), seed=rate)
    c = M.ceiling(-1.0)
    for g in (1.0, 1.3):
        r = restated(x, rate, la, rel, g)
        assert r["limited_samples"] > 0 and r["min_gain"] < 1
        assert float(np.abs(r["out"]).max()) <= float(c) * M.SAMPLE_BOUND                     # by construction, after rounding too
        assert np.all(r["curve"] <= r["r"]) and np.all(r["curve"] > 0)
        r64 = M.limit64(x, g, c, H, P, taps(rate, "f64"))
        assert float(np.abs(r64["out"]).max()) <= float(c) * (1 + 1e-12)
        assert np.max(np.abs(r64["curve"] - r["curve"])) <= M.curve_bound(x, g, c, H, P, taps(rate, "f32"))
    # an item under the ceiling: d is exactly 0, s exactly 1.0f, out the one product
    q = M.crest_signal(n, (), seed=rate)
    r = restated(q, rate, la, rel, 1.3)
    assert r["limited_samples"] == 0 and r["min_gain"] == 1 and np.all(r["curve"] == 1)
    assert np.array_equal(r["out"].view(np.int32), O.apply_f32(q, np.float32(1.3)).view(np.int32))
    assert np.array_equal(r["out16"], O.apply_i16(q, np.float32(1.3)))


def test_oracle_is_invariant_to_the_buffer_around_the_item():
    """An item whose crests stand at least the reach H + P + 1 (and the interpolator's K) inside it: in a zero-padded buffer, wherever it
    sits, the item's span leaves with the same bits and the padding as zeros.  (A crest nearer to an edge differs by definition: d is 0
    outside the ITEM, and a buffer's zeros are inside it.)"""
    rate, (la, rel) = 8000, M.GPU_TIMES[8000]
    H, P = M.plan(rate, la, rel)
    n, reach = 2 * M.TILE + 5, H + P + 1 + 36
    x = M.crest_signal(n, ((reach + 3, 6), (M.TILE, 8), (n - reach - 4, 5)), seed=5)
    alone = restated(x, rate, la, rel, 1.3)
    assert 0 < alone["limited_samples"] < n
    for front, back in ((1, 0), (37, 500), (M.TILE - 1, M.TILE + 1)):
        buf = np.concatenate([np.zeros(front, np.float32), x, np.zeros(back, np.float32)])
        r = restated(buf, rate, la, rel, 1.3)
        assert np.array_equal(r["out"][front:front + n].view(np.int32), alone["out"].view(np.int32)), (front, back)
        assert np.array_equal(r["curve"][front:front + n].view(np.int32), alone["curve"].view(np.int32))
        assert not r["out"][:front].any() and not r["out"][front + n:].any() and r["limited_samples"] >= alone["limited_samples"]


# ---- 4. the input choices of the GPU tests -----------------------------------------------------------------------------------------------
def test_gpu_cases_engage_the_limiter():
    for rate, (la, rel) in M.GPU_TIMES.items():
        H, P = M.plan(rate, la, rel)
        assert R.factor(rate) == M.GPU_FACTOR[rate]
        for n in M.lengths(H):
            r = restated(M.crest_signal(n, M.crests(n, P), seed=rate), rate, la, rel, 1.3)
            assert r["limited_samples"] > 0, (rate, n)
        # the long 8 kHz item keeps tiles on either path: a lone crest, the reach inside a tile
        if H + P + 1 < M.TILE // 2:
            n = 5 * M.TILE + 3
            r = restated(M.crest_signal(n, M.LONE, seed=rate), rate, la, rel, 1.3)
            assert 0 < r["limited_samples"] < M.TILE and np.all(r["curve"][M.TILE + M.TILE // 2:] == 1)
    assert M.plan(8000, *M.GPU_TIMES[8000]) == (12, 240) and M.plan(44100, *M.GPU_TIMES[44100])[1] == 1323 > M.TILE
    assert M.plan(8000, *M.MIN_LOOKAHEAD)[0] == 1


def test_the_voiced_signal_misses_its_target_statically_and_holds_it_limited():
    """-16 LUFS under -1 dBTP at 44.1 kHz: the static path lands at least 2 LU low; the limiter's share of samples is above 0 and below
    one half; with one make-up pass the fp64 oracle is within 0.25 LU of the target."""
    rate, target = 44100, -16.0
    x = M.voiced_bursts()
    t64 = taps(rate, "f64")
    H, P = M.plan(rate)
    c = float(M.ceiling(-1.0))
    lufs = O.measure([x], rate)["lufs"]
    g = 10.0 ** ((target - lufs) / 20.0)
    static = min(g, c / R.true_peak(x, t64))
    assert target - (lufs + 20.0 * math.log10(static)) >= 2.0
    r = M.limit64(x, g, c, H, P, t64)
    out0 = O.measure([r["out"]], rate)["lufs"]
    g1 = g * 10.0 ** ((target - out0) / 20.0)
    r = M.limit64(x, g1, c, H, P, t64)
    out1 = O.measure([r["out"]], rate)["lufs"]
    share = float((r["curve"] < 1).mean())
    print(f"static short by {target - (lufs + 20.0 * math.log10(static)):.3f} LU, limiter {target - out0:.3f} LU, one make-up pass "
          f"{target - out1:.3f} LU, limited share {share:.3f}, true peak / c {R.true_peak(r['out'], t64) / c:.7f}")
    assert 0.0 < share < 0.5
    assert abs(target - out1) <= 0.25
