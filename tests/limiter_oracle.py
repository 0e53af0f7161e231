"""The look-ahead true-peak limiter as include/bv2.h defines it (bv2_limit), in numpy — the reference kernels/limiter.hip is held to.
numpy only.  Two forms:

``limit64``   the definition in fp64, the envelope interpolated with the fp64 table the caller passes (``bv2_resample_taps_f64`` at
              rate -> F rate), the window in fp64.
``limit32``   the fp32 restatement of everything AFTER the envelope: it takes ``e`` (fp32) as input and performs every operation as the
              header says — one rounding each, the FIR accumulated from 0 over ascending k — so the device's ``curve`` and ``out`` must
              equal it as BITS.

All indices count from the item's first sample:
  r[i] = min(1, c / (e[i] g)), 1 outside [0, n);  m[j] = min r[j - H - 1 .. j + P + 1];  d[j] = 1 - m[j], 0 outside [0, n);
  A[i] = sum_{k = -P..H} w[k] d[i + k];  s[i] = min(1 - A[i], r[i - 1], r[i], r[i + 1]);  out[i] = (x[i] g) s[i].
"""
import math

import numpy as np

from tests import r128_oracle as R

U = 2.0 ** -24                        # half an ulp of fp32, relative: the error of one rounded operation


def plan(rate, lookahead_ms=3.0, release_ms=60.0):
    """(H, P): round = floor(x + 0.5), as bv2_limiter_plan."""
    H = max(1, int(math.floor(lookahead_ms * rate / 2000.0 + 0.5)))
    P = max(H, int(math.floor(release_ms * rate / 2000.0 + 0.5)))
    return H, P


def window64(H, P):
    """w[k] at index k + P: a half-Hann on either side of k = 0, normalised to sum 1."""
    k = np.arange(-P, H + 1, dtype=np.float64)
    u = np.where(k >= 0, 0.5 + 0.5 * np.cos(np.pi * k / (H + 1)), 0.5 + 0.5 * np.cos(np.pi * k / (P + 1)))
    return u / u.sum()


def window32(H, P):
    return window64(H, P).astype(np.float32)


def ceiling(ceiling_db):
    """c: formed in fp64, rounded once."""
    return np.float32(10.0 ** (ceiling_db / 20.0))


def envelope64(x, taps64=None):
    """e[i] = max(|x[i]|, max_p |y[i F + p]|); ``taps64`` None: F = 1."""
    x = np.asarray(x, np.float64)
    e = np.abs(x)
    if taps64 is not None and len(x):
        e = np.maximum(e, np.abs(R.oversample(x, taps64)).max(0))
    return e


def _hold(r, H, P):
    """m[j] for j in [-P, n + H): the values the FIR of the outputs [0, n) reads."""
    n = len(r)
    W = H + P + 3
    pad = np.concatenate([np.ones(P + H + 1, r.dtype), r, np.ones(H + P + 1, r.dtype)])    # pad[e] = r[e - (P + H + 1)]
    return np.lib.stride_tricks.sliding_window_view(pad, W).min(1)[:n + H + P]              # [u]: j = u - P, window from j - H - 1


def _curve(r, w, H, P):
    """s from r, in r's own precision: every operation a separate numpy operation, hence one rounding each."""
    n = len(r)
    one = r.dtype.type(1)
    m = _hold(r, H, P)
    j = np.arange(-P, n + H)
    d = np.where((j >= 0) & (j < n), one - m, r.dtype.type(0)).astype(r.dtype)
    A = np.zeros(n, r.dtype)
    for kk in range(P + H + 1):                                       # ascending k = kk - P; d[i + k] sits at index i + kk
        A = A + w[kk] * d[kk:kk + n]
    rp = np.concatenate([[one], r, [one]])
    return np.fmin(one - A, np.fmin(rp[:-2], np.fmin(rp[1:-1], rp[2:])))


def limit64(x, g, c, H, P, taps64=None):
    x = np.asarray(x, np.float64)
    e = envelope64(x, taps64)
    with np.errstate(divide="ignore"):
        r = np.minimum(1.0, float(c) / (e * float(g)))
    s = _curve(r, window64(H, P), H, P)
    return dict(e=e, r=r, curve=s, out=x * float(g) * s)


def pcm16(v):
    """bv2_loudness_apply's 16-bit rule on fp32 values."""
    v = np.asarray(v, np.float32)
    return np.trunc(np.clip(v * np.float32(32767.0), np.float32(-32768.0), np.float32(32767.0))).astype(np.int16)


def limit32(x, e, g, c, H, P, w32):
    """``x`` fp32 (int16 input: x / 32768, exact), ``e`` fp32 [n], ``g`` and ``c`` fp32 scalars, ``w32`` the fp32 window."""
    x, e, w32 = np.asarray(x, np.float32), np.asarray(e, np.float32), np.asarray(w32, np.float32)
    g, c = np.float32(g), np.float32(c)
    with np.errstate(divide="ignore"):
        r = np.fmin(np.float32(1), c / (e * g))
    s = _curve(r, w32, H, P)
    assert r.dtype == np.float32 and s.dtype == np.float32
    out = (x * g) * s
    return dict(r=r, curve=s, out=out, out16=pcm16(out), min_gain=np.float32(s.min()) if len(s) else np.float32(1),
                limited_samples=int((s < 1).sum()))


def curve_bound(x, g, c, H, P, taps32=None):
    """|device curve - fp64 curve|, derived.  The device's envelope differs from the oracle's by at most be = R.true_peak_bound (0 for
    F = 1: |x| is exact).  Wherever r < 1, |dr/de| = c / (e^2 g) = r^2 g / c <= g / c, and min(1, .) is 1-Lipschitz: |dr| <= be g / c,
    plus the roundings of e g and of the division, 2 U (r <= 1).  Hold and fmin do not amplify an error.  d = 1 - m: one rounding, U.
    The FIR: its weights sum to 1, so the error of d passes through unamplified, and P + H + 1 additions of partial sums <= 1 plus the
    rounding of the window add (P + H + 2) U.  1 - A: one more, U."""
    be = R.true_peak_bound(x, taps32) if taps32 is not None else 0.0
    return be * float(g) / float(c) + (2 + 1 + (P + H + 2) + 1) * U


def out_bound(x, g, c, H, P, taps32=None):
    """out = (x g) s: the curve's error times |x g|, and two more roundings of a value <= |x g|."""
    v = float(np.max(np.abs(np.asarray(x, np.float64)))) * float(g) if len(x) else 0.0
    return v * (curve_bound(x, g, c, H, P, taps32) + 2 * U)


SAMPLE_BOUND = 1.0 + 3 * U            # |out| <= c SAMPLE_BOUND, include/bv2.h "sample peak"


def crest_signal(n, crests, seed=0, level=0.25, dtype="float32"):
    """Uniform noise at ``level`` with crests planted: ``crests`` = ((index, factor), ...), the sample becomes +-factor * level."""
    rng = np.random.RandomState(7919 * seed + n)
    x = rng.uniform(-level, level, n)
    for i, (at, f) in enumerate(crests):
        if 0 <= at < n:
            x[at] = f * level * (1 if i % 2 == 0 else -1)
    if dtype == "int16":
        return np.round(np.clip(x, -1, 32767 / 32768) * 32768).astype(np.int16)
    return x.astype(np.float32)


# ---- the cases of tests/test_limiter_gpu.py (tests/test_limiter_cpu.py verifies them in numpy) ------------------------------------------
TILE = 1024                                                          # lib.LIMITER_TILE
GPU_TIMES = {8000: (3.0, 60.0), 44100: (3.0, 60.0), 96000: (3.0, 60.0)}   # H, P = 12, 240 (the reach inside a tile); 66, 1323 (beyond one); 144, 2880
GPU_FACTOR = {8000: 4, 44100: 4, 96000: 2}
MIN_LOOKAHEAD = (0.0, 60.0)                                          # H = 1
LONE = ((700, 6),)                                                   # one crest in tile 0 of a long item: the other tiles pass through


def lengths(H):
    return (1, 2, H, 2 * H + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 17)


def crests(n, P):
    """(index, factor over the noise level 0.25): the item's first and last sample, either side of a tile boundary, two crests P apart."""
    return ((0, 6), (n - 1, 5), (TILE - 1, 4), (TILE, 8), (100, 7), (100 + P, 5))


def as_f32(x):
    x = np.asarray(x)
    return x.astype(np.float32) / np.float32(32768.0) if x.dtype == np.int16 else x.astype(np.float32)


def voiced_bursts(seconds=3.0, rate=44100, seed=3):
    """A synthetic voiced signal with plosive-like bursts (fp32, peak about 0.7): a 140 Hz harmonic stack under a syllable envelope at
    an RMS of 0.1, and every 370 ms a 2 ms burst of amplitude 0.5 on top — a crest factor that makes a -1 dBTP ceiling bind at -16 LUFS:
    the static path lands 5.4 LU low, the limiter with one make-up pass within 0.05 LU (tests/test_limiter_cpu.py holds both)."""
    n = int(seconds * rate)
    t = np.arange(n) / rate
    rng = np.random.RandomState(seed)
    voice = sum(np.sin(2 * np.pi * 140.0 * h * t + h) / h for h in range(1, 9))
    voice *= 0.5 + 0.5 * np.sin(2 * np.pi * 3.1 * t) ** 2
    voice *= 0.1 / np.sqrt(np.mean(voice ** 2))
    x = voice.copy()
    blen = int(0.002 * rate)
    for at in range(int(0.11 * rate), n - blen, int(0.37 * rate)):
        x[at:at + blen] += 0.5 * np.hanning(blen) * np.sign(rng.uniform(-1, 1, blen))
    return x.astype(np.float32)
