"""The rest of an EBU R128 delivery sheet as include/bv2.h defines it, in numpy fp64 — the reference the device kernels
(kernels/truepeak.hip, the step / range kernels of kernels/loudness.hip) are held to.  numpy only; the K-weighting is
tests/loudness_oracle.py's.

True peak (``true_peak``): the larger of the sample peak and the peak of the F-times interpolated signal, interpolated with the fp64
table the caller passes (``bv2_resample_taps_f64`` at rate -> F rate): y[i F + p] = sum_jj x[i + jj - K] T[p][jj], x = 0 outside the item.
Loudness range (``loudness_range``, EBU Tech 3342): step energies -> 3 s short-term blocks every 100 ms -> the -70 LUFS gate, the gate
20 LU under the mean of what passed, the 10th and 95th percentile by a plain sort.
"""
import math

import numpy as np

from tests import loudness_oracle as O

ST_STEPS = 30
ABS_GATE = -70.0
REL_GATE = -20.0


# ---- true peak -----------------------------------------------------------------------------------------------------------------------
def factor(rate):
    return 4 if rate < 96000 else (2 if rate < 192000 else 1)


def oversample(x, taps):
    """[F, n]: row p holds the outputs i F + p.  ``taps`` [F, 2K + 1] in fp64 (or the fp32 table, widened)."""
    x = O.as_float64(x)
    taps = np.asarray(taps, np.float64)
    K = (taps.shape[1] - 1) // 2
    xp = np.concatenate([np.zeros(K), x, np.zeros(K)])
    return np.stack([np.correlate(xp, t, mode="valid") for t in taps])


def true_peak(x, taps=None):
    """``taps`` None: F = 1, the sample peak."""
    x = O.as_float64(x)
    if len(x) == 0:
        return 0.0
    peak = float(np.max(np.abs(x)))
    if taps is None:
        return peak
    return max(peak, float(np.max(np.abs(oversample(x, taps)))))


def true_peak_bound(x, taps32):
    """|device - oracle| of one interpolated output: 2K + 1 products and additions in fp32, each within 2^-24 relative of a partial sum
    that sum_j |T[p][j]| max|x| bounds, plus the fp32 rounding of every tap — (2K + 2) 2^-24 max_p sum_j |T[p][j]| max|x|."""
    t = np.abs(np.asarray(taps32, np.float64))
    K = (t.shape[1] - 1) // 2
    return (2 * K + 2) * 2.0 ** -24 * float(np.max(t.sum(1))) * float(np.max(np.abs(O.as_float64(x))))


def faded_sine(amp, cycles_per_sample, phase_deg, rate=48000, fade=0.1, steady=0.1):
    """A sine under a raised-cosine fade in and out of ``fade`` seconds around ``steady`` seconds at full amplitude: band-limited enough
    that its reconstruction does not overshoot (a sine that starts or stops abruptly reads 0.3 to 0.7 dB high — correctly)."""
    nf, ns = int(round(fade * rate)), int(round(steady * rate))
    n = 2 * nf + ns
    env = np.ones(n)
    ramp = 0.5 - 0.5 * np.cos(np.pi * (np.arange(nf) + 0.5) / nf)
    env[:nf] = ramp
    env[n - nf:] = ramp[::-1]
    return amp * env * np.sin(2 * np.pi * cycles_per_sample * np.arange(n) + math.radians(phase_deg))


# (amplitude, frequency as a fraction of fs, phase in degrees)
SINES = ((0.5, 1 / 4, 0.0), (0.5, 1 / 4, 45.0), (0.5, 1 / 6, 60.0), (0.5, 1 / 8, 67.5), (1.41, 1 / 4, 45.0), (0.5, 1 / 2.5, 10.0))
EBU_TP_WINDOW = (-0.4, 0.2)       # dB around the amplitude, EBU Tech 3341


# ---- step energies, short-term loudness, loudness range -----------------------------------------------------------------------------------
def step_energies(x, rate):
    """Sum of squares of the K-weighted samples of every WHOLE 100 ms step."""
    y = O.k_weight(x, rate)
    step, _ = O.plan(rate)
    sq = y * y
    return np.array([np.sum(sq[k * step:(k + 1) * step]) for k in range(len(y) // step)], np.float64)


def lufs(ms):
    return -0.691 + 10.0 * math.log10(ms) if ms > 0 else -math.inf


def short_term(e, rate):
    step, _ = O.plan(rate)
    return np.array([np.sum(e[j:j + ST_STEPS]) / (ST_STEPS * step) for j in range(max(len(e) - ST_STEPS + 1, 0))], np.float64)


def momentary(e, rate):
    step, block = O.plan(rate)
    return np.array([np.sum(e[j:j + 4]) / block for j in range(max(len(e) - 3, 0))], np.float64)


def percentile_indices(n):
    return ((n - 1) * 10 + 50) // 100, ((n - 1) * 95 + 50) // 100


def loudness_range(step_items, rate):
    """One group from its items' step energies.  ``margin``: the smallest distance (LU) of any short-term value to a threshold that
    exists — fp64 round-off cannot move a block across a gate while it is far above 1e-10."""
    st = np.concatenate([short_term(np.asarray(e, np.float64), rate) for e in step_items]) if len(step_items) else np.zeros(0)
    mo = np.concatenate([momentary(np.asarray(e, np.float64), rate) for e in step_items]) if len(step_items) else np.zeros(0)
    res = dict(lra=0.0, st_low=-math.inf, st_high=-math.inf, max_short_term=-math.inf, max_momentary=-math.inf, short=False, silent=False,
               n_blocks=len(st), n_kept=0, margin=math.inf)
    if len(st) == 0:
        res["short"] = True
        return res
    l = np.array([lufs(v) for v in st])
    keep = l > ABS_GATE
    res["margin"] = float(np.min(np.abs(l - ABS_GATE)))
    if not keep.any():
        res["silent"] = True
        return res
    rel = lufs(float(np.mean(st[keep]))) + REL_GATE
    res["margin"] = min(res["margin"], float(np.min(np.abs(l - rel))))
    r = np.sort(st[keep & (l > rel)])
    lo, hi = percentile_indices(len(r))
    res.update(lra=10.0 * math.log10(r[hi] / r[lo]), st_low=lufs(r[lo]), st_high=lufs(r[hi]), max_short_term=lufs(float(np.max(st))),
               max_momentary=lufs(float(np.max(mo))), n_kept=len(r), rel_threshold=rel)
    return res


def level_tone(levels_dbfs, seconds, rate=8000, f=1000.0):
    """Segments of a 1 kHz sine, one level after another (peak level in dBFS), phase-continuous."""
    n = int(seconds * rate)
    t = np.arange(n * len(levels_dbfs)) / rate
    amp = np.repeat([10.0 ** (v / 20.0) for v in levels_dbfs], n)
    return amp * np.sin(2 * np.pi * f * t)


# (levels in dBFS, seconds per segment, the LRA Tech 3342 expects)
RANGE_CASES = {
    "20_30": ((-20.0, -30.0), 20.0, 10.0),
    "20_15": ((-20.0, -15.0), 20.0, 5.0),
    "40_20": ((-40.0, -20.0), 20.0, 20.0),                      # the relative gate keeps the quiet half
    "five": ((-50.0, -35.0, -20.0, -35.0, -50.0), 20.0, 15.0),
}
LRA_TOLERANCE = 1.0                # LU, EBU Tech 3342
MARGIN = 1e-6                      # LU: the precondition of every case that runs on the device


def envelope_noise(seed, seconds=6.0, rate=8000):
    """White noise under a slowly moving random envelope (fp32): short-term loudness that wanders by several LU."""
    rng = np.random.RandomState(seed)
    n = int(seconds * rate)
    knots = rng.uniform(-30.0, -6.0, int(seconds * 2) + 2)                  # dB, one knot per half second
    env = 10.0 ** (np.interp(np.arange(n) / (rate / 2.0), np.arange(len(knots)), knots) / 20.0)
    return (env * rng.uniform(-1.0, 1.0, n)).astype(np.float32)
