"""ITU-R BS.1770-4 loudness (mono) as include/bv2.h defines it, in numpy fp64 with a plain sample loop — the reference the device meter
(kernels/loudness.hip) is held to.  numpy only.

``measure(items, rate)`` takes the items of ONE group (1-D arrays, fp32 / fp64 in [-1, 1] or int16 read as x / 32768) and returns a dict:
``block_ms`` (one fp64 array per item), ``lufs``, ``silent``, ``peak`` (the group's sample peak), ``margins`` (per item, per block: the
distance in LU of the block's loudness to the absolute threshold and to the relative one; inf where a threshold or a block's loudness
does not exist) and ``gain(target, ceiling_db) -> (gain fp32, limited)``.
"""
import math

import numpy as np

BS1770_48K = {  # ITU-R BS.1770-4, tables 1 and 2 (48 kHz)
    "b": (1.53512485958697, -2.69169618940638, 1.19839281085285),
    "a1": (-1.69065929318241, 0.73248077421585),
    "a2": (-1.99004745483398, 0.99007225036621),
}
ABS_GATE = -70.0


def coeffs(rate):
    """b0 b1 b2 a1 a2 of the high shelf, then of the high pass (a0 = 1): the bilinear forms of the header."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    s1 = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0,
          (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / rate)
    a0 = 1.0 + K / Q + K * K
    s2 = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array(s1 + s2, np.float64)


def plan(rate):
    step = int(math.floor(rate / 10.0 + 0.5))
    return step, 4 * step


def n_blocks(n, rate):
    step, block = plan(rate)
    return 0 if n <= 0 else (1 if n < block else (n - block) // step + 1)


def as_float64(x):
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.float64) / 32768.0
    return x.astype(np.float64)


def k_weight(x, rate):
    """Both biquads in direct form I, one sample after another, in Python floats (IEEE fp64)."""
    b0, b1, b2, a1, a2, c0, c1, c2, d1, d2 = [float(v) for v in coeffs(rate)]
    xs = as_float64(x).tolist()
    out = [0.0] * len(xs)
    x1 = x2 = y1 = y2 = 0.0          # stage 1 history
    u1 = u2 = v1 = v2 = 0.0          # stage 2 history (input u = stage 1's output, output v)
    for i, xv in enumerate(xs):
        y = b0 * xv + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        x2, x1, y2, y1 = x1, xv, y1, y
        v = c0 * y + c1 * u1 + c2 * u2 - d1 * v1 - d2 * v2
        u2, u1, v2, v1 = u1, y, v1, v
        out[i] = v
    return np.array(out, np.float64)


def block_mean_squares(x, rate):
    y = k_weight(x, rate)
    n = len(y)
    step, block = plan(rate)
    if n == 0:
        return np.zeros(0, np.float64)
    if n < block:
        return np.array([np.sum(y * y) / n], np.float64)
    sq = y * y
    return np.array([np.sum(sq[j * step:j * step + block]) / block for j in range((n - block) // step + 1)], np.float64)


def _lk(ms):
    return -0.691 + 10.0 * math.log10(ms) if ms > 0 else -math.inf


def gate(block_ms_items, peak):
    """The gating of one group from its items' block mean squares."""
    allms = np.concatenate([np.asarray(b, np.float64) for b in block_ms_items]) if block_ms_items else np.zeros(0)
    l = np.array([_lk(v) for v in allms])
    keep = l > ABS_GATE
    res = {"block_ms": [np.asarray(b, np.float64) for b in block_ms_items], "peak": float(peak)}
    if not keep.any():
        rel = None
        res.update(lufs=-math.inf, silent=True)
    else:
        rel = _lk(float(np.mean(allms[keep]))) - 10.0
        keep2 = keep & (l > rel)
        res.update(lufs=_lk(float(np.mean(allms[keep2]))), silent=False)
    margins, o = [], 0
    for b in block_ms_items:
        lb = l[o:o + len(b)]
        o += len(b)
        margins.append(np.stack([np.abs(lb - ABS_GATE), np.abs(lb - rel) if rel is not None else np.full(len(lb), np.inf)], 1))
    res["margins"] = margins
    res["rel_threshold"] = rel

    def gain(target, ceiling_db):
        if res["silent"]:
            return np.float32(1.0), False
        g = 10.0 ** ((target - res["lufs"]) / 20.0)
        ceil = 10.0 ** (ceiling_db / 20.0)
        if res["peak"] * g > ceil:
            return np.float32(ceil / res["peak"]), True
        return np.float32(g), False

    res["gain"] = gain
    return res


def measure(items, rate):
    items = [np.asarray(x) for x in items]
    peak = max([float(np.max(np.abs(as_float64(x)))) if len(x) else 0.0 for x in items] + [0.0])
    return gate([block_mean_squares(x, rate) for x in items], peak)


def min_margin(res):
    """The smallest distance of any block to a threshold that exists (LU)."""
    m = [float(np.min(v)) for v in res["margins"] if v.size]
    return min(m) if m else math.inf


def apply_f32(x, gain):
    """out = x * gain, one fp32 multiply (int16 input read as x / 32768 in fp32: exact)."""
    x = np.asarray(x)
    xf = x.astype(np.float32) / np.float32(32768.0) if x.dtype == np.int16 else x.astype(np.float32)
    return xf * np.float32(gain)


def apply_i16(x, gain):
    """trunc(clamp(v * 32767.0f, -32768, 32767)) of the fp32 product v: every step rounded to fp32, nothing fused."""
    v = apply_f32(x, gain)
    w = (v * np.float32(32767.0)).astype(np.float32)
    return np.trunc(np.clip(w, np.float32(-32768.0), np.float32(32767.0))).astype(np.int16)
