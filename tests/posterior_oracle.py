"""Host-side oracles of the forced-alignment kernels (kernels/align.hip), written from their description, numpy only.

``maximum_path``       fp32 restatement of the monotonic-alignment dynamic programme: for item b with t_x symbols and t_y frames, rows y in
                       sequence, inside the band ``max(0, t_x + y - t_y) <= x < min(t_x, y + 1)``
                           v_cur  = -1e9 if x == y else value[y - 1, x]
                           v_prev = (0 if y == 0 else -1e9) if x == 0 else value[y - 1, x - 1]
                           value[y, x] += max(v_prev, v_cur)                 (fp32 add, fp32 max)
                       then from (t_y - 1, t_x - 1) back to row 0: mark (y, index); step to ``index - 1`` only when ``index != 0`` and
                       (``index == y`` or the left predecessor ``value[y - 1, index - 1]`` is STRICTLY greater than ``value[y - 1, index]``).
                       Returns durations [B, T] int64, the one-hot path [B, Ty, T] fp32 and the score [B] fp32 (the cumulative value of
                       the last cell).  The input is not modified.  ``dtype=np.float64`` runs the same programme in fp64 (the optimum
                       of a matrix up to fp64 round-off, for optimality checks).
``brute_force_path``   every monotone path of a small matrix enumerated; the best score in fp64 and the set of optimal paths.
``neg_cent_f64``       the negative cross-entropy matrix straight from its definition, in fp64.
``path_score``         the fp64 sum of a matrix's cells along a path given by durations.
"""
from __future__ import annotations

import itertools

import numpy as np

NEG = np.float32(-1e9)


def maximum_path(neg_cent, x_lengths, y_lengths, dtype=np.float32):
    neg_cent = np.asarray(neg_cent, dtype=dtype)
    B, Ty, T = neg_cent.shape
    durations = np.zeros((B, T), dtype=np.int64)
    attn = np.zeros((B, Ty, T), dtype=np.float32)
    score = np.zeros((B,), dtype=dtype)
    for b in range(B):
        t_x, t_y = int(x_lengths[b]), int(y_lengths[b])
        if t_x <= 0 or t_y <= 0:
            continue
        assert t_x <= t_y <= Ty and t_x <= T, "the band is empty when x_lengths > y_lengths"
        value = neg_cent[b].copy()
        for y in range(t_y):
            lo, hi = max(0, t_x + y - t_y), min(t_x, y + 1)
            if hi <= lo:
                continue
            x = np.arange(lo, hi)
            if y == 0:
                v_cur = np.full(x.shape, NEG, dtype=dtype)               # x == y == 0
                v_prev = np.zeros(x.shape, dtype=dtype)
            else:
                v_cur = np.where(x == y, NEG, value[y - 1, np.minimum(x, T - 1)]).astype(dtype)
                v_prev = np.where(x == 0, NEG, value[y - 1, np.maximum(x - 1, 0)]).astype(dtype)
            value[y, lo:hi] = value[y, lo:hi] + np.maximum(v_prev, v_cur)     # fp32 + fp32 -> fp32
        index = t_x - 1
        score[b] = value[t_y - 1, index]
        for y in range(t_y - 1, -1, -1):
            attn[b, y, index] = 1.0
            durations[b, index] += 1
            if index != 0 and (index == y or value[y - 1, index] < value[y - 1, index - 1]):
                index -= 1
    return durations, attn, score


def path_from_durations(d, Ty, T):
    """[Ty, T] one-hot matrix of the path that gives symbol x ``d[x]`` consecutive frames."""
    p = np.zeros((Ty, T), dtype=np.float32)
    y = 0
    for x, n in enumerate(d):
        p[y:y + int(n), x] = 1.0
        y += int(n)
    return p


def path_score(matrix, d):
    """fp64 sum of ``matrix`` [Ty, T] along the path of durations ``d``."""
    m = np.asarray(matrix, dtype=np.float64)
    y, s = 0, 0.0
    for x, n in enumerate(d):
        s += float(m[y:y + int(n), x].sum())
        y += int(n)
    return s


def brute_force_path(matrix, t_x, t_y):
    """All monotone paths (every symbol >= 1 frame, frames sum to t_y): (best fp64 score, list of optimal duration tuples)."""
    m = np.asarray(matrix, dtype=np.float64)
    best, arg = None, []
    for cuts in itertools.combinations(range(1, t_y), t_x - 1):
        edges = (0,) + cuts + (t_y,)
        d = tuple(edges[i + 1] - edges[i] for i in range(t_x))
        s = path_score(m, d)
        if best is None or s > best:
            best, arg = s, [d]
        elif s == best:
            arg.append(d)
    return best, arg


def neg_cent_f64(z_p, m_p, logs_p, x_lengths=None, y_lengths=None):
    """sum_d [-1/2 log 2pi - logs_p[d, x] - 1/2 (z_p[d, y] - m_p[d, x])^2 exp(-2 logs_p[d, x])] -> [B, Ty, T] fp64; 0 outside the lengths."""
    z = np.asarray(z_p, dtype=np.float64)
    m = np.asarray(m_p, dtype=np.float64)
    ls = np.asarray(logs_p, dtype=np.float64)
    B, D, Ty = z.shape
    T = m.shape[2]
    out = np.zeros((B, Ty, T), dtype=np.float64)
    for b in range(B):
        diff = z[b][:, :, None] - m[b][:, None, :]                            # [D, Ty, T]
        out[b] = (-0.5 * np.log(2 * np.pi) - ls[b][:, None, :] - 0.5 * diff * diff * np.exp(-2 * ls[b])[:, None, :]).sum(0)
        if x_lengths is not None:
            out[b, :, int(x_lengths[b]):] = 0
        if y_lengths is not None:
            out[b, int(y_lengths[b]):, :] = 0
    return out
