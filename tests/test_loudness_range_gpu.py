"""GPU: step energies, short-term loudness and loudness range (bv2_loudness_steps / bv2_loudness_range, kernels/loudness.hip;
``audio.loudness(want_range=True)``) against the numpy oracle (tests/r128_oracle.py).

Bars.  Step energies: 1e-10 relative, what the block energies are held to (README, loudness); four of them against ``block_ms``: the
header promises the same bits, the bar of the issue is 1e-14 relative — both are asserted.  LUFS figures 2e-11 LU (the meter's bar), the
range 4e-11 LU (a difference of two).  The percentile selection is exact, so a gated result is compared only where the oracle puts every
short-term value at least 1e-6 LU from both thresholds — asserted for every case.  The stepped tones of Tech 3342 read their analytic
range within +-1 LU."""
import functools
import math

import numpy as np
import pytest
import torch

from bert_vits2_amd import audio, lib as L
from tests import loudness_oracle as O
from tests import r128_oracle as R

pytestmark = pytest.mark.gpu

BAR_STEP = 1e-10
BAR_BLOCK = 1e-14
BAR_LUFS = 2e-11
BAR_LRA = 4e-11
RATE = 8000
FIGURES = ("st_low", "st_high", "max_short_term", "max_momentary")


def noise44(n, seed):
    rng = np.random.RandomState(seed)
    return (0.3 * rng.uniform(-1.0, 1.0, n) * (0.2 + np.abs(np.sin(np.arange(n) / 9000.0))) + 0.05).astype(np.float32)


@functools.lru_cache(maxsize=None)
def items(name):
    if name == "8k":                                       # 6 s, 2.9 s and a bit, shorter than a block
        return RATE, (R.envelope_noise(0), R.envelope_noise(1, 2.9)[:-3], R.envelope_noise(3, 0.35))
    if name == "44k":                                      # more than three tiles, a last step that must not count
        step, block, tile = audio.loudness_plan(44100)
        return 44100, (noise44(3 * tile + step + 7, 5), noise44(block, 6))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle_steps(name):
    rate, xs = items(name)
    return tuple(R.step_energies(x, rate) for x in xs)


def batch(xs, order=None, extra=0):
    order = list(range(len(xs))) if order is None else order
    S = max(len(x) for x in xs) + extra
    w = np.full((len(order), S), np.nan, np.float32)
    for r, i in enumerate(order):
        w[r, :len(xs[i])] = xs[i]
    return torch.from_numpy(w).cuda(), torch.tensor([len(xs[i]) for i in order]).cuda()


# ---- step energies -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["8k", "44k"])
def test_step_energies(name):
    rate, xs = items(name)
    step, block, _ = audio.loudness_plan(rate)
    w, wl = batch(xs)
    got = audio.loudness_steps(w, wl, rate, want_blocks=True)
    plain = audio.loudness_measure(w, wl, rate, gate=False)
    assert torch.equal(got["block_ms"], plain["block_ms"]) and torch.equal(got["peak"], plain["peak"])
    only = audio.loudness_steps(w, wl, rate)
    assert set(only) == {"step_ss"} and torch.equal(only["step_ss"], got["step_ss"])
    ss, ms = got["step_ss"].cpu().numpy(), got["block_ms"].cpu().numpy()
    assert ss.shape == (len(xs), audio.loudness_steps_count(rate, w.shape[1])) and not np.isnan(ss).any()
    worst = worst_b = 0.0
    for b, (x, ref) in enumerate(zip(xs, oracle_steps(name))):
        n = len(x) // step
        assert len(ref) == n and np.all(ss[b, n:] == 0)
        worst = max(worst, float(np.max(np.abs(ss[b, :n] - ref) / ref)))
        if len(x) >= block:
            e = ss[b]
            four = np.array([(((e[j] + e[j + 1]) + e[j + 2]) + e[j + 3]) / block for j in range(n - 3)])
            assert len(four) == O.n_blocks(len(x), rate)
            worst_b = max(worst_b, float(np.max(np.abs(four - ms[b, :n - 3]) / ms[b, :n - 3])))
            assert np.array_equal(four, ms[b, :n - 3]), (name, b)          # the same expression: the same bits
    print(f"{name}: step_ss {worst:.3e} relative to the oracle (bar {BAR_STEP:.0e}); four steps against block_ms {worst_b:.3e} (bar {BAR_BLOCK:.0e})")
    assert worst <= BAR_STEP and worst_b <= BAR_BLOCK
    # an item's steps are the same bits alone and at any row, under a larger S
    w2, wl2 = batch(xs, list(range(len(xs)))[::-1], 4099)
    ss2 = audio.loudness_steps(w2, wl2, rate)["step_ss"]
    for r, i in enumerate(list(range(len(xs)))[::-1]):
        n = len(xs[i]) // step
        assert torch.equal(ss2[r, :n], got["step_ss"][i, :n]) and not ss2[r, n:].any()
        alone = audio.loudness_steps(torch.from_numpy(xs[i])[None].cuda(), None, rate)["step_ss"]
        assert alone.shape[1] == n and torch.equal(alone[0], got["step_ss"][i, :n])


# ---- range ---------------------------------------------------------------------------------------------------------------------------------
def check(got, g, ref, tag):
    assert ref["margin"] >= R.MARGIN, (tag, ref["margin"])
    d = {k: abs(float(got[k][g]) - ref[k]) for k in FIGURES}
    d["lra"] = abs(float(got["lra"][g]) - ref["lra"])
    print(f"{tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()) + f" LU; LRA {ref['lra']:.4f}, {ref['n_kept']} of {ref['n_blocks']} blocks")
    assert not bool(got["range_short"][g]) and not bool(got["silent"][g])
    assert all(d[k] <= BAR_LUFS for k in FIGURES) and d["lra"] <= BAR_LRA, (tag, d)


@pytest.mark.parametrize("seed", [0, 1, 3])
def test_range_of_noise_against_the_oracle(seed):
    x = R.envelope_noise(seed)
    ref = R.loudness_range([R.step_energies(x, RATE)], RATE)
    got = audio.loudness(torch.from_numpy(x), None, RATE, want_range=True, want_blocks=True)
    check(got, 0, ref, f"seed {seed}")
    plain = audio.loudness(torch.from_numpy(x), None, RATE, want_blocks=True)      # the integrated figures do not depend on the path
    assert torch.equal(got["lufs"], plain["lufs"]) and torch.equal(got["block_ms"], plain["block_ms"]) and torch.equal(got["peak"], plain["peak"])
    assert set(got) - set(plain) == {"lra", "st_low", "st_high", "max_short_term", "max_momentary", "range_short"}


@pytest.mark.parametrize("name", sorted(R.RANGE_CASES))
def test_range_of_stepped_tones(name):
    levels, seconds, want = R.RANGE_CASES[name]
    x = R.level_tone(levels, seconds).astype(np.float32)
    got = audio.loudness(torch.from_numpy(x), None, RATE, want_range=True)
    ref = R.loudness_range([R.step_energies(x, RATE)], RATE)
    assert ref["margin"] >= R.MARGIN
    lra = float(got["lra"][0])
    print(f"{name}: LRA {lra:.6f} LU (analytic {want}, oracle {ref['lra']:.6f}, difference {abs(lra - ref['lra']):.2e}); "
          f"max short-term {float(got['max_short_term'][0]):.4f}, max momentary {float(got['max_momentary'][0]):.4f} LUFS")
    assert abs(lra - want) <= R.LRA_TOLERANCE and abs(ref["lra"] - want) <= R.LRA_TOLERANCE
    assert not bool(got["range_short"][0]) and not bool(got["silent"][0])
    assert abs(float(got["st_high"][0]) - float(got["st_low"][0]) - lra) <= 1e-9
    assert float(got["max_momentary"][0]) >= float(got["max_short_term"][0]) - 1e-9 >= float(got["st_high"][0]) - 2e-9


def test_short_and_silent_items_are_flagged():
    xs = (R.envelope_noise(0, 2.9), np.zeros(4 * RATE, np.float32), R.envelope_noise(1))
    w, wl = batch(xs)
    got = audio.loudness(w, wl, RATE, want_range=True)
    assert got["range_short"].tolist() == [True, False, False] and got["silent"].tolist() == [False, True, False]
    st = audio.loudness_steps(w, wl, RATE)["step_ss"]
    raw = audio.loudness_range(st, wl, w.shape[1], RATE)
    assert raw["flags"].tolist() == [L.RANGE_SHORT, L.RANGE_SILENT, 0]
    for g in (0, 1):
        assert float(got["lra"][g]) == 0.0 and all(float(got[k][g]) == -math.inf for k in FIGURES)
    check(got, 2, R.loudness_range([R.step_energies(xs[2], RATE)], RATE), "beside a short and a silent item")


def test_a_group_pools_its_short_term_blocks_whatever_the_rows():
    xs = (R.envelope_noise(0), (R.envelope_noise(1, 4.0) * np.float32(0.03)).astype(np.float32), R.envelope_noise(3, 5.05),
          R.envelope_noise(4), (R.envelope_noise(5, 1.25) * np.float32(3.0)).astype(np.float32))
    steps = [R.step_energies(x, RATE) for x in xs]
    pooled = R.loudness_range([steps[0], steps[1], steps[2], steps[4]], RATE)
    assert 0 < pooled["n_kept"] < pooled["n_blocks"]                          # the relative gate removes the quiet piece's blocks
    # the 1.25 s piece has no short-term block, but its 400 ms blocks count: the group's maximum momentary loudness is its own
    assert pooled["max_momentary"] > R.loudness_range(steps[:3], RATE)["max_momentary"] + 1.0
    alone = R.loudness_range([steps[3]], RATE)
    for order, groups in (([0, 1, 2, 3, 4], [0, 0, 0, 1, 0]), ([2, 3, 1, 4, 0], [0, 1, 0, 0, 0]), ([3, 4, 0, 2, 1], [1, 0, 0, 0, 0])):
        w, wl = batch(xs, order)
        got = audio.loudness(w, wl, RATE, groups=groups, want_range=True)
        assert got["lra"].shape == (2,)
        check(got, 0, pooled, f"pooled, rows {order}")
        check(got, 1, alone, f"alone, rows {order}")
    assert abs(pooled["lra"] - R.loudness_range([steps[0]], RATE)["lra"]) > 1e-3      # pooling is not a no-op on these items
