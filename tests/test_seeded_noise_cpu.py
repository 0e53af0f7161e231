"""CPU: the seeded-noise generator (csrc/kernels/rng.h) on the host — Philox4x32-10 against published known answers, the host
instantiation of the N(0,1) value against the numpy restatement (tests/seeded_noise_ref.py), that restatement's own statistics, and the
parts of the new ABI that need no device (exports, argument checks, ``Utterance(seed=...)``)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from bert_vits2_amd import lib as L, serving, synth
from tests import seeded_noise_ref as R

# Random123's known-answer vectors for philox4x32_10: (counter, key, output)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
SEEDS = [0, 1, -1, 2 ** 63 - 1, 0x9E3779B97F4A7C15 - 2 ** 64]       # the last: the golden-ratio constant's bit pattern as int64
BOUND = 4e-6                                                         # the bar of the GPU fill test (test_seeded_noise_gpu.py)


@pytest.fixture(scope="module")
def lib():
    lib = L.load()
    lib.bv2_test_philox4x32_10.argtypes = [C.POINTER(C.c_uint32)] * 3
    lib.bv2_test_philox4x32_10.restype = None
    lib.bv2_test_seeded_normal.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int]
    lib.bv2_test_seeded_normal.restype = C.c_float
    return lib


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(lib, ctr, key, want):
    out = (C.c_uint32 * 4)()
    lib.bv2_test_philox4x32_10((C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), out)
    assert tuple(out) == want, [hex(v) for v in out]
    assert tuple(R.philox4x32_10_py(ctr, key)) == want
    assert tuple(int(v) for v in R.philox4x32_10(ctr, key)) == want


def test_host_normal_matches_the_fp64_helper(lib):
    rows = list(range(8)) + list(range(188, 192))
    ts = [0, 1, 255, 256, 65535]
    worst = 0.0
    for seed in SEEDS:
        for which in range(3):
            ref = R.seeded_normal(seed, which, np.array(rows)[:, None], np.array(ts)[None, :])
            assert np.abs(ref).max() <= np.sqrt(48 * np.log(2)) + 1e-9
            for i, row in enumerate(rows):
                for j, t in enumerate(ts):
                    d = abs(lib.bv2_test_seeded_normal(seed, which, row, t) - ref[i, j])
                    worst = max(worst, d)
                    assert d <= BOUND, (seed, which, row, t, d)
    print(f"host instantiation vs fp64 helper: max |diff| = {worst:.3e}")


def _corr(a, b):
    return float(np.mean(a * b))                       # both are N(0,1) samples: the lag product's mean is the correlation


@pytest.mark.parametrize("seed", [0, 12345, -1])
def test_helper_statistics(seed):
    """N = 2^20 values of one seed as [rows = 256, T = 4096]: mean, variance and the four lag-1 correlations inside 5 sigma."""
    rows, T = 256, 4096
    N = rows * T
    v = R.seeded_normal(seed, 1, np.arange(rows)[:, None], np.arange(T)[None, :])
    tol = 5 / np.sqrt(N)
    assert abs(v.mean()) <= tol, v.mean()
    assert abs(v.var() - 1) <= 5 * np.sqrt(2 / N), v.var()
    assert abs(_corr(v[:, :-1], v[:, 1:])) <= tol                                 # along t
    assert abs(_corr(v[:-1], v[1:])) <= tol                                       # along rows
    w = R.seeded_normal(seed, 2, np.arange(rows)[:, None], np.arange(T)[None, :])
    assert abs(_corr(v, w)) <= tol                                                  # across which
    nxt = int(np.array(seed, dtype=np.int64) + np.int64(1))
    s1 = R.seeded_normal(nxt, 1, np.arange(rows)[:, None], np.arange(T)[None, :])
    assert abs(_corr(v, s1)) <= tol                                                 # across seeds s and s + 1


def test_abi_exports_and_version(lib):
    for name in ("bv2_set_noise_seeds", "bv2_seeded_noise", "bv2_test_philox4x32_10", "bv2_test_seeded_normal"):
        assert hasattr(lib, name), name
    declared = {s[0] for s in L.SYMBOLS}
    assert {"bv2_set_noise_seeds", "bv2_seeded_noise"} <= declared
    assert lib.bv2_abi_version() == 3


def test_seeded_noise_argument_checks(lib):
    """Every argument is checked before anything touches the device: the pointers below are never dereferenced."""
    p = C.c_void_p(256)
    ok = dict(seeds=p, B=1, which=0, rows=2, T=4, out=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.bv2_seeded_noise(None, a["seeds"], a["B"], a["which"], a["rows"], a["T"], None, a["out"], 8, 4, 1)

    for kw, word in ((dict(B=0), b"B"), (dict(B=-3), b"B"), (dict(which=-1), b"which"), (dict(which=3), b"which"),
                     (dict(rows=0), b"rows"), (dict(out=None), b"out"), (dict(seeds=None), b"seeds"), (dict(T=0), b"T")):
        assert call(**kw) != 0, kw
        msg = lib.bv2_last_error(None)
        assert b"bv2_seeded_noise" in msg and word in msg, (kw, msg)


def test_set_noise_seeds_needs_a_handle_and_a_count(lib):
    from bert_vits2_amd import hparams as H
    assert lib.bv2_set_noise_seeds(None, C.c_void_p(256), 1) != 0
    h = C.c_void_p()
    assert lib.bv2_create(C.byref(L.make_config(H.default_v23())), C.byref(h)) == 0
    try:
        assert lib.bv2_set_noise_seeds(h, C.c_void_p(256), 0) != 0 and b"bv2_set_noise_seeds" in lib.bv2_last_error(h)
        assert lib.bv2_set_noise_seeds(h, C.c_void_p(256), 3) == 0
        assert lib.bv2_set_noise_seeds(h, None, 0) == 0
    finally:
        lib.bv2_destroy(h)


def _utt(**kw):
    b = synth.synthetic_batch([5], languages=[0], sids=[1])
    return serving.Utterance(b["x"][0], b["tone"][0], b["language"][0], b["bert"][0], b["ja_bert"][0], b["en_bert"][0], 1, **kw)


def test_utterance_seed_validation_and_fields():
    assert [f.name for f in dataclasses.fields(serving.Utterance)] == [
        "phones", "tones", "lang_ids", "bert", "ja_bert", "en_bert", "sid", "sdp_ratio", "noise_scale", "noise_scale_w", "length_scale",
        "g", "ref_spec"]
    assert _utt().seed is None
    for s in (0, -1, 2 ** 63 - 1, -2 ** 63, np.int64(7)):
        u = _utt(seed=s)
        assert u.seed == int(s) and type(u.seed) is int
    for bad in (2 ** 63, -2 ** 63 - 1, 1.5, "7", True, torch.tensor(3)):
        with pytest.raises(ValueError, match="seed"):
            _utt(seed=bad)


def test_item_seeds_forms():
    from bert_vits2_amd import models
    assert models.item_seeds(None, 3, "cpu") is None
    assert models.item_seeds(7, 3, "cpu").tolist() == [7, 7, 7]
    assert models.item_seeds([1, -1, 2 ** 63 - 1], 3, "cpu").tolist() == [1, -1, 2 ** 63 - 1]
    t = torch.tensor([4, 5], dtype=torch.int64)
    assert models.item_seeds(t, 2, "cpu").tolist() == [4, 5]
    for bad in ([1, 2], torch.tensor([1, 2, 3], dtype=torch.int32), [2 ** 63, 0, 0], torch.zeros(3, 1, dtype=torch.int64)):
        with pytest.raises(ValueError, match="seeds"):
            models.item_seeds(bad, 3, "cpu")
