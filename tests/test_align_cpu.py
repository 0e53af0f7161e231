"""CPU: the host side of forced alignment — the C ABI of the two align.hip calls (declared, exported, argument checks that run before
anything touches a device), the numpy restatement of the dynamic programme against a brute-force enumeration of every monotone path
(tie rule included), ``with_durations`` and ``serving.Utterance(durations=...)``."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from bert_vits2_amd import align, hparams as H, lib as L, models, serving, synth
from tests import posterior_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("bv2_neg_cent", "bv2_maximum_path_workspace_bytes", "bv2_maximum_path", "bv2_stage_flow_forward")


def test_alignment_exports_are_declared_and_abi_stays_3():
    """The acceptance test: before this feature the library has no aligner (AttributeError on the first symbol)."""
    hdr = open(os.path.join(ROOT, "include", "bv2.h")).read()
    assert re.search(r"#define BV2_ABI_VERSION 3\b", hdr) and re.search(r"#define BV2_PACK_LAYOUT 16\b", hdr)
    lib = L.load()
    assert lib.bv2_abi_version() == 3
    bound = {s[0] for s in L.SYMBOLS}
    for name in NEW_EXPORTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name + " is not declared in include/bv2.h"
        assert name in bound and getattr(lib, name) is not None
    assert callable(models.with_durations) and callable(align.neg_cent) and callable(align.maximum_path)
    assert hasattr(models.SynthesizerTrn, "align_latent") and hasattr(models.SynthesizerTrn, "stage_flow_forward") and callable(serving.align)


def test_argument_checks_run_before_the_device():
    lib = L.load()
    err = lambda: lib.bv2_last_error(None).decode()
    # workspace: Ty * ceil(T / 64) 64-bit words per item
    assert lib.bv2_maximum_path_workspace_bytes(1, 1, 1) == 8
    assert lib.bv2_maximum_path_workspace_bytes(3, 65, 130) == 3 * 130 * 2 * 8
    assert lib.bv2_maximum_path_workspace_bytes(1, 512, 2584) == 2584 * 8 * 8        # a 30 s recording at hop 512 / 44.1 kHz against 512 symbols
    assert lib.bv2_maximum_path_workspace_bytes(1, 4097, 10) < 0 and "4096" in err()
    assert lib.bv2_maximum_path_workspace_bytes(0, 4, 10) < 0
    one = C.c_void_p(8)            # never dereferenced: every call below fails its checks first
    assert lib.bv2_neg_cent(None, 1, 192, 4, 8, None, one, one, None, None, one) == -1 and "null" in err()
    assert lib.bv2_neg_cent(None, 1, 190, 4, 8, one, one, one, None, None, one) == -1 and "multiple of 4" in err()
    assert lib.bv2_neg_cent(None, 1, 260, 4, 8, one, one, one, None, None, one) == -1 and "256" in err()
    assert lib.bv2_neg_cent(None, 0, 192, 4, 8, one, one, one, None, None, one) == -1
    assert lib.bv2_maximum_path(None, 1, 4, 8, None, None, None, one, None, None, one, 64) == -1 and "null" in err()
    assert lib.bv2_maximum_path(None, 1, 4097, 8, one, None, None, one, None, None, one, 1 << 20) == -1 and "4096" in err()
    assert lib.bv2_maximum_path(None, 1, 4, 8, one, None, None, one, None, None, None, 64) == -1 and "workspace" in err()
    assert lib.bv2_maximum_path(None, 1, 4, 8, one, None, None, one, None, None, C.c_void_p(12), 64) == -1 and "aligned" in err()
    assert lib.bv2_maximum_path(None, 1, 4, 8, one, None, None, one, None, None, one, 63) == -5 and "too small" in err()


def test_python_layer_refuses_host_tensors_and_bad_lengths():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        align.neg_cent(torch.zeros(1, 4, 8), torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        align.maximum_path(torch.zeros(1, 8, 3), [3], [8])
    with pytest.raises(ValueError, match="must not exceed y_lengths"):
        align.check_lengths([5], [4], 8, 8)
    with pytest.raises(ValueError, match="do not fit"):
        align.check_lengths([9], [12], 8, 12)
    with pytest.raises(ValueError, match="do not fit"):
        align.check_lengths([0], [4], 8, 8)
    with pytest.raises(ValueError, match="one entry per batch item"):
        align.check_lengths([1, 2], [4], 8, 8)
    align.check_lengths([4, 1], [4, 8], 8, 8)
    align.check_lengths(np.array([3]), torch.tensor([8]), 8, 8)


def _all_small_shapes():
    return [(tx, ty) for tx in range(1, 5) for ty in range(tx, 8)]


def test_dp_restatement_against_every_monotone_path():
    """T <= 4, Ty <= 7, integer-valued matrices (every sum is exact in fp32 and fp64, ties are frequent with values in [-1, 1]): the
    restatement's score is the brute-force optimum, its path is optimal, and among the optimal paths it is THE one the tie rule
    selects — walking back, the path stays on its symbol whenever staying is optimal (a step to x - 1 needs a strictly greater left
    predecessor), i.e. the reversed duration tuple is lexicographically largest."""
    rng = np.random.RandomState(0)
    ties_seen = 0
    for tx, ty in _all_small_shapes():
        for rep in range(6):
            T, Ty = tx + rep % 2, ty + rep % 3                                 # padded matrices too: cells outside the lengths are not read
            m = rng.randint(-1, 2, size=(1, Ty, T)).astype(np.float32)
            m[0, ty:, :] = 99.0
            m[0, :, tx:] = 99.0
            keep = m.copy()
            d, attn, score = PO.maximum_path(m, [tx], [ty])
            assert np.array_equal(m, keep), "the input is const"
            best, arg = PO.brute_force_path(m[0, :ty, :tx], tx, ty)
            ties_seen += len(arg) > 1
            assert float(score[0]) == best
            assert tuple(d[0, :tx]) in arg and not d[0, tx:].any()
            assert tuple(d[0, :tx]) == max(arg, key=lambda t: t[::-1])
            assert np.array_equal(attn[0, :ty, :tx], PO.path_from_durations(d[0, :tx], ty, tx)) and attn[0].sum() == ty
    assert ties_seen > 20, "the matrices were meant to tie"


def test_dp_restatement_tie_matrix_and_forced_diagonal():
    # all-equal cells: every path ties; the rule gives the LAST symbol every spare frame
    d, attn, score = PO.maximum_path(np.zeros((1, 7, 3), np.float32), [3], [7])
    assert d[0].tolist() == [1, 1, 5] and score[0] == 0
    # t_x == t_y: the band is the diagonal
    m = np.arange(25, dtype=np.float32).reshape(1, 5, 5)
    d, attn, score = PO.maximum_path(m, [5], [5])
    assert d[0].tolist() == [1] * 5 and np.array_equal(attn[0], np.eye(5, dtype=np.float32)) and score[0] == np.trace(m[0])
    # one symbol takes everything
    d, _, score = PO.maximum_path(np.ones((1, 9, 1), np.float32), [1], [9])
    assert d[0].tolist() == [9] and score[0] == 9


def test_dp_restatement_on_random_floats_is_optimal_up_to_roundoff():
    rng = np.random.RandomState(1)
    for tx, ty in _all_small_shapes():
        m = (rng.randn(1, ty, tx) * 30).astype(np.float32)
        d, _, score = PO.maximum_path(m, [tx], [ty])
        best, _ = PO.brute_force_path(m[0], tx, ty)
        tol = 2 * ty * ty * np.abs(m).max() * 2.0 ** -24                       # ty fp32 additions of partial sums <= ty max|m|, two paths compared
        assert abs(PO.path_score(m[0], d[0]) - best) <= tol and abs(float(score[0]) - best) <= tol
        assert d[0].min() >= 1 and d[0].sum() == ty


def test_neg_cent_formula_matches_the_expanded_form():
    """The K = 2 inter product plus two column constants IS the definition (fp64 both ways)."""
    rng = np.random.RandomState(2)
    z, m, ls = rng.randn(2, 8, 5), rng.randn(2, 8, 3), rng.randn(2, 8, 3) * 0.3
    r = np.exp(-2 * ls)
    a = np.concatenate([-0.5 * z * z, z], 1).transpose(0, 2, 1)                # [B, Ty, 2 D]
    b = np.concatenate([r, m * r], 1)                                          # [B, 2 D, T]
    const = (-0.5 * np.log(2 * np.pi) - ls).sum(1) + (-0.5 * m * m * r).sum(1)
    assert np.allclose(a @ b + const[:, None, :], PO.neg_cent_f64(z, m, ls), rtol=1e-12, atol=1e-12)
    out = PO.neg_cent_f64(z, m, ls, [2, 3], [5, 4])
    assert not out[0, :, 2:].any() and not out[1, 4:, :].any() and out[0, :, :2].all()


def test_with_durations_shapes_and_values():
    enc = dict(w_ceil=torch.ones(2, 5), y_lengths=torch.tensor([5, 5]), m_p=torch.zeros(2, 4, 5), x_mask=torch.ones(2, 5))
    d = torch.tensor([[3, 1, 2, 0, 0], [1, 1, 1, 1, 7]])
    out = models.with_durations(enc, d)
    assert out is not enc and enc["w_ceil"].sum() == 10                        # a copy: the given dict keeps its durations
    assert out["w_ceil"].dtype == torch.float32 and out["w_ceil"].shape == (2, 5) and torch.equal(out["w_ceil"], d.float())
    assert out["y_lengths"].dtype == torch.int64 and out["y_lengths"].tolist() == [6, 11]
    assert out["m_p"] is enc["m_p"] and out["x_mask"] is enc["x_mask"]
    assert models.with_durations(enc, d.numpy())["y_lengths"].tolist() == [6, 11]
    assert models.with_durations(enc, np.zeros((2, 5)))["y_lengths"].tolist() == [1, 1]       # clamp_min(sum, 1), models.py:1057
    enc3 = dict(enc, w_ceil=torch.ones(2, 1, 5))
    assert models.with_durations(enc3, d)["w_ceil"].shape == (2, 1, 5)
    with pytest.raises(ValueError, match=r"\[2, 5\]"):
        models.with_durations(enc, torch.ones(2, 4))
    with pytest.raises(ValueError, match="negative"):
        models.with_durations(enc, -d)


def _utt(T, **kw):
    b = synth.synthetic_batch([T], languages=[0], sids=[1])
    return serving.Utterance(b["x"][0], b["tone"][0], b["language"][0], b["bert"][0], b["ja_bert"][0], b["en_bert"][0], 1, **kw)


def test_utterance_durations_validation():
    assert _utt(6).durations is None
    u = _utt(6, durations=np.array([2, 1, 1, 3, 1, 1]))
    assert isinstance(u.durations, torch.Tensor) and u.durations.dtype == torch.float32 and u.durations.tolist() == [2, 1, 1, 3, 1, 1]
    assert _utt(6, durations=torch.tensor([2, 0, 1, 3, 1, 1], dtype=torch.int64)).durations.sum() == 8
    for bad, msg in ((np.ones(5), "one entry per phone"), (np.ones((1, 6)), "one entry per phone"), ([1, 1, 1, 1, 1, -1], "whole, non-negative"),
                     ([1.5, 1, 1, 1, 1, 1], "whole, non-negative"), ([float("nan")] + [1] * 5, "whole, non-negative"), (np.zeros(6), "at least one frame")):
        with pytest.raises(ValueError, match=msg):
            _utt(6, durations=bad)


def test_bucket_inputs_carry_given_durations():
    utts = [_utt(6, durations=[2, 1, 1, 3, 1, 1]), _utt(4), _utt(5, durations=[1, 1, 1, 1, 4])]
    hp = H.default_v23()

    class M:            # _bucket_inputs reads nothing but hp from the model when no utterance carries a voice vector or noise
        pass
    M.hp = hp
    batch, kw = serving._bucket_inputs(M, utts, [0, 1, 2], "cpu", None, [None] * 3)
    assert kw["w_ceil"].shape == (3, 6) and kw["w_ceil"][0].tolist() == [2, 1, 1, 3, 1, 1] and kw["w_ceil"][2].tolist() == [1, 1, 1, 1, 4, 0]
    assert kw["w_ceil_items"].tolist() == [True, False, True]
    batch, kw = serving._bucket_inputs(M, utts, [0, 2], "cpu", None, [None] * 3)
    assert "w_ceil_items" not in kw and kw["w_ceil"].shape == (2, 6)
    batch, kw = serving._bucket_inputs(M, utts, [1], "cpu", None, [None] * 3)
    assert "w_ceil" not in kw


@pytest.mark.parametrize("name", ["narrow_b2_t18", "mix_b2_ragged", "wn_b1_t16"])
def test_reference_fixtures_are_consistent(name):
    """tests/golden/align_*.npz (tools/gen_align_golden.py): the stored path is the restatement's on the stored matrix, the matrix is the
    definition on the stored tensors up to the recorded fp32 error, and the fp64 flow result is what the recorded error refers to."""
    from tests.helpers import load_golden
    meta, G = load_golden("align_" + name)
    xl, yl = G["x_lengths"].tolist(), G["y_lengths"].tolist()
    assert G["z"].shape == G["z_p"].shape == G["z_p64"].shape and G["z_p64"].dtype == torch.float64
    assert G["neg_cent"].shape == (len(xl), max(yl), G["m_p"].shape[2])
    d, _, score = PO.maximum_path(G["neg_cent"].numpy(), xl, yl)
    assert np.array_equal(d, G["durations"].numpy()) and np.array_equal(score, G["score"].numpy())
    nc64 = PO.neg_cent_f64(G["z_p"].numpy(), G["m_p"].numpy(), G["logs_p"].numpy(), xl, yl)
    assert abs(np.abs(G["neg_cent"].double().numpy() - nc64).max() - meta["ref_err_neg_cent"]) <= 1e-12
    assert abs(float((G["z_p"].double() - G["z_p64"]).abs().max()) - meta["ref_err_z_p"]) <= 1e-12
    for b in range(len(xl)):
        assert not G["neg_cent"][b, yl[b]:].any() and not G["neg_cent"][b, :, xl[b]:].any() and not G["z"][b, :, yl[b]:].any()
