"""CPU: the host side of the document assembly (include/bv2.h bv2_assemble_*): the proof that the reference's tail is "each piece under its
own peak, zero pauses between", the pause arithmetic, and every refusal — made before the device is touched, so they run here without one."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from bert_vits2_amd import audio, build, lib as L, serving
from tests import assemble_oracle as O
from tests.helpers import ROOT


def err():
    return L.load().bv2_last_error(None).decode()


def table(rows):
    """rows: dicts of bv2_assemble_segment fields; a piece gets a made-up non-null src that nothing follows."""
    t = (L.AssembleSegment * len(rows))()
    for e, r in zip(t, rows):
        e.hop = 1
        for k, v in r.items():
            setattr(e, k, v)
    return t


PIECE = dict(src=4096, length=8192, samples=100)


# ---- 1. the oracle proof -------------------------------------------------------------------------------------------------------------
def test_the_second_normalisation_is_the_identity_on_every_16_bit_value():
    k = np.arange(-32767, 32768).astype(np.float64)
    assert np.array_equal(np.trunc(k / 32767.0 * 32767.0), k)


def _paragraphs(rng):
    """Random fp32 pieces: a 1-sample piece, a piece whose peak is negative, a piece with |x| <= 2^-20; every paragraph has a non-silent
    piece (the domain on which the reference is defined: elsewhere it divides 0 by 0)."""
    piece = lambda n, scale=1.0: (rng.standard_normal(n) * scale).astype(np.float32)
    neg = piece(257, 0.3)
    neg[100] = -np.float32(np.abs(neg).max() * 1.5)
    tiny = np.clip(piece(301, 2.0 ** -22), -2.0 ** -20, 2.0 ** -20).astype(np.float32)
    tiny[7] = np.float32(2.0 ** -20)
    gap = piece(90)
    gap[10:50] = 0.0                                              # a run of digital silence inside a piece
    return [[[piece(1000)], [np.array([0.25], np.float32)], [neg, piece(33, 0.01)]],
            [[tiny, piece(513, 0.7)]],
            [[gap], [piece(64, 1e-3)]]]


@pytest.mark.parametrize("cut_by_sent", [True, False])
@pytest.mark.parametrize("para,sent", [(1.0, 0.2), (0.2, 0.5), (0.0, 0.0), (0.013, 0.0031)])
def test_reference_tail_is_each_piece_under_its_own_peak_with_zero_pauses(cut_by_sent, para, sent):
    paragraphs = _paragraphs(np.random.default_rng(5))
    want = O.reference_tail(paragraphs, para, sent, cut_by_sent)
    got = O.simple_document(paragraphs, para, sent, cut_by_sent)
    assert want.dtype == np.int16 and got.dtype == np.int16 and np.array_equal(want, got)
    assert int(np.abs(got).max()) == 32767


# ---- 2. pauses -----------------------------------------------------------------------------------------------------------------------
def test_pause_arithmetic():
    assert audio.pause_samples(44100, 0.2) == 8820
    assert audio.paragraph_pause_samples(44100, 1.0, 0.2) == 35280 == int(44100 * (1.0 - 0.2))
    assert audio.paragraph_pause_samples(44100, 0.2, 0.2) == 0 and audio.paragraph_pause_samples(44100, 0.1, 0.5) == 0
    assert audio.pause_samples(44100, 0.0) == 0 and audio.paragraph_pause_samples(44100, 0.0, 0.0) == 0
    assert audio.pause_samples(16000, 0.2) == 3200 and audio.paragraph_pause_samples(16000, 1.0, 0.2) == 12800
    assert audio.pause_samples(22050, 0.33) == int(22050 * 0.33) == 7276
    assert O.pauses(44100, 1.0, 0.2) == (8820, 35280, 44100)


def test_document_timeline_follows_tts_split():
    u = [serving.Utterance(torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64),
                           *(torch.zeros(1024, 3) for _ in range(3))) for _ in range(5)]
    docs = [[[u[0], [u[1], u[2]]], [u[3]]], [[u[4]]]]
    utts, tl = serving.document_timeline(docs, 44100)
    assert [x is y for x, y in zip(utts, u)] == [True] * 5
    assert tl[0] == [("piece", 0, 0), ("silence", 8820), ("piece", 1, 0), ("piece", 2, 0), ("silence", 8820), ("silence", 35280),
                     ("piece", 3, 1), ("silence", 8820), ("silence", 35280)]
    assert tl[1] == [("piece", 4, 2), ("silence", 8820), ("silence", 35280)]
    _, tl = serving.document_timeline(docs, 16000, interval_between_para=0.5, interval_between_sent=0.5)
    assert tl[1] == [("piece", 4, 2), ("silence", 8000)]
    _, tl = serving.document_timeline(docs, 44100, cut_by_sent=False)
    assert tl[0] == [("piece", 0, 0), ("piece", 1, 0), ("piece", 2, 0), ("silence", 44100), ("piece", 3, 1), ("silence", 44100)]
    for bad in ([], [[]], [[[]]], [[[[]]]], [[u[0]]], [u[0]], [[["text"]]]):
        with pytest.raises(ValueError, match="must be"):
            serving.document_timeline(bad, 44100)
    with pytest.raises(ValueError, match="finite and not negative"):
        serving.document_timeline(docs, 44100, interval_between_sent=-0.1)


# ---- 3. bv2_assemble_plan --------------------------------------------------------------------------------------------------------------
def plan(rows, n_groups=1, n_docs=1, cfg=None, n=None):
    lib = L.load()
    t = table(rows)
    cap = (C.c_int64 * max(n_docs, 1))()
    tile = C.c_int32()
    rc = lib.bv2_assemble_plan(C.byref(cfg or audio.assemble_config("piece", True)), t, len(rows) if n is None else n, n_groups, n_docs,
                               cap, C.byref(tile))
    return rc, list(cap), tile.value


def test_plan_sums_the_capacities():
    rows = [dict(PIECE, samples=100), dict(samples=50), dict(PIECE, samples=7, hop=512, group=1, doc=1), dict(samples=0, doc=1),
            dict(PIECE, samples=3, doc=3, length=None)]
    rc, cap, tile = plan(rows, 2, 4)
    assert rc == 0 and cap == [150, 7, 0, 3] and tile >= 64 and tile % 8 == 0
    assert audio.assemble_plan(table(rows), 2, 4) == ([150, 7, 0, 3], tile)
    assert C.sizeof(L.AssembleSegment) == 40 and C.sizeof(L.AssembleConfig) == 24


@pytest.mark.parametrize("rows,n_groups,n_docs,msg", [
    ([dict(PIECE, group=1)], 1, 1, "group 1 is outside"),
    ([dict(PIECE, group=-1)], 1, 1, "group -1 is outside"),
    ([dict(PIECE, doc=2)], 1, 2, "doc 2 is outside"),
    ([dict(samples=5, doc=-1)], 1, 1, "doc -1 is outside"),
    ([dict(PIECE, doc=1), dict(samples=4, doc=0)], 1, 2, "non-decreasing"),
    ([dict(PIECE, hop=0)], 1, 1, "hop must be >= 1"),
    ([dict(samples=-1)], 1, 1, "samples must not be negative"),
    ([dict(PIECE, samples=0)], 1, 1, "a piece needs a cap"),
    ([dict(length=8192, samples=4)], 1, 1, "a piece needs src"),
    ([dict(PIECE, reserved=1)], 1, 1, "reserved must be 0"),
    ([dict(samples=2 ** 40 + 1)], 1, 1, "at most 2\\^40"),
])
def test_plan_refuses_a_bad_table(rows, n_groups, n_docs, msg):
    rc, _, _ = plan([dict(samples=1)] + rows if "non-decreasing" not in msg else rows, n_groups, n_docs)
    assert rc == -1 and re.search(msg, err()), err()
    with pytest.raises(ValueError, match=msg):
        audio.assemble_plan(table(rows), n_groups, n_docs)


def test_plan_refuses_bad_counts_and_configs():
    lib = L.load()
    rows = [dict(PIECE)]
    for n, msg in ((0, "n_segments must be in"), ((1 << 20) + 1, "n_segments must be in")):
        rc, _, _ = plan(rows, n=n)
        assert rc == -1 and msg in err()
    assert plan(rows, n_groups=0)[0] == -1 and "n_groups" in err()
    assert plan(rows, n_groups=2)[0] == -1 and "n_groups" in err()
    assert plan(rows, n_docs=0)[0] == -1 and "n_docs" in err()
    assert plan(rows, n_docs=65536)[0] == -1 and "n_docs" in err()
    c = audio.assemble_config("piece", True)
    c.struct_bytes -= 4
    assert plan(rows, cfg=c)[0] == -1 and "struct_bytes" in err()
    c = audio.assemble_config("piece", True)
    c.level = 4
    assert plan(rows, cfg=c)[0] == -1 and "level" in err()
    c = audio.assemble_config("piece", True)
    c.output_format = 2
    assert plan(rows, cfg=c)[0] == -1 and "output_format" in err()
    cap = (C.c_int64 * 1)()
    assert lib.bv2_assemble_plan(C.byref(audio.assemble_config("piece", True)), None, 1, 1, 1, cap, None) == -1 and "null" in err()
    assert lib.bv2_assemble_plan(None, table(rows), 1, 1, 1, cap, None) == -1 and "cfg is null" in err()
    assert lib.bv2_assemble_workspace_bytes(C.byref(audio.assemble_config("piece", True)), 0, 1, 1) == -1
    assert lib.bv2_assemble_workspace_bytes(C.byref(audio.assemble_config("piece", True)), 65536, 65536, 3) > 0


def test_assemble_refuses_before_the_device():
    """Made-up non-null pointers are never followed: every argument is checked first."""
    lib = L.load()
    p = C.c_void_p(4096)
    cfg = audio.assemble_config("piece", True, 1000)
    need = lib.bv2_assemble_workspace_bytes(C.byref(cfg), 4, 2, 2)
    call = lambda cfg=cfg, seg=p, n=4, g=2, d=2, gain=None, bases=p, cap=p, off=p, tot=p, ws=p, wsb=need: lib.bv2_assemble(
        None, C.byref(cfg), seg, n, g, d, gain, bases, cap, off, tot, ws, wsb)
    for kw in (dict(seg=None), dict(bases=None), dict(cap=None), dict(off=None), dict(tot=None)):
        assert call(**kw) == -1 and "must not be null" in err()
    assert call(n=0) == -1 and "n_segments" in err()
    assert call(n=(1 << 20) + 1) == -1 and "n_segments" in err()
    assert call(g=5) == -1 and "n_groups" in err()
    assert call(d=0) == -1 and "n_docs" in err()
    assert call(gain=p) == -1 and "BV2_LEVEL_GAIN" in err()
    assert call(ws=None) == -5 and call(wsb=need - 9) == -5 and "workspace" in err()
    bad = audio.assemble_config("piece", True, -1)
    assert call(cfg=bad) == -1 and "max_capacity" in err()
    bad = audio.assemble_config("piece", True, 1000)
    bad.struct_bytes = 16
    assert call(cfg=bad) == -1 and "struct_bytes" in err()


# ---- 4. wrappers and exports -------------------------------------------------------------------------------------------------------------
def test_python_wrappers_refuse_before_any_device_call():
    x = torch.zeros(2, 100)
    with pytest.raises(ValueError, match="at least one segment"):
        audio.assemble([x], [None], [])
    with pytest.raises(ValueError, match="one entry per source"):
        audio.assemble([x], [], [audio.Silence(4)])
    with pytest.raises(ValueError, match="device float32 tensor"):
        audio.assemble([x], [None], [audio.Piece(0, 0)])
    with pytest.raises(ValueError, match="level must be one of"):
        audio.assemble_config("loud", True)
    with pytest.raises(ValueError, match="samples must not be negative"):
        audio.assemble([], [], [audio.Silence(-1)])
    with pytest.raises(ValueError, match="Piece or an audio.Silence"):
        audio.assemble([], [], [("silence", 3)])
    with pytest.raises(ValueError, match="source 0 is outside"):
        audio.assemble([], [], [audio.Piece(0, 0)])
    with pytest.raises(ValueError, match="non-decreasing"):
        audio.assemble([], [], [audio.Silence(3, 1), audio.Silence(3, 0)])

    class OnCpu:
        device = torch.device("cpu")
    with pytest.raises(RuntimeError, match="needs the model on a GPU"):
        serving.synthesize_documents(OnCpu(), [[[None]]])


def test_abi_version_exports_and_sources():
    lib = L.load()
    assert lib.bv2_abi_version() == 3 == L.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "bv2.h")).read()
    assert re.search(r"#define BV2_ABI_VERSION 3\b", hdr) and re.search(r"#define BV2_PACK_LAYOUT 16\b", hdr)
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(bv2_[a-z0-9_]+)\s*\(", src))
    for name in ("bv2_assemble_plan", "bv2_assemble_workspace_bytes", "bv2_assemble"):
        assert name in declared and hasattr(lib, name) and name in [s[0] for s in L.SYMBOLS]
    assert "kernels/assemble.hip" in build.SOURCES
    assert (L.LEVEL_NONE, L.LEVEL_PIECE_PEAK, L.LEVEL_GROUP_PEAK, L.LEVEL_GAIN) == (0, 1, 2, 3)
    for k, v in (("NONE", 0), ("PIECE_PEAK", 1), ("GROUP_PEAK", 2), ("GAIN", 3)):
        assert re.search(rf"BV2_LEVEL_{k} = {v}\b", src)
