"""GPU: documents joined on the device (include/bv2.h bv2_assemble, kernels/assemble.hip) against tests/assemble_oracle.py.  Every comparison
of samples is ``np.array_equal``: the layout is integer arithmetic and every value rule is one numpy reproduces bit for bit.  The edges are
placed from the tile ``audio.assemble_plan`` reports; a sentinel fill in front of every document's base and at or behind its total shows
that nothing else is written."""
import functools

import numpy as np
import pytest
import torch

from bert_vits2_amd import audio, lib as L, serving
from tests import assemble_oracle as O
from tests.test_resample_gpu import KW, _utts, narrow_model

pytestmark = pytest.mark.gpu

SENTINEL = {True: 0x5A5A, False: -7777.0}
FORMATS = [True, False]
LEVELS = ["none", "piece", "group", "gain"]


@functools.lru_cache(maxsize=None)
def tile():
    t = (L.AssembleSegment * 1)()
    t[0].samples, t[0].hop = 1, 1
    return audio.assemble_plan(t, 1, 1)[1]


def device_rows(x, shift=0):
    """``x`` [B, S] on the device, its first element ``shift`` floats behind an allocation's (256-byte aligned) start."""
    flat = torch.zeros(shift + x.size + 8, dtype=torch.float32, device="cuda")
    flat[shift:shift + x.size] = torch.from_numpy(x.reshape(-1)).cuda()
    return flat[shift:shift + x.size].view(*x.shape)


def run(sources, lengths, segments, level, as_pcm16, gain=None, shifts=(0,), base_offs=(0, 1, 3)):
    """``sources[k]``: fp32 [B, S] arrays; ``lengths[k]``: ``(int list, hop)`` or ``None``.  Runs ``audio.assemble`` into sentinel-filled
    buffers whose document bases sit ``base_offs`` elements behind a 16-byte boundary, checks everything the call must NOT touch, and
    returns ``(documents cut to their totals, offsets, totals)`` plus the oracle's segments."""
    dev_src = [device_rows(x, shifts[k % len(shifts)]) for k, x in enumerate(sources)]
    dev_len = [None if ln is None else (torch.tensor(ln[0], dtype=torch.int64).cuda(), ln[1]) for ln in lengths]
    table, n_groups, n_docs = audio._segment_table(dev_src, dev_len, segments)
    capacity, _ = audio.assemble_plan(table, n_groups, n_docs, level, as_pcm16)
    dtype = torch.int16 if as_pcm16 else torch.float32
    pad = 64
    bigs, outs = [], []
    for d, cap in enumerate(capacity):
        off = pad + base_offs[d % len(base_offs)]
        big = torch.full((off + cap + pad,), SENTINEL[as_pcm16], dtype=dtype, device="cuda")
        bigs.append((big, off))
        outs.append(big[off:off + cap])
    g = None if gain is None else torch.tensor(gain, dtype=torch.float32).cuda()
    bufs, offsets, totals = audio.assemble(dev_src, dev_len, segments, level=level, gain=g, as_pcm16=as_pcm16, out=outs)
    torch.cuda.synchronize()
    totals = [int(v) for v in totals.cpu()]
    docs = []
    for d, (big, off) in enumerate(bigs):
        host = big.cpu().numpy()
        assert 0 <= totals[d] <= capacity[d]
        sent = host.dtype.type(SENTINEL[as_pcm16])
        assert np.all(host[:off] == sent), f"document {d}: written in front of its base"
        assert np.all(host[off + totals[d]:] == sent), f"document {d}: written at or behind its total"
        docs.append(host[off:off + totals[d]])
    ref = []
    for sg in segments:
        if isinstance(sg, audio.Silence):
            ref.append(("silence", sg.samples, sg.doc))
        else:
            x = sources[sg.source][sg.row]
            n = len(x) if lengths[sg.source] is None else min(max(lengths[sg.source][0][sg.row], 0) * lengths[sg.source][1], len(x))
            ref.append(("piece", x[:n], sg.group, sg.doc))
    return docs, [int(v) for v in offsets.cpu()], totals, ref


def check(sources, lengths, segments, level, as_pcm16, gain=None, **kw):
    docs, offsets, totals, ref = run(sources, lengths, segments, level, as_pcm16, gain, **kw)
    want, want_off, want_tot = O.assemble(ref, level, as_pcm16, gain)
    assert offsets == want_off and totals == want_tot
    for d, (a, b) in enumerate(zip(docs, want)):
        assert a.dtype == b.dtype and np.array_equal(a, b), f"document {d} ({level}, pcm16={as_pcm16})"
    return docs, offsets, totals


def noise(rng, B, S, scale=0.3):
    return (rng.standard_normal((B, S)) * scale).astype(np.float32)


# ---- 1. layout -------------------------------------------------------------------------------------------------------------------------
def test_layout_is_a_cumsum_per_document():
    rng = np.random.default_rng(0)
    a = noise(rng, 6, 1537)                                  # hop 512: counters in frames, the cap is the row's S
    b = noise(rng, 5, 33)
    la = ([0, -5, 2, 100, 3, 1], 512)                        # 0, negative, inside, above the cap (1537 < 100 * 512), exactly 3 * 512, one frame
    lb = ([33, 0, -1, 1000, 1], 1)
    P, Z = audio.Piece, audio.Silence
    segments = [Z(9, 0), Z(0, 0), Z(40, 0),                  # a document of silence only
                P(1, 4, 0, 1),                               # a document of one 1-sample piece
                P(0, 0, 0, 2), P(0, 1, 1, 2), Z(7, 2), P(0, 2, 0, 2), P(0, 3, 1, 2), P(1, 0, 2, 2), Z(1, 2), P(1, 1, 0, 2), P(1, 2, 0, 2),
                P(0, 4, 1, 2), P(1, 3, 2, 2), P(0, 5, 0, 2)]
    lens = [9, 0, 40, 1, 0, 0, 7, 1024, 1537, 33, 1, 0, 0, 1536, 33, 512]
    for as_pcm16 in FORMATS:
        _, offsets, totals = check([a, b], [la, lb], segments, "none", as_pcm16)
        docs = np.array([s.doc for s in segments])
        for d in range(3):
            own = np.array(lens)[docs == d]
            assert [offsets[i] for i in np.flatnonzero(docs == d)] == list(np.cumsum(own) - own) and totals[d] == own.sum()


def test_a_document_without_segments_has_total_zero():
    a = noise(np.random.default_rng(1), 2, 9)
    docs, offsets, totals = check([a], [None], [audio.Piece(0, 0, 0, 0), audio.Piece(0, 1, 0, 2)], "piece", True)
    assert totals == [9, 0, 9] and offsets == [0, 0]


# ---- 2. edges --------------------------------------------------------------------------------------------------------------------------
def edge_case():
    t = tile()
    piece_lens = [0, 1, 3, 4, 7, 8, 9, 15, 16, 17, t - 1, t, t + 1, 2 * t + 5]
    silences = [0, 1, 2, 7, 8, 9]
    rng = np.random.default_rng(2)
    S = 2 * t + 7                                            # odd: consecutive rows start on every 4-byte phase of a 16-byte line
    assert S % 2 == 1
    srcs = [noise(rng, len(piece_lens), S), noise(rng, len(piece_lens), S)]
    srcs[1][13] *= 8.0                                       # the longest piece: the 16-bit gain forms clamp
    segments = []
    for d in range(3):                                       # three documents, their bases 0, 1 and 3 elements off a 16-byte boundary
        order = np.roll(np.arange(len(piece_lens)), 5 * d)
        for j, r in enumerate(order):
            segments.append(audio.Piece((d + j) % 2, int(r), int((r + d) % 3), d))
            segments.append(audio.Silence(silences[(j + d) % len(silences)], d))
    return srcs, [(piece_lens, 1), (piece_lens, 1)], segments


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("as_pcm16", FORMATS)
def test_edges_of_tiles_vectors_and_phases(as_pcm16, level):
    srcs, lens, segments = edge_case()
    gain = [0.5, 1.25, 4.0] if level == "gain" else None
    docs, _, totals = check(srcs, lens, segments, level, as_pcm16, gain, shifts=(0, 1))      # the second tensor starts one element off
    assert min(totals) > 4 * tile()
    if level == "gain" and as_pcm16:
        assert max(int(d.max()) for d in docs) == 32767 and min(int(d.min()) for d in docs) == -32768


# ---- 3. dense --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", ["piece", "group"])
@pytest.mark.parametrize("as_pcm16", FORMATS)
def test_more_segments_in_one_tile_than_a_workgroup_has_threads_to_spare(as_pcm16, level):
    rng = np.random.default_rng(3)
    n = 640
    a = noise(rng, n, 3)
    lens = [int(v) for v in rng.integers(0, 3, n)]
    segments = []
    for i in range(n):
        segments.append(audio.Piece(0, i, i % 7, 0) if i % 5 else audio.Silence(int(rng.integers(0, 3)), 0))
    assert len(segments) >= 600
    _, _, totals = check([a], [(lens, 1)], segments, level, as_pcm16)
    assert 0 < totals[0] < tile()


# ---- 4. peaks --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_pcm16", FORMATS)
def test_group_peaks_across_tensors(as_pcm16):
    rng = np.random.default_rng(4)
    t = tile()
    a, b = noise(rng, 3, t + 9, 0.2), noise(rng, 2, 501, 0.2)
    b[1, 400] = -3.5                                         # the group's peak: negative, in the last piece, in the other tensor
    a[2] = 0.0                                               # an all-zero group
    tiny = (rng.integers(-1024, 1025, (1, 77)) * 2.0 ** -30).astype(np.float32)
    tiny[0, 5] = -np.float32(2.0 ** -20)                     # a group whose peak is 2^-20
    P, Z = audio.Piece, audio.Silence
    segments = [P(0, 0, 0, 0), Z(5, 0), P(0, 1, 0, 0), P(0, 2, 1, 0), Z(3, 0), P(2, 0, 2, 0), P(1, 0, 3, 0), P(1, 1, 0, 0)]
    for level in ("group", "piece"):
        docs, offsets, _ = check([a, b, tiny], [None, None, None], segments, level, as_pcm16)
        doc = docs[0]
        assert not doc[offsets[3]:offsets[4]].any()          # peak 0: zeros
        if level == "group":
            first = doc[:t + 9]                              # group 0's first piece sits under the peak of its last
            assert np.array_equal(first, O.pcm16_rule(a[0], 3.5) if as_pcm16 else O.peak_f32(a[0], 3.5))
            assert doc[offsets[7] + 400] == (-32767 if as_pcm16 else -1.0)
        small = doc[offsets[5]:offsets[6]]
        assert small[5] == (-32767 if as_pcm16 else -1.0)
        assert np.array_equal(small, O.pcm16_rule(tiny[0]) if as_pcm16 else (tiny[0] * np.float32(2.0 ** 20)))      # exact: a power of two


# ---- 5. placement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", ["group", "gain"])
def test_placement_does_not_change_a_bit(level):
    rng = np.random.default_rng(5)
    t = tile()
    lens = [t + 3, 17, 0, 300, 2 * t - 1]
    pieces = [noise(rng, 1, n)[0] for n in lens]
    groups = [0, 1, 0, 2, 1]
    gain = [0.7, 1.9, 0.33]
    P, Z = audio.Piece, audio.Silence

    def timeline(where, renumber):
        out = []
        for i, (k, r) in enumerate(where):
            out += [P(k, r, renumber[groups[i]], 0), Z(11 * i, 0)]
        return out

    def packed(S, rows):
        """One tensor [len(rows), S]: piece i in row rows[i], garbage behind its length."""
        x = noise(rng, len(rows), S, 5.0)
        ln = [0] * len(rows)
        for i, r in enumerate(rows):
            if r is not None:
                x[r, :lens[i]] = pieces[i]
                ln[r] = lens[i]
        return x, ln

    xa, la = packed(2 * t + 1, [0, 1, 2, 3, 4])
    base, _, _ = check([xa], [(la, 1)], timeline([(0, i) for i in range(5)], [0, 1, 2]), level, True, gain if level == "gain" else None)
    xb, lb = packed(2 * t + 64, [4, None, 0, None, 2])       # other rows, another S, two tensors, another first-element phase
    xc, lc = packed(2 * t + 6, [None, 1, None, 0, None])
    where = [(0, 4), (1, 1), (0, 0), (1, 0), (0, 2)]
    renumber = [2, 0, 1]
    g2 = [gain[renumber.index(j)] for j in range(3)]
    moved, _, _ = check([xb, xc], [(lb, 1), (lc, 1)], timeline(where, renumber), level, True, g2 if level == "gain" else None,
                        shifts=(3, 2), base_offs=(5,))
    assert np.array_equal(base[0], moved[0])


# ---- 6. serving ------------------------------------------------------------------------------------------------------------------------
LENGTHS = [17, 24, 9, 30, 12, 20, 14, 27]                    # 2 documents x 2 paragraphs x (2, 1) sentences; two sentences are two pieces
SERVE = dict(max_batch=4, max_pad_ratio=1.5, **KW)


def _seeded():
    out = _utts(LENGTHS)
    for i, u in enumerate(out):
        u.seed = 2000 + i
    return out


def _documents(u):
    return [[[u[0], [u[1], u[2]]], [u[3]]], [[u[4], u[5]], [[u[6], u[7]]]]]


def _shape(x):
    """The pieces of ``_documents`` as nested lists of whatever ``x`` holds per utterance."""
    return [[[[x[0]], [x[1], x[2]]], [[x[3]]]], [[[x[4]], [x[5]]], [[x[6], x[7]]]]]


DOC_OF = [0, 0, 0, 0, 1, 1, 1, 1]
IDENT = lambda v: v


@functools.lru_cache(maxsize=None)
def _pieces(**kw):
    m = narrow_model()
    assert len(serving.plan_batches(LENGTHS, 4, 1.5)) >= 2
    a = serving.synthesize(m, _seeded(), **kw, **SERVE)
    b = serving.synthesize(m, _seeded(), **kw, **SERVE)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), "precondition: two synthesize calls give equal bits"
    return a


@pytest.mark.parametrize("cut_by_sent", [True, False])
def test_documents_are_synthesize_joined_by_the_oracle(cut_by_sent):
    m = narrow_model()
    rate = m.hp.sampling_rate
    pcm = _pieces(as_pcm16=True)
    got, offsets = serving.synthesize_documents(m, _documents(_seeded()), cut_by_sent=cut_by_sent, return_offsets=True, **SERVE)
    assert len(got) == 2
    k = 0
    for d, paragraphs in enumerate(_shape(pcm)):
        want = O.simple_document(paragraphs, 1.0, 0.2, cut_by_sent, rate, IDENT)
        assert got[d].dtype == np.int16 and np.array_equal(got[d], want), f"document {d}"
        for start, n in offsets[d]:                          # the start and length of every piece, in reading order
            assert n == len(pcm[k]) and np.array_equal(got[d][start:start + n], pcm[k])
            k += 1
    assert k == len(LENGTHS)
    other = serving.synthesize_documents(m, _documents(_seeded()), cut_by_sent=cut_by_sent, interval_between_sent=0.013,
                                         interval_between_para=0.0031, **SERVE)
    for d, paragraphs in enumerate(_shape(pcm)):
        assert np.array_equal(other[d], O.simple_document(paragraphs, 0.0031, 0.013, cut_by_sent, rate, IDENT))


def test_documents_under_the_document_and_paragraph_peak():
    m = narrow_model()
    f32 = _pieces()
    for level, group_of in (("document", DOC_OF), ("paragraph", [0, 0, 0, 1, 2, 2, 3, 3])):
        peaks = {g: max(np.abs(f32[i]).max() for i in range(8) if group_of[i] == g) for g in set(group_of)}
        for as_pcm16 in FORMATS:
            got = serving.synthesize_documents(m, _documents(_seeded()), level=level, as_pcm16=as_pcm16, **SERVE)
            lv = [(O.pcm16_rule if as_pcm16 else O.peak_f32)(x, peaks[group_of[i]]) for i, x in enumerate(f32)]
            for d, paragraphs in enumerate(_shape(lv)):
                assert np.array_equal(got[d], O.simple_document(paragraphs, 1.0, 0.2, True, m.hp.sampling_rate, IDENT)), (level, as_pcm16, d)


def test_documents_to_a_target_loudness():
    m = narrow_model()
    kw = dict(target_lufs=-23.0, peak_ceiling_db=60.0)
    for as_pcm16 in FORMATS:
        want = serving.synthesize(m, _seeded(), loudness_groups=DOC_OF, as_pcm16=as_pcm16, **kw, **SERVE)
        got = serving.synthesize_documents(m, _documents(_seeded()), as_pcm16=as_pcm16, **kw, **SERVE)
        for d, paragraphs in enumerate(_shape(want)):
            assert np.array_equal(got[d], O.simple_document(paragraphs, 1.0, 0.2, True, m.hp.sampling_rate, IDENT)), (as_pcm16, d)


def test_documents_at_another_rate_and_with_two_requests_in_flight():
    m = narrow_model()
    pcm = _pieces(as_pcm16=True, output_rate=16000)
    got, offsets = serving.synthesize_documents(m, _documents(_seeded()), output_rate=16000, return_offsets=True, **SERVE)
    for d, paragraphs in enumerate(_shape(pcm)):
        assert np.array_equal(got[d], O.simple_document(paragraphs, 1.0, 0.2, True, 16000, IDENT))
    assert [n for doc in offsets for _, n in doc] == [len(p) for p in pcm]
    for kw in (dict(), dict(output_rate=16000), dict(target_lufs=-23.0, peak_ceiling_db=60.0), dict(level="paragraph", as_pcm16=False)):
        one = serving.synthesize_documents(m, _documents(_seeded()), return_offsets=True, **kw, **SERVE)
        two = serving.synthesize_documents(m, _documents(_seeded()), return_offsets=True, requests_in_flight=2, **kw, **SERVE)
        assert all(np.array_equal(a, b) for a, b in zip(one[0], two[0])) and one[1] == two[1], kw
    with pytest.raises(ValueError, match="level must be one of"):
        serving.synthesize_documents(m, _documents(_seeded()), level="sentence", **SERVE)
