"""CPU: speaker conditioning from a reference spectrogram (ReferenceEncoder, n_speakers == 0) or a given vector — configuration, schema,
packing, the C ABI's new entry points, the serving fields and the fixtures' metadata (tests/golden/ref_enc_*.npz,
tools/gen_ref_enc_golden.py).  Everything that computes g runs on the GPU: tests/test_ref_enc_gpu.py."""
import ctypes as C
import dataclasses
import hashlib
import os
import re

import pytest
import torch

from bert_vits2_amd import hparams as H, lib as L, models, schema, serving, synth
from oracle import cases
from tests.helpers import ROOT, load_golden

MODEL_CASE = "narrow_b2_t18"
DEFAULT_BLOB_BYTES = 421940224       # packed blob of the released v2.3 shapes (H.default_v23()) — the same number before this feature
DEFAULT_BLOB_SHA256 = "98de17f97d2702a851d726c657d4f31f602dab6950455b690335a06fbd884e9a"   # synthetic_state_dict(seed 0), packed by the parent commit


def narrow_hp(spec_channels=1025, **kw):
    return H.default_v23(**dict(cases.CASES[MODEL_CASE]["hp"], n_speakers=0, spec_channels=spec_channels, **kw))


def _create(cfg):
    lib = L.load()
    h = C.c_void_p()
    rc = lib.bv2_create(C.byref(cfg), C.byref(h))
    return lib, h, rc, ("" if rc == 0 else lib.bv2_last_error(None).decode())


def test_n_speakers_zero_is_accepted_on_both_sides():
    """The acceptance test: fails on the parent commit with NotImplementedError('n_speakers == 0 needs ReferenceEncoder ...')."""
    for spec in H.ENVELOPE["spec_channels"]:
        hp = narrow_hp(spec)
        hp.validate()
        lib, h, rc, msg = _create(L.make_config(hp))
        assert rc == 0, (spec, msg)
        assert lib.bv2_packed_bytes(h) > 0
        assert lib.bv2_ref_workspace_bytes(h, 1, 400) > 0
        lib.bv2_destroy(h)
    assert H.ENVELOPE["spec_channels"] == [80, 513, 1025]
    hp = H.default_v23(n_speakers=0)
    hp.validate()
    m = models.from_hparams(hp)
    assert m.n_speakers == 0 and "ref_enc.gru.weight_hh_l0" in dict(m.named_parameters())


def test_spec_channels_outside_the_envelope_is_rejected_with_a_message():
    for spec in (1024, 257, 81, 0):
        hp = narrow_hp(spec)
        with pytest.raises(ValueError, match="spec_channels"):
            hp.validate()
        cfg = L.make_config(narrow_hp(1025))
        cfg.spec_channels = spec
        lib, h, rc, msg = _create(cfg)
        assert rc != 0 and "spec_channels" in msg, (spec, rc, msg)
    # with a speaker table the field is not read: any value is legal and changes nothing
    hp = H.default_v23(spec_channels=257)
    hp.validate()
    cfg = L.make_config(hp)
    cfg.spec_channels = 257
    lib, h, rc, msg = _create(cfg)
    assert rc == 0, msg
    ref = _create(L.make_config(H.default_v23()))
    assert lib.bv2_packed_bytes(h) == lib.bv2_packed_bytes(ref[1])
    lib.bv2_destroy(h)
    lib.bv2_destroy(ref[1])
    with pytest.raises(ValueError, match="n_speakers"):
        H.default_v23(n_speakers=-1).validate()


def test_shorter_config_struct_needs_a_speaker_table():
    cfg = L.make_config(narrow_hp())
    cfg.struct_bytes = C.sizeof(L.Config) - 4            # the struct before spec_channels was appended
    lib, h, rc, msg = _create(cfg)
    assert rc != 0 and "spec_channels" in msg, (rc, msg)
    cfg = L.make_config(H.default_v23())
    cfg.struct_bytes = C.sizeof(L.Config) - 4
    lib, h, rc, msg = _create(cfg)
    assert rc == 0, msg
    lib.bv2_destroy(h)


def test_config_struct_mirrors_the_header():
    src = open(os.path.join(ROOT, "include", "bv2.h")).read()
    body = re.search(r"typedef struct bv2_config \{(.*?)\} bv2_config;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in re.findall(r"int32_t ([^;]+);", body) for n in re.findall(r"(\w+)(?:\[[^\]]*\])*\s*(?:,|$)", decl)]
    assert names == [n for n, _ in L.Config._fields_]
    assert names[-2:] == ["resblock_type", "spec_channels"]
    assert L.Config.spec_channels.offset == C.sizeof(L.Config) - 4


def test_schema_lists_ref_enc_and_no_speaker_table():
    hp = narrow_hp()
    d = schema.param_shapes(hp)
    assert "emb_g.weight" not in d
    ref = {k: v for k, v in d.items() if k.startswith("ref_enc.")}
    want = {}
    cin = 1
    for i, cout in enumerate((32, 32, 64, 64, 128, 128)):
        want[f"ref_enc.convs.{i}.bias"] = (cout,)
        want[f"ref_enc.convs.{i}.weight_g"] = (cout, 1, 1, 1)
        want[f"ref_enc.convs.{i}.weight_v"] = (cout, cin, 3, 3)
        cin = cout
    want.update({"ref_enc.gru.weight_ih_l0": (384, 2176), "ref_enc.gru.weight_hh_l0": (384, 128), "ref_enc.gru.bias_ih_l0": (384,),
                 "ref_enc.gru.bias_hh_l0": (384,), "ref_enc.proj.weight": (hp.gin_channels, 128), "ref_enc.proj.bias": (hp.gin_channels,)})
    assert ref == want
    assert hp.ref_enc_freqs == [513, 257, 129, 65, 33, 17]
    assert narrow_hp(513).ref_enc_freqs[-1] == 9 and narrow_hp(80).ref_enc_freqs == [40, 20, 10, 5, 3, 2]
    assert schema.param_shapes(narrow_hp(80))["ref_enc.gru.weight_ih_l0"] == (384, 256)
    # with a speaker table nothing changed
    d1 = schema.param_shapes(H.default_v23())
    assert "emb_g.weight" in d1 and not any(k.startswith("ref_enc.") for k in d1)
    assert set(synth.synthetic_state_dict(hp, 0)) == set(d)


def _fold(sd):
    """The checkpoint as remove_weight_norm would leave ref_enc: folded `.weight` instead of weight_g / weight_v."""
    out = {}
    for k, v in sd.items():
        if k.startswith("ref_enc.convs.") and k.endswith(".weight_v"):
            g = sd[k[:-1] + "g"]
            out[k[:-2]] = v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1, 1))
        elif k.startswith("ref_enc.convs.") and k.endswith(".weight_g"):
            continue
        else:
            out[k] = v
    return out


def test_pack_host_blob_in_both_weight_norm_forms():
    hp = narrow_hp()
    sd = synth.synthetic_state_dict(hp, 0)
    m = models.from_hparams(hp)
    m.load_state_dict(sd, strict=False)
    blob = m.pack_host_blob()
    assert blob.numel() == m._lib.bv2_packed_bytes(m._handle) > 0
    # the folded form through the C ABI: the same handle type, tensors handed over one by one
    lib, h, rc, msg = _create(L.make_config(hp))
    assert rc == 0, msg
    for k, v in _fold(sd).items():
        t = v.contiguous()
        shape = (C.c_int64 * t.dim())(*t.shape)
        assert lib.bv2_load_tensor(h, k.encode(), C.c_void_p(t.data_ptr()), shape, t.dim(), L.F32) >= 0, k
    n = lib.bv2_packed_bytes(h)
    blob2 = torch.empty(n, dtype=torch.uint8)
    assert lib.bv2_pack_weights(h, C.c_void_p(blob2.data_ptr()), n) == 0, lib.bv2_last_error(h)
    f1, f2 = blob.view(torch.float32), blob2.view(torch.float32)
    assert f1.shape == f2.shape
    assert torch.equal(f1[:4].view(torch.int32), f2[:4].view(torch.int32))      # same header (magic, ABI, config hash, layout)
    ne = f1.view(torch.int32) != f2.view(torch.int32)             # the fold done here in fp32 and in the packer: last-bit differences,
    n_conv = sum(v.numel() for k, v in sd.items() if k.startswith("ref_enc.convs.") and k.endswith("weight_v"))
    assert int(ne.sum()) <= n_conv                                # confined to the ReferenceEncoder's conv weights
    assert not ne.any() or float((f1[ne] - f2[ne]).abs().max()) < 1e-6
    lib.bv2_destroy(h)
    # a missing ref_enc tensor is named
    lib, h, rc, msg = _create(L.make_config(hp))
    for k, v in sd.items():
        if k == "ref_enc.gru.weight_hh_l0":
            continue
        t = v.contiguous()
        shape = (C.c_int64 * t.dim())(*t.shape)
        lib.bv2_load_tensor(h, k.encode(), C.c_void_p(t.data_ptr()), shape, t.dim(), L.F32)
    assert lib.bv2_pack_weights(h, C.c_void_p(blob2.data_ptr()), n) != 0
    assert b"ref_enc.gru.weight_hh_l0" in lib.bv2_last_error(h)
    lib.bv2_destroy(h)


def test_default_model_blob_is_byte_identical_to_the_parents():
    hp = H.default_v23()
    m = models.from_hparams(hp)
    m.load_state_dict(synth.synthetic_state_dict(hp, 0), strict=False)
    blob = m.pack_host_blob()
    assert blob.numel() == DEFAULT_BLOB_BYTES
    assert hashlib.sha256(blob.numpy().tobytes()).hexdigest() == DEFAULT_BLOB_SHA256
    # and a caller built against the shorter struct gets the same layout
    cfg = L.make_config(hp)
    cfg.struct_bytes = C.sizeof(L.Config) - 4
    lib, h, rc, msg = _create(cfg)
    assert rc == 0 and lib.bv2_packed_bytes(h) == DEFAULT_BLOB_BYTES
    lib.bv2_destroy(h)


def test_new_symbols_and_argument_checks():
    lib = L.load()
    assert lib.bv2_abi_version() == 3 and L.ABI_VERSION == 3
    for name in ("bv2_ref_encode", "bv2_ref_workspace_bytes", "bv2_encode_durations_g", "bv2_infer_g", "bv2_graph_capture_encode_g"):
        assert hasattr(lib, name) and name in [s[0] for s in L.SYMBOLS]
        assert name in open(os.path.join(ROOT, "include", "bv2.h")).read()
    ein, eout, dout = L.EncodeIn(B=1, T=1), L.EncodeOut(), L.DecodeOut(o=8)
    ws, gr, ty = C.c_void_p(8), C.c_void_p(), C.c_int32()
    # a model without a speaker table: every phase-A call without g fails with a message, before anything is read
    _, h, rc, msg = _create(L.make_config(narrow_hp()))
    assert rc == 0, msg
    calls = {
        "bv2_encode_durations": lambda g: lib.bv2_encode_durations_g(h, None, C.byref(ein), C.byref(eout), None, g, ws, 8),
        "bv2_infer": lambda g: lib.bv2_infer_g(h, None, C.byref(ein), C.byref(eout), None, 0, 0, 0, 0.5, 0, 16, C.byref(dout),
                                               C.byref(ty), None, g, ws, 8),
        "bv2_graph_capture_encode": lambda g: lib.bv2_graph_capture_encode_g(h, C.c_void_p(16), C.byref(ein), C.byref(eout), None, g,
                                                                             ws, 8, C.byref(gr)),
    }
    for name, call in calls.items():
        assert call(None) != 0, name
        assert b"no speaker table" in lib.bv2_last_error(h), (name, lib.bv2_last_error(h))
        assert call(C.c_void_p(64)) != 0, name                       # with a g the call gets as far as the missing weights
        assert b"no weights attached" in lib.bv2_last_error(h), (name, lib.bv2_last_error(h))
    assert lib.bv2_encode_durations(h, None, C.byref(ein), C.byref(eout), ws, 8) != 0 and b"no speaker table" in lib.bv2_last_error(h)
    bad = L.ItemControls()
    bad.struct_bytes = 12
    assert lib.bv2_encode_durations_g(h, None, C.byref(ein), C.byref(eout), C.byref(bad), C.c_void_p(64), ws, 8) != 0
    assert b"struct_bytes" in lib.bv2_last_error(h)
    assert lib.bv2_ref_encode(h, None, C.c_void_p(64), None, None, 1, 61, C.c_void_p(64), ws, 8) != 0
    assert b"no weights attached" in lib.bv2_last_error(h)
    assert lib.bv2_ref_workspace_bytes(h, 0, 61) < 0 and lib.bv2_ref_workspace_bytes(h, 1, 0) < 0
    # the workspace covers the two ping-pong activation buffers and the GRU's input projection
    f = [513, 257, 129, 65, 33, 17]
    t = [200, 100, 50, 25, 13, 7]
    c = [32, 32, 64, 64, 128, 128]
    sizes = [ci * ti * fi for ci, ti, fi in zip(c, t, f)]
    need = 4 * (max(sizes[0::2]) + max(sizes[1::2]) + 7 * 384)
    assert need <= lib.bv2_ref_workspace_bytes(h, 1, 400) <= need + 4096
    lib.bv2_destroy(h)
    # a model WITH a table has no ReferenceEncoder
    _, h, rc, msg = _create(L.make_config(H.default_v23()))
    assert lib.bv2_ref_encode(h, None, C.c_void_p(64), None, None, 1, 61, C.c_void_p(64), ws, 8) != 0
    assert b"no ReferenceEncoder" in lib.bv2_last_error(h)
    assert lib.bv2_ref_workspace_bytes(h, 1, 61) < 0
    lib.bv2_destroy(h)


def _utt(T=5, **kw):
    u = synth.synthetic_utterance(T, 0)
    return serving.Utterance(u["x"], u["tone"], u["language"], u["bert"], u["ja_bert"], u["en_bert"], **kw)


def test_serving_utterance_checks_g_and_ref_spec():
    assert [f.name for f in dataclasses.fields(serving.Utterance)][-2:] == ["g", "ref_spec"]
    u = _utt()
    assert u.g is None and u.ref_spec is None and u.sid == 0
    _utt(g=torch.zeros(256))
    _utt(ref_spec=torch.zeros(1025, 61))
    for bad in (torch.zeros(1, 256), torch.zeros(256, 1), 3.0, torch.zeros(0)):
        with pytest.raises(ValueError, match="g must be"):
            _utt(g=bad)
    for bad in (torch.zeros(1025), torch.zeros(1, 1025, 61), torch.zeros(1025, 0)):
        with pytest.raises(ValueError, match="ref_spec must be"):
            _utt(ref_spec=bad)
    with pytest.raises(ValueError, match="not both"):
        _utt(g=torch.zeros(256), ref_spec=torch.zeros(1025, 61))


def test_shim_rejects_misshapen_speaker_vectors_without_a_gpu():
    hp = narrow_hp()
    m = models.from_hparams(hp)
    assert m._speaker_vector(torch.zeros(2, hp.gin_channels, 1), 2).shape == (2, hp.gin_channels)
    assert m._speaker_vector(torch.zeros(2, hp.gin_channels, dtype=torch.float64), 2).dtype == torch.float32
    for bad in (torch.zeros(hp.gin_channels), torch.zeros(3, hp.gin_channels), torch.zeros(2, 1, hp.gin_channels)):
        with pytest.raises(ValueError, match="g must be"):
            m._speaker_vector(bad, 2)
    with pytest.raises(RuntimeError, match="n_speakers=0"):
        models.from_hparams(H.default_v23()).reference_embedding(torch.zeros(1, 1025, 8))


def test_synthetic_reference_spec_is_seeded_nonnegative_and_tilted():
    a = synth.synthetic_reference_spec(1025, 96, 1)
    assert a.shape == (1025, 96) and a.dtype == torch.float32 and float(a.min()) >= 0
    assert torch.equal(a, synth.synthetic_reference_spec(1025, 96, 1))
    assert torch.equal(a[:, :61], synth.synthetic_reference_spec(1025, 61, 1))       # a shorter reference is a prefix
    assert not torch.equal(a, synth.synthetic_reference_spec(1025, 96, 2))
    assert float(a[:100].mean()) > 5 * float(a[-100:].mean())                        # falls off with frequency


def test_fixture_metadata_rebuilds_the_inputs():
    meta, arr = load_golden("ref_enc_g")
    assert meta["model_case"] == MODEL_CASE and meta["gin_channels"] == narrow_hp().gin_channels
    assert sorted(meta["cases"]) == sorted(f"s{s}_l{n}" for s in (1025, 513, 80) for n in (61, 96, 400, 7))
    for name, c in meta["cases"].items():
        y = synth.synthetic_reference_spec(c["spec_channels"], c["L"], c["index"])
        assert y.shape == (c["spec_channels"], c["L"])
        g, g64 = arr[name + "_g"], arr[name + "_g64"]
        assert g.shape == g64.shape == (meta["gin_channels"],) and g64.dtype == torch.float64
        assert abs(float((g.double() - g64).abs().max()) - c["ref_err"]) < 1e-12 and 0 < c["ref_err"] < 1e-5 * c["rms"]
    meta, arr = load_golden("ref_enc_narrow_b2")
    hp = narrow_hp(meta["spec_channels"])
    sd = synth.synthetic_state_dict(hp, meta["seed"])
    assert cases.weight_checksums(sd) == pytest.approx(meta["checksums"])
    assert meta["lengths"] == [18, 11] and meta["ref_lengths"] == [61, 61]
    assert arr["g"].shape == (2, hp.gin_channels) and arr["o"].shape[0] == 2 and "identical" in meta["knife_edge"]
    assert arr["y_lengths"].tolist() == arr["y_mask"].sum([1, 2]).long().tolist()
