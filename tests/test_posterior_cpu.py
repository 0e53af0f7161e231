"""CPU: the posterior encoder's host side — its schema, its own weight blob (packing, both weight-norm forms, header, what it leaves
untouched), ``load_posterior`` on a stripped checkpoint, the C ABI, and the calls that need it loaded."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest
import torch

from bert_vits2_amd import hparams as H, lib as L, models, schema, serving, synth
from oracle import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("bv2_posterior_packed_bytes", "bv2_posterior_load_tensor", "bv2_posterior_pack", "bv2_posterior_attach", "bv2_posterior_detach",
           "bv2_posterior_workspace_bytes", "bv2_posterior_encode", "bv2_align", "bv2_align_workspace_bytes")


def narrow_hp(spec=80):
    return H.default_v23(**dict(cases.CASES["narrow_b2_t18"]["hp"], spec_channels=spec))


def _model(hp):
    m = models.from_hparams(hp)
    m.load_state_dict(synth.synthetic_state_dict(hp, 0), strict=False)
    return m


def test_acceptance_load_posterior_align_exist_and_a_posterior_state_dict_packs():
    """Fails on the parent: no posterior blob, no load_posterior / posterior_encode / align."""
    hdr = open(os.path.join(ROOT, "include", "bv2.h")).read()
    assert re.search(r"#define BV2_ABI_VERSION 3\b", hdr) and re.search(r"#define BV2_PACK_LAYOUT 16\b", hdr)
    lib = L.load()
    assert lib.bv2_abi_version() == 3
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert getattr(lib, name) is not None and name in {s[0] for s in L.SYMBOLS}
    for attr in ("load_posterior", "has_posterior", "posterior_encode", "align", "stage_flow_forward"):
        assert hasattr(models.SynthesizerTrn, attr), attr
    hp = narrow_hp()
    m = _model(hp)
    blob = m.pack_posterior_host_blob(synth.synthetic_posterior_state_dict(hp, 0))
    assert blob.dtype == torch.uint8 and blob.numel() == m._lib.bv2_posterior_packed_bytes(m._handle, 80) > 0
    assert not m.has_posterior                                                # packed on the host, nothing attached


def test_posterior_schema():
    hp = H.default_v23()
    shapes = schema.posterior_param_shapes(hp)
    assert all(k.startswith("enc_q.") for k in shapes) and not any(k.startswith("enc_q.") for k in schema.param_shapes(hp))
    Hc, Ci, G = hp.hidden_channels, hp.inter_channels, hp.gin_channels
    assert shapes["enc_q.pre.weight"] == (Hc, hp.spec_channels, 1) and shapes["enc_q.proj.weight"] == (2 * Ci, Hc, 1)
    assert shapes["enc_q.enc.cond_layer.weight_v"] == (2 * Hc * 16, G, 1)
    assert shapes["enc_q.enc.in_layers.15.weight_v"] == (2 * Hc, Hc, 5)
    assert shapes["enc_q.enc.res_skip_layers.14.weight_v"] == (2 * Hc, Hc, 1) and shapes["enc_q.enc.res_skip_layers.15.weight_v"] == (Hc, Hc, 1)
    assert len(shapes) == 2 + 3 + 16 * 3 * 2 + 2
    sd = synth.synthetic_posterior_state_dict(hp, 3)
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(shapes)
    assert all(torch.equal(a, b) for a, b in zip(sd.values(), synth.synthetic_posterior_state_dict(hp, 3).values()))
    assert not torch.equal(sd["enc_q.pre.weight"], synth.synthetic_posterior_state_dict(hp, 4)["enc_q.pre.weight"])


def test_posterior_blob_round_trip_and_weight_norm_forms():
    hp = narrow_hp()
    m = _model(hp)
    sd = synth.synthetic_posterior_state_dict(hp, 0)
    b1 = m.pack_posterior_host_blob(sd)
    assert torch.equal(b1, m.pack_posterior_host_blob(sd))                      # a pure function of the tensors
    hdr = np.frombuffer(b1[:32].numpy().tobytes(), dtype=np.uint32)
    assert hdr[0] == 0x71765642 and hdr[1] == 3 and hdr[3] == 1
    assert int(np.frombuffer(b1[16:24].numpy().tobytes(), dtype=np.int64)[0]) * 4 == b1.numel()
    # the folded form a remove_weight_norm'ed checkpoint carries packs to the same weights (the norm's last rounding apart)
    folded = {}
    for k, v in sd.items():
        if k.endswith(".weight_v"):
            g = sd[k[:-1] + "g"]
            folded[k[:-2]] = g * v / v.flatten(1).norm(dim=1).view(-1, 1, 1)
        elif not k.endswith(".weight_g"):
            folded[k] = v
    m2 = _model(hp)
    b2 = m2.pack_posterior_host_blob(folded)
    f1, f2 = b1[256:].view(torch.float32), b2[256:].view(torch.float32)
    assert torch.equal(b1[:256], b2[:256]) and (f1 - f2).abs().max() <= 1e-6 * f1.abs().max()
    # every weight landed exactly once (padding is zeros): the blob's sum of squares is the tensors'
    want = sum(float(v.double().pow(2).sum()) for v in folded.values())
    assert abs(float(f2.double().pow(2).sum()) - want) <= 1e-9 * want and abs(float(f1.double().pow(2).sum()) - want) <= 1e-5 * want
    # another seed packs to other bytes; a missing tensor is named
    assert not torch.equal(b1, _model(hp).pack_posterior_host_blob(synth.synthetic_posterior_state_dict(hp, 1)))
    short = {k: v for k, v in sd.items() if k != "enc_q.enc.in_layers.7.bias"}
    with pytest.raises(RuntimeError, match=r"enc_q\.enc\.in_layers\.7\.bias"):
        _model(hp).pack_posterior_host_blob(short)
    bad = dict(sd)
    bad["enc_q.pre.weight"] = torch.zeros(hp.hidden_channels, 81, 1)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        _model(hp).pack_posterior_host_blob(bad)


def test_inference_blob_is_unchanged_by_the_posterior():
    hp = narrow_hp()
    m = _model(hp)
    before = m.pack_host_blob()
    n = m._lib.bv2_packed_bytes(m._handle)
    m.pack_posterior_host_blob(synth.synthetic_posterior_state_dict(hp, 0))
    after = m.pack_host_blob()
    assert m._lib.bv2_packed_bytes(m._handle) == n == before.numel()
    assert hashlib.sha256(before.numpy().tobytes()).hexdigest() == hashlib.sha256(after.numpy().tobytes()).hexdigest()
    assert {k for k, _ in m.named_parameters()} == set(schema.param_shapes(hp))  # the shim's state_dict did not grow
    # bv2_load_tensor keeps ignoring enc_q.*; the posterior loader ignores everything else
    t = torch.zeros(4)
    shape = (C.c_int64 * 1)(4)
    assert m._lib.bv2_load_tensor(m._handle, b"enc_q.pre.bias", C.c_void_p(t.data_ptr()), shape, 1, L.F32) == 1
    assert m._lib.bv2_posterior_load_tensor(m._handle, b"dec.conv_pre.bias", C.c_void_p(t.data_ptr()), shape, 1, L.F32) == 1
    assert m._lib.bv2_posterior_load_tensor(m._handle, b"enc_q.pre.bias", C.c_void_p(t.data_ptr()), shape, 1, L.F32) == 0


def test_spec_channels_is_checked_where_the_posterior_is_created():
    m = _model(narrow_hp())
    lib = m._ensure_handle()
    for spec in (1025, 513, 80):
        assert lib.bv2_posterior_packed_bytes(m._handle, spec) > 0
    assert lib.bv2_posterior_packed_bytes(m._handle, 1025) > lib.bv2_posterior_packed_bytes(m._handle, 80)
    for spec in (0, 81, 1024, 2049):
        assert lib.bv2_posterior_packed_bytes(m._handle, spec) < 0 and b"1025, 513 or 80" in lib.bv2_last_error(m._handle)
    assert lib.bv2_posterior_workspace_bytes(m._handle, 2, 64) > 0 and lib.bv2_posterior_workspace_bytes(m._handle, 0, 64) < 0
    one = C.c_void_p(8)
    assert lib.bv2_posterior_encode(m._handle, None, 1, 8, one, one, one, None, 1.0, one, None, None, None, one, 1 << 20) == -8
    assert b"compress_model.py" in lib.bv2_last_error(m._handle)
    assert lib.bv2_posterior_detach(m._handle) == 0


def test_stripped_checkpoint_and_calls_without_the_posterior_raise_with_the_hint(tmp_path):
    hp = narrow_hp()
    m = _model(hp)
    stripped = synth.synthetic_state_dict(hp, 0)                                 # what compress_model.py leaves: no enc_q.*
    with pytest.raises(ValueError, match="compress_model.py"):
        m.load_posterior(stripped)
    path = tmp_path / "G_0.pth"
    torch.save({"model": stripped, "iteration": 0, "optimizer": None, "learning_rate": 1e-4}, path)   # utils.save_checkpoint's dict
    with pytest.raises(ValueError, match="compress_model.py"):
        m.load_posterior(str(path))
    assert not m.has_posterior
    z = torch.zeros(1, 80, 8)
    with pytest.raises(RuntimeError, match="compress_model.py"):
        m.posterior_encode(z, [8], sid=torch.tensor([0]))
    b = synth.synthetic_batch([4])
    with pytest.raises(RuntimeError, match="compress_model.py"):
        m.align(b["x"], b["x_lengths"], b["sid"], b["tone"], b["language"], b["bert"], b["ja_bert"], b["en_bert"], z, [8])
    with pytest.raises(ValueError, match="exactly one"):
        serving.align(m.to("meta") if False else _Cuda(m), [], None)


class _Cuda:
    """Stands in for a model on a GPU in argument checks that run before anything touches one."""
    def __init__(self, m):
        self.hp, self.device = m.hp, torch.device("cuda")
