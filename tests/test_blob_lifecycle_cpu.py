"""CPU: the host half of the packed weight blobs' lifecycle — tensors in, size, pack — asked the same questions for each of the three kinds
(the inference blob, the posterior encoder's, the forward duration predictor's).  The library runs one implementation for all three; these
pin what every kind answered before that was so."""
import ctypes as C
import os
import re
from collections import namedtuple

import numpy as np
import pytest
import torch

from bert_vits2_amd import hparams as H, lib as L, synth
from oracle import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = H.default_v23(**cases.CASES["narrow_b2_t18"]["hp"])
Kind = namedtuple("Kind", "name load size pack takes_spec magic layout_macro own foreign withheld reshaped")
KINDS = [
    Kind("inference", "bv2_load_tensor", "bv2_packed_bytes", "bv2_pack_weights", False, 0x32765642, "BV2_PACK_LAYOUT",
         "enc_p.emb.weight", "enc_q.pre.bias", "dec.ups.1.bias", "sdp.pre.weight"),
    Kind("posterior", "bv2_posterior_load_tensor", "bv2_posterior_packed_bytes", "bv2_posterior_pack", True, 0x71765642, "BV2_POSTERIOR_LAYOUT",
         "enc_q.pre.bias", "sdp.post_pre.bias", "enc_q.enc.in_layers.7.bias", "enc_q.proj.weight"),
    Kind("sdp_forward", "bv2_sdp_forward_load_tensor", "bv2_sdp_forward_packed_bytes", "bv2_sdp_forward_pack", False, 0x66765642,
         "BV2_SDP_FORWARD_LAYOUT", "sdp.flows.1.pre.bias", "sdp.flows.3.pre.bias", "sdp.post_flows.5.convs.norms_2.1.beta", "sdp.post_pre.weight"),
]
DTYPES = {L.F32: torch.float32, L.F16: torch.float16, L.BF16: torch.bfloat16}


@pytest.fixture(scope="module")
def tensors():
    """What each kind is fed: every tensor of a training checkpoint; each kind keeps its own and answers 1 to the rest."""
    sd = dict(synth.synthetic_state_dict(HP, 0))
    sd.update(synth.synthetic_posterior_state_dict(HP, 0))
    sd.update(synth.synthetic_sdp_forward_state_dict(HP, 0))
    return sd


@pytest.fixture(scope="module")
def rounded(tensors):
    return {d: {k: v.to(t) for k, v in tensors.items()} for d, t in DTYPES.items() if d != L.F32}


class Handle:
    def __init__(self, kind):
        self.kind, self.lib, self.h = kind, L.load(), C.c_void_p()
        cfg = L.make_config(HP)
        assert self.lib.bv2_create(C.byref(cfg), C.byref(self.h)) == 0, self.lib.bv2_last_error(None)
        self.spec = (int(HP.spec_channels),) if kind.takes_spec else ()

    def __del__(self):
        self.lib.bv2_destroy(self.h)

    def err(self):
        return self.lib.bv2_last_error(self.h).decode()

    def load(self, key, t, dtype=L.F32, ndim=None, key_arg=True, data=True):
        t = t.contiguous()
        nd = t.dim() if ndim is None else ndim
        shape = (C.c_int64 * max(nd, 1))(*(list(t.shape) + [1] * 9)[:max(nd, 1)])
        return getattr(self.lib, self.kind.load)(self.h, key.encode() if key_arg else None, C.c_void_p(t.data_ptr()) if data else None, shape,
                                                 nd, dtype)

    def load_all(self, sd, dtype=L.F32, skip=()):
        """``sd`` holds tensors of ``dtype``.  Returns the keys this kind kept."""
        kept = []
        for k, v in sd.items():
            if k in skip:
                continue
            assert v.dtype == DTYPES[dtype]
            rc = self.load(k, v, dtype)
            assert rc in (0, 1), (k, rc, self.err())
            if rc == 0:
                kept.append(k)
        return kept

    def size(self):
        return getattr(self.lib, self.kind.size)(self.h, *self.spec)

    def pack(self, short=0):
        n = self.size()
        assert n > 0, self.err()
        blob = torch.zeros(n, dtype=torch.uint8)
        return getattr(self.lib, self.kind.pack)(self.h, *self.spec, C.c_void_p(blob.data_ptr()), n - short), blob


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.name)
def test_ingest_keeps_its_own_keys_and_checks_its_arguments(kind, tensors):
    H_ = Handle(kind)
    t = tensors[kind.own]
    assert H_.load(kind.own, t) == 0
    # a foreign key is answered with 1 and nothing is kept: with only foreign tensors offered, the own ones are still all missing
    G = Handle(kind)
    assert G.load(kind.foreign, tensors[kind.foreign]) == 1
    rc, _ = G.pack()
    assert rc == -2 and kind.foreign not in G.err()
    for kw in (dict(key_arg=False), dict(data=False), dict(ndim=9), dict(ndim=-1)):
        assert H_.load(kind.own, t, **kw) == -1, kw
        assert H_.err().startswith(kind.load + ":") and "bad argument" in H_.err(), (kw, H_.err())
    assert H_.load(kind.own, t, dtype=7) == -1 and H_.err().startswith(kind.load + ":") and "dtype" in H_.err()
    assert getattr(H_.lib, kind.load)(None, kind.own.encode(), C.c_void_p(t.data_ptr()), (C.c_int64 * 1)(1), 1, L.F32) == -1
    assert H_.load(kind.own, torch.zeros(()), ndim=0) == 0                       # a scalar: ndim 0 needs no shape


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.name)
def test_half_precision_tensors_pack_as_their_widened_values(kind, tensors, rounded):
    """The F16 / BF16 conversion of the load call: a tensor handed over in 16 bits packs to the bytes of the same values widened by torch."""
    for dtype in (L.F16, L.BF16):
        a, b = Handle(kind), Handle(kind)
        kept = a.load_all(rounded[dtype], dtype)
        assert kind.own in kept and kind.foreign not in kept
        b.load_all({k: rounded[dtype][k].float() for k in kept})
        (ra, blob_a), (rb, blob_b) = a.pack(), b.pack()
        assert ra == 0 and rb == 0, (a.err(), b.err())
        assert torch.equal(blob_a, blob_b), (kind.name, dtype)
    c = Handle(kind)
    c.load_all(tensors)
    rc, blob_c = c.pack()
    assert rc == 0 and not torch.equal(blob_c, blob_b)                           # ... and rounding to 16 bits is not a no-op on these weights


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.name)
def test_pack_refusals_and_header(kind, tensors):
    hdr_text = open(os.path.join(ROOT, "include", "bv2.h")).read()
    layout = int(re.search(r"#define " + kind.layout_macro + r" (\d+)\b", hdr_text).group(1))
    a = Handle(kind)
    a.load_all(tensors)
    rc, _ = a.pack(short=1)
    assert rc == -1 and a.err().startswith(kind.pack + ":") and "too small" in a.err()
    n = a.size()
    assert getattr(a.lib, kind.pack)(a.h, *a.spec, None, n) == -1 and "too small" in a.err()
    rc, blob = a.pack()
    assert rc == 0, a.err()
    hdr = np.frombuffer(blob[:32].numpy().tobytes(), dtype=np.uint32)
    assert (int(hdr[0]), int(hdr[1]), int(hdr[3])) == (kind.magic, L.ABI_VERSION, layout)
    assert int(np.frombuffer(blob[16:24].numpy().tobytes(), dtype=np.int64)[0]) == n // 4 and n % 4 == 0
    assert not blob[32:256].any()                                                # the rest of the header stays zero
    b = Handle(kind)
    b.load_all(tensors, skip=(kind.withheld,))
    rc, _ = b.pack()
    assert rc == -2 and kind.withheld in b.err() and "missing/invalid tensors (1)" in b.err(), b.err()
    c = Handle(kind)
    c.load_all(tensors)
    t = tensors[kind.reshaped]
    assert c.load(kind.reshaped, torch.zeros(*t.shape[:-1], t.shape[-1] + 1)) == 0
    rc, _ = c.pack()
    assert rc == -2 and "shape mismatch" in c.err() and kind.reshaped in c.err(), c.err()
    assert getattr(a.lib, kind.size)(None, *a.spec) == -1
    assert getattr(a.lib, kind.pack)(None, *a.spec, C.c_void_p(blob.data_ptr()), n) == -1


def test_the_posterior_layout_follows_spec_channels():
    a = Handle(KINDS[1])
    sizes = {s: a.lib.bv2_posterior_packed_bytes(a.h, s) for s in (1025, 513, 80)}
    assert sizes[1025] > sizes[513] > sizes[80] > 0
    assert a.lib.bv2_posterior_packed_bytes(a.h, 512) == -1
    assert a.err().startswith("bv2_posterior_packed_bytes:") and "1025, 513 or 80" in a.err()
    blob = torch.zeros(sizes[1025], dtype=torch.uint8)
    assert a.lib.bv2_posterior_pack(a.h, 512, C.c_void_p(blob.data_ptr()), blob.numel()) == -1 and a.err().startswith("bv2_posterior_pack:")
    assert a.lib.bv2_posterior_packed_bytes(a.h, 80) == sizes[80]                 # a refused width leaves the layout usable
