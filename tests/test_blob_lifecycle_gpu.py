"""GPU: the device half of the packed weight blobs' lifecycle — attach, the header read back from the device, detach — asked the same
questions for each of the three kinds.  No kernel of the library runs: every refusal sits in front of the first launch, and every pointer
handed over is a device allocation of the stated size."""
import ctypes as C
from collections import namedtuple

import pytest
import torch

from bert_vits2_amd import hparams as H, models, synth
from oracle import cases

pytestmark = pytest.mark.gpu
HP = H.default_v23(**cases.CASES["narrow_b2_t18"]["hp"])
Kind = namedtuple("Kind", "name attach detach takes_spec")
KINDS = [Kind("inference", "bv2_attach_weights", "bv2_detach_weights", False),
         Kind("posterior", "bv2_posterior_attach", "bv2_posterior_detach", True),
         Kind("sdp_forward", "bv2_sdp_forward_attach", "bv2_sdp_forward_detach", False)]
B, T, TY = 2, 5, 12


@pytest.fixture(scope="module")
def blobs():
    """The three packed blobs of one model, on the device."""
    m = models.from_hparams(HP)
    m.load_state_dict(synth.synthetic_state_dict(HP, 0), strict=False)
    host = dict(inference=m.pack_host_blob(), posterior=m.pack_posterior_host_blob(synth.synthetic_posterior_state_dict(HP, 0)),
                sdp_forward=m.pack_sdp_forward_host_blob(synth.synthetic_sdp_forward_state_dict(HP, 0)))
    return {k: v.cuda() for k, v in host.items()}


@pytest.fixture()
def model():
    m = models.from_hparams(HP)
    m._ensure_handle()
    return m


def attach(m, kind, blob, nbytes=None):
    spec = (int(HP.spec_channels),) if kind.takes_spec else ()
    rc = getattr(m._lib, kind.attach)(m._handle, *spec, C.c_void_p(blob.data_ptr()), blob.numel() if nbytes is None else nbytes)
    return rc, m._lib.bv2_last_error(m._handle).decode()


def with_header_word(blob, word, value):
    out = blob.clone()
    out[4 * word:4 * word + 4] = torch.tensor(list(int(value).to_bytes(4, "little")), dtype=torch.uint8)
    return out


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.name)
def test_attach_reads_the_header_back(kind, blobs, model):
    good = blobs[kind.name]
    n = good.numel()
    rc, msg = attach(model, kind, good, n - 1)
    assert rc == -1 and msg.startswith(kind.attach + ":") and "too small" in msg
    # another kind's blob at this kind's length: the magic gives it away
    other = blobs[KINDS[(KINDS.index(kind) + 1) % 3].name]
    padded = torch.zeros(max(n, other.numel()), dtype=torch.uint8, device="cuda")
    padded[:other.numel()] = other
    rc, msg = attach(model, kind, padded)
    assert rc == -7 and msg.startswith(kind.attach + ":") and "another model" in msg, msg
    hash_word = int.from_bytes(bytes(good[8:12].tolist()), "little")
    rc, msg = attach(model, kind, with_header_word(good, 2, hash_word ^ 1))
    assert rc == -7 and "another model" in msg, msg
    if kind.name == "inference":
        layout = int.from_bytes(bytes(good[12:16].tolist()), "little")
        rc, msg = attach(model, kind, with_header_word(good, 3, layout - 1))
        assert rc == -7 and "repack" in msg, msg
    rc, msg = attach(model, kind, good)
    assert rc == 0, msg
    assert getattr(model._lib, kind.detach)(model._handle) == 0 and getattr(model._lib, kind.detach)(None) == -1


def _loaded():
    m = models.from_hparams(HP)
    m.load_state_dict(synth.synthetic_state_dict(HP, 0), strict=False)
    m = m.to("cuda").eval()
    m.repack()
    m.load_posterior(synth.synthetic_posterior_state_dict(HP, 0))
    m.load_sdp_forward(synth.synthetic_sdp_forward_state_dict(HP, 0))
    return m


def _calls(m):
    """The three calls that need a blob, with arguments that would run: each is made through the model's own method, which sizes and
    allocates every tensor (the Python side still believes the blob attached, so nothing is repacked)."""
    z = lambda *s: torch.zeros(*s, device="cuda")
    enc = dict(x=z(B, HP.hidden_channels, T), m_p=z(B, HP.inter_channels, T), logs_p=z(B, HP.inter_channels, T), x_mask=torch.ones(B, 1, T, device="cuda"),
               w_ceil=torch.full((B, 1, T), 2.0, device="cuda"), y_lengths=torch.full((B,), 2 * T, dtype=torch.int64, device="cuda"),
               g=z(B, HP.gin_channels))
    return dict(
        posterior=lambda: m.posterior_encode(z(B, HP.spec_channels, TY), torch.full((B,), TY), g=enc["g"], noise_q=z(B, HP.inter_channels, TY)),
        sdp_forward=lambda: m.duration_nll(enc, torch.full((B, T), 2.0), noise_e=z(B, 2, T)),
        inference=lambda: m.decode(enc, z(B, HP.inter_channels, 2 * T), 2 * T))


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.name)
def test_a_detached_blob_is_missed_before_any_launch(kind):
    m = _loaded()
    assert getattr(m._lib, kind.detach)(m._handle) == 0
    with pytest.raises(RuntimeError, match=r"failed \(-8\).*attached"):
        _calls(m)[kind.name]()


def test_another_spec_channels_drops_the_attached_posterior_blob():
    m = _loaded()
    other = 513 if HP.spec_channels != 513 else 80
    assert m._lib.bv2_posterior_packed_bytes(m._handle, other) > 0
    with pytest.raises(RuntimeError, match=r"bv2_posterior_encode failed \(-8\)"):
        _calls(m)["posterior"]()
