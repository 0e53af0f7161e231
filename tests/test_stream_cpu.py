"""CPU: the bookkeeping of streamed synthesis (include/bv2.h "streamed synthesis") — the Generator's halo from the hyper-parameters on both
sides of the C ABI, a window cut with it against the whole decode in fp64 (oracle), the windowed workspace plan, and the argument checks of
bv2_stream_chunk, which run before anything touches a device."""
import ctypes as C

import pytest
import torch

from bert_vits2_amd import hparams as H, lib as L, synth
from oracle import bv2_oracle as O
from oracle import cases

# the receptive-field walk of the issue, run by hand per config: conv_post +-3, per stage the widest ResBlock branch and the ConvTranspose1d
# index map, conv_pre +-3
HALO = dict(default=13, hp01=8, hp02=17, hp03=16, hp04=26, hp05=13, hp06=9, hp07=7, hp08=10, hp09=13, hp10=7, hp11=13, hp12=63)


def _hps():
    out = {"default": H.default_v23()}
    for name, c in cases.ENVELOPE.items():
        out[name[:4]] = H.default_v23(**c["hp"])
    return out


def _handle(hp):
    lib = L.load()
    cfg = L.make_config(hp)
    h = C.c_void_p()
    assert lib.bv2_create(C.byref(cfg), C.byref(h)) == 0, lib.bv2_last_error(None)
    return lib, h


def test_halo_values_python_and_c_agree_with_the_table():
    hps = _hps()
    assert sorted(hps) == sorted(HALO)
    for name, hp in hps.items():
        assert H.generator_halo(hp) == HALO[name], name
        lib, h = _handle(hp)
        assert lib.bv2_generator_halo(h) == HALO[name], name
        lib.bv2_destroy(h)
    assert L.load().bv2_generator_halo(None) == -1


@pytest.mark.parametrize("name,Ty", [("default", 48), ("hp04", 80), ("hp10", 80)])
def test_window_cut_with_the_halo_equals_the_whole_decode_fp64(name, Ty):
    """oracle.generator in fp64 on synthetic weights: first, interior and last 11-frame windows, each decoded from frames
    [t0 - H, t1 + H) clipped to the utterance, reproduce the whole decode's samples [t0*U, t1*U)."""
    hp = _hps()[name]
    sd = {k: v.double() for k, v in synth.synthetic_state_dict(hp, seed=1).items() if k.startswith("dec.")}
    gen = torch.Generator().manual_seed(3)
    z = torch.randn(1, hp.inter_channels, Ty, generator=gen, dtype=torch.float64)
    g = torch.randn(1, hp.gin_channels, 1, generator=gen, dtype=torch.float64)
    Hh, U = H.generator_halo(hp), hp.total_upsample
    fold = {}
    with torch.no_grad():
        whole = O.generator(sd, hp, z, g, fold)
        assert whole.shape[-1] == Ty * U and float(whole.abs().max()) > 0.05
        for t0 in (0, (Ty - 11) // 2, Ty - 11):
            t1 = t0 + 11
            w0, w1 = max(0, t0 - Hh), min(Ty, t1 + Hh)
            win = O.generator(sd, hp, z[:, :, w0:w1], g, fold)
            kept = win[..., (t0 - w0) * U:(t1 - w0) * U]
            err = float((kept - whole[..., t0 * U:t1 * U]).abs().max())
            print(f"{name} window [{t0}, {t1}) of {Ty}: max |window - whole| = {err:.3e}")
            assert err <= 1e-12, (name, t0, err)


def test_windowed_workspace_is_a_fraction_of_the_whole_and_monotone():
    lib, h = _handle(H.default_v23())
    whole = lib.bv2_workspace_bytes(h, 1, 512, 1536)
    win = lib.bv2_stream_workspace_bytes(h, 1, 512, 1536, 64)
    print(f"B = 1, T = 512, Ty = 1536: whole {whole / 1e6:.1f} MB, streamed at 64 frames {win / 1e6:.1f} MB")
    # derived: the Generator buffers alone are ~705 MB whole against ~42 MB at 64 + 2 * 13 frames; flow scratch + kept state ~20 MB
    assert 0 < win <= 0.25 * whole
    prev = 0
    for w in (1, 2, 8, 63, 64, 65, 128, 512, 1536, 4096):
        n = lib.bv2_stream_workspace_bytes(h, 1, 512, 1536, w)
        assert n >= prev > -1, w
        prev = n
    # a window that covers the utterance needs no more than the whole decode plus the window's output and length array
    assert prev <= whole + 1536 * 512 * 4 + 4096
    assert lib.bv2_stream_workspace_bytes(h, 8, 512, 1536, 64) > win
    for bad in ((0, 512, 1536, 64), (1, 0, 1536, 64), (1, 512, 0, 64), (1, 512, 1536, 0)):
        assert lib.bv2_stream_workspace_bytes(h, *bad) == -1
    assert lib.bv2_stream_workspace_bytes(None, 1, 512, 1536, 64) == -1
    lib.bv2_destroy(h)


def _args(**kw):
    a = L.StreamChunkArgs()
    a.struct_bytes = C.sizeof(L.StreamChunkArgs)
    a.B, a.Ty, a.t0, a.t1 = 2, 100, 0, 16
    a.y_lengths = 256                       # never read: every call below is refused before the device is touched
    a.exact_lengths = 1
    a.dst, a.dst_bstride = 512, 16 * 512
    a.window_frames = 16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_stream_chunk_refuses_bad_arguments_before_any_device_call():
    lib, h = _handle(H.default_v23())
    need = lib.bv2_stream_workspace_bytes(h, 2, 8, 100, 16)
    ws = C.c_void_p(4096)                   # a fake address: nothing below may reach the device (there is none here, and no weights)

    def call(a, nbytes=need):
        rc = lib.bv2_stream_chunk(h, None, C.byref(a), ws, nbytes)
        return rc, lib.bv2_last_error(h).decode()

    for a, word in ((_args(t0=16, t1=16), "t0 < t1"), (_args(t0=20, t1=16), "t0 < t1"), (_args(t0=-1), "t0 < t1"),
                    (_args(t0=90, t1=101), "past the last frame"), (_args(t0=0, t1=17), "window_frames"),
                    (_args(t0=60, t1=70, max_len=64), "past the last frame"),
                    (_args(dst16=1024, dst16_bstride=16 * 512), "exactly one of dst / dst16"), (_args(dst=None), "exactly one of dst / dst16"),
                    (_args(dst_bstride=16 * 512 - 1), "batch stride"), (_args(exact_lengths=2), "exact_lengths"),
                    (_args(y_lengths=None), "y_lengths"), (_args(struct_bytes=8), "struct_bytes"), (_args(B=0), "B")):
        rc, msg = call(a)
        assert rc == -1 and word in msg and msg.startswith("bv2_stream_chunk"), (rc, msg, word)
    assert lib.bv2_stream_chunk(h, None, None, ws, need) == -1
    rc, msg = call(_args(), need // 2)
    assert rc == -5 and "workspace" in msg
    rc, msg = call(_args())                 # everything in order: only now the missing weights are noticed (still no device call)
    assert rc == -8 and "no weights attached" in msg
    # bv2_stream_begin and bv2_emit check theirs first as well
    din, dout = L.DecodeIn(), L.DecodeOut()
    assert lib.bv2_stream_begin(h, None, C.byref(din), C.byref(dout), None, ws, need) == -1
    assert "bad argument" in lib.bv2_last_error(h).decode()
    assert lib.bv2_emit(None, C.c_void_p(256), 8, 0, None, 1, 0, 1, 8, None, None, 8, 1.0) == -1
    assert b"exactly one of dst / dst16" in lib.bv2_last_error(None)
    assert lib.bv2_emit(None, C.c_void_p(256), 8, 0, None, 1, 0, 1, 8, C.c_void_p(512), None, 7, 1.0) == -1
    lib.bv2_destroy(h)
