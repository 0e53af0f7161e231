"""CPU: the split-K head's packed fields (bv2_kernels.h sk_head_pack / sk_head_unpack) through the host-only entry
bv2_test_splitk_head: every field survives the round trip at both ends of its range, and one past each end — or a launch that is not
the head form's — falls back to the generic kernel.  k, dil, pad_left and ksplit travel in 8 bits each, cin and cin_pad in 16."""
import ctypes as C
import functools

import pytest

FIELDS = ("k", "dil", "pad_left", "ksplit", "cin", "cin_pad")
LOW = dict(k=1, dil=1, pad_left=0, ksplit=1, cin=1, cin_pad=1)
HIGH = dict(k=255, dil=255, pad_left=255, ksplit=255, cin=65535, cin_pad=65535)


@functools.lru_cache(maxsize=None)
def _lib():
    from bert_vits2_amd import lib as L
    lib = L.load()
    lib.bv2_test_splitk_head.restype = C.c_int
    lib.bv2_test_splitk_head.argtypes = [C.c_int] * 9 + [C.c_void_p]
    return lib


def head(B=1, has_lens=0, nprob=1, **f):
    out = (C.c_int32 * 6)(*([-1] * 6))
    rc = _lib().bv2_test_splitk_head(f["k"], f["dil"], f["pad_left"], f["ksplit"], f["cin"], f["cin_pad"], B, has_lens, nprob, out)
    return rc, dict(zip(FIELDS, out))


@pytest.mark.parametrize("name", FIELDS)
def test_round_trip_at_the_extremes_of_each_field(name):
    for base, other in ((LOW, HIGH), (HIGH, LOW)):
        f = dict(base)
        f[name] = other[name]                                      # one field at the far end, the others at this one: fields do not bleed
        rc, got = head(**f)
        assert rc == 1 and got == f, (f, got)
    rc, got = head(**HIGH)
    assert rc == 1 and got == HIGH
    rc, got = head(**LOW)
    assert rc == 1 and got == LOW


@pytest.mark.parametrize("name", FIELDS)
def test_one_past_each_extreme_falls_back(name):
    mid = dict(k=5, dil=2, pad_left=4, ksplit=2, cin=192, cin_pad=192)
    assert head(**mid)[0] == 1
    for v in (LOW[name] - 1, HIGH[name] + 1):
        f = dict(mid)
        f[name] = v
        assert head(**f)[0] == 0, (name, v)


def test_launches_outside_the_head_form_fall_back():
    mid = dict(k=5, dil=2, pad_left=4, ksplit=2, cin=192, cin_pad=192)
    assert head(B=2, **mid)[0] == 0                                # a batch: the bases would need their strides
    assert head(has_lens=1, **mid)[0] == 0                         # exact lengths: the clamp of Lin needs a load first
    assert head(nprob=2, **mid)[0] == 0                            # several problems: the descriptor is picked by a computed index
