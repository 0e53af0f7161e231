"""CPU: the host-side polyphase split of ConvTranspose1d (bv2_internal.h ups_geometry — what the packer, the executors and the GPU tests'
entry points all use), through bv2_test_ups_split, for EVERY (u, k) pair the envelope admits: u = 2..8, k / u = 1..4, (k - u) even.
Small-integer weights and inputs make every fp64 sum exact, so the comparison with F.conv_transpose1d is torch.equal."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from bert_vits2_amd import lib as L

PAIRS = [(u, u * r) for u in range(2, 9) for r in range(1, 5) if (u * r - u) % 2 == 0]


def _lib():
    lib = L.load()
    lib.bv2_test_ups_split.restype = C.c_int
    lib.bv2_test_ups_split.argtypes = [C.c_int] * 4 + [C.c_void_p] * 6
    return lib


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def split(lib, u, k, w):
    """(phase_w [u][cout][cin][k/u], pad_left [u], cl_w [u*cout][cin][kk], cl_pad_left, kk, cl_offs [u]) of w [cin][cout][k]"""
    cin, cout = w.shape[0], w.shape[1]
    dims = torch.zeros(2, dtype=torch.int32)
    assert lib.bv2_test_ups_split(u, k, cin, cout, None, None, None, None, P(dims), None) == 0
    kk = int(dims[1])
    phase_w = torch.full((u, cout, cin, k // u), float("nan"))
    cl_w = torch.full((u * cout, cin, kk), float("nan"))
    pad_left, offs = torch.full((u,), -99, dtype=torch.int32), torch.full((u,), -99, dtype=torch.int32)
    w32 = w.float().contiguous()
    assert lib.bv2_test_ups_split(u, k, cin, cout, P(w32), P(phase_w), P(pad_left), P(cl_w), P(dims), P(offs)) == 0
    return phase_w, pad_left.tolist(), cl_w, int(dims[0]), kk, offs.tolist()


def test_the_envelope_has_22_pairs():
    assert len(PAIRS) == 22 and (8, 16) in PAIRS and (2, 4) in PAIRS


@pytest.mark.parametrize("u,k", PAIRS)
def test_phase_convs_and_window_conv_equal_conv_transpose1d(u, k):
    lib = _lib()
    g = torch.Generator().manual_seed(100 * u + k)
    cin, cout, B, Lx = 5, 3, 2, 11
    w = torch.randint(-4, 5, (cin, cout, k), generator=g).double()
    b = torch.randint(-4, 5, (cout,), generator=g).double()
    x = torch.randint(-4, 5, (B, cin, Lx), generator=g).double()
    ref = F.conv_transpose1d(x, w, b, stride=u, padding=(k - u) // 2)
    assert ref.shape == (B, cout, Lx * u)
    phase_w, pad_left, cl_w, cl_pad_left, kk, offs = split(lib, u, k, w)
    nt = k // u
    # the u stride-1 phase convs, interleaved: output n = u * s + ph
    got = torch.full_like(ref, float("nan"))
    for ph in range(u):
        assert 0 <= pad_left[ph] <= nt - 1
        got[:, :, ph::u] = F.conv1d(F.pad(x, (pad_left[ph], nt - 1 - pad_left[ph])), phase_w[ph].double(), b)
    assert torch.equal(got, ref)
    # the one channels-last conv over the union window: channel ph * cout + co of step s is sample s * u + ph of channel co
    y = F.conv1d(F.pad(x, (cl_pad_left, kk - 1 - cl_pad_left)), cl_w.double(), b.repeat(u))
    assert torch.equal(y.view(B, u, cout, Lx).permute(0, 2, 3, 1).reshape(B, cout, Lx * u), ref)
    # each phase's taps inside the window: [off, off + ntaps), zero outside — what ClProb::ph_offs tells the kernel to skip
    assert cl_pad_left == max(pad_left) and 1 <= kk <= 7
    for ph in range(u):
        assert offs[ph] == cl_pad_left - pad_left[ph] and 0 <= offs[ph] <= 15
        rows = cl_w[ph * cout:(ph + 1) * cout]
        assert torch.equal(rows[:, :, offs[ph]:offs[ph] + nt], phase_w[ph])
        assert rows[:, :, :offs[ph]].abs().sum() == 0 and rows[:, :, offs[ph] + nt:].abs().sum() == 0


@pytest.mark.parametrize("u,k", [(2, 3), (2, 5), (3, 6), (3, 4), (4, 6), (2, 10), (8, 40), (9, 18), (1, 1), (1, 3), (4, 2), (8, 12), (0, 0)])
def test_pairs_outside_the_envelope_are_refused(u, k):
    dims = torch.zeros(2, dtype=torch.int32)
    assert _lib().bv2_test_ups_split(u, k, 4, 4, None, None, None, None, P(dims), None) == -2
