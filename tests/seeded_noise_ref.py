"""numpy restatement of the seeded-noise generator (csrc/kernels/rng.h, DESIGN.md "Seeded noise"): the reference of
tests/test_seeded_noise_cpu.py and tests/test_seeded_noise_gpu.py.  The integer core in uint64 arithmetic, the normal in fp64.

    key     = (seed & 0xffffffff, seed >> 32)            seed: the int64's bit pattern as uint64
    counter = (t, row >> 2, which, 0)                    which: 0 = noise_w, 1 = noise_z, 2 = noise_q
    w[0..3] = philox4x32_10(counter, key)
    p       = (row >> 1) & 1;  a = w[2p], b = w[2p+1]
    u1 = ((a >> 9) + 0.5) * 2^-23,  u2 = ((b >> 9) + 0.5) * 2^-23
    value   = sqrt(-2 ln u1) * (cos(2 pi u2) if row is even else sin(2 pi u2))
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: four, key: two array-likes of 32-bit words (broadcast together) -> four uint64 arrays holding 32-bit words."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in ctr]
    k0, k1 = (np.asarray(v, dtype=np.uint64) & MASK for v in key)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]                      # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & MASK, (p0 >> S32) ^ c[3] ^ k1, p0 & MASK]
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return c


def philox4x32_10_py(ctr, key):
    """The same in plain Python integers (the known-answer vectors are checked through both)."""
    c, k = [int(v) & 0xFFFFFFFF for v in ctr], [int(v) & 0xFFFFFFFF for v in key]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + W0) & 0xFFFFFFFF, (k[1] + W1) & 0xFFFFFFFF]
    return c


def seeded_normal(seed, which, row, t):
    """fp64 value(s) at (seed, which, row, t); the four arguments broadcast (seed: int64 or Python ints in the int64 range)."""
    s = np.asarray(seed, dtype=np.int64).astype(np.uint64)       # the bit pattern
    row = np.asarray(row, dtype=np.int64)
    t = np.asarray(t, dtype=np.int64)
    which = np.asarray(which, dtype=np.int64)
    s, which, row, t = np.broadcast_arrays(s, which, row, t)
    w = philox4x32_10((t.astype(np.uint64), (row >> 2).astype(np.uint64), which.astype(np.uint64), np.zeros(t.shape, np.uint64)),
                      (s & MASK, s >> S32))
    p = ((row >> 1) & 1).astype(bool)
    a = np.where(p, w[2], w[0])
    b = np.where(p, w[3], w[1])
    u1 = ((a >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = ((b >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    r = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    return np.where(row & 1, r * np.sin(ang), r * np.cos(ang))


def fill(seeds, which, rows, T, lengths=None):
    """fp64 [B, rows, T]: what bv2_seeded_noise writes (frames at or past lengths[b] are 0)."""
    seeds = np.asarray(seeds, dtype=np.int64)
    out = seeded_normal(seeds[:, None, None], which, np.arange(rows)[None, :, None], np.arange(T)[None, None, :])
    if lengths is not None:
        out = np.where(np.arange(T)[None, None, :] < np.asarray(lengths, dtype=np.int64)[:, None, None], out, 0.0)
    return out
