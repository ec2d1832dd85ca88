"""An independent restatement of the counter-based noise stream for the tests (it imports nothing from latentblending_amd):
Philox4x32-10 in plain Python integers (the Random123 construction: Salmon et al., SC'11), the pair-wise Box-Muller transform of
include/lb_hip.h in float64 with ``cos(pi t)`` / ``sin(pi t)`` written the plain way, and the SplitMix64 fold of the
trajectory ids.  Scalar and slow on purpose where it defines something; ``words`` has a vectorised twin for the larger shapes,
checked against the scalar form by the CPU tests."""
import math
import struct

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32, MASK64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF

# Random123's known answers for philox4x32_10 (kat_vectors): (ctr, key) -> words
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK32,) * 4, (MASK32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox_scalar(ctr, key):
    c0, c1, c2, c3 = (int(v) & MASK32 for v in ctr)
    k0, k1 = (int(v) & MASK32 for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def words_scalar(row, per_sample):
    """The Philox words of one row (key0, key1, ctr1, ctr2, ctr3) as a list of Python ints."""
    out = []
    for q in range(per_sample // 4):
        out += philox_scalar((q, row[2], row[3], row[4]), (row[0], row[1]))
    return out


def words(rows, per_sample):
    """uint32 [n, per_sample]; 32 x 32 -> 64-bit products from 16-bit halves, so nothing here shares a line with the code under test."""
    n, q = len(rows), per_sample // 4
    r = np.array([[int(v) & MASK32 for v in row] for row in rows], dtype=np.uint64).reshape(n, 5)
    c = [np.tile(np.arange(q, dtype=np.uint64), (n, 1))] + [np.repeat(r[:, k:k + 1], q, axis=1) for k in (2, 3, 4)]
    k0, k1 = np.repeat(r[:, 0:1], q, axis=1), np.repeat(r[:, 1:2], q, axis=1)

    def mul(m, x):                      # (hi, lo) of m * x for 32-bit m, x
        xl, xh = x & np.uint64(0xFFFF), x >> np.uint64(16)
        ml, mh = np.uint64(m & 0xFFFF), np.uint64(m >> 16)
        ll, lh, hl, hh = ml * xl, ml * xh, mh * xl, mh * xh
        mid = (ll >> np.uint64(16)) + (lh & np.uint64(0xFFFF)) + (hl & np.uint64(0xFFFF))
        lo = (ll & np.uint64(0xFFFF)) | ((mid & np.uint64(0xFFFF)) << np.uint64(16))
        hi = hh + (lh >> np.uint64(16)) + (hl >> np.uint64(16)) + (mid >> np.uint64(16))
        return hi & np.uint64(MASK32), lo
    for _ in range(10):
        h0, l0 = mul(M0, c[0])
        h1, l1 = mul(M1, c[2])
        c = [h1 ^ c[1] ^ k0, l1, h0 ^ c[3] ^ k1, l0]
        k0, k1 = (k0 + np.uint64(W0)) & np.uint64(MASK32), (k1 + np.uint64(W1)) & np.uint64(MASK32)
    return np.stack(c, axis=-1).reshape(n, per_sample).astype(np.uint32)


def normals_from_words(w):
    """float64 normals of a uint32 [n, per_sample] word array: (w0, w1) -> elements 0, 1; (w2, w3) -> elements 2, 3."""
    w = np.asarray(w, dtype=np.uint32)
    u1 = ((w[:, 0::2] >> np.uint32(8)).astype(np.float64) + 0.5) / 2.0 ** 24
    t = ((w[:, 1::2] >> np.uint32(8)).astype(np.float64) + 0.5) / 2.0 ** 23
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.empty(w.shape, dtype=np.float64)
    z[:, 0::2] = r * np.cos(np.pi * t)
    z[:, 1::2] = r * np.sin(np.pi * t)
    return z


def normal_pair_scalar(wa, wb):
    """The same through ``math``, one pair at a time."""
    u1 = ((wa >> 8) + 0.5) / 2.0 ** 24
    t = ((wb >> 8) + 0.5) / 2.0 ** 23
    r = math.sqrt(-2.0 * math.log(u1))
    return r * math.cos(math.pi * t), r * math.sin(math.pi * t)


def normals_f64(rows, per_sample):
    return normals_from_words(words(rows, per_sample))


def normals_f16(rows, per_sample):
    return normals_f64(rows, per_sample).astype(np.float16)


# ---- trajectory ids: SplitMix64's finaliser folded over (tag, *words) -------------------------
TAG_ANCHOR, TAG_MID, TAG_FREE = 1, 2, 3


def mix64(z):
    z &= MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def fold(*ws):
    h = 0
    for w in ws:
        h = mix64(h + 0x9E3779B97F4A7C15 + (int(w) & MASK64))
    return h


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def row_of(tid, step, kind=0):
    return (tid & MASK32, tid >> 32, step, kind, 0)


def mixed_rows():
    """Rows that exercise every word: zeros, all ones, and a few ordinary (id, step) rows."""
    rows = [(0, 0, 0, 0, 0), (MASK32,) * 5, (1, 0, 0, 0, 0), (0, 0, 0, 0, 1)]
    rows += [row_of(fold(TAG_ANCHOR, 420), s) for s in (0, 3)]
    rows += [row_of(fold(TAG_MID, 420, 421, f64_bits(0.375), 2), 2), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822)]
    return rows
