"""tests/blend_ref.py — helper of soft stereo's tests (not a test).

The numpy restatement of include/fmrx.h's soft-stereo section: float32 arrays throughout, an
explicit four-term sum, integer q, pass-through where q == 16 A.  Everything the GPU writes is compared
with this for equality on the bits, never with a tolerance.

One thing the definition leaves open and canon() closes for the comparison: the bits of a NaN that the
arithmetic itself makes (Inf - Inf in L - R, in L - e).  IEEE 754 fixes neither its sign nor its payload;
x86 makes 0xFFC00000, the GPU 0x7FC00000.  canon() maps every NaN of a blended (not passed-through) pair to
0x7FC00000 on both sides.  Pairs that pass through (q == 16 A) are compared as they are, payload included.
"""
from __future__ import annotations

import numpy as np

GM = (1, 1, 20, 20)                  # meter frames a granule, modes 0..3
A = (3072, 3072, 56448, 56448)       # audio frames a granule
BLOCKS = (24, 24, 3, 1)              # blocks a granule
LO_DB, HI_DB = np.float32(10.0), np.float32(22.0)
STEPS, CARRY = 16, 8


def design(lo_db=LO_DB, hi_db=HI_DB) -> np.ndarray:
    lo, hi = float(np.float32(lo_db)), float(np.float32(hi_db))
    j = np.arange(STEPS, dtype=np.float64)
    return (0.5 * 10.0 ** ((lo + j * (hi - lo) / 15.0) / 10.0)).astype(np.float32)


def levels(power, T, carry=None):
    """One stream: power float32 (F, 7), thresholds T (16), carry (8 floats; None: zeros) ->
    (row uint8 (F + 1): entry 0 the carried-in level, entry 1 + f frame f's; the next carry)."""
    pw = np.asarray(power, np.float32).reshape(-1, 7)
    T = np.asarray(T, np.float32)
    c = np.zeros(CARRY, np.float32) if carry is None else np.asarray(carry, np.float32)
    F = pw.shape[0]
    with np.errstate(all="ignore"):
        a = np.concatenate([c[0:3], pw[:, 1]]).astype(np.float32)            # frames -3 .. F - 1
        g = np.concatenate([c[3:6], pw[:, 0] + pw[:, 2]]).astype(np.float32)
        S = ((a[0:F] + a[1:F + 1]) + a[2:F + 2]) + a[3:F + 3]
        G = ((g[0:F] + g[1:F + 1]) + g[2:F + 2]) + g[3:F + 3]
        assert S.dtype == np.float32 and G.dtype == np.float32
        prod = T[None, :] * G[:, None]
        assert prod.dtype == np.float32
        lv = (S[:, None] >= prod).sum(axis=1).astype(np.uint8)               # a NaN compares false
    first = np.uint8(c[6]) if 0.0 <= c[6] <= 16.0 else np.uint8(0)
    row = np.concatenate([[first], lv]).astype(np.uint8)
    nxt = np.array([a[F], a[F + 1], a[F + 2], g[F], g[F + 1], g[F + 2], np.float32(row[-1]), 0.0], np.float32)
    return row, nxt


def mix(mode: int, n: int, row) -> tuple[np.ndarray, np.ndarray]:
    """(k float32 (n), passes bool (n)) of audio frames 0 .. n - 1 of a call whose level row is `row`."""
    Am, Gm = A[mode], GM[mode]
    row = np.asarray(row, np.int64)
    i = np.arange(n, dtype=np.int64)
    r, a = i // Am, i % Am
    u = a * Gm
    f, t = r * Gm + u // Am, u % Am
    q = row[f] * (Am - t) + row[f + 1] * t
    c = np.float32(1.0 / (32.0 * Am))
    k = (16 * Am - q).astype(np.float32) * c
    assert k.dtype == np.float32 and q.max(initial=0) <= 16 * Am < 2 ** 24
    return k, q == 16 * Am


def apply(mode: int, rl, row) -> np.ndarray:
    """One stream's (n, 2) float32 (R, L) rows blended by the level row: (n, 2) float32."""
    x = np.ascontiguousarray(rl, np.float32).reshape(-1, 2)
    k, passes = mix(mode, x.shape[0], row)
    R, L = x[:, 0], x[:, 1]
    with np.errstate(all="ignore"):
        d = L - R
        e = k * d
        out = np.stack([R + e, L - e], axis=1)
    assert out.dtype == np.float32
    out[passes] = x[passes]
    return out


def canon(y, passes) -> np.ndarray:
    """The bits (uint32) of blended rows with every NaN the arithmetic could have made set to 0x7FC00000."""
    b = np.ascontiguousarray(y, np.float32).reshape(-1, 2).view(np.uint32).copy()
    made = np.isnan(np.asarray(y, np.float32).reshape(-1, 2)) & ~np.asarray(passes, bool)[:, None]
    b[made] = 0x7FC00000
    return b


def quant(orc, y) -> np.ndarray:
    """Interleaved R, L int16 of (n, 2) floats through the oracle's quantiser."""
    return orc.quant(np.ascontiguousarray(y, np.float32).reshape(-1))


def histogram(rows) -> list:
    """level_frames of a stream whose calls' rows are given (entry 0 of each is a carried-in level)."""
    h = [0] * 17
    for row in rows:
        for v in np.asarray(row)[1:]:
            h[int(v)] += 1
    return h
