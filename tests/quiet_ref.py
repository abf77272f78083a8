"""tests/quiet_ref.py — helper of quieting's tests (not a test).

The numpy restatement of include/fmrx.h's quieting section: float32 arrays throughout, an explicit
four-term sum, integer qc and qm, a 64-tap FIR accumulated in ascending k, pass-through where a q is 16 A.
Everything the GPU writes is compared with this for equality on the bits, never with a tolerance.

One thing the definition leaves open and canon() closes for the comparison, as blend_ref's does: the bits of a
NaN that the arithmetic itself makes or passes on (Inf - Inf in v - x, a NaN through g y).  canon() maps every NaN
of a sample that either step touched to 0x7FC00000 on both sides.  Samples that pass both steps (qc == qm == 16 A)
are compared as they are, payload included.
"""
from __future__ import annotations

import math

import numpy as np

from blend_ref import A, BLOCKS, GM  # the granule's constants are soft stereo's

STEPS, CARRY, TAPS, HIST = 16, 8, 64, 63
DEFAULTS = dict(cut_lo_db=22.0, cut_hi_db=34.0, mute_lo_db=36.0, mute_hi_db=44.0, mute_depth_db=20.0, corner_hz=2500)
N61, N63 = 5, 6                      # the meter's tones the levels read
RATES = ((48000, 240000), (48000, 288000), (44100, 240000), (44100, 256000))  # (audio_fs, bp_fs) of modes 0..3


def design(audio_fs: int, bp_fs: int, **kw) -> dict:
    k = dict(DEFAULTS, **kw)
    Am = {48000: 3072, 44100: 56448}[audio_fs]
    P = bp_fs // 1000
    j = np.arange(STEPS, dtype=np.float64)

    def thresholds(lo, hi):
        lo, hi = float(np.float32(lo)), float(np.float32(hi))
        return (4.0 * (P / 240.0) * 10.0 ** ((hi - j * (hi - lo) / 15.0) / 10.0)).astype(np.float32)

    p = math.exp(-2.0 * math.pi * k["corner_hz"] / audio_fs)
    h, r = np.zeros(TAPS, np.float32), 1.0 - p
    for n in range(TAPS):
        h[n] = np.float32(r)
        r = r * p
    g0 = np.float32(10.0 ** (-float(np.float32(k["mute_depth_db"])) / 20.0))
    return {"Tc": thresholds(k["cut_lo_db"], k["cut_hi_db"]), "Tm": thresholds(k["mute_lo_db"], k["mute_hi_db"]), "h": h,
            "g0": g0, "cg": np.float32((1.0 - float(g0)) / (16.0 * Am)), "cw": np.float32(1.0 / (16.0 * Am)), "p": p}


def reading_db(N, bp_fs: int = 240000) -> np.ndarray:
    """The four-frame sum N as the dB the thresholds are stated in."""
    with np.errstate(all="ignore"):
        return 10.0 * np.log10(np.asarray(N, np.float64) / 4.0 / ((bp_fs // 1000) / 240.0))


def sums(power, carry=None) -> np.ndarray:
    """N_f float32 (F) of one stream's powers (F, 7)."""
    pw = np.asarray(power, np.float32).reshape(-1, 7)
    c = np.zeros(CARRY, np.float32) if carry is None else np.asarray(carry, np.float32)
    F = pw.shape[0]
    with np.errstate(all="ignore"):
        n = np.concatenate([c[0:3], pw[:, N61] + pw[:, N63]]).astype(np.float32)  # frames -3 .. F - 1
        N = ((n[0:F] + n[1:F + 1]) + n[2:F + 2]) + n[3:F + 3]
    assert N.dtype == np.float32
    return N, n


def levels(power, d: dict, carry=None):
    """One stream: power float32 (F, 7), a design, carry (8 floats; None: zeros) ->
    (rows uint8 (F + 1, 2): pair 0 the carried-in (c, m), pair 1 + f frame f's; the next carry)."""
    c = np.zeros(CARRY, np.float32) if carry is None else np.asarray(carry, np.float32)
    N, n = sums(power, c)
    F = N.shape[0]
    with np.errstate(all="ignore"):
        lc = (N[:, None] <= d["Tc"][None, :]).sum(axis=1).astype(np.uint8)  # a NaN compares false
        lm = (N[:, None] <= d["Tm"][None, :]).sum(axis=1).astype(np.uint8)
    first = [np.uint8(v) if 0.0 <= v <= 16.0 else np.uint8(0) for v in (c[3], c[4])]
    rows = np.concatenate([[first], np.stack([lc, lm], axis=1)]).astype(np.uint8)
    nxt = np.array([n[F], n[F + 1], n[F + 2], np.float32(rows[-1, 0]), np.float32(rows[-1, 1]), 0.0, 0.0, 0.0], np.float32)
    return rows, nxt


def ramps(mode: int, n: int, rows) -> tuple[np.ndarray, np.ndarray]:
    """(qc, qm) int64 (n) of audio frames 0 .. n - 1 of a call whose level pairs are `rows` (E, 2)."""
    Am, Gm = A[mode], GM[mode]
    rows = np.asarray(rows, np.int64).reshape(-1, 2)
    i = np.arange(n, dtype=np.int64)
    r, a = i // Am, i % Am
    u = a * Gm
    f, t = r * Gm + u // Am, u % Am
    qc = rows[f, 0] * (Am - t) + rows[f + 1, 0] * t
    qm = rows[f, 1] * (Am - t) + rows[f + 1, 1] * t
    assert max(qc.max(initial=0), qm.max(initial=0)) <= 16 * Am < 2 ** 24
    return qc, qm


def fir(x, h, hist=None) -> np.ndarray:
    """v float32 (n): acc = fl(acc + fl(h[k] x[n - k])) from 0, k ascending; hist: the 63 inputs in front (None: zeros)."""
    x = np.asarray(x, np.float32)
    xx = np.concatenate([np.zeros(HIST, np.float32) if hist is None else np.asarray(hist, np.float32), x])
    acc = np.zeros(x.size, np.float32)
    with np.errstate(all="ignore"):
        for k in range(TAPS):
            acc = acc + h[k] * xx[HIST - k: HIST - k + x.size]
    assert acc.dtype == np.float32
    return acc


def apply(mode: int, x, rows, d: dict, hist=None):
    """One row (a stream's channel): x float32 (n) through the two steps by the level pairs ->
    (z float32 (n), the next history (63), touched bool (n): a step did arithmetic on the sample)."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    full = 16 * A[mode]
    qc, qm = ramps(mode, x.size, rows)
    with np.errstate(all="ignore"):
        v = fir(x, d["h"], hist)
        w = (full - qc).astype(np.float32) * d["cw"]
        e = w * (v - x)
        y = np.where(qc == full, x, x + e)
        g = d["g0"] + qm.astype(np.float32) * d["cg"]
        z = np.where(qm == full, y, g * y)
    assert z.dtype == np.float32 and w.dtype == np.float32 and g.dtype == np.float32
    xx = np.concatenate([np.zeros(HIST, np.float32) if hist is None else np.asarray(hist, np.float32), x])
    return z, xx[-HIST:].copy(), (qc != full) | (qm != full)


def apply_rows(mode: int, x, rows, d: dict, hist=None):
    """One stream: x float32 (n, channels) (interleaved frames), hist (channels, 63) ->
    (z (n, channels), next history (channels, 63), touched (n))."""
    x = np.ascontiguousarray(x, np.float32)
    x = x.reshape(x.shape[0], -1)
    out = [apply(mode, x[:, ch], rows, d, None if hist is None else np.asarray(hist, np.float32).reshape(-1, HIST)[ch])
           for ch in range(x.shape[1])]
    return np.stack([o[0] for o in out], axis=1), np.stack([o[1] for o in out]), out[0][2]


def canon(z, touched) -> np.ndarray:
    """The bits (uint32) of rows (n, channels) with every NaN of a touched sample set to 0x7FC00000."""
    z = np.ascontiguousarray(z, np.float32)
    z = z.reshape(z.shape[0], -1)
    b = z.view(np.uint32).copy()
    b[np.isnan(z) & np.asarray(touched, bool)[:, None]] = 0x7FC00000
    return b


def quant(orc, z) -> np.ndarray:
    """S16 of floats (interleaved as they are) through the oracle's quantiser."""
    return orc.quant(np.ascontiguousarray(z, np.float32).reshape(-1))


def histograms(rows_of_calls) -> tuple[list, list]:
    """(cut_frames, mute_frames) of a stream whose calls' level pairs are given (pair 0 of each is carried in)."""
    hc, hm = [0] * 17, [0] * 17
    for rows in rows_of_calls:
        for c, m in np.asarray(rows).reshape(-1, 2)[1:]:
            hc[int(c)] += 1
            hm[int(m)] += 1
    return hc, hm
