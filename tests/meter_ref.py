"""tests/meter_ref.py — helper of the subcarrier meter's tests (not a test).

The numpy restatement of include/fmrx.h's meter section: float32 arrays throughout, an
explicit loop over i, the two stride-halving folds, accumulate and detect in float64.  Everything the GPU
writes is compared with this for equality, never with a tolerance.  Also a multiplex generator with
switches for pilot, L-R and RDS on rds_ref's pieces, and a float64 front end (rotate, RF low-pass,
decimate, discriminate) that is used only to choose test signals, never as a reference for bits.
"""
from __future__ import annotations

import numpy as np

import iqgen
import oracle
import rds_ref as R

TONES = (17, 19, 21, 56, 58, 61, 63)
W = 64
PILOT_MIN_SNR_DB, RDS_MIN_SNR_DB = np.float32(10.0), np.float32(1.94)
FLOOR = 1e-30


def window(mode: int) -> int:
    return R.bp_fs(mode) // 1000


def frame_samples(mode: int) -> int:
    return W * window(mode)


def design(bp_fs: int) -> np.ndarray:
    """The tables in numpy: float32 of shape (7, 2, P)."""
    P = bp_fs // 1000
    n = np.arange(P, dtype=np.int64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n.astype(np.float64) / P)
    out = np.zeros((len(TONES), 2, P), np.float32)
    for t, k in enumerate(TONES):
        a = 2.0 * np.pi * ((k * n) % P).astype(np.float64) / P
        out[t, 0] = (w * np.cos(a)).astype(np.float32)
        out[t, 1] = (w * np.sin(a)).astype(np.float32)
    return out


def _fold(a: np.ndarray, first: int) -> np.ndarray:
    """a_j = fl(a_j + a_{j+s}) for j < s, s = first, first / 2, .. 1, along the last axis; a_0."""
    a = a.copy()
    s = first
    while s >= 1:
        a[..., :s] = a[..., :s] + a[..., s: 2 * s]
        s //= 2
    return a[..., 0]


def power(demod: np.ndarray, tables: np.ndarray) -> np.ndarray:
    """One stream's row (whole frames) -> float32 (frames, 7)."""
    tables = np.asarray(tables, np.float32)
    P = tables.shape[2]
    x = np.asarray(demod, np.float32)
    F = x.size // (W * P)
    assert F * W * P == x.size, "whole frames"
    x = x.reshape(F, W, P // 16, 16)
    out = np.zeros((F, len(TONES)), np.float32)
    with np.errstate(all="ignore"):
        for t in range(len(TONES)):
            part = []
            for cs in range(2):
                tab = tables[t, cs].reshape(P // 16, 16)
                a = np.zeros((F, W, 16), np.float32)
                for i in range(P // 16):
                    a = a + x[:, :, i, :] * tab[i]  # float32: the product rounded, then the sum
                part.append(_fold(a, 8))
            re, im = part
            p = re * re + im * im
            assert p.dtype == np.float32
            out[:, t] = _fold(p, W // 2)
    return out


def accumulate(pw: np.ndarray, sums=None, frames: int = 0):
    """The report after these frames: (sum[7] float64, frames), sequential and ascending."""
    sums = np.zeros(len(TONES), np.float64) if sums is None else np.array(sums, np.float64)
    for row in np.asarray(pw, np.float32).reshape(-1, len(TONES)):
        sums = sums + row.astype(np.float64)
    return sums, frames + np.asarray(pw).reshape(-1, len(TONES)).shape[0]


def detect(sums, frames: int, pilot_min=PILOT_MIN_SNR_DB, rds_min=RDS_MIN_SNR_DB) -> dict:
    s = np.asarray(sums, np.float64)
    assert frames > 0
    with np.errstate(all="ignore"):
        pilot = np.maximum(s[1], FLOOR)
        guard = np.maximum((s[0] + s[2]) / 2.0, FLOOR)
        side = np.maximum((s[3] + s[4]) / 2.0, FLOOR)
        above = np.maximum((s[5] + s[6]) / 2.0, FLOOR)
        pilot_snr = 10.0 * np.log10(pilot / guard)
        rds_snr = 10.0 * np.log10(side / above)
        n = 64.0 * float(frames)
        return {"pilot_db": np.float32(10.0 * np.log10(pilot / n)), "pilot_snr_db": np.float32(pilot_snr),
                "rds_db": np.float32(10.0 * np.log10(side / n)), "rds_snr_db": np.float32(rds_snr),
                "stereo": int(pilot_snr >= np.float64(np.float32(pilot_min))),
                "rds": int(rds_snr >= np.float64(np.float32(rds_min)))}


def levels(demod: np.ndarray, tables: np.ndarray, **kw) -> dict:
    sums, frames = accumulate(power(demod, tables))
    return detect(sums, frames, **kw)


# ---- test signals -----------------------------------------------------------------------------

def multiplex(t: np.ndarray, bits=None, pilot: float = 0.05, rds: float = 0.04, lr: float = 0.0, audio_hz: float = 1000.0,
              audio: float = 0.30, lr_hz: float = 700.0, noise: float = 0.002, seed: int = 1) -> np.ndarray:
    """rds_ref.multiplex's signal with switches: mono audio tone, pilot (amplitude 0 = none), L-R as a
    double-sideband tone pair around 38 kHz, RDS on 57 kHz (0 or bits None = none)."""
    m = audio * np.sin(2 * np.pi * audio_hz * t)
    if pilot:
        m = m + pilot * np.cos(2 * np.pi * 19000.0 * t)
    if lr:
        m = m + lr * np.sin(2 * np.pi * lr_hz * t) * np.cos(2 * np.pi * 38000.0 * t)
    if rds and bits is not None:
        d = np.bitwise_xor.accumulate(np.asarray(bits, np.uint8))
        sym = 2.0 * d.astype(np.float64) - 1.0
        ph = t * R.BITRATE
        k = np.floor(ph).astype(np.int64)
        m = m + rds * sym[k % sym.size] * np.where(ph - k < 0.5, 1.0, -1.0) * np.cos(2 * np.pi * 57000.0 * t)
    nz = (iqgen.rand_bytes(seed + 17, t.size).astype(np.float64) - 127.5) / 127.5
    return m + noise * nz


def fm_signal(mode: int, n_pairs: int, offset_hz: float = 0.0, rf_fs: int | None = None, **kw) -> np.ndarray:
    """rds_ref.fm_signal over this file's multiplex: complex128, unit amplitude."""
    fs = rf_fs or oracle.MODES[mode][3]
    rf_decim = oracle.MODES[mode][3] // oracle.MODES[mode][5]
    n = np.arange(n_pairs, dtype=np.float64)
    mpx = multiplex(n / fs, **kw) * (oracle.MODES[mode][3] / fs)
    return np.exp(1j * (np.cumsum(mpx / rf_decim) + 2 * np.pi * offset_hz * n / fs))


def station_bits(pi: int, ps: str, seconds: float) -> np.ndarray:
    return R.stream_bits(R.groups(pi, ps, None, R.n_groups_for(seconds)))


def demod_f64(orc, mode: int, z: np.ndarray, offset_hz: float = 0.0) -> np.ndarray:
    """A float64 front end over normalised complex samples at rf_fs: rotate by -offset, the 51-tap RF
    low-pass, decimate, the discriminator (I dQ - Q dI) / (I^2 + Q^2).  For choosing signals only."""
    rf_fs, bp = oracle.MODES[mode][3], oracle.MODES[mode][5]
    dec = rf_fs // bp
    n = np.arange(z.size, dtype=np.float64)
    y = z * np.exp(-2j * np.pi * offset_hz * n / rf_fs)
    h = orc.lpf(float(rf_fs), 100000.0, 51, 1).astype(np.float64)
    y = np.convolve(y, h)[: z.size][::dec]
    prev = np.concatenate(([0.0], y[:-1]))
    den = np.abs(y) ** 2
    with np.errstate(all="ignore"):
        d = (y.real * (y.imag - prev.imag) - y.imag * (y.real - prev.real)) / den
    return np.where(den > 0, d, 0.0).astype(np.float32)


def u8_complex(iq: np.ndarray) -> np.ndarray:
    a = (np.asarray(iq, np.uint8).astype(np.float64) - 128.0) / 128.0
    return a[0::2] + 1j * a[1::2]
