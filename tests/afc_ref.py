"""tests/afc_ref.py — helper of the AFC tests (not a test).

The numpy restatement of include/fmrx.h's AFC section: the carrier sums in float32 with an
explicit loop over i and the two stride-halving folds, accumulate and the decision in float64.  Everything
the GPU writes is compared with this for equality, never with a tolerance.
"""
from __future__ import annotations

import math

import numpy as np

W = 64
DEFAULTS = dict(step_hz=1000, deadband_hz=1000, max_pull_hz=50000, frames=16, track=1, max_mean_square=1.0)


def _fold(a: np.ndarray, first: int) -> np.ndarray:
    """a_j = fl(a_j + a_{j+s}) for j < s, s = first, first / 2, .. 1, along the last axis; a_0."""
    a = a.copy()
    s = first
    while s >= 1:
        a[..., :s] = a[..., :s] + a[..., s: 2 * s]
        s //= 2
    return a[..., 0]


def sums(demod: np.ndarray, P: int) -> np.ndarray:
    """One stream's row (whole frames of 64 windows of P samples) -> float32 (frames, 2): S, Q."""
    x = np.asarray(demod, np.float32)
    F = x.size // (W * P)
    assert F * W * P == x.size and P % 16 == 0, "whole frames"
    x = x.reshape(F, W, P // 16, 16)
    with np.errstate(all="ignore"):
        a = np.zeros((F, W, 16), np.float32)
        b = np.zeros((F, W, 16), np.float32)
        for i in range(P // 16):
            v = x[:, :, i, :]
            p = v * v  # float32: the product rounded, then the sum
            a = a + v
            b = b + p
        assert a.dtype == np.float32 and b.dtype == np.float32
        return np.stack([_fold(_fold(a, 8), W // 2), _fold(_fold(b, 8), W // 2)], axis=-1)


def accumulate(sq: np.ndarray, report=None):
    """The report after these frames: (sum, sumsq, frames) in float64, sequential and ascending."""
    s, q, n = (np.float64(0.0), np.float64(0.0), 0) if report is None else report
    for row in np.asarray(sq, np.float32).reshape(-1, 2):
        s = s + np.float64(row[0])
        q = q + np.float64(row[1])
        n += 1
    return np.float64(s), np.float64(q), n


def _round_half_away(x: float) -> float:
    return math.copysign(math.floor(abs(x) + 0.5), x)


def decide(report, bp_fs: int, **kw) -> dict:
    cfg = {**DEFAULTS, **kw}
    s, q, frames = report
    assert frames > 0
    n = 64.0 * float(bp_fs // 1000) * float(frames)
    mean, ms = float(s) / n, float(q) / n
    err = math.asin(min(1.0, max(-1.0, mean))) * float(bp_fs) / (2.0 * math.pi)
    carrier = int(ms <= float(np.float32(cfg["max_mean_square"])))
    corr = 0
    if carrier and abs(err) >= cfg["deadband_hz"]:
        corr = int(cfg["step_hz"] * _round_half_away(err / cfg["step_hz"]))
    return {"err_hz": err, "mean": mean, "mean_square": ms, "carrier": carrier, "correction_hz": corr}


def report_of(demod: np.ndarray, P: int):
    return accumulate(sums(demod, P))


# ---- test signals -----------------------------------------------------------------------------
# Capture 5 of the meter's tests (pilot + L-R + RDS, pilot + L-R, mono audio alone) with every carrier off its
# raster point, by 7, -13 and 31 kHz; the second station is loud (audio = 1.2 rad a sample of the IF rate,
# about 46 kHz deviation), so its reading shrinks and it needs a second retune.  A fourth stream sits on a
# raster point that holds no station.  Mode 0 throughout.

FRAME_PAIRS = 24 * 6400  # an RDS granule of 24 blocks is one 64 ms frame
TUNED = [-600000, 100000, 700000, 400000]  # what a scan on the 100 kHz raster reports; the last is empty
TRUE = [-593000, 87000, 731000]
STATION_KW = [dict(pilot=0.05, lr=0.10, rds=0.04, audio_hz=1000.0), dict(pilot=0.05, lr=0.10, rds=0.0, audio_hz=2000.0, audio=1.2),
              dict(pilot=0.0, lr=0.0, rds=0.0, audio_hz=3000.0)]
_cache = {}


def stations_iq(frames: int, shift_hz: float = 0.0, offsets=None, kws=None, rf_fs: int | None = None) -> np.ndarray:
    """The sum of the stations as complex samples at rf_fs (the mode's rate when None), unit amplitude each."""
    import meter_ref as M
    import oracle

    offsets = TRUE if offsets is None else offsets
    kws = STATION_KW if kws is None else kws
    key = (frames, shift_hz, tuple(offsets), repr(kws), rf_fs)
    if key not in _cache:
        fs = rf_fs or oracle.MODES[0][3]
        n = frames * FRAME_PAIRS * fs // oracle.MODES[0][3]
        bits = M.station_bits(0x4D54, "METER FM", frames * 0.064)
        _cache[key] = sum(M.fm_signal(0, n, offset_hz=off + shift_hz, rf_fs=rf_fs, bits=bits, seed=k + 1, **kw)
                          for k, (off, kw) in enumerate(zip(offsets, kws)))
    return _cache[key]


def landing_capture(frames: int) -> np.ndarray:
    """u8 I/Q of the three stations: amplitude 38 each, 2 LSB of noise."""
    import rds_ref as R

    if ("u8", frames) not in _cache:
        _cache["u8", frames] = R.to_u8(stations_iq(frames), amp=38.0, noise_lsb=2.0)
    return _cache["u8", frames]


SCAN = [-600000, 100000, 700000]
CAPTURE5_KW = [dict(pilot=0.05, lr=0.10, rds=0.04, audio_hz=1000.0), dict(pilot=0.05, lr=0.10, rds=0.0, audio_hz=2000.0),
               dict(pilot=0.0, lr=0.0, rds=0.0, audio_hz=3000.0)]


def shifted_capture5():
    """Capture 5 of the meter's tests, 20 frames, every carrier 7 kHz up (a crystal's error)."""
    import rds_ref as R

    if "shifted" not in _cache:
        _cache["shifted"] = R.to_u8(stations_iq(20, shift_hz=7000.0, offsets=SCAN, kws=CAPTURE5_KW), amp=38.0, noise_lsb=2.0)
    return _cache["shifted"]


def tracking_capture(kind):
    """8 frames holding the first two stations, 7 and -13 kHz off their raster points: u8 at the mode's rate, at
    twice it, or at 10 MS/s (25/6 of it)."""
    import oracle
    import rds_ref as R

    if ("track", kind) not in _cache:
        fs = {"narrow": None, "decim2": 2 * oracle.MODES[0][3], "rate": 10000000}[kind]
        z = stations_iq(8, offsets=TRUE[:2], kws=STATION_KW[:2], rf_fs=fs)
        _cache["track", kind] = R.to_u8(z, amp=55.0, noise_lsb=2.0)
    return _cache["track", kind]


def reference_rule(orc, iq_u8: np.ndarray, tuned, calls: int, call_frames: int, **kw) -> list:
    """The tracking rule in float64 on a shared u8 capture of mode 0: per call and stream the front end of
    meter_ref.demod_f64 (the oracle's RF taps) at the stream's current offset, afc_ref's sums and decision over
    the call, the offset moved within origin +- max_pull_hz.  A list a stream of (offsets after every call,
    decisions)."""
    import meter_ref as M

    cfg = {**DEFAULTS, **kw}
    z = M.u8_complex(iq_u8)
    per = call_frames * FRAME_PAIRS
    out = []
    for origin in tuned:
        off, offs, decs = origin, [], []
        for c in range(calls):
            d = M.demod_f64(orc, 0, z[c * per: (c + 1) * per], off)
            dec = decide(report_of(d, 240), 240000, **kw)
            off = min(origin + cfg["max_pull_hz"], max(origin - cfg["max_pull_hz"], off + dec["correction_hz"]))
            offs.append(off)
            decs.append(dec)
        out.append((offs, decs))
    return out
