"""The subcarrier meter's host side, no GPU: the tables against numpy, the refusals, the
report and the decision against meter_ref.py bit for bit, and the separation of the classes (pilot or
none, RDS or none) re-derived through the oracle's demod."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import iqgen
import meter_ref as M
import rds_ref as R


def bits_eq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("bp_fs", [240000, 256000, 288000])
def test_design_against_numpy(fmrx, bp_fs):
    P, got = fmrx.meter_design(bp_fs)
    want = M.design(bp_fs)
    assert P == bp_fs // 1000 and got.shape == want.shape == (7, 2, P)
    diff = got != want
    print(f"bp_fs {bp_fs}: {int(diff.sum())} of {got.size} entries differ from numpy")
    assert diff.mean() <= 0.01
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp)
    assert np.all(got[:, :, 0] == 0)  # the Hann window starts at zero
    assert fmrx.METER_TONES_KHZ == M.TONES


@pytest.mark.parametrize("bp_fs", [0, -240000, 250000, 8000, 304000, 480000])
def test_design_refusals(fmrx, bp_fs):
    p = C.c_int(-5)
    tab = np.full(14 * 480, -7.0, np.float32)
    assert fmrx.lib().fmrx_meter_design(bp_fs, C.byref(p), tab.ctypes.data) == fmrx.FMRX_EINVAL
    assert p.value == -5 and np.all(tab == -7.0)


def test_small_windows_are_designed(fmrx):
    P, tab = fmrx.meter_design(16000)
    assert P == 16 and tab.shape == (7, 2, 16)


def _powers(seed, frames):
    raw = np.frombuffer(iqgen.rand_bytes(seed, 4 * 7 * frames).tobytes(), np.uint32)
    return ((raw / 2.0 ** 32) ** 4 * 1e4 + 1e-3).astype(np.float32).reshape(frames, 7)


def test_accumulate_and_detect_equal_the_restatement(fmrx):
    pw = _powers(3, 5)
    whole = fmrx.meter_accumulate(pw)
    parts = fmrx.meter_accumulate(pw[3:], fmrx.meter_accumulate(pw[:3]))
    sums, frames = M.accumulate(pw)
    for rep in (whole, parts):
        assert rep.frames == frames == 5 and bits_eq(np.array(rep.sum), sums)
    for kw in ({}, {"pilot_min_snr_db": -3.5}, {"rds_min_snr_db": 0.25}):
        got = fmrx.meter_detect(whole, **kw)
        want = M.detect(sums, frames, kw.get("pilot_min_snr_db", M.PILOT_MIN_SNR_DB), kw.get("rds_min_snr_db", M.RDS_MIN_SNR_DB))
        for k in ("pilot_db", "pilot_snr_db", "rds_db", "rds_snr_db"):
            assert bits_eq(np.float32(got[k]), want[k]), k
        assert (got["stereo"], got["rds"]) == (want["stereo"], want["rds"])
    # the thresholds decide: a report whose ratios are known
    rep = fmrx.MeterReport()
    rep.frames = 2
    for t, v in enumerate((1.0, 10.0, 1.0, 4.0, 4.0, 2.0, 2.0)):
        rep.sum[t] = v
    lv = fmrx.meter_detect(rep)
    assert abs(lv["pilot_snr_db"] - 10.0) < 1e-5 and abs(lv["rds_snr_db"] - 3.0103) < 1e-4 and (lv["stereo"], lv["rds"]) == (1, 1)
    assert abs(lv["pilot_db"] - 10 * np.log10(10.0 / 128)) < 1e-5
    assert (fmrx.meter_detect(rep, pilot_min_snr_db=10.5)["stereo"], fmrx.meter_detect(rep, rds_min_snr_db=3.1)["rds"]) == (0, 0)


def test_defaults_and_refusals(fmrx):
    cfg = fmrx.MeterConfig()
    assert fmrx.lib().fmrx_meter_config_default(C.byref(cfg)) == fmrx.FMRX_OK
    assert (np.float32(cfg.pilot_min_snr_db), np.float32(cfg.rds_min_snr_db)) == (M.PILOT_MIN_SNR_DB, M.RDS_MIN_SNR_DB)
    out = fmrx.Subcarriers()
    assert fmrx.lib().fmrx_meter_detect(C.byref(fmrx.MeterReport()), None, C.byref(out)) == fmrx.FMRX_EINVAL  # no frames
    assert fmrx.lib().fmrx_meter_detect(None, None, C.byref(out)) == fmrx.FMRX_EINVAL
    assert fmrx.lib().fmrx_meter_accumulate(None, None, 0) == fmrx.FMRX_EINVAL
    silent = fmrx.meter_detect(fmrx.meter_accumulate(np.zeros((1, 7), np.float32)))  # the floor, no log of zero
    assert silent["pilot_snr_db"] == 0.0 and silent["rds_snr_db"] == 0.0 and silent["stereo"] == 0


# ---- the separation of the classes through the oracle's demod -----------------------------------
# u8 at amplitude 100 with Gaussian noise of sigma LSB on I and on Q, 6 frames (0.384 s) of mode 0.  Levels
# are fractions of the broadcast's peak deviation of 75 kHz: the multiplex, in radians a sample of the IF
# rate, is the fraction times DEV (a pilot at 0.1 is 7.5 kHz, RDS at 0.04 is 3 kHz, as on the air).

FRAMES = 6
SIGMAS = (2, 16, 40)
DEV = 2.0 * np.pi * 75000.0 / 240000.0
_levels = {}


def _u8(z, sigma, seed):
    rng = np.random.default_rng(seed)
    out = np.empty(2 * z.size)
    out[0::2] = 128.0 + 100.0 * z.real
    out[1::2] = 128.0 + 100.0 * z.imag
    return np.clip(np.round(out + rng.normal(0.0, sigma, out.size)), 0, 255).astype(np.uint8)


def class_levels(fmrx, orc, sigma):
    """{signal: meter_ref.detect's dict} at this noise, computed once."""
    if sigma not in _levels:
        tab = fmrx.meter_design(240000)[1]
        n = FRAMES * 24 * 6400
        bits = M.station_bits(0x1234, "TEST  FM", FRAMES * 0.064)
        signals = {"pilot 0.1 + rds": dict(pilot=0.1 * DEV, rds=0.04 * DEV, audio=0.3 * DEV, bits=bits),
                   "pilot 0.05 + rds": dict(pilot=0.05 * DEV, rds=0.04 * DEV, audio=0.3 * DEV, bits=bits),
                   "mono 14 kHz": dict(pilot=0.0, rds=0.0, audio_hz=14000.0, audio=0.8 * DEV),
                   "mono 15 kHz": dict(pilot=0.0, rds=0.0, audio_hz=15000.0, audio=0.8 * DEV)}
        out = {}
        for name, kw in signals.items():
            iq = _u8(M.fm_signal(0, n, **kw), sigma, 7 + sigma)
            out[name] = M.levels(orc.run(0, 51, iq, ["demod"])["demod"], tab)
        out["random bytes"] = M.levels(orc.run(0, 51, iqgen.rand_bytes(5, 2 * n), ["demod"])["demod"], tab)
        for name, lv in out.items():
            print(f"sigma {sigma:2d} {name:17s} pilot_snr {lv['pilot_snr_db']:6.2f} dB  rds_snr {lv['rds_snr_db']:6.2f} dB")
        _levels[sigma] = out
    return _levels[sigma]


@pytest.mark.parametrize("sigma", SIGMAS)
def test_pilot_classes_stay_6_db_either_side_of_the_default(fmrx, orc, sigma):
    """Measured (dB, run of 6 frames): with a pilot at 0.1 / 0.05 of deviation 26.4 / 26.3 at sigma 2, 25.6 /
    23.7 at 16, 22.7 / 18.1 at 40; without one -0.5 .. +0.4.  The default of 10 dB has 8 dB and more either side."""
    lv = class_levels(fmrx, orc, sigma)
    for name, v in lv.items():
        if name.startswith("pilot"):
            assert v["pilot_snr_db"] >= M.PILOT_MIN_SNR_DB + 6.0 and v["stereo"] == 1, (name, v)
        else:
            assert v["pilot_snr_db"] <= M.PILOT_MIN_SNR_DB - 6.0 and v["stereo"] == 0, (name, v)


@pytest.mark.parametrize("sigma", SIGMAS)
def test_rds_classes_stay_2_db_either_side_of_the_default(fmrx, orc, sigma):
    """Measured (dB, run of 6 frames): with RDS at 0.04 of deviation 12.9 at sigma 2, 9.1 at 16, 3.98 at 40;
    without it -0.75 .. -0.10.  3.98 is less than 2 dB above 3 dB, so the default is the midpoint of 3.98 and
    -0.10, 1.94 dB, with 2.04 dB either side."""
    lv = class_levels(fmrx, orc, sigma)
    for name, v in lv.items():
        if name.startswith("pilot"):
            assert v["rds_snr_db"] >= M.RDS_MIN_SNR_DB + 2.0 and v["rds"] == 1, (name, v)
        else:
            assert v["rds_snr_db"] <= M.RDS_MIN_SNR_DB - 2.0 and v["rds"] == 0, (name, v)
