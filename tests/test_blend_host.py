"""Soft stereo's host side, no GPU: the thresholds against numpy, the refusals, the properties
of the restatement (blend_ref.py) that the GPU tests lean on, the rule behind the default hi_db re-derived
through the oracle's demod, and the Python argument checks that need no device."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import blend_ref as B
import iqgen
import meter_ref as M
import oracle
from test_meter_host import DEV, _powers, _u8


def test_design_against_numpy(fmrx):
    for kw in ({}, {"lo_db": 3.0, "hi_db": 30.0}, {"lo_db": -20.0, "hi_db": 60.0}):
        got = fmrx.blend_design(**kw)
        want = B.design(kw.get("lo_db", B.LO_DB), kw.get("hi_db", B.HI_DB))
        assert got.dtype == np.float32 and got.shape == want.shape == (16,)
        diff = got != want
        print(f"{kw}: {int(diff.sum())} of 16 thresholds differ from numpy")
        ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp)
        assert np.all(np.diff(got) > 0)
    T = fmrx.blend_design()
    assert T[0] == np.float32(5.0)  # 0.5 * 10^(10 / 10): the meter's pilot threshold with the guard bins' mean folded in
    assert abs(float(T[15]) - 0.5 * 10 ** 2.2) <= np.spacing(T[15])


def test_defaults(fmrx):
    cfg = fmrx.BlendConfig()
    assert fmrx.lib().fmrx_blend_config_default(C.byref(cfg)) == fmrx.FMRX_OK
    assert (np.float32(cfg.lo_db), np.float32(cfg.hi_db)) == (B.LO_DB, B.HI_DB) == (np.float32(10.0), np.float32(22.0))
    assert np.float32(cfg.lo_db) == M.PILOT_MIN_SNR_DB
    assert fmrx.lib().fmrx_blend_config_default(None) == fmrx.FMRX_EINVAL
    T = np.zeros(16, np.float32)
    assert fmrx.lib().fmrx_blend_design(None, T.ctypes.data) == fmrx.FMRX_OK  # NULL: the defaults
    assert np.array_equal(T, fmrx.blend_design())
    assert (fmrx.BLEND_STEPS, fmrx.BLEND_CARRY) == (B.STEPS, B.CARRY)


@pytest.mark.parametrize("lo,hi", [(10.0, 10.0), (22.0, 10.0), (-20.5, 10.0), (10.0, 60.5), (np.nan, 22.0), (10.0, np.nan),
                                   (-np.inf, 22.0), (10.0, np.inf)])
def test_config_refusals(fmrx, lo, hi):
    T = np.full(16, -7.0, np.float32)
    cfg = fmrx.BlendConfig(lo, hi)
    assert fmrx.lib().fmrx_blend_design(C.byref(cfg), T.ctypes.data) == fmrx.FMRX_EINVAL
    assert np.all(T == -7.0)
    assert fmrx.lib().fmrx_blend_design(C.byref(fmrx.BlendConfig(10.0, 22.0)), None) == fmrx.FMRX_EINVAL


# ---- the restatement's properties ----------------------------------------------------------------

def _rows(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.5, 1.5, 2 * n).astype(np.float32)
    x[::97] *= np.float32(40.0)
    return x.reshape(n, 2)


def test_mode_constants_are_the_issue_s():
    for mode in range(4):
        bb, nif, na, _, _, bp_fs = oracle.MODES[mode][:6]
        frame = 64 * (bp_fs // 1000)
        assert B.BLOCKS[mode] * nif == B.GM[mode] * frame and B.BLOCKS[mode] * na == B.A[mode]
        assert 16 * B.A[mode] < 2 ** 24  # q converts to float exactly


@pytest.mark.parametrize("mode", range(4))
def test_all_16_is_the_identity_and_0_is_mono(mode):
    n = B.A[mode]
    x = _rows(n, mode)
    x[5, 0], x[9, 1] = np.nan, np.inf
    full = np.full(B.GM[mode] + 1, 16, np.uint8)
    assert np.array_equal(B.apply(mode, x, full).view(np.uint32), x.view(np.uint32))
    k, passes = B.mix(mode, n, full)
    assert passes.all() and np.all(k == 0)
    k0, p0 = B.mix(mode, n, np.zeros(B.GM[mode] + 1, np.uint8))
    assert not p0.any() and np.all(k0 == np.float32(0.5))  # 16 A c rounds to 0.5 exactly in every mode
    # |L' - R'| within one ulp of the larger input: exactly L - e and R + e differ by the rounding of d = fl(L - R)
    # alone (e = d / 2 is exact), the two results round to neighbours at most.  (Where L is near -R the mono
    # sum is near zero and has a far finer ulp of its own; the inputs' is the one that can be promised.)
    x0 = _rows(n, 10 + mode)
    y = B.apply(mode, x0, np.zeros(B.GM[mode] + 1, np.uint8))
    gap = np.abs(y[:, 1].astype(np.float64) - y[:, 0].astype(np.float64))
    assert np.all(gap <= np.spacing(np.max(np.abs(x0), axis=1)))


def test_ramp_is_linear_and_continuous_across_frames():
    mode = 2
    row = np.array([0] + [16] * 19 + [4] + [16] * 20, np.uint8)  # two granules; a change at frames 19 -> 20
    k, passes = B.mix(mode, 2 * B.A[mode], row)
    assert k[0] == np.float32(0.5) and not passes[0]
    f1 = -(-B.A[mode] // 20)  # the first audio frame of meter frame 1
    assert passes[f1:B.A[mode] - 2822].all()  # frames 1 .. 18 at 16 either side
    assert np.all(np.diff(k[:f1].astype(np.float64)) <= 0)
    assert not passes[B.A[mode]] and abs(float(k[B.A[mode]]) - 12 / 32) < 1e-6  # the granule boundary: level 4 reached
    assert abs(float(k[B.A[mode] - 1]) - 12 / 32) < 1e-3 and np.all(np.abs(np.diff(k.astype(np.float64))) < 1e-3)


def test_levels_carry_any_split():
    T = B.design()
    pw = _powers(5, 37)
    pw[7] = 0.0
    pw[11, 1], pw[20, 0] = np.nan, np.inf
    whole, c_whole = B.levels(pw, T)
    assert whole[0] == 0 and whole.shape == (38,)
    for cut in (1, 3, 36):
        r1, c1 = B.levels(pw[:cut], T)
        r2, c2 = B.levels(pw[cut:], T, c1)
        assert r2[0] == r1[-1]
        assert np.array_equal(np.concatenate([r1, r2[1:]]), whole)
        assert np.array_equal(c2.view(np.uint32), c_whole.view(np.uint32))
    # a threshold decides: S / G = 2 T[j] exactly is level j + 1 at powers of two
    one = np.zeros((4, 7), np.float32)
    one[:, 1], one[:, 0], one[:, 2] = 16.0, 0.5, 0.5  # 10 log10(2 S / G) = 15.05 dB
    assert B.levels(one, T)[0][-1] == int(np.sum(16.0 >= T * np.float32(1.0)))


# ---- where the default hi_db comes from ------------------------------------------------------------
# meter_ref.power over the oracle's mode-0 demod of test_meter_host's classes, 12 frames: the four-frame
# readings 10 log10(2 S / G).  Measured here (dB): pilot 0.1 with L-R at 0.2: see the print-out of the test;
# DESIGN §5.14 records the table.

RULE_FRAMES = 12
RULE_SIGMAS = (0, 2, 16, 40, 80)


def four_frame_db(pw):
    T = B.design()
    a, g = pw[:, 1], pw[:, 0] + pw[:, 2]
    out = []
    for f in range(3, pw.shape[0]):
        S = ((a[f - 3] + a[f - 2]) + a[f - 1]) + a[f]
        G = ((g[f - 3] + g[f - 2]) + g[f - 1]) + g[f]
        out.append(10.0 * np.log10(2.0 * float(S) / float(G)))
    return np.array(out), B.levels(pw, T)[0][4:]


def test_default_hi_db_rule(fmrx, orc):
    """hi_db stays 22 if every four-frame reading of the pilot classes at sigma <= 16 is at least 1 dB above
    it; otherwise it is 1 dB below the lowest such reading."""
    tab = fmrx.meter_design(240000)[1]
    n = RULE_FRAMES * 24 * 6400
    bits = M.station_bits(0x1234, "TEST  FM", RULE_FRAMES * 0.064)
    signals = {"pilot 0.1": dict(pilot=0.1 * DEV, lr=0.2 * DEV, rds=0.04 * DEV, audio=0.3 * DEV, bits=bits),
               "pilot 0.05": dict(pilot=0.05 * DEV, rds=0.04 * DEV, audio=0.3 * DEV, bits=bits),
               "no pilot": dict(pilot=0.0, rds=0.0, audio_hz=14000.0, audio=0.8 * DEV)}
    lowest = np.inf
    for name, kw in signals.items():
        z = M.fm_signal(0, n, **kw)
        for sigma in RULE_SIGMAS:
            pw = M.power(orc.run(0, 51, _u8(z, sigma, 7 + sigma), ["demod"])["demod"], tab)
            db, lv = four_frame_db(pw)
            print(f"{name:10s} sigma {sigma:2d}: {db.min():6.2f} .. {db.max():6.2f} dB, levels {lv.min()} .. {lv.max()}")
            if name.startswith("pilot") and sigma <= 16:
                lowest = min(lowest, db.min())
                assert lv.min() == 16, (name, sigma)  # a good station is untouched
            if name == "no pilot":
                assert db.max() < float(B.LO_DB) - 6.0 and lv.max() == 0, sigma
    cfg = fmrx.blend_config()
    want = 22.0 if lowest >= 23.0 else lowest - 1.0
    print(f"lowest reading of the pilot classes at sigma <= 16: {lowest:.2f} dB -> hi_db {want:.2f}")
    assert abs(cfg.hi_db - want) < 0.005


# ---- Python argument checks that need no device ----------------------------------------------------

def test_python_argument_checks(fmrx):
    rx = fmrx.Receiver.__new__(fmrx.Receiver)  # no context: the checks come first
    rx.n_streams, rx.h = 2, None
    for bad in (np.zeros((2, 3, 6), np.float32), np.zeros((1, 3, 7), np.float32), np.zeros((2, 0, 7), np.float32),
                np.zeros((6, 7), np.float32)):
        with pytest.raises(fmrx.FmrxError) as e:
            rx.blend_levels(bad)
        assert e.value.code == fmrx.FMRX_EINVAL
    with pytest.raises(fmrx.FmrxError) as e:
        rx.blend_levels(np.zeros((2, 3, 7), np.float32), carry=np.zeros((2, 7), np.float32))
    assert e.value.code == fmrx.FMRX_EINVAL
    with pytest.raises(ValueError):
        fmrx.decode_stations(np.zeros(16, np.uint8), blend=True)  # channels defaults to MONO
    with pytest.raises(fmrx.FmrxError) as e:
        fmrx.blend_design(lo_db=30.0)
    assert e.value.code == fmrx.FMRX_EINVAL
    # every function of the header's section is bound
    for name in ("fmrx_blend_config_default", "fmrx_blend_design", "fmrx_blend_levels", "fmrx_blend_levels_device",
                 "fmrx_blend_apply_device", "fmrx_set_stereo_blend", "fmrx_stereo_blend", "fmrx_blend_get", "fmrx_blend_hold"):
        assert name in fmrx.PROTOTYPES and name in fmrx.header_symbols()
