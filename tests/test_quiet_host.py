"""Quieting's host side, no GPU: the design against numpy in every mode, the refusals, the
properties of the restatement (quiet_ref.py) that the GPU tests lean on, the rule behind the default bounds
re-derived through the oracle's demod, and the Python argument checks that need no device."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import iqgen
import meter_ref as M
import oracle
import quiet_ref as Q
from test_meter_host import DEV, _powers, _u8


def _design(fmrx, mode, **kw):
    return fmrx.quiet_design(*Q.RATES[mode], **kw)


# ---- the design ------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", range(4))
@pytest.mark.parametrize("kw", [{}, dict(cut_lo_db=-40.0, cut_hi_db=80.0, mute_lo_db=0.5, mute_hi_db=3.25, mute_depth_db=60.0, corner_hz=8000),
                                dict(mute_depth_db=0.0, corner_hz=2069)])
def test_design_against_numpy(fmrx, mode, kw):
    """pow and exp in double may differ by an ulp of double between libm and numpy, which the rounding to float32
    turns into one float32 ulp at the most; what follows from stored values by exact double arithmetic is equal."""
    got, want = _design(fmrx, mode, **kw), Q.design(*Q.RATES[mode], **kw)
    for k in ("Tc", "Tm", "h"):
        assert got[k].dtype == np.float32 and got[k].shape == want[k].shape
        ulp = np.spacing(np.maximum(np.abs(got[k]), np.abs(want[k])))
        print(f"mode {mode} {k}: {int((got[k] != want[k]).sum())} of {got[k].size} differ from numpy")
        assert np.all(np.abs(got[k].astype(np.float64) - want[k].astype(np.float64)) <= ulp)
    assert np.all(np.diff(got["Tc"]) < 0) and np.all(np.diff(got["Tm"]) < 0)  # level j needs N <= T[j]: T falls
    assert abs(float(got["g0"]) - float(want["g0"])) <= np.spacing(want["g0"])
    Am = Q.A[mode]
    assert got["cg"] == np.float32((1.0 - float(got["g0"])) / (16.0 * Am)) and got["cw"] == np.float32(1.0 / (16.0 * Am))
    assert np.float32(16 * Am) * got["cw"] == np.float32(1.0)  # c = 0 is w = 1 exactly
    assert got["g0"] + np.float32(16 * Am) * got["cg"] <= np.float32(1.0)
    # the one-pole's tail past the 64 taps is below half an ulp of its sum
    assert want["p"] ** 64 < 2.0 ** -25 and abs(float(got["h"].astype(np.float64).sum()) - 1.0) < 1e-6


def test_defaults_and_null_outputs(fmrx):
    cfg = fmrx.QuietConfig()
    assert fmrx.lib().fmrx_quiet_config_default(C.byref(cfg)) == fmrx.FMRX_OK
    assert {k: getattr(cfg, k) for k in Q.DEFAULTS} == Q.DEFAULTS
    assert fmrx.lib().fmrx_quiet_config_default(None) == fmrx.FMRX_EINVAL
    assert fmrx.lib().fmrx_quiet_design(48000, 240000, None, None, None, None, None) == fmrx.FMRX_OK  # every output may be NULL
    Tc = np.zeros(16, np.float32)
    assert fmrx.lib().fmrx_quiet_design(48000, 240000, None, Tc.ctypes.data, None, None, None) == fmrx.FMRX_OK  # NULL: the defaults
    assert np.array_equal(Tc, fmrx.quiet_design(48000, 240000)["Tc"])
    assert (fmrx.QUIET_STEPS, fmrx.QUIET_CARRY, fmrx.QUIET_HIST) == (Q.STEPS, Q.CARRY, Q.HIST)


BAD = [dict(cut_lo_db=34.0), dict(cut_lo_db=35.0), dict(mute_hi_db=36.0), dict(mute_lo_db=50.0), dict(cut_lo_db=-40.5),
       dict(cut_hi_db=80.5), dict(mute_lo_db=-41.0), dict(mute_hi_db=81.0), dict(mute_depth_db=-0.5), dict(mute_depth_db=60.5),
       dict(corner_hz=8001), dict(corner_hz=0), dict(corner_hz=-2500)]
BAD += [{k: v} for k in ("cut_lo_db", "cut_hi_db", "mute_lo_db", "mute_hi_db", "mute_depth_db") for v in (np.nan, np.inf, -np.inf)]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_config_refusals(fmrx, kw):
    out = [np.full(n, -7.0, np.float32) for n in (16, 16, 64, 3)]
    for audio_fs, bp_fs in Q.RATES:
        rc = fmrx.lib().fmrx_quiet_design(audio_fs, bp_fs, C.byref(fmrx.quiet_config(**kw)), *[o.ctypes.data for o in out])
        assert rc == fmrx.FMRX_EINVAL and all(np.all(o == -7.0) for o in out)


def test_corner_bound_and_rate_refusals(fmrx):
    """exp(-128 pi corner / audio_fs) < 2^-25: 2069 Hz at 48 kHz and 1901 Hz at 44.1 kHz pass, one Hz under does not."""
    out = np.full(64, -7.0, np.float32)
    for audio_fs, bp_fs, least in ((48000, 240000, 2069), (44100, 240000, 1901)):
        assert math.exp(-128 * math.pi * least / audio_fs) < 2.0 ** -25 <= math.exp(-128 * math.pi * (least - 1) / audio_fs)
        ok = fmrx.lib().fmrx_quiet_design(audio_fs, bp_fs, C.byref(fmrx.quiet_config(corner_hz=least)), None, None, out.ctypes.data, None)
        assert ok == fmrx.FMRX_OK and out[0] > 0
        out[:] = -7.0
        bad = fmrx.lib().fmrx_quiet_design(audio_fs, bp_fs, C.byref(fmrx.quiet_config(corner_hz=least - 1)), None, None, out.ctypes.data, None)
        assert bad == fmrx.FMRX_EINVAL and np.all(out == -7.0)
    for audio_fs, bp_fs in ((0, 240000), (32000, 240000), (-48000, 240000), (48000, 0), (48000, 250000), (48000, 304000)):
        assert fmrx.lib().fmrx_quiet_design(audio_fs, bp_fs, None, None, None, out.ctypes.data, None) == fmrx.FMRX_EINVAL
        assert np.all(out == -7.0)


# ---- the restatement's properties ----------------------------------------------------------------

def _rows(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.5, 1.5, n).astype(np.float32)
    x[::97] *= np.float32(40.0)
    return x


def test_mode_constants_are_the_issue_s():
    for mode in range(4):
        nif, na, bp_fs = oracle.MODES[mode][1], oracle.MODES[mode][2], oracle.MODES[mode][5]
        assert Q.BLOCKS[mode] * nif == Q.GM[mode] * 64 * (bp_fs // 1000) and Q.BLOCKS[mode] * na == Q.A[mode]
        audio_fs = Q.RATES[mode][0]
        assert Q.RATES[mode][1] == bp_fs and Q.A[mode] * 1000 == audio_fs * Q.GM[mode] * 64  # a meter frame is 64 ms
        assert 16 * Q.A[mode] < 2 ** 24  # the q convert to float exactly


@pytest.mark.parametrize("mode", range(4))
def test_all_16_is_the_identity_on_random_bit_patterns(mode):
    n = Q.A[mode]
    x = np.frombuffer(iqgen.rand_bytes(40 + mode, 4 * n).tobytes(), np.uint32).view(np.float32)
    assert np.isnan(x).any() and np.isinf(x).sum() >= 0
    full = np.full((Q.GM[mode] + 1, 2), 16, np.uint8)
    z, hist, touched = Q.apply(mode, x, full, Q.design(*Q.RATES[mode]))
    assert np.array_equal(z.view(np.uint32), x.view(np.uint32)) and not touched.any()
    assert np.array_equal(hist.view(np.uint32), x[-63:].view(np.uint32))


@pytest.mark.parametrize("mode", (0, 2))
@pytest.mark.parametrize("corner", (2500, 4000))
def test_closed_high_cut_is_the_one_pole_at_10_khz(mode, corner):
    """c = 0 throughout: w = 1, y = fl(x + fl(v - x)), the FIR's output to a rounding.  64 float32 accumulations are
    worth at most about 4e-6 of the amplitude; 1e-4 relative holds the rest as margin."""
    audio_fs = Q.RATES[mode][0]
    d = Q.design(*Q.RATES[mode], corner_hz=corner)
    period = audio_fs // math.gcd(audio_fs, 10000)  # samples of a whole number of cycles
    n = Q.A[mode] // period * period
    w = 2.0 * math.pi * 10000.0 / audio_fs
    x = np.sin(w * np.arange(n)).astype(np.float32)
    rows = np.zeros((Q.GM[mode] + 1, 2), np.uint8)
    rows[:, 1] = 16
    z, _, touched = Q.apply(mode, x, rows, d)
    assert touched.all()
    keep = slice(-(-Q.HIST // period) * period, n)  # whole cycles past the 63 samples of transient
    e = np.exp(-1j * w * np.arange(n))[keep]
    gain = abs(np.sum(z[keep].astype(np.float64) * e)) / abs(np.sum(x[keep].astype(np.float64) * e))
    want = abs((1.0 - d["p"]) / (1.0 - d["p"] * np.exp(-1j * w)))
    print(f"mode {mode} corner {corner}: gain {gain:.6f}, one-pole {want:.6f}")
    assert abs(gain - want) <= 1e-4 * want


@pytest.mark.parametrize("mode", (1, 3))
def test_closed_mute_is_g0(mode):
    d = Q.design(*Q.RATES[mode])
    x = _rows(Q.A[mode], mode)
    for c in (16, 5):
        rows = np.zeros((Q.GM[mode] + 1, 2), np.uint8)
        rows[:, 0] = c
        y_rows = rows.copy()
        y_rows[:, 1] = 16
        y = Q.apply(mode, x, y_rows, d)[0]
        z = Q.apply(mode, x, rows, d)[0]
        assert np.array_equal(z.view(np.uint32), (d["g0"] * y).view(np.uint32))
    assert np.array_equal(Q.apply(mode, x, np.full((Q.GM[mode] + 1, 2), (16, 0), np.uint8), d)[0], d["g0"] * x)


def test_levels_carry_any_split():
    d = Q.design(48000, 240000)
    pw = _powers(5, 37)
    pw[:, 5:7] = (10.0 ** np.random.default_rng(9).uniform(0.0, 4.3, (37, 2))).astype(np.float32)  # across the thresholds
    pw[7] = 0.0
    pw[11, 5], pw[20, 6] = np.nan, np.inf
    whole, c_whole = Q.levels(pw, d)
    assert tuple(whole[0]) == (0, 0) and whole.shape == (38, 2)
    assert tuple(whole[12]) == (0, 0) and tuple(whole[21]) == (0, 0)  # a NaN and an Inf close the stream
    assert len(set(whole[:, 0])) > 3 and len(set(whole[:, 1])) > 2
    for cut in (1, 3, 36):
        r1, c1 = Q.levels(pw[:cut], d)
        r2, c2 = Q.levels(pw[cut:], d, c1)
        assert tuple(r2[0]) == tuple(r1[-1])
        assert np.array_equal(np.concatenate([r1, r2[1:]]), whole)
        assert np.array_equal(c2.view(np.uint32), c_whole.view(np.uint32))
    # a threshold decides: N == T[j] exactly is inside level j's count
    one = np.zeros((4, 7), np.float32)
    one[:, 5] = d["Tc"][3] / np.float32(4.0)
    N = Q.sums(one)[0][-1]
    assert tuple(Q.levels(one, d)[0][-1]) == (int(np.sum(N <= d["Tc"])), int(np.sum(N <= d["Tm"])))
    # a carried level outside 0 .. 16 counts as 0
    bad = np.array([0, 0, 0, 17.0, -1.0, 0, 0, 0], np.float32)
    assert tuple(Q.levels(pw[:2], d, bad)[0][0]) == (0, 0)
    assert tuple(Q.levels(pw[:2], d, np.array([0, 0, 0, 16.0, 3.0, 0, 0, 0], np.float32))[0][0]) == (16, 3)


@pytest.mark.parametrize("mode", (0, 2))
def test_apply_any_split_with_the_history_carried(mode):
    d = Q.design(*Q.RATES[mode])
    Am, Gm = Q.A[mode], Q.GM[mode]
    rng = np.random.default_rng(mode)
    rows = rng.integers(0, 17, (2 * Gm + 1, 2)).astype(np.uint8)
    x = _rows(2 * Am, 3 + mode)
    whole, h_whole, _ = Q.apply(mode, x, rows, d)
    z1, h1, _ = Q.apply(mode, x[:Am], rows[: Gm + 1], d)
    z2, h2, _ = Q.apply(mode, x[Am:], rows[Gm:], d, h1)
    assert np.array_equal(np.concatenate([z1, z2]).view(np.uint32), whole.view(np.uint32))
    assert np.array_equal(h2.view(np.uint32), h_whole.view(np.uint32))
    assert not np.array_equal(Q.apply(mode, x[Am:], rows[Gm:], d)[0], z2)  # the history matters
    # the ramp is continuous across frames: the pair in front of frame f is the one behind frame f - 1
    qc, qm = Q.ramps(mode, 2 * Am, rows)
    step = np.abs(np.diff(qc)).max()
    assert step <= 16 * Gm and qc[0] == int(rows[0, 0]) * Am and qm[Am] == int(rows[Gm, 1]) * Am


# ---- where the defaults come from ------------------------------------------------------------------
# meter_ref.power over the oracle's mode-0 demod of two classes of station and of random bytes, 8 frames: the
# four-frame readings 10 log10(N / 4 / (P / 240)), windows that reach into f < 0 left out.  DESIGN §5.16 records
# the table, with modes 1 to 3 beside it.  All of it is synthetic: nobody has measured an off-air capture.

RULE_FRAMES = 8
RULE_SIGMAS = (0, 16, 40, 80, 160)


def rule_readings(fmrx, orc, mode=0, sigmas=RULE_SIGMAS, frames=RULE_FRAMES):
    """{(class, sigma): the four-frame readings (dB)} in one mode."""
    bb, nif, na, rf_fs, if_fs, bp_fs = oracle.MODES[mode][:6]
    tab = fmrx.meter_design(bp_fs)[1]
    n = frames * 64 * (bp_fs // 1000) * (rf_fs // bp_fs)  # I/Q pairs of the frames
    bits = M.station_bits(0x1234, "TEST  FM", frames * 0.064)
    signals = {"stereo": dict(pilot=0.1 * DEV, lr=0.2 * DEV, rds=0.04 * DEV, audio=0.3 * DEV, bits=bits),
               "mono": dict(pilot=0.0, rds=0.0, audio_hz=1000.0, audio=0.3 * DEV)}
    out = {}

    def read(iq):
        pw = M.power(orc.run(mode, 51, iq, ["demod"])["demod"], tab)
        return Q.reading_db(Q.sums(pw)[0][3:], bp_fs)

    for name, kw in signals.items():
        z = M.fm_signal(mode, n, **kw)
        for sigma in sigmas:
            out[name, sigma] = read(_u8(z, sigma, 7 + sigma))
    out["random", None] = read(iqgen.rand_bytes(5, 2 * n))
    return out


def test_default_rule(fmrx, orc):
    """Every reading at sigma <= 16 is at least 3 dB under cut_lo_db, every reading at sigma <= 80 is under
    mute_lo_db, every reading at sigma 160 is at least mute_lo_db, every reading of random bytes is at least
    mute_hi_db."""
    cfg = fmrx.quiet_config()
    for (name, sigma), db in rule_readings(fmrx, orc).items():
        print(f"{name:7s} sigma {sigma}: {db.min():6.2f} .. {db.max():6.2f} dB")
        assert db.size == RULE_FRAMES - 3 and np.all(np.isfinite(db))
        if sigma is None:
            assert db.min() >= cfg.mute_hi_db, (name, db)
            continue
        if sigma <= 16:
            assert db.max() <= cfg.cut_lo_db - 3.0, (name, sigma, db)
        if sigma <= 80:
            assert db.max() < cfg.mute_lo_db, (name, sigma, db)
        if sigma == 160:
            assert db.min() >= cfg.mute_lo_db, (name, sigma, db)


# ---- Python argument checks that need no device ----------------------------------------------------

def test_python_argument_checks(fmrx):
    rx = fmrx.Receiver.__new__(fmrx.Receiver)  # no context: the checks come first
    rx.n_streams, rx.h = 2, None
    for bad in (np.zeros((2, 3, 6), np.float32), np.zeros((1, 3, 7), np.float32), np.zeros((2, 0, 7), np.float32),
                np.zeros((6, 7), np.float32)):
        with pytest.raises(fmrx.FmrxError) as e:
            rx.quiet_levels(bad)
        assert e.value.code == fmrx.FMRX_EINVAL
    with pytest.raises(fmrx.FmrxError) as e:
        rx.quiet_levels(np.zeros((2, 3, 7), np.float32), carry=np.zeros((2, 7), np.float32))
    assert e.value.code == fmrx.FMRX_EINVAL
    with pytest.raises(TypeError):
        fmrx.quiet_config(cut_db=3.0)
    with pytest.raises(fmrx.FmrxError) as e:
        fmrx.quiet_design(48000, 240000, cut_lo_db=40.0)
    assert e.value.code == fmrx.FMRX_EINVAL
    # every function of the header's section is bound
    for name in ("fmrx_quiet_config_default", "fmrx_quiet_design", "fmrx_quiet_levels", "fmrx_quiet_levels_device",
                 "fmrx_quiet_apply_device", "fmrx_set_quieting", "fmrx_quieting", "fmrx_quiet_get", "fmrx_quiet_hold"):
        assert name in fmrx.PROTOTYPES and name in fmrx.header_symbols()
