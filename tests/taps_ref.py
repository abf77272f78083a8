"""tests/taps_ref.py — helper of the demod-row taps' tests (not a test).

The composed reference: what every tap on the demod rows of a tuned call -- the subcarrier meter, soft stereo's
levels and apply, de-emphasis, the RDS decode with its block sync, the AFC carrier sums -- must report after
a list of calls, per stream, from ONE oracle run of the capture and the numpy restatements meter_ref,
afc_ref, blend_ref, deemph_ref, rds_ref and rds_sync_ref.  Nothing here comes from the library under test
except its design tables (meter_design, blend_design, deemph_design), which the per-stage tests fetch too.
Everything is compared for equality, never with a tolerance.

Also the signal makers: station() and reference() of soft stereo's tests (tests/test_gpu_blend.py imports
them from here) and rds_capture(), test_gpu_rds_decode.station_iq's clean station in any mode.
"""
from __future__ import annotations

import hashlib

import numpy as np

import afc_ref as A
import blend_ref as B
import deemph_ref as dr
import meter_ref as M
import oracle
import rds_ref as R
import rds_sync_ref as S
from test_meter_host import _u8

SWITCHES = ("meter", "rds", "sync", "afc", "blend", "deemph")
ALL_MONO = frozenset(("meter", "rds", "sync", "afc"))
ALL_STEREO = frozenset(SWITCHES)
TAU = 50
PI, PS = 0x54A8, "RADIO 42"  # test_gpu_rds_decode's station

_cache: dict = {}


def _digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).view(np.uint8)).digest()


# ---- signals ------------------------------------------------------------------------------------------

def dev_of(mode):
    """test_meter_host's DEV at the mode's demod rate: the broadcast's peak deviation in radians a sample."""
    return 2.0 * np.pi * 75000.0 / oracle.MODES[mode][5]


def station(mode, frames, sigmas, pilot=0.05, seed=7, pi=0x1234, ps="TEST  FM", rds=0.04, run=4):
    """A stereo station with RDS as u8 at amplitude 100 (read-only): frames meter frames, Gaussian noise of
    sigmas[i] LSB over the i-th run of `run` frames (the last one to the end).  pilot = 0 and rds = 0 leave the
    subcarrier out."""
    key = ("iq", mode, frames, tuple(sigmas), pilot, seed, pi, ps, rds, run)
    if key not in _cache:
        bb, nif = oracle.MODES[mode][0], oracle.MODES[mode][1]
        blocks = frames * M.frame_samples(mode) // nif
        assert blocks * nif == frames * M.frame_samples(mode)
        n, dev = blocks * bb // 2, dev_of(mode)
        z = M.fm_signal(mode, n, pilot=pilot * dev, lr=0.2 * dev, rds=rds * dev, audio=0.3 * dev,
                        bits=M.station_bits(pi, ps, frames * 0.064 + 0.1))
        per = run * (n // frames)
        parts = []
        for i, sg in enumerate(sigmas):
            lo, hi = i * per, n if i == len(sigmas) - 1 else (i + 1) * per
            parts.append(_u8(z[lo:hi], sg, seed + i))
        iq = np.concatenate(parts)
        iq.setflags(write=False)
        _cache[key] = iq
    return _cache[key]


def reference(orc, fm, mode, iq, key, tau=0):
    """(pcm, level row with entry 0, blended floats, powers) of one stream over the whole of iq from the reset."""
    if (key, tau) not in _cache:
        o = orc.run(mode, 51, iq, ["left", "right", "demod"])
        pw = M.power(o["demod"], fm.meter_design(oracle.MODES[mode][5])[1])
        row, _ = B.levels(pw, fm.blend_design())
        y = B.apply(mode, np.stack([o["right"], o["left"]], axis=1), row)
        if tau:
            pcm = dr.pcm_stereo(orc, y[:, 1], y[:, 0], fm.deemph_design(48000 if mode < 2 else 44100, tau))
        else:
            pcm = B.quant(orc, y)
        for a in (pcm, row, y, pw):
            a.setflags(write=False)
        _cache[key, tau] = (pcm, row, y, pw, orc.quant(np.stack([o["right"], o["left"]], axis=1).reshape(-1)))
    return _cache[key, tau]


def rds_capture(mode, granules, pi=PI, ps=PS, seed=1):
    """test_gpu_rds_decode.station_iq's station (rds_ref.fm_signal: 1 kHz tone, pilot, RDS, no L-R) at offset 0
    through rds_ref.to_u8's defaults, in any mode: `granules` RDS granules as u8 (read-only)."""
    key = ("rds", mode, granules, pi, ps, seed)
    if key not in _cache:
        secs = granules * R.granule_samples(mode) / R.bp_fs(mode)
        bits = R.stream_bits(R.groups(pi, ps, None, R.n_groups_for(secs)))
        iq = R.to_u8(R.fm_signal(mode, int(round(secs * oracle.MODES[mode][3])), bits, seed=seed))
        assert iq.size == granules * B.BLOCKS[mode] * oracle.MODES[mode][0]
        iq.setflags(write=False)
        _cache[key] = iq
    return _cache[key]


def audio_fs(mode):
    return 48000 if mode < 2 else 44100


# ---- the composed reference ---------------------------------------------------------------------------

def frames_of(mode, blocks):
    """The meter frames of a call of `blocks` blocks (whole RDS granules)."""
    assert blocks % B.BLOCKS[mode] == 0, "whole granules"
    return blocks // B.BLOCKS[mode] * B.GM[mode]


def demod_reports(orc, fm, mode, demod, calls, switches):
    """The reports of one stream whose demod row over all the calls is `demod`: calls in blocks, switches a
    subset of SWITCHES.  A tap that is off reports its power-on values."""
    nif, bp = oracle.MODES[mode][1], oracle.MODES[mode][5]
    demod = np.asarray(demod, np.float32)
    assert demod.size == sum(calls) * nif
    P, fs = bp // 1000, M.frame_samples(mode)
    out = {"meter": (np.zeros(7, np.float64), 0), "detect": None, "afc": (np.float64(0.0), np.float64(0.0), 0),
           "rds": R.parse(np.zeros(0, np.uint8), np.zeros(0, np.uint8)), "ext": S.ext_dict(S.ext_init()),
           "rows": [], "hist": [0] * 17, "row": None}
    need_pw = {"meter", "blend"} & set(switches)
    tab = fm.meter_design(bp)[1] if need_pw else None
    T = fm.blend_design() if "blend" in switches else None
    carry, f0 = None, 0
    for nb in calls:
        F = frames_of(mode, nb)
        part = demod[f0 * fs: (f0 + F) * fs]
        f0 += F
        if need_pw:
            pw = M.power(part, tab)
        if "meter" in switches:
            out["meter"] = M.accumulate(pw, *out["meter"])
        if "blend" in switches:
            row, carry = B.levels(pw, T, carry)
            out["rows"].append(row)
        if "afc" in switches:
            out["afc"] = A.accumulate(A.sums(part, P), out["afc"])
    assert f0 * fs == demod.size
    if "meter" in switches:
        out["detect"] = M.detect(*out["meter"])
    if "blend" in switches:
        out["hist"] = B.histogram(out["rows"])
        out["row"] = np.concatenate([out["rows"][0]] + [r[1:] for r in out["rows"][1:]])
        assert all(int(a[-1]) == int(b[0]) for a, b in zip(out["rows"], out["rows"][1:]))  # the level carried in
    if "rds" in switches:
        key = ("rdsd", mode, _digest(demod))
        if key not in _cache:
            _cache[key] = R.from_demod(orc, mode, demod)
        dec = _cache[key]
        out["rds"] = dec["info"]
        if "sync" in switches:
            out["ext"] = S.parse_stream(dec["bits"])
    return out


def oracle_run(orc, mode, iq, stereo):
    """The one oracle run of a capture: demod and the taps-off PCM, plus left and right on a stereo context."""
    key = ("run", mode, bool(stereo), _digest(iq))
    if key not in _cache:
        o = orc.run(mode, 51, iq, ["demod", "pcm", "left", "right"] if stereo else ["demod", "pcm_mono"])
        for v in o.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = o
    return _cache[key]


def oracle_demod(orc, mode, iq):
    """The oracle's demod of a capture alone."""
    key = ("demod", mode, _digest(iq))
    if key not in _cache:
        for stereo in (False, True):
            if ("run", mode, stereo, key[2]) in _cache:
                return _cache["run", mode, stereo, key[2]]["demod"]
        _cache[key] = orc.run(mode, 51, iq, ["demod"])["demod"]
        _cache[key].setflags(write=False)
    return _cache[key]


def expected(orc, fm, mode, iq, calls, switches, stereo):
    """What every tap reports after `calls` (blocks each, whole RDS granules) of the u8 capture iq on a MONO or
    STEREO context with `switches` on, and the PCM of those calls: demod_reports' dict plus pcm_off (every
    tap off) and pcm (soft stereo and de-emphasis applied where they are on; otherwise pcm_off)."""
    assert set(switches) <= set(SWITCHES) and (stereo or not {"blend"} & set(switches))
    assert iq.size == sum(calls) * oracle.MODES[mode][0]
    o = oracle_run(orc, mode, iq, stereo)
    out = demod_reports(orc, fm, mode, o["demod"], calls, switches)
    out["pcm_off"] = o["pcm"] if stereo else o["pcm_mono"]
    out["pcm"] = out["pcm_off"]
    h = fm.deemph_design(audio_fs(mode), TAU) if "deemph" in switches else None
    if stereo and ("blend" in switches or h is not None):
        y = np.stack([o["right"], o["left"]], axis=1)
        if "blend" in switches:
            y = B.apply(mode, y, out["row"])
        out["pcm"] = dr.pcm_stereo(orc, y[:, 1], y[:, 0], h) if h is not None else B.quant(orc, y)
    elif h is not None:
        raise AssertionError("the matrix de-emphasises stereo contexts only")
    return out


# ---- the matrix's captures and call patterns -------------------------------------------------------------
# MONO contexts decode rds_capture's clean station (the RDS conditions of tests/test_taps_host.py hold on it);
# STEREO contexts decode station() with runs of noise, so that soft stereo's levels visit 16, <= 4 and the range
# between.  Mode 0 keeps test_gpu_rds_sync's 6 granules, mode 1 has 24 (1.536 s); a granule of modes 2 and 3
# is 1.28 s already.

GRANULES = {0: 6, 1: 24, 2: 1, 3: 1}
STEREO_KW = {0: dict(sigmas=(2, 80), run=3), 1: dict(sigmas=(2, 80, 40, 16, 2, 2)),
             2: dict(sigmas=(2, 80, 40, 16, 2), seed=32), 3: dict(sigmas=(2, 80, 40, 16, 2), seed=33)}


def capture(mode, stereo, granules=None):
    g = GRANULES[mode] if granules is None else granules
    return station(mode, g * B.GM[mode], **STEREO_KW[mode]) if stereo else rds_capture(mode, g)


def patterns(mode, granules):
    """The call patterns of a capture of `granules` granules, in blocks, to run in turn on one context with a
    reset between them.  From six granules on (the matrix's modes 0 and 1 have 6 and 24) the first is small, large,
    small: 1, 3, 2 granules and the rest.  It comes first because a reset does not shrink a row: on a fresh
    context the second call regrows every row and carries its history over, and the third runs below the stride.
    Then the capture as one call (which regrows the rows once more where there is a rest) and a granule at a
    time, at the largest stride.  Below six granules nothing regrows while history is held."""
    g = B.BLOCKS[mode]
    out = []
    if granules >= 6:
        out.append([k * g for k in (1, 3, 2, granules - 6) if k > 0])
        assert sum(out[-1]) == granules * g
    out.append([granules * g])
    if granules > 1:
        out.append([g] * granules)
    return out
