"""AFC's host side, no GPU: the exports, the defaults, the decision against afc_ref.py on
hand-made reports, every refusal, and the report's independence of how a stream is split into calls."""
from __future__ import annotations

import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import afc_ref as A
import iqgen

BP_FS = 240000
ENTRY_POINTS = ["fmrx_carrier", "fmrx_carrier_device", "fmrx_carrier_accumulate", "fmrx_afc_config_default", "fmrx_afc_decide",
                "fmrx_set_afc", "fmrx_afc_get"]


def bits_eq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def report(fmrx, mean, ms=0.25, frames=16, bp_fs=BP_FS):
    """A report whose mean and mean square are the given ones (up to the rounding of the products)."""
    n = 64.0 * (bp_fs // 1000) * frames
    r = fmrx.CarrierReport()
    r.sum, r.sumsq, r.frames = mean * n, ms * n, frames
    return r


def mean_of(hz, bp_fs=BP_FS):
    """The demod mean of an unmodulated carrier hz above the tuned offset: the sine of the phase step."""
    return math.sin(2.0 * math.pi * hz / bp_fs)


def as_ref(r):
    return np.float64(r.sum), np.float64(r.sumsq), int(r.frames)


def same(got, want):
    # libm's asin is not specified to the bit: a few units in the last place of a double, everything else exactly
    assert abs(got["err_hz"] - want["err_hz"]) <= 4 * np.spacing(abs(want["err_hz"])), (got, want)
    for k in ("mean", "mean_square", "carrier", "correction_hz"):
        assert got[k] == want[k], (k, got, want)


def test_the_library_exports_the_entry_points(fmrx):
    assert set(ENTRY_POINTS) <= set(fmrx.header_symbols()) and set(ENTRY_POINTS) <= set(fmrx.PROTOTYPES)
    out = subprocess.run(["nm", "-D", "--defined-only", fmrx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRY_POINTS) <= names
    # the kernel's three instantiations (P = 240, 256, 288), by the host stubs' names as test_variants_host reads them
    table = subprocess.run(["nm", "-C", fmrx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for ni in (15, 16, 18):
        assert f"carrier_kernel<{ni}>" in table, ni


def test_config_default(fmrx):
    cfg = fmrx.afc_config_default()
    want = dict(A.DEFAULTS)
    assert cfg.as_dict() == want == dict(step_hz=1000, deadband_hz=1000, max_pull_hz=50000, frames=16, track=1, max_mean_square=1.0)
    assert fmrx.lib().fmrx_afc_config_default(None) == fmrx.FMRX_EINVAL


@pytest.mark.parametrize("bp_fs", [240000, 256000, 288000])
def test_decide_equals_the_restatement(fmrx, bp_fs):
    for hz, ms, frames in ((7000.0, 0.25, 16), (-13000.0, 0.3, 3), (31000.0, 0.9, 16), (120.0, 0.05, 1), (5100.0, 6.0, 16),
                           (-2500.0, 0.1, 7), (2500.0, 0.1, 7)):
        r = report(fmrx, mean_of(hz, bp_fs), ms, frames, bp_fs)
        same(fmrx.afc_decide(r, bp_fs), A.decide(as_ref(r), bp_fs))
    r = report(fmrx, mean_of(7400.0, bp_fs), 0.2, 16, bp_fs)
    for kw in (dict(step_hz=2500), dict(deadband_hz=8000), dict(max_mean_square=0.1), dict(step_hz=1, deadband_hz=0)):
        same(fmrx.afc_decide(r, bp_fs, **kw), A.decide(as_ref(r), bp_fs, **kw))
    big = report(fmrx, 1.5, 0.5, 2, bp_fs)  # a mean past 1 is clamped: a quarter of the rate
    same(fmrx.afc_decide(big, bp_fs), A.decide(as_ref(big), bp_fs))
    assert fmrx.afc_decide(big, bp_fs)["correction_hz"] == bp_fs // 4


def test_decide_on_hand_made_reports(fmrx):
    d = fmrx.afc_decide(report(fmrx, mean_of(7000.0)), BP_FS)
    assert abs(d["err_hz"] - 7000.0) <= 1e-6 * 7000.0 and d["correction_hz"] == 7000 and d["carrier"] == 1
    for hz, want in ((499.0, 0), (-499.0, 0), (1500.0, 2000), (-1500.0, -2000)):
        d = fmrx.afc_decide(report(fmrx, mean_of(hz)), BP_FS)
        assert d["correction_hz"] == want, (hz, d)
        same(d, A.decide(as_ref(report(fmrx, mean_of(hz))), BP_FS))
    # the gate: a mean square of 1.0 passes, the next double above it does not
    n = 64.0 * 240 * 16
    r = report(fmrx, mean_of(7000.0))
    r.sumsq = n
    assert fmrx.afc_decide(r, BP_FS)["carrier"] == 1 and fmrx.afc_decide(r, BP_FS)["correction_hz"] == 7000
    r.sumsq = n * float(np.nextafter(1.0, 2.0))  # n is a power of two times 15: the quotient is that double exactly
    d = fmrx.afc_decide(r, BP_FS)
    assert d["mean_square"] == float(np.nextafter(1.0, 2.0)) and d["carrier"] == 0 and d["correction_hz"] == 0
    assert abs(d["err_hz"] - 7000.0) <= 1e-6 * 7000.0  # the reading stays, only the correction is withheld


BAD = [dict(step_hz=0), dict(step_hz=-1000), dict(frames=0), dict(frames=-1), dict(max_pull_hz=0), dict(max_pull_hz=-5),
       dict(deadband_hz=-1), dict(max_mean_square=0.0), dict(max_mean_square=-1.0), dict(max_mean_square=float("nan")),
       dict(max_mean_square=float("inf"))]


@pytest.mark.parametrize("kw", BAD, ids=[f"{k}={v}" for d in BAD for k, v in d.items()])
def test_bad_configurations_are_refused_and_nothing_is_written(fmrx, kw):
    out = fmrx.AfcDecision()
    C.memset(C.byref(out), 0xA5, C.sizeof(out))
    before = bytes(out)
    cfg = fmrx.afc_config_default(**kw)
    r = report(fmrx, mean_of(7000.0))
    assert fmrx.lib().fmrx_afc_decide(C.byref(r), BP_FS, C.byref(cfg), C.byref(out)) == fmrx.FMRX_EINVAL
    assert bytes(out) == before


def test_other_refusals(fmrx):
    out = fmrx.AfcDecision()
    C.memset(C.byref(out), 0xA5, C.sizeof(out))
    before = bytes(out)
    r = report(fmrx, mean_of(7000.0))
    empty = fmrx.CarrierReport()
    L = fmrx.lib()
    assert L.fmrx_afc_decide(C.byref(empty), BP_FS, None, C.byref(out)) == fmrx.FMRX_EINVAL  # no frames
    assert L.fmrx_afc_decide(None, BP_FS, None, C.byref(out)) == fmrx.FMRX_EINVAL
    assert L.fmrx_afc_decide(C.byref(r), BP_FS, None, None) == fmrx.FMRX_EINVAL
    for bp_fs in (0, -240000, 250000, 304000):
        assert L.fmrx_afc_decide(C.byref(r), bp_fs, None, C.byref(out)) == fmrx.FMRX_EINVAL
    assert bytes(out) == before
    assert L.fmrx_carrier_accumulate(None, None, 0) == fmrx.FMRX_EINVAL
    assert L.fmrx_carrier_accumulate(C.byref(empty), None, 3) == fmrx.FMRX_EINVAL and empty.frames == 0


def test_accumulate_split_equals_one_call(fmrx):
    raw = np.frombuffer(iqgen.rand_bytes(9, 4 * 2 * 11).tobytes(), np.uint32)
    sq = ((raw / 2.0 ** 32 - 0.5) * 1e3).astype(np.float32).reshape(11, 2)
    sq[:, 1] = np.abs(sq[:, 1]) * np.float32(7.3)
    whole = fmrx.carrier_accumulate(sq)
    parts = fmrx.carrier_accumulate(sq[4:], fmrx.carrier_accumulate(sq[:4]))
    want = A.accumulate(sq)
    for rep in (whole, parts):
        assert rep.frames == 11 == want[2]
        assert bits_eq(np.float64(rep.sum), want[0]) and bits_eq(np.float64(rep.sumsq), want[1])


def test_the_reference_rule_lands_on_the_test_stations(orc):
    """What test_gpu_afc asks of the GPU, asked of the rule itself first: afc_ref's sums and decision behind a
    float64 front end with the oracle's RF taps, 4 calls of 16 frames, the default configuration.  Every
    station ends within step_hz of its carrier after at most 3 retunes; the empty raster point never passes the
    carrier gate and never moves."""
    res = A.reference_rule(orc, A.landing_capture(64), A.TUNED, calls=4, call_frames=16)
    for k, (offs, decs) in enumerate(res):
        print(f"stream {k}: tuned {A.TUNED[k]} -> {offs}; err_hz {[round(d['err_hz']) for d in decs]}; "
              f"mean_square {[round(d['mean_square'], 3) for d in decs]}")
    for k, true in enumerate(A.TRUE):
        offs, decs = res[k]
        assert abs(offs[-1] - true) <= A.DEFAULTS["step_hz"], (k, offs)
        assert sum(a != b for a, b in zip([A.TUNED[k]] + offs, offs)) <= 3
        assert all(d["carrier"] == 1 for d in decs)
    offs, decs = res[3]
    assert offs == [A.TUNED[3]] * 4 and all(d["carrier"] == 0 for d in decs)


def test_the_restatement_sums_what_it_says():
    """afc_ref.sums on a row small enough to fold by hand: P = 16, one frame."""
    x = np.arange(64 * 16, dtype=np.float32) / np.float32(64.0) - np.float32(3.0)
    got = A.sums(x, 16)
    assert got.shape == (1, 2) and got.dtype == np.float32
    w = x.reshape(64, 16)

    def tree(v):
        v = list(v)
        while len(v) > 1:
            h = len(v) // 2
            v = [np.float32(v[j] + v[j + h]) for j in range(h)]
        return v[0]
    want_s = tree([tree(row) for row in w])
    want_q = tree([tree(row * row) for row in w])
    assert bits_eq(got[0], np.array([want_s, want_q], np.float32))
