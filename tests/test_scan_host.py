"""CPU tests of the band scan's station detector (fmrx_scan_detect, include/fmrx.h): the spectrum is
computed here in numpy float64 (the definition in fmrx.h), handed to the library as float32, and the
library's station list is compared with a numpy float64 restatement of the detector's seven steps.
The reference project has no band scan, so these restatements are the yardstick.

Tolerance of the dB figures, 1e-3 dB: both sides add at most 8192 doubles and take one log10 (errors
near 1e-13 dB); the library then rounds to float, which for a value of up to 200 dB in magnitude moves
it by at most 200 * 2^-24 = 1.2e-5 dB."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import iqgen
import oracle

DEFAULTS = dict(raster_hz=100000, raster_origin_hz=0, channel_hz=150000, min_separation_hz=200000,
                dc_notch_bins=1, floor_percentile=25, min_snr_db=10.0)
DB_TOL = 1e-3

# name -> (mode, [(synth seed, offset Hz, amplitude)], detector settings)
STATION_CAPTURES = {
    "two": (0, [(3, -300000, 0.5), (4, 300000, 0.5)], {}),
    "three": (0, [(1, -900000, 0.5), (2, 100000, 0.25), (3, 700000, 0.06)], {}),
    "adjacent": (0, [(3, -100000, 0.4), (4, 100000, 0.4)], {}),
    "one": (0, [(5, 0, 1.0)], {}),
    "m1": (1, [(6, 200000, 0.8)], {}),
    "origin50": (0, [(3, -250000, 0.5), (4, 350000, 0.5)], {"raster_origin_hz": 50000}),
}
EMPTY_CAPTURES = {"rand": "rand:3", "const128": "const128"}
N_BLOCKS = 4


def rotated(iq, rf_fs, f, amp=1.0):
    """iq moved to +f Hz in float64 (times amp), as complex samples."""
    z = (iq[0::2].astype(np.float64) - 128.0) / 128.0 + 1j * (iq[1::2].astype(np.float64) - 128.0) / 128.0
    n = np.arange(z.size, dtype=np.float64)
    return amp * z * np.exp(2j * np.pi * (f / rf_fs) * n)


def quantised(z):
    out = np.empty(2 * z.size, np.uint8)
    out[0::2] = np.clip(np.rint(z.real * 128.0) + 128.0, 0, 255).astype(np.uint8)
    out[1::2] = np.clip(np.rint(z.imag * 128.0) + 128.0, 0, 255).astype(np.uint8)
    return out


def rf_fs_of(mode):
    return oracle.MODES[mode][3]


@functools.lru_cache(maxsize=None)
def capture(name, n_blocks=N_BLOCKS):
    """(u8 I/Q, mode, placed offsets, detector settings) of a named capture; read-only."""
    if name in STATION_CAPTURES:
        mode, stations, cfg = STATION_CAPTURES[name]
        bb, rf_fs = oracle.MODES[mode][0], rf_fs_of(mode)
        if name == "one":
            iq = iqgen.make("synth:5", n_blocks * bb, rf_fs)
        else:
            z = sum(rotated(iqgen.make(f"synth:{seed}", n_blocks * bb, rf_fs), rf_fs, f, amp) for seed, f, amp in stations)
            iq = quantised(z)
        offsets = sorted(f for _, f, _ in stations)
    else:
        recipe = EMPTY_CAPTURES.get(name, name)  # any iqgen recipe, e.g. const130
        mode, cfg, offsets = 0, {}, []
        iq = iqgen.make(recipe, n_blocks * oracle.MODES[0][0])
    iq.setflags(write=False)
    return iq, mode, offsets, dict(cfg)


def welch64(iq, n):
    """fmrx.h's power spectrum in float64: (P, FFT-shifted; n_segments)."""
    z = (iq[0::2].astype(np.float64) - 128.0) / 128.0 + 1j * (iq[1::2].astype(np.float64) - 128.0) / 128.0
    nseg = z.size // n
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)
    x = np.fft.fft(z[: nseg * n].reshape(nseg, n) * w, axis=1)
    p = 8.0 / (3.0 * n * n * nseg) * (np.abs(x) ** 2).sum(axis=0)
    return np.fft.fftshift(p), nseg


def candidate_bins(n, rf_fs, f, channel_hz, notch):
    j = np.arange(n, dtype=np.int64)
    kept = np.abs(j - n // 2) >= notch
    return kept & (2 * np.abs((j - n // 2) * rf_fs - f * n) <= channel_hz * n)


def detect_ref(power, rf_fs, max_out=None, **kw):
    """Steps 1-7 of fmrx_scan_detect in float64: (stations [(offset, power_db, snr_db)], floor_db,
    every candidate's {offset: snr_db})."""
    c = dict(DEFAULTS, **kw)
    n = power.size
    p = np.maximum(np.asarray(power, np.float32).astype(np.float64), 1e-20)
    j = np.arange(n, dtype=np.int64)
    kept = np.abs(j - n // 2) >= c["dc_notch_bins"]
    srt = np.sort(p[kept])
    floor = srt[(c["floor_percentile"] * (srt.size - 1)) // 100]
    reach = (rf_fs - c["channel_hz"]) // 2
    cands = []
    m = -((reach + c["raster_origin_hz"]) // c["raster_hz"])
    while c["raster_origin_hz"] + m * c["raster_hz"] <= reach:
        f = c["raster_origin_hz"] + m * c["raster_hz"]
        assert 2 * abs(f) + c["channel_hz"] <= rf_fs
        sel = candidate_bins(n, rf_fs, f, c["channel_hz"], c["dc_notch_bins"])
        if sel.any():
            cm = p[sel].sum()
            cands.append((f, cm, 10.0 * np.log10(cm), 10.0 * np.log10(cm / (floor * sel.sum()))))
        m += 1
    acc = []
    for f, cm, pdb, snr in sorted(cands, key=lambda t: (-t[1], t[0])):
        if snr >= np.float32(c["min_snr_db"]) and all(abs(f - a[0]) >= c["min_separation_hz"] for a in acc):
            acc.append((f, pdb, snr))
    if max_out is not None:
        acc = acc[:max_out]
    return sorted(acc), 10.0 * np.log10(floor), {f: snr for f, _, _, snr in cands}


def as_tuples(stations):
    return [(s.offset_hz, s.power_db, s.snr_db) for s in stations]


def assert_stations(got, want):
    assert [g[0] for g in got] == [w[0] for w in want]
    for g, w in zip(got, want):
        assert abs(g[1] - w[1]) <= DB_TOL and abs(g[2] - w[2]) <= DB_TOL, (g, w)


ALL_CAPTURES = list(STATION_CAPTURES) + list(EMPTY_CAPTURES)


@pytest.mark.parametrize("n", [256, 4096, 8192])
@pytest.mark.parametrize("name", ALL_CAPTURES)
def test_detect_equals_restatement_and_placed_offsets(fmrx, name, n):
    iq, mode, offsets, cfg = capture(name)
    power = welch64(iq, n)[0].astype(np.float32)
    got, floor_db = fmrx.scan_detect(power, rf_fs_of(mode), **cfg)
    want, want_floor, _ = detect_ref(power, rf_fs_of(mode), **cfg)
    assert_stations(as_tuples(got), want)
    assert abs(floor_db - want_floor) <= DB_TOL
    assert [s.offset_hz for s in got] == offsets


@pytest.mark.parametrize("single_segment", [False, True])
@pytest.mark.parametrize("n", [256, 1024, 2048, 4096, 8192])
@pytest.mark.parametrize("name", ALL_CAPTURES)
def test_threshold_margins(name, n, single_segment):
    """The 10 dB threshold has 3 dB of room on both sides on every whole capture (what every detection
    test here and on the GPU scans): each placed station scores at least 13 dB, every candidate outside
    the separation zone of a placed station at most 7 dB.  Numpy only: this pins the inputs, not the
    library.  On a capture cut to ONE segment the floor is the 25th percentile of a single periodogram
    (chi-square with 2 degrees of freedom: 5.4 dB under the mean, and a 16-bin candidate at 256 bins
    scatters by a further +-1 dB), so an empty candidate sits near 5.4 dB instead of 0: there the room
    asked for is 2 dB (rand:3 at 256 bins scores 7.5 dB); no detection test uses such a capture."""
    iq, mode, offsets, cfg = capture(name)
    power = welch64(iq[: 2 * n] if single_segment else iq, n)[0].astype(np.float32)
    _, _, snr = detect_ref(power, rf_fs_of(mode), **cfg)
    sep = DEFAULTS["min_separation_hz"]
    for f in offsets:
        assert snr[f] >= 13.0, (f, snr[f])
    for f, v in snr.items():
        if all(abs(f - o) >= sep for o in offsets):
            assert v <= (8.0 if single_segment else 7.0), (f, v)


def test_max_out_keeps_the_strongest_sorted_by_offset(fmrx):
    iq, mode, offsets, _ = capture("three")
    power = welch64(iq, 4096)[0].astype(np.float32)
    got, _ = fmrx.scan_detect(power, rf_fs_of(mode), max_out=2)
    want, _, _ = detect_ref(power, rf_fs_of(mode), max_out=2)
    assert_stations(as_tuples(got), want)
    assert [s.offset_hz for s in got] == [-900000, 100000]  # amplitudes 0.5 and 0.25; 0.06 dropped
    got1, _ = fmrx.scan_detect(power, rf_fs_of(mode), max_out=1)
    assert [s.offset_hz for s in got1] == [-900000]
    got0, _ = fmrx.scan_detect(power, rf_fs_of(mode), max_out=0)
    assert got0 == []


def test_dc_notch_on_a_dc_line(fmrx):
    """const130: all the power sits on the DC bin and its two neighbours.  With the notch the centre
    bin leaves both the floor's bins and the 0 Hz candidate; without it, it is counted."""
    iq, mode, _, _ = capture("const130")
    power = welch64(iq, 1024)[0].astype(np.float32)
    res = {}
    for notch in (0, 1):
        got, floor_db = fmrx.scan_detect(power, rf_fs_of(mode), dc_notch_bins=notch)
        want, want_floor, _ = detect_ref(power, rf_fs_of(mode), dc_notch_bins=notch)
        assert_stations(as_tuples(got), want)
        assert abs(floor_db - want_floor) <= DB_TOL
        assert [s.offset_hz for s in got] == [0]
        res[notch] = got[0]
    # Hann: the neighbours hold 1/2 of the centre bin's amplitude each, 1/4 of its power: 1.5 against 0.5
    assert abs((res[0].power_db - res[1].power_db) - 10.0 * np.log10(3.0)) <= 1e-2


def test_config_defaults(fmrx):
    c = fmrx.scan_config()
    assert (c.fft_bins, c.raster_hz, c.raster_origin_hz, c.channel_hz, c.min_separation_hz, c.dc_notch_bins,
            c.floor_percentile, c.min_snr_db) == (4096, 100000, 0, 150000, 200000, 1, 25, 10.0)


@pytest.mark.parametrize("bins,rf_fs,kw", [
    (300, 2400000, {}),                         # not a power of two
    (128, 2400000, {}),                         # below 256
    (16384, 2400000, {}),                       # above 8192
    (1024, 2400000, {"raster_hz": 0}),
    (1024, 2400000, {"raster_hz": -100000}),
    (1024, 2400000, {"channel_hz": 0}),
    (1024, 2400000, {"min_separation_hz": 0}),
    (1024, 2400000, {"channel_hz": 2400000}),   # channel_hz >= rf_fs
    (1024, 2400000, {"floor_percentile": 0}),
    (1024, 2400000, {"floor_percentile": 100}),
    (1024, 2400000, {"raster_origin_hz": 1}),   # 1 Hz off the raster: a rotator period fmrx_tuner_design refuses
    (1024, 2400000, {"raster_hz": 100001}),
])
def test_detect_refuses_bad_arguments(fmrx, bins, rf_fs, kw):
    import ctypes as C

    power = np.ones(bins, np.float32)
    with pytest.raises(fmrx.FmrxError) as e:
        fmrx.scan_detect(power, rf_fs, **kw)
    assert e.value.code == fmrx.FMRX_EINVAL
    # nothing written
    out = (fmrx.Station * 4)()
    out[0].offset_hz = 77
    n, fl = C.c_int(-5), C.c_float(-7.0)
    rc = fmrx.lib().fmrx_scan_detect(power.ctypes.data, bins, rf_fs, C.byref(fmrx.scan_config(**kw)), out, 4,
                                     C.byref(n), C.byref(fl))
    assert rc == fmrx.FMRX_EINVAL and n.value == -5 and fl.value == -7.0 and out[0].offset_hz == 77
