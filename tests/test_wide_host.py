"""CPU tests of the wide-capture design (fmrx_wide_design, fmrx_scan_detect_wide; host only): the
split of an offset into a coarse and a fine part, the coarse rotator, the low-pass and its response,
and -- with the pinned oracle alone -- what the definition of the down-converter costs in audio
quality.  wide_compose() is the expected output of the GPU path; tests/test_gpu_wide.py compares
the kernels with it bit for bit, which is what makes the quality test here valid for them."""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest

import iqgen
import oracle
from test_formats_host import S16, U8, normalise

RATES = (2400000, 1152000, 2304000)
DECIMS = tuple(range(2, 11))


def design(fm, rf_fs, d, f):
    w = fm.wide_design(rf_fs, d, f)
    q, rem = divmod(w["coarse_hz"], rf_fs // 4)
    assert rem == 0
    return w, q


# ---- the split ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("rf_fs,d,f,q,f_r,n_c,k_c", [
    (2400000, 8, 0, 0, 0, 1, 0),
    (2400000, 8, 600000, 1, 0, 32, 1),
    (2400000, 8, 300000, 1, -300000, 32, 1),      # the tie rounds away from zero
    (2400000, 8, -300000, -1, 300000, 32, 31),
    (2400000, 8, 299000, 0, 299000, 1, 0),
    (2400000, 8, 9500000, 16, -100000, 2, 1),     # f_c = cap_fs / 2
    (2400000, 8, -4700000, -8, 100000, 4, 3),     # k_c = (-1) mod 4
    (1152000, 3, 1500000, 5, 60000, 12, 5),
    (2304000, 10, -11000000, -19, -56000, 40, 21),
])
def test_split(fmrx, rf_fs, d, f, q, f_r, n_c, k_c):
    w, got_q = design(fmrx, rf_fs, d, f)
    cap_fs = d * rf_fs
    assert (got_q, w["fine_hz"], w["N"], w["k"]) == (q, f_r, n_c, k_c)
    assert w["coarse_hz"] + w["fine_hz"] == f
    assert 8 * abs(w["fine_hz"]) <= rf_fs
    # k_c cap_fs / N_c is f_c mod cap_fs: the rotator turns by exactly the coarse part
    assert (w["k"] * cap_fs) % w["N"] == 0 and (w["k"] * cap_fs // w["N"] - w["coarse_hz"]) % cap_fs == 0
    assert w["table"].shape == (n_c, 2) and w["h"].shape == (16 * d + 1,)
    if f == 0:
        assert w["table"].tolist() == [[1.0, 0.0]]


@pytest.mark.parametrize("d,f", [(0, 0), (1, 0), (11, 0), (8, 9600000), (8, -9600000), (2, 2400000), (8, 600001)])
def test_refusals(fmrx, d, f):
    """decim outside 2..10, |f| >= cap_fs / 2, and a fine part of 1 Hz (a period of 2.4 M pairs)."""
    with pytest.raises(fmrx.FmrxError) as e:
        fmrx.wide_design(2400000, d, f)
    assert e.value.code == fmrx.FMRX_EINVAL


def test_refusal_writes_nothing(fmrx):
    import ctypes as C
    vals = [C.c_int(-7) for _ in range(5)]
    tab, h = np.full(80, 9.0, np.float32), np.full(161, 9.0, np.float32)
    rc = fmrx.lib().fmrx_wide_design(2400000, 8, 600001, C.byref(vals[0]), C.byref(vals[1]), C.byref(vals[2]),
                                     C.byref(vals[3]), tab.ctypes.data, C.byref(vals[4]), h.ctypes.data)
    assert rc == fmrx.FMRX_EINVAL
    assert [v.value for v in vals] == [-7] * 5 and np.all(tab == 9.0) and np.all(h == 9.0)
    rc = fmrx.lib().fmrx_wide_design(2401002, 8, 0, None, None, None, None, None, None, None)  # rf_fs % 4 != 0
    assert rc == fmrx.FMRX_EINVAL


@pytest.mark.parametrize("d", DECIMS)
def test_table_within_one_ulp_of_float64(fmrx, d):
    rf_fs = 2400000
    for q in (1, 3, 2 * d - 1, -(2 * d - 1)):  # odd q: the full period 4 D
        w = fmrx.wide_design(rf_fs, d, q * rf_fs // 4)
        n, tab = w["N"], w["table"]
        assert n == 4 * d // math.gcd(abs(q), 4 * d)
        a = 2 * np.pi * np.arange(n, dtype=np.float64) / n
        for col, ref in ((0, np.cos(a)), (1, np.sin(a))):
            r32 = ref.astype(np.float32)
            err = np.abs(tab[:, col].astype(np.float64) - r32.astype(np.float64))
            assert np.all(err <= np.spacing(np.abs(r32)).astype(np.float64)), (col, int(np.argmax(err)))


@pytest.mark.parametrize("rf_fs", RATES)
@pytest.mark.parametrize("d", DECIMS)
def test_taps_are_the_library_low_pass(fmrx, rf_fs, d):
    h = fmrx.wide_design(rf_fs, d, 0)["h"]
    want = fmrx.lpf(d * rf_fs, 3 * rf_fs / 8, 16 * d + 1)
    assert h.dtype == np.float32 and np.array_equal(h.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("rf_fs", RATES)
@pytest.mark.parametrize("d", DECIMS)
def test_response(fmrx, rf_fs, d):
    """Float64 response of the float32 taps on 32768 points of [0, cap_fs / 2]: flat over the fine
    offset plus a channel, and down by 65 dB over everything that aliases onto that band."""
    h = fmrx.wide_design(rf_fs, d, 0)["h"].astype(np.float64)
    cap_fs, n = d * rf_fs, 32768
    f = np.arange(n + 1, dtype=np.float64) * (cap_fs / 2) / n
    k = np.arange(h.size, dtype=np.float64)
    mag = np.empty(n + 1)
    for a in range(0, n + 1, 4096):
        mag[a:a + 4096] = np.abs(np.exp(-2j * np.pi * np.outer(f[a:a + 4096] / cap_fs, k)) @ h)
    db = 20 * np.log10(np.maximum(mag, 1e-30))
    passband, stopband = f <= rf_fs / 8 + 100e3, f >= 7 * rf_fs / 8 - 200e3
    assert passband.sum() > 100 and stopband.sum() > 100
    print(f"rf_fs {rf_fs} D {d}: passband {db[passband].min():+.4f} .. {db[passband].max():+.4f} dB, "
          f"stopband max {db[stopband].max():.2f} dB")
    assert np.all(np.abs(db[passband]) <= 0.05)
    assert np.all(db[stopband] <= -65.0)


# ---- the expected output of the wide path ----------------------------------------------------------------

_ORC = None


def _orc():
    global _ORC
    if _ORC is None:
        _ORC = oracle.Oracle()
    return _ORC


def narrow_compose(raw, fmt, mode, rf_taps, offset, first_pair=0, fields=("pcm_mono",)):
    """tests/test_gpu_formats.py's compose: one stream of format fmt tuned to `offset` at rf_fs."""
    fm, orc = iqgen.load_fmrx(), _orc()
    rf_fs, bp_fs = oracle.MODES[mode][3], oracle.MODES[mode][5]
    x = normalise(raw, fmt)
    xi, xq = x[0::2], x[1::2]
    n_per, k, tab = fm.tuner_design(rf_fs, offset)
    n = (int(first_pair) % n_per + np.arange(xi.size, dtype=np.int64)) % n_per
    p = (k * n) % n_per
    c, s = tab[p, 0], tab[p, 1]
    assert c.dtype == np.float32 and xi.dtype == np.float32
    ri = xi * c + xq * s
    rq = xq * c - xi * s
    h = orc.lpf(rf_fs, 100e3, rf_taps)
    zeros = np.zeros(rf_taps - 1, np.float32)
    i_ds, _ = orc.resample(ri, zeros, h, 1, rf_fs // bp_fs)
    q_ds, _ = orc.resample(rq, zeros, h, 1, rf_fs // bp_fs)
    demod, _ = orc.fmdemod(i_ds, q_ds, [0.0, 0.0])
    out = orc.run_audio(mode, demod, list(fields))
    out["demod"] = demod
    return out


def wide_y(raw, fmt, rf_fs, d, offset, first_pair=0):
    """The cf32 stream at rf_fs the down-converter makes of a wide capture (interleaved float32), and
    the fine offset: normalise, rotate by the coarse table in numpy float32 (every product and sum
    rounded separately, integer phases), the oracle's resample of I' and Q' with the oracle's taps."""
    fm, orc = iqgen.load_fmrx(), _orc()
    w = fm.wide_design(rf_fs, d, offset)
    x = normalise(raw, fmt)
    xi, xq = x[0::2], x[1::2]
    n_per, k, tab = w["N"], w["k"], w["table"]
    n = (int(first_pair) % n_per + np.arange(xi.size, dtype=np.int64)) % n_per
    p = (k * n) % n_per
    c, s = tab[p, 0], tab[p, 1]
    assert c.dtype == np.float32 and xi.dtype == np.float32
    ri = xi * c + xq * s
    rq = xq * c - xi * s
    h = orc.lpf(d * rf_fs, 3 * rf_fs / 8, 16 * d + 1)
    zeros = np.zeros(16 * d, np.float32)
    y = np.empty(2 * (xi.size // d), np.float32)
    y[0::2], _ = orc.resample(ri, zeros, h, 1, d)
    y[1::2], _ = orc.resample(rq, zeros, h, 1, d)
    return y, w["fine_hz"]


def wide_compose(raw, fmt, mode, rf_taps, d, offset, first_pair=0, fields=("pcm_mono",)):
    """The expected outputs of one station at `offset` of a wide capture at d * rf_fs, from wide
    position first_pair (a multiple of d), over the whole of raw in one piece."""
    from test_formats_host import F32
    assert first_pair % d == 0
    y, fine = wide_y(raw, fmt, oracle.MODES[mode][3], d, offset, first_pair)
    return narrow_compose(y, F32, mode, rf_taps, fine, first_pair // d, fields)


# ---- quality of the definition --------------------------------------------------------------------------

Q_MODE, Q_D, Q_BLOCKS, Q_SKIP = 0, 4, 12, 4
Q_STATIONS = ((31, 1700000), (32, -3100000))  # (synth seed, offset against the wide capture's centre)


@functools.lru_cache(maxsize=None)
def narrow_station(seed):
    a = iqgen.make(f"synth:{seed}", Q_BLOCKS * oracle.MODES[Q_MODE][0], oracle.MODES[Q_MODE][3])
    a.setflags(write=False)
    return a


def as_complex(iq):
    return (iq[0::2].astype(np.float64) - 128.0) / 128.0 + 1j * (iq[1::2].astype(np.float64) - 128.0) / 128.0


@functools.lru_cache(maxsize=None)
def two_station_capture():
    """A mode-0 capture at 4 x 2.4 MS/s in float64: each narrow synth station FFT-interpolated by 4,
    moved to its offset, times 0.45; the sum as int16."""
    total = 0
    for seed, f in Q_STATIONS:
        z = as_complex(narrow_station(seed))
        n = z.size
        spec = np.fft.fft(z)
        wide = np.zeros(Q_D * n, np.complex128)
        wide[: n // 2], wide[-(n // 2):] = spec[: n // 2], spec[n // 2:]
        up = np.fft.ifft(wide) * Q_D
        total = total + 0.45 * up * np.exp(2j * np.pi * (f / (Q_D * oracle.MODES[Q_MODE][3])) * np.arange(up.size))
    out = np.empty(2 * total.size, np.float64)
    out[0::2], out[1::2] = total.real, total.imag
    a = np.clip(np.rint(out * 32768.0), -32768, 32767).astype(np.int16)
    a.setflags(write=False)
    return a


def welch64(raw, n):
    """fmrx.h's spectrum in float64: Hann, no overlap, 8 / (3 N^2 nseg), FFT-shifted."""
    x = raw.astype(np.float64) / 32768.0
    z = (x[0::2] + 1j * x[1::2])
    nseg = z.size // n
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)
    p = (np.abs(np.fft.fft(z[: nseg * n].reshape(nseg, n) * w, axis=1)) ** 2).sum(axis=0)
    return np.fft.fftshift(p) * 8.0 / (3.0 * n * n * nseg)


def peak_correlation(a, b, skip):
    """Peak normalised correlation of two PCM rows over lags -2 .. +2, past the first `skip` samples."""
    a, b = a[skip:].astype(np.float64), b[skip:].astype(np.float64)
    best = -1.0
    for lag in range(-2, 3):
        u, v = (a[lag:], b[: b.size - lag]) if lag >= 0 else (a[:lag], b[-lag:])
        best = max(best, float(np.dot(u, v) / np.sqrt(np.dot(u, u) * np.dot(v, v))))
    return best


# The capture's noise is the 8-bit quantisation noise of the two narrow streams: after the
# interpolation it covers 2.4 MHz around each station, half of the band, 60 dB above the int16 noise of
# the rest.  The floor percentile is therefore taken inside it (75: the lower half of the bins is the
# int16 floor), as a scan of a real capture finds its floor in the receiver noise.
Q_SCAN = dict(floor_percentile=75)


def test_two_stations_are_found(fmrx):
    raw = two_station_capture()
    rf_fs = oracle.MODES[Q_MODE][3]
    stations, _ = fmrx.scan_detect_wide(welch64(raw, 4096), rf_fs, Q_D, **Q_SCAN)
    assert [s.offset_hz for s in stations] == sorted(f for _, f in Q_STATIONS)
    # the narrow detector is what it was: the same spectrum read as a capture at cap_fs (every
    # multiple of 100 kHz is an offset both designs accept)
    narrow, _ = fmrx.scan_detect(welch64(raw, 4096), Q_D * rf_fs, **Q_SCAN)
    assert [(s.offset_hz, s.power_db, s.snr_db) for s in narrow] == [(s.offset_hz, s.power_db, s.snr_db) for s in stations]


def test_quality_of_the_definition(fmrx):
    """The wide path's mono PCM of each station against the oracle's PCM of the narrow stream it was
    built from.  The floor is the same figure for the existing narrow tuner on the first station moved
    by +300 kHz inside a narrow u8 capture, minus 0.01: the wide path adds a filter with 0.02 dB of
    ripple and must not cost more.  Measured: narrow tuner 1.00000, wide 0.99829 for both stations
    (the low-pass delays the stream by 8 pairs at rf_fs, 0.16 of an audio sample, which the whole-sample
    lags of the figure do not take out: against the clean PCM delayed by 0.16 samples it is 1.00000)."""
    rf_fs, na = oracle.MODES[Q_MODE][3], oracle.MODES[Q_MODE][2]
    skip = Q_SKIP * na
    iq0 = narrow_station(Q_STATIONS[0][0])
    clean0 = _orc().run(Q_MODE, 51, iq0, ["pcm_mono"])["pcm_mono"]
    z = as_complex(iq0) * np.exp(2j * np.pi * (300000 / rf_fs) * np.arange(iq0.size // 2, dtype=np.float64))
    moved = np.empty(iq0.size, np.uint8)
    moved[0::2] = np.clip(np.rint(z.real * 128.0) + 128.0, 0, 255).astype(np.uint8)
    moved[1::2] = np.clip(np.rint(z.imag * 128.0) + 128.0, 0, 255).astype(np.uint8)
    base = peak_correlation(narrow_compose(moved, U8, Q_MODE, 51, 300000)["pcm_mono"], clean0, skip)
    print(f"narrow tuner at +300 kHz: {base:.5f}")
    assert base > 0.9
    raw = two_station_capture()
    for seed, f in Q_STATIONS:
        clean = _orc().run(Q_MODE, 51, narrow_station(seed), ["pcm_mono"])["pcm_mono"]
        got = peak_correlation(wide_compose(raw, S16, Q_MODE, 51, Q_D, f)["pcm_mono"], clean, skip)
        print(f"wide station at {f:+d} Hz: {got:.5f}")
        assert got >= base - 0.01
