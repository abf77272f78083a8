"""GPU tests of the band scan (csrc/scan.hip, fmrx_scan*): the spectrum against numpy float64 (the
definition in include/fmrx.h, restated in tests/test_scan_host.py), bit identity between the entry
points, runs and alignments, the scan end to end and through the CLI, and that a scan leaves the
receiver state alone.

Tolerances (a numpy float32 radix-2 prototype, every product and sum in float32, against float64 on
these inputs): one bin differed by at most 5e-4 dB (single-segment low-power bins), the power
integrated over a 150 kHz candidate by at most 1.6e-5 dB; the bounds are 0.01 dB and 1e-3 dB."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import oracle
from test_scan_host import (DEFAULTS, candidate_bins, capture, quantised, rf_fs_of, welch64)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BIN_TOL_DB = 0.01
CAND_TOL_DB = 1e-3


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


@pytest.fixture(scope="module")
def rx(fmrx):
    with fmrx.Receiver(0, fmrx.MONO) as r:
        yield r


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def db(p):
    return 10.0 * np.log10(p)


DUST = 1e-12  # of the total power: see check_spectrum


def check_spectrum(got, iq, n, rf_fs=2400000, dust=False):
    """got (float32, from the GPU) against float64 on iq: every bin and every default candidate.
    dust: the input is exactly periodic in the segment (a constant, a tone on a bin centre), so most
    bins are zero but for rounding (float64: 1e-30 of the total and less) and have no dB value to
    compare; those -- under DUST of the total in float64 -- must stay under DUST of the total on the GPU
    (a float32 transform leaves (2^-24 * a few)^2 * (3N/8) / (N^2/4) ~ 1e-16 of a line's power on a
    bin).  Without it every bin must be above DUST and is compared in dB."""
    want, _ = welch64(iq, n)
    assert got.dtype == np.float32 and got.shape == (n,)
    real = want >= DUST * want.sum()
    assert dust or real.all()
    worst = float(np.max(np.abs(db(got[real].astype(np.float64)) - db(want[real]))))
    print(f"bins={n} pairs={iq.size // 2}: worst bin {worst:.2e} dB")
    assert worst <= BIN_TOL_DB
    assert real.all() or got[~real].max() <= DUST * want.sum()
    reach = (rf_fs - DEFAULTS["channel_hz"]) // 2
    for f in range(-(reach // 100000) * 100000, reach + 1, 100000):
        sel = candidate_bins(n, rf_fs, f, DEFAULTS["channel_hz"], 1)
        if want[sel].sum() < DUST * want.sum():
            assert dust and got[sel].sum() <= DUST * want.sum() * sel.sum()
            continue
        d = abs(db(got[sel].astype(np.float64).sum()) - db(want[sel].sum()))
        assert d <= CAND_TOL_DB, (f, d)


# ---- spectrum against numpy float64 ----------------------------------------------------------------

@pytest.mark.parametrize("pairs", ["N", "3N+100", "25600"])
@pytest.mark.parametrize("n", [256, 1024, 4096, 8192])
def test_spectrum_three(rx, n, pairs):
    iq = capture("three")[0]
    n_pairs = {"N": n, "3N+100": 3 * n + 100, "25600": 25600}[pairs]
    part = iq[: 2 * n_pairs]
    got, nseg = rx.scan_spectrum(part, n)
    assert nseg == n_pairs // n
    check_spectrum(got, part, n)


def test_spectrum_more_segments_than_workgroups(rx):
    """8192 segments of 256 bins (a 4 MiB capture): every workgroup accumulates several segments and the
    reduce kernel sums a full set of partial rows."""
    iq = capture("three")[0]
    big = np.tile(iq, (1 << 22) // iq.size + 1)[: 1 << 22]
    got, nseg = rx.scan_spectrum(big, 256)
    assert nseg == 8192
    check_spectrum(got, big, 256)


def test_spectrum_rand(rx):
    iq = capture("rand")[0]
    for n in (256, 4096):
        got, _ = rx.scan_spectrum(iq, n)
        check_spectrum(got, iq, n)
        # sum of P ~ mean |x|^2 (white input, 25600 pairs: the estimate scatters by about 0.05 dB)
        mean_sq = 2.0 * np.mean(((iq.astype(np.float64) - 128.0) / 128.0) ** 2)
        assert abs(db(float(got.astype(np.float64).sum())) - db(mean_sq)) < 0.2


def test_spectrum_const128_is_exactly_zero(rx):
    iq = capture("const128")[0]
    for n in (256, 4096, 8192):
        got, _ = rx.scan_spectrum(iq, n)
        assert not got.any() and not np.signbit(got).any()


@pytest.mark.parametrize("byte", [255, 0])
def test_spectrum_dc_line(rx, byte):
    """const255 / const0: x = +-(127 or 128)/128 on both rails.  All the power sits on the centre bin
    (N/2: 0 Hz after the shift) and its two neighbours, which hold a quarter of the centre bin each
    (Hann); their sum is |x|^2.  The float64 value of every other bin is rounding dust (1e-30 and
    less), so those are checked against the total instead of in dB: the float32 transform leaves at
    most (2^-24 * a few)^2 * (3N/8) / (N^2/4) ~ 1e-16 of the total there; the bound is 1e-12."""
    iq = capture(f"const{byte}")[0]
    a = (byte - 128.0) / 128.0
    for n in (256, 4096):
        got, _ = rx.scan_spectrum(iq, n)
        got = got.astype(np.float64)
        want, _ = welch64(iq, n)
        mid = slice(n // 2 - 1, n // 2 + 2)
        assert np.max(np.abs(db(got[mid]) - db(want[mid]))) <= BIN_TOL_DB
        assert abs(db(got[mid].sum()) - db(2.0 * a * a)) <= CAND_TOL_DB
        assert abs(db(got[n // 2]) - db(2.0 * a * a * 2.0 / 3.0)) <= BIN_TOL_DB
        rest = np.delete(got, np.arange(n // 2 - 1, n // 2 + 2))
        assert rest.max() <= 1e-12 * got.sum()


def test_spectrum_tone_lands_above_centre(rx):
    """A complex tone at +300 kHz peaks at bin N/2 + 300000 N / rf_fs: a swap of I and Q or a shift
    in the wrong direction would mirror it below the centre."""
    n, rf_fs = 1024, 2400000
    t = np.arange(8 * n, dtype=np.float64)
    iq = quantised(0.5 * np.exp(2j * np.pi * (300000.0 / rf_fs) * t))
    got, _ = rx.scan_spectrum(iq, n)
    assert int(np.argmax(got)) == n // 2 + 300000 * n // rf_fs == 640
    check_spectrum(got, iq, n, dust=True)  # period 8 samples: lines on every 128th bin only


# ---- identity ---------------------------------------------------------------------------------------

def device_spectrum(rx, d_iq_ptr, n_pairs, n):
    d_p = torch.zeros(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rx.scan_spectrum_device(d_iq_ptr, n_pairs, n, d_p.data_ptr())
    rx.synchronize()
    return d_p.cpu().numpy()


@pytest.mark.parametrize("n", [256, 4096, 8192])
def test_host_device_and_repeat_runs_are_bit_identical(rx, n):
    iq = capture("three")[0]
    host, _ = rx.scan_spectrum(iq, n)
    again, _ = rx.scan_spectrum(iq, n)
    assert np.array_equal(bits(host), bits(again))
    d_iq = torch.from_numpy(np.array(iq)).cuda()
    dev = device_spectrum(rx, d_iq.data_ptr(), iq.size // 2, n)
    assert np.array_equal(bits(host), bits(dev))
    assert np.array_equal(bits(dev), bits(device_spectrum(rx, d_iq.data_ptr(), iq.size // 2, n)))


@pytest.mark.parametrize("n", [256, 4096])
def test_two_byte_aligned_device_pointer(rx, n):
    """d_iq advanced by one pair: the capture starts 2 bytes off a dword."""
    iq = capture("three")[0]
    d_iq = torch.from_numpy(np.array(iq)).cuda()
    assert d_iq.data_ptr() % 4 == 0
    n_pairs = iq.size // 2 - 1
    dev = device_spectrum(rx, d_iq.data_ptr() + 2, n_pairs, n)
    host, _ = rx.scan_spectrum(iq[2:], n)
    assert np.array_equal(bits(dev), bits(host))
    # and up to the capture's last byte: the last segment ends where the buffer ends
    tail_pairs = (n_pairs // n) * n
    d_tail = torch.from_numpy(np.array(iq[: 2 + 2 * tail_pairs])).cuda()
    dev = device_spectrum(rx, d_tail.data_ptr() + 2, tail_pairs, n)
    assert np.array_equal(bits(dev), bits(host))


# ---- end to end ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["two", "three", "adjacent", "m1", "rand"])
def test_scan_finds_the_placed_stations(fmrx, name):
    iq, mode, offsets, cfg = capture(name)
    with fmrx.Receiver(mode, fmrx.MONO) as r:
        got = r.scan(iq, **cfg)
        assert r.geo.rf_fs == rf_fs_of(mode)
    assert [s.offset_hz for s in got] == offsets


def test_decode_stations(fmrx):
    iq = capture("two", 20)[0]
    stations, pcm = fmrx.decode_stations(iq)
    assert [s.offset_hz for s in stations] == [-300000, 300000]
    with fmrx.Receiver(0, fmrx.MONO, n_streams=2) as r:
        r.tune([-300000, 300000])
        want = r.process_shared(iq)
    assert pcm.dtype == np.int16 and np.array_equal(pcm, want) and want.any()
    none, empty = fmrx.decode_stations(capture("rand")[0])
    assert none == [] and empty.size == 0


# ---- state --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", ["mono", "stereo"])
def test_scan_between_calls_leaves_the_receiver_alone(fmrx, channels):
    ch = fmrx.MONO if channels == "mono" else fmrx.STEREO
    bb = oracle.MODES[0][0]
    a, c = capture("one")[0][: 2 * bb], capture("one")[0][2 * bb:]
    b = capture("three")[0]
    with fmrx.Receiver(0, ch) as r:
        want = [r.process(a), r.process(c)]
    with fmrx.Receiver(0, ch) as r:
        got = [r.process(a)]
        assert [s.offset_hz for s in r.scan(b)] == [-900000, 100000, 700000]
        r.scan_spectrum(b, 8192)
        got.append(r.process(c))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- errors -------------------------------------------------------------------------------------------

def test_refused_calls(fmrx):
    iq, bb = capture("one")[0], oracle.MODES[0][0]
    with fmrx.Receiver(0, fmrx.MONO) as r:
        want = [r.process(iq[:bb]), r.process(iq[bb: 2 * bb])]
    d = torch.zeros(iq.size, dtype=torch.uint8, device="cuda")
    d_p = torch.zeros(8192, dtype=torch.float32, device="cuda")
    with fmrx.Receiver(0, fmrx.MONO) as r:
        first = r.process(iq[:bb])
        for bins in (300, 128, 16384, 0, -4096):
            with pytest.raises(fmrx.FmrxError) as e:
                r.scan_spectrum(iq, bins)
            assert e.value.code == fmrx.FMRX_EINVAL
            with pytest.raises(fmrx.FmrxError) as e:
                r.scan_spectrum_device(d.data_ptr(), iq.size // 2, bins, d_p.data_ptr())
            assert e.value.code == fmrx.FMRX_EINVAL
            with pytest.raises(fmrx.FmrxError) as e:
                r.scan(iq, fft_bins=bins)
            assert e.value.code == fmrx.FMRX_EINVAL
        for short in (iq[: 2 * 4096 - 2], iq[:0]):  # n_pairs < fft_bins
            with pytest.raises(fmrx.FmrxError) as e:
                r.scan_spectrum(short, 4096)
            assert e.value.code == fmrx.FMRX_EINVAL
            with pytest.raises(fmrx.FmrxError) as e:
                r.scan(short)
            assert e.value.code == fmrx.FMRX_EINVAL
        with pytest.raises(fmrx.FmrxError) as e:
            r.scan_spectrum_device(d.data_ptr(), 4095, 4096, d_p.data_ptr())
        assert e.value.code == fmrx.FMRX_EINVAL
        for kw in ({"raster_hz": 0}, {"channel_hz": 0}, {"min_separation_hz": -1}, {"channel_hz": 2400000},
                   {"floor_percentile": 0}, {"floor_percentile": 100}, {"raster_origin_hz": 1}):
            with pytest.raises(fmrx.FmrxError) as e:
                r.scan(iq, **kw)
            assert e.value.code == fmrx.FMRX_EINVAL
        r.synchronize()
        assert not d_p.cpu().numpy().any()  # nothing written
        second = r.process(iq[bb: 2 * bb])
    assert np.array_equal(first, want[0]) and np.array_equal(second, want[1])


# ---- CLI ----------------------------------------------------------------------------------------------

def test_cli_scan(fmrx):
    exe = os.path.join(os.path.dirname(fmrx.LIB_PATH), "bin", "fmrx")
    iq = capture("three")[0]
    r = subprocess.run([exe, "0", "1", "--scan"], input=iq.tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [ln.split() for ln in r.stdout.decode().splitlines()]
    assert [int(x[0]) for x in rows] == [-900000, 100000, 700000] and all(len(x) == 3 for x in rows)
    with fmrx.Receiver(0, fmrx.MONO) as rx_:
        want = rx_.scan(iq)
    for x, s in zip(rows, want):
        assert abs(float(x[1]) - s.power_db) <= 0.01 and abs(float(x[2]) - s.snr_db) <= 0.01
    # --scan-bytes: only the first bytes are scanned (the rest of stdin is not needed)
    r2 = subprocess.run([exe, "0", "1", "--scan", "--scan-bytes", str(iq.size // 2)], input=iq.tobytes(),
                        capture_output=True, timeout=120)
    assert r2.returncode == 0 and [int(ln.split()[0]) for ln in r2.stdout.decode().splitlines()] == [-900000, 100000, 700000]
    empty = subprocess.run([exe, "0", "1", "--scan"], input=b"", capture_output=True, timeout=120)
    assert empty.returncode == 1 and b"--scan" in empty.stderr and empty.stdout == b""
