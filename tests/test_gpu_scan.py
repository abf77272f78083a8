"""GPU tests of the band scan (csrc/scan.hip, fmrx_scan*): the spectrum against numpy float64 (the
definition in include/fmrx.h, restated in tests/test_scan_host.py), bit identity between the entry
points, runs and alignments, the scan end to end and through the CLI, and that a scan leaves the
receiver state alone.  SCAN_CASES names every compiled scan_segments_kernel<log2 N, F>
(tests/test_variants_host.py compares the list with the library): each meets float64 on one segment,
on a few, and on more segments than the launch has workgroups.

Tolerances (a numpy float32 radix-2 prototype, every product and sum in float32, against float64 on
these inputs): one bin differed by at most 5e-4 dB (single-segment low-power bins), the power
integrated over a 150 kHz candidate by at most 1.6e-5 dB; the bounds are 0.01 dB and 1e-3 dB."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import oracle
from test_formats_host import DTYPES, F32, S8, S16, U8, normalise
from test_scan_host import (DEFAULTS, candidate_bins, capture, quantised, rf_fs_of, welch64)

pytestmark = pytest.mark.gpu

torch = None  # imported by the _gpu fixture, like gf (tests/test_gpu_formats.py): SCAN_CASES imports without them
gf = None

BIN_TOL_DB = 0.01
CAND_TOL_DB = 1e-3

NAMES = {U8: "u8", S8: "s8", S16: "s16", F32: "f32"}
# scan_segments_kernel<log2 N, F>: six sizes in four formats
SCAN_CASES = [(log2n, fmt) for log2n in range(8, 14) for fmt in (U8, S8, S16, F32)]
# the cases that also run with more segments than workgroups: u8 at every size, the three pairs whose
# loads happen at staging time (PF false in the kernel), and each other format with its loads in flight
SCAN_WALK_CASES = [(log2n, U8) for log2n in range(8, 14)] + [(13, S16), (12, F32), (13, F32), (9, S8), (8, S16), (9, F32)]


def case_id(case):
    return f"{1 << case[0]}-{NAMES[case[1]]}"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    global torch, gf
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()
    import test_gpu_formats

    gf = test_gpu_formats


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


# ---- every instantiation against numpy float64 -------------------------------------------------------

def welch64_slabs(raw, fmt, n, slab=128):
    """gf.welch64 (fmrx.h's power spectrum in float64 on the format's normalised samples, FFT-shifted)
    summed over slabs of segments, so that a long capture never stands in memory as complex128."""
    nseg = raw.size // 2 // n
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)
    total = np.zeros(n, np.float64)
    for s0 in range(0, nseg, slab):
        x = normalise(raw[2 * n * s0: 2 * n * min(nseg, s0 + slab)], fmt).astype(np.float64)
        z = (x[0::2] + 1j * x[1::2]).reshape(-1, n)
        total += (np.abs(np.fft.fft(z * w, axis=1)) ** 2).sum(axis=0)
    return np.fft.fftshift(8.0 / (3.0 * n * n * nseg) * total)


def check_bins(got, want, label):
    """Every bin of got (float32, from the GPU) against want (float64), which must keep every bin off
    float32's rounding floor."""
    assert got.dtype == np.float32 and got.shape == want.shape
    assert want.min() >= 1e-6 * want.max(), label
    worst = float(np.max(np.abs(db(got.astype(np.float64)) - db(want))))
    print(f"{label}: worst bin {worst:.2e} dB")
    assert worst <= BIN_TOL_DB, label


def white(fmt, n_pairs, seed):
    """Non-repeating white noise: uniform random bytes, or normal samples of sigma 1/4 of full scale
    (int16 by rint with clipping)."""
    rng = np.random.default_rng(seed)
    if fmt in (U8, S8):
        return rng.integers(0, 256, 2 * n_pairs, dtype=np.uint8).view(DTYPES[fmt])
    x = rng.standard_normal(2 * n_pairs, dtype=np.float32) * np.float32(0.25)
    if fmt == S16:
        return np.clip(np.rint(x * np.float32(32768.0)), -32768, 32767).astype(np.int16)
    return x


# Seeds of the one-segment inputs.  One Hann-windowed segment of white noise has a smallest bin near
# 1 / (9 N) of its largest (the smallest of N exponential variates over the largest), 1.4e-5 at 8192
# bins, so check_bins' 1e-6 leaves little room and the seeds are chosen on the float64 spectra alone:
# uniform bytes of seed 1 give 1.0e-5 (8192 bins) .. 2.0e-4 (512), the normal samples of seed 14 give
# 8.2e-6 at the least over every size here.  (Two stations plus noise of sigma 2^-8, the input of
# tests/test_gpu_formats.py::test_scan_real_data_against_float64, cannot serve for one segment: an FM
# carrier is nearly a line within so short a time and the smallest bin falls to 2e-9 .. 8e-8 of it.  That
# test runs the stations at every size over 6 to 200 segments instead.)
BYTE_SEED, NORMAL_SEED = 1, 14


def noise_like(fmt, n_pairs):
    return white(fmt, n_pairs, BYTE_SEED if fmt in (U8, S8) else NORMAL_SEED)


@pytest.mark.parametrize("case", SCAN_CASES, ids=case_id)
def test_every_instantiation_one_segment_and_a_few(fmrx, case):
    """N pairs (one segment: nothing is averaged) and 3 N + 100 pairs (three segments and a dropped tail)."""
    log2n, fmt = case
    n = 1 << log2n
    raw = noise_like(fmt, 3 * n + 100)
    with gf.receiver(fmrx, fmt) as r:
        for n_pairs in (n, 3 * n + 100):
            part = raw[: 2 * n_pairs]
            got, nseg = r.scan_spectrum(part, n)
            assert nseg == n_pairs // n
            want = gf.welch64(part, fmt, n)
            assert np.allclose(welch64_slabs(part, fmt, n, 2), want, rtol=1e-12, atol=0.0)
            check_bins(got, want, f"{NAMES[fmt]} bins={n} pairs={n_pairs}")
            if fmt == U8:
                check_spectrum(got, part, n)  # and the candidates


def walk_segments(n, cus):
    """2 G_max + 1 segments, G_max the most workgroups scan_workgroups can make: workgroups of 256 threads
    (32 waves a CU: 8) with 8 (N + N / 16) bytes of static LDS (160 KiB a CU).  The occupancy call can only
    return this or less, so every workgroup takes at least two segments and some take three."""
    return 2 * cus * min(8, 160 * 1024 // (8 * (n + n // 16))) + 1


@pytest.mark.parametrize("case", SCAN_WALK_CASES, ids=case_id)
def test_more_segments_than_workgroups(fmrx, case):
    """The grid-stride loop on white noise that never repeats: segments past a workgroup's first come
    through the loads inside the loop (in flight during the transform, or at staging time where they do
    not fit the registers) and add to a live accumulator.  A stale segment in place of half of them moves
    the worst bin of the float64 average by 0.2 dB (256 bins) to 0.55 dB (8192), twenty times the bound."""
    log2n, fmt = case
    n = 1 << log2n
    nseg = walk_segments(n, torch.cuda.get_device_properties(0).multi_processor_count)
    raw = white(fmt, nseg * n, 2)
    with gf.receiver(fmrx, fmt) as r:
        got, got_seg = r.scan_spectrum(raw, n)
    assert got_seg == nseg
    check_bins(got, welch64_slabs(raw, fmt, n), f"{NAMES[fmt]} bins={n} nseg={nseg} white")


@pytest.mark.parametrize("case", SCAN_WALK_CASES, ids=case_id)
def test_one_live_segment_among_blanks(fmrx, case):
    """Every pair the format's zero but for one segment of noise, first at index 0, then at nseg - 1, then
    in the middle: the spectrum is that segment's float64 spectrum divided by nseg, bin by bin.  Nothing is
    averaged away: at nseg - 1 the segment is some workgroup's second or third, so its samples came through
    the loads inside the loop; at 0 the later blank segments add exactly nothing to a live accumulator."""
    log2n, fmt = case
    n = 1 << log2n
    nseg = walk_segments(n, torch.cuda.get_device_properties(0).multi_processor_count)
    blank = 128 if fmt == U8 else 0
    live = noise_like(fmt, n)
    want = gf.welch64(live, fmt, n) / nseg
    raw = np.full(2 * nseg * n, blank, DTYPES[fmt])
    with gf.receiver(fmrx, fmt) as r:
        for at in (0, nseg - 1, nseg // 2):
            raw[2 * n * at: 2 * n * (at + 1)] = live
            got, got_seg = r.scan_spectrum(raw, n)
            assert got_seg == nseg
            check_bins(got, want, f"{NAMES[fmt]} bins={n} nseg={nseg} live segment at {at}")
            raw[2 * n * at: 2 * n * (at + 1)] = blank


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


@pytest.mark.parametrize("n", [256, 512, 1024, 2048, 4096])
def test_two_byte_aligned_device_pointer(rx, n):
    """d_iq advanced by one pair: the capture starts 2 bytes off a dword (one, one, two, four and eight
    funnel-shifted dwords a thread and segment)."""
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
