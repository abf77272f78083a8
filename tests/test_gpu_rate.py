"""GPU tests of captures at a rational rate (csrc/rate.hip; fmrx_set_capture_rate, then fmrx_tune_wide,
fmrx_process_wide, fmrx_scan_wide): every output is compared bit for bit with rate_compose of
tests/test_rate_host.py -- the format's normalisation and the coarse rotation in numpy float32, the
oracle's resample of I' and Q' by L / M with the oracle's taps, then the narrow composition of an f32
stream tuned to the fine offset.  No tolerance anywhere."""
from __future__ import annotations

import functools
import math
import os
import subprocess

import numpy as np
import pytest

import iqgen
import oracle
from test_formats_host import F32, S8, S16, U8, identity_map
from test_rate_host import R_CAP_FS, R_STATIONS, rate_compose, two_station_capture_10ms
from test_wide_host import Q_SCAN, wide_compose

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAMES = {U8: "u8", S8: "s8", S16: "s16", F32: "f32"}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def ratio(mode, cap_fs):
    rf_fs = oracle.MODES[mode][3]
    g = math.gcd(rf_fs, cap_fs)
    return rf_fs // g, cap_fs // g


def granule(mode, cap_fs):
    """(narrow blocks, array elements -- two a pair -- of the wide capture) of one granule."""
    up, down = ratio(mode, cap_fs)
    ip = oracle.MODES[mode][0] // 2
    b = up // math.gcd(up, ip)
    return b, 2 * (b * ip * down // up)


@functools.lru_cache(maxsize=None)
def capture(seed, mode, cap_fs, n_granules, fmt=U8):
    """Deterministic u8 I/Q (the synthetic station's bytes, read at the capture's rate) carried into
    fmt with the same normalised samples; read-only."""
    a = identity_map(iqgen.make(f"synth:{seed}", n_granules * granule(mode, cap_fs)[1], oracle.MODES[mode][3]), fmt)
    a.setflags(write=False)
    return a


def receiver(fm, fmt, cap_fs, mode=0, channels=None, **kw):
    rx = fm.Receiver(mode, fm.MONO if channels is None else channels, **kw)
    if fmt != U8:
        rx.set_input_format(fmt)
    rx.set_capture_rate(cap_fs)
    b, ge = granule(mode, cap_fs)
    assert (rx.input_format, rx.capture_decim, rx.capture_rate) == (fmt, 0, (cap_fs,) + ratio(mode, cap_fs))
    assert rx.wide_granule == (b, ge // 2)
    return rx


def in_calls(fn, raw, ge, calls):
    out, g = [], 0
    for ng in calls:
        out.append(fn(raw[..., g * ge:(g + ng) * ge]))
        g += ng
    return np.concatenate(out, axis=-1)


def mode0_offsets(cap_fs):
    rf_fs = oracle.MODES[0][3]
    return [0, rf_fs // 4, rf_fs // 8, -125000 + 2 * (rf_fs // 4), cap_fs // 2 - 100000]


# ---- mode 0, mono, u8: chunk edges, call edges, the history, the granule ---------------------------------------

@pytest.mark.parametrize("rf_taps", [51, 101])
@pytest.mark.parametrize("cap_fs", [10000000, 6000000, 2500000, 12500000])
def test_mode0_u8_matches_composition(fmrx, cap_fs, rf_taps):
    """6/25 (B = 3), 2/5 (L = 2, B = 1), 24/25 (the largest useful L; a call of one granule is 19,200
    outputs = 12.5 chunks of 64 L, a ragged tail chunk) and 24/125 (the largest M: 81,800 B of LDS).
    Five offsets: q = 0 (N_c = 1), q = 1 (the ratio's longest period, 4 M / gcd(L, 4 M): L is even in all
    four, so 4 M itself is not reached here -- test_other_modes reaches it at 9/16 and 9/10), the tie at
    rf_fs / 8, q = 2 with a fine part, and cap_fs / 2 - 100 kHz (N_c = 2 at 2/5, where 2 M / L is whole)."""
    up, down = ratio(0, cap_fs)
    (b, ge), calls = granule(0, cap_fs), [1, 2, 3]
    raw = capture(40 + up, 0, cap_fs, sum(calls))
    periods = set()
    with receiver(fmrx, U8, cap_fs, rf_taps=rf_taps) as rx:
        for f in mode0_offsets(cap_fs):
            periods.add(fmrx.rate_design(oracle.MODES[0][3], cap_fs, f)["N"])
            want = rate_compose(raw, U8, 0, rf_taps, cap_fs, f)["pcm_mono"]
            rx.reset()
            rx.tune_wide(f)
            got = in_calls(rx.process_wide, raw, ge, calls)
            assert rx.wide_info() == ([f], sum(calls) * ge // 2, True)
            assert rx.tuner_info()[1] == sum(calls) * b * oracle.MODES[0][0] // 2
            assert np.array_equal(got, want) and got.any(), f
            rx.reset()  # the same granules in one call (and after a reset: the same PCM again)
            assert rx.wide_info() == ([f], 0, True)
            assert np.array_equal(rx.process_wide(raw), want), f
    assert {1, 4 * down // math.gcd(up, 4 * down)} <= periods and (up != 2 or 2 in periods)


def test_blocks_outside_the_granule_are_refused(fmrx):
    cap_fs = 10000000
    (b, ge), na = granule(0, cap_fs), oracle.MODES[0][2]
    raw = capture(49, 0, cap_fs, 2)
    d_iq = torch.from_numpy(np.array(raw)).cuda()
    d_pcm = torch.zeros(2 * b * na, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with receiver(fmrx, U8, cap_fs) as rx:
        rx.tune_wide(700000, 50)
        for nb in (1, 2, 4, 5):
            with pytest.raises(fmrx.FmrxError) as e:
                rx.process_wide_device(d_iq.data_ptr(), nb, d_pcm.data_ptr())
            assert e.value.code == fmrx.FMRX_EINVAL
        for call in (rx.get_state, lambda: rx.set_state(b"\0" * 64), lambda: rx.seek(raw[:64])):
            with pytest.raises(fmrx.FmrxError) as e:
                call()
            assert e.value.code == fmrx.FMRX_ESTATE
        for bad in (2000000, 25200000, 2448000):  # below rf_fs, M > 10 L, L > 48: nothing changes
            with pytest.raises(fmrx.FmrxError) as e:
                rx.set_capture_rate(bad)
            assert e.value.code == fmrx.FMRX_EINVAL
        rx.synchronize()
        assert rx.wide_info() == ([700000], 50, True) and rx.capture_rate == (cap_fs, 6, 25)
        assert not d_pcm.cpu().numpy().any()  # no launch
        rx.process_wide_device(d_iq.data_ptr(), 2 * b, d_pcm.data_ptr())
        rx.synchronize()
    assert np.array_equal(d_pcm.cpu().numpy(), rate_compose(raw, U8, 0, 51, cap_fs, 700000, 50)["pcm_mono"])


# ---- formats ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [S8, S16, F32], ids=NAMES.get)
def test_formats(fmrx, fmt):
    cap_fs, f = 10000000, -(600000 + 200000)
    raw = capture(60, 0, cap_fs, 3, fmt)
    if fmt == S16:  # not only multiples of 256
        raw = (raw.astype(np.int32) + (np.arange(raw.size) * 7919) % 251 - 125).clip(-32768, 32767).astype(np.int16)
    elif fmt == F32:  # inside the promised range: 0 or [2^-20, 4]
        raw = (raw * np.float32(1.7)).astype(np.float32)
        assert np.abs(raw).max() <= 4.0 and np.all((raw == 0) | (np.abs(raw) >= 2.0 ** -20))
    with receiver(fmrx, fmt, cap_fs) as rx:
        rx.tune_wide(f)
        got = in_calls(rx.process_wide, raw, granule(0, cap_fs)[1], [1, 2])
    assert np.array_equal(got, rate_compose(raw, fmt, 0, 51, cap_fs, f)["pcm_mono"]) and got.any()


def test_format_set_after_rate(fmrx):
    """fmrx_set_input_format keeps the rate and re-makes the wide history at the new pair size."""
    cap_fs, f = 10000000, 1200000 + 100000
    raw = capture(66, 0, cap_fs, 2, S16)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        rx.set_capture_rate(cap_fs)
        rx.tune_wide(f)
        rx.process_wide(capture(67, 0, cap_fs, 1))  # u8 history behind it
        rx.set_input_format(S16)
        assert rx.capture_rate == (cap_fs, 6, 25) and rx.capture_decim == 0 and rx.wide_info() == ([f], 0, True)
        got = rx.process_wide(raw)
    assert np.array_equal(got, rate_compose(raw, S16, 0, 51, cap_fs, f)["pcm_mono"]) and got.any()


# ---- the other modes ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,cap_fs,calls,f", [(1, 2048000, [1, 2], 288000 + 50000), (2, 6000000, [1], -(1200000 + 100000)),
                                                 (3, 2560000, [1], 576000 - 30000)])
def test_other_modes(fmrx, mode, cap_fs, calls, f):
    """Mode 1 at 9/16 and mode 3 at 9/10 with q = 1: odd L, so N_c = 4 M (64 and 40)."""
    up, down = ratio(mode, cap_fs)
    if up % 2:
        assert fmrx.rate_design(oracle.MODES[mode][3], cap_fs, f)["N"] == 4 * down
    raw = capture(70 + mode, mode, cap_fs, sum(calls))
    with receiver(fmrx, U8, cap_fs, mode) as rx:
        rx.tune_wide(f)
        got = in_calls(rx.process_wide, raw, granule(mode, cap_fs)[1], calls)
    assert np.array_equal(got, rate_compose(raw, U8, mode, 51, cap_fs, f)["pcm_mono"]) and got.any()


def test_internal_pieces(fmrx):
    """Nine mode-2 streams make 74 MB of cf32 rows a block, more than half the 128 MiB a piece may hold:
    a call of two granules (one block each at 2/5) runs as two pieces, the second finding its history in
    the capture, and gives the bits of the composition in one piece."""
    mode, cap_fs, ns = 2, 6000000, 9
    offsets = [300000 + 100000 * s for s in range(ns)]
    raw = capture(75, mode, cap_fs, 2)
    with receiver(fmrx, U8, cap_fs, mode, n_streams=ns) as rx:
        rx.tune_wide(offsets)
        got = rx.process_wide(raw)
        assert rx.wide_info() == (offsets, raw.size // 2, True)
    for s in (0, ns - 1):
        assert np.array_equal(got[s], rate_compose(raw, U8, mode, 51, cap_fs, offsets[s])["pcm_mono"]) and got[s].any(), s
    assert len({row.tobytes() for row in got}) == ns


def test_workgroups_walk_several_chunks(fmrx):
    """16 stations on one mode-0 capture at 10 MS/s of 3 granules (9 blocks, 57,600 outputs a station).  A
    chunk is 64 L = 384 outputs, so a station has 150 chunks; a workgroup takes 8 (500 + 25 * 67 + 64 * 7)
    = 20,984 B of LDS, 7 fit a CU, and rate_segments' target is 7 workgroups a CU: 1,792 on 256 CUs,
    below the 16 * 150 = 2,400 chunks.  Hence segments of at least four chunks (min(1792 / 16, 150 / 4) =
    37 a station): every workgroup's chunks past its first take their history from the copy in LDS."""
    cap_fs, ns = 10000000, 16
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lds = 8 * (500 + 25 * 67 + 64 * 7)
    chunks = 3 * 3 * 6400 // (64 * 6)
    target = cus * min(8, 160 * 1024 // lds)
    assert chunks == 150 and ns * chunks > target, "the shape no longer makes a workgroup walk chunks"
    offsets = [-4000000 + 500000 * s + 7000 * (s % 3) for s in range(ns)]
    raw = capture(76, 0, cap_fs, 3)
    with receiver(fmrx, U8, cap_fs, n_streams=ns) as rx:
        rx.tune_wide(offsets)
        got = rx.process_wide(raw)
    for s in (0, 7, ns - 1):
        assert np.array_equal(got[s], rate_compose(raw, U8, 0, 51, cap_fs, offsets[s])["pcm_mono"]) and got[s].any(), s
    assert len({row.tobytes() for row in got}) == ns


# ---- stereo: two stations of one capture -------------------------------------------------------------------------

def test_stereo_two_streams(fmrx):
    offsets = [f for _, f in R_STATIONS]
    ge = granule(0, R_CAP_FS)[1]
    raw = two_station_capture_10ms()[: 2 * ge]
    want = np.stack([rate_compose(raw, S16, 0, 51, R_CAP_FS, f, fields=("pcm",))["pcm"] for f in offsets])
    with receiver(fmrx, S16, R_CAP_FS, channels=fmrx.STEREO, n_streams=2) as rx:
        rx.tune_wide(offsets)
        got = in_calls(rx.process_wide, raw, ge, [1, 1])
    assert np.array_equal(got, want) and got[0].any() and got[1].any()
    assert not np.array_equal(got[0], got[1])


# ---- position: the 64-bit reduction --------------------------------------------------------------------------

def test_far_position(fmrx):
    """A first pair past 2^33: the first multiple of M = 25 above it, plus 25 * 6."""
    cap_fs, f = 10000000, 600000 + 7000  # N_c = 50, and a fine period of 2400 pairs at rf_fs
    first = (2 ** 33 + 24) // 25 * 25 + 25 * 6
    raw = capture(80, 0, cap_fs, 1)
    with receiver(fmrx, U8, cap_fs) as rx:
        for bad in (first + 1, first + 6, 2 ** 33):  # no multiple of M
            with pytest.raises(fmrx.FmrxError) as e:
                rx.tune_wide(f, bad)
            assert e.value.code == fmrx.FMRX_EINVAL
        assert rx.wide_info() == ([0], 0, False)
        rx.tune_wide(f, first)
        assert rx.tuner_info()[1] == first // 25 * 6
        got = rx.process_wide(raw)
        assert rx.wide_info() == ([f], first + raw.size // 2, True)
    assert np.array_equal(got, rate_compose(raw, U8, 0, 51, cap_fs, f, first)["pcm_mono"]) and got.any()
    assert not np.array_equal(got, rate_compose(raw, U8, 0, 51, cap_fs, f, 0)["pcm_mono"])


# ---- isolation ------------------------------------------------------------------------------------------------

def test_scan_between_calls_and_timing(fmrx):
    cap_fs, f = 6000000, 600000 + 100000
    ge = granule(0, cap_fs)[1]
    raw = capture(81, 0, cap_fs, 4)
    with receiver(fmrx, U8, cap_fs) as rx:
        rx.tune_wide(f)
        whole = rx.process_wide(raw)
        rx.reset()
        a = rx.process_wide(raw[: 2 * ge])
        rx.scan_wide(raw)
        rx.kernel_timing(reset=1)  # armed: the down-converter's launches are timed
        b = rx.process_wide(raw[2 * ge:])
        ms, n = rx.kernel_timing()
    assert np.array_equal(np.concatenate([a, b]), whole) and whole.any()
    assert n == 1 and ms > 0.0


def test_integer_rate_is_the_decimating_stage(fmrx):
    """set_capture_rate(4 rf_fs) does what set_capture_decim(4) does: the same bits, capture_decim 4."""
    d, f = 4, 600000 + 7000
    rf_fs = oracle.MODES[0][3]
    raw = iqgen.make("synth:82", 3 * d * oracle.MODES[0][0], rf_fs)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        rx.set_capture_decim(d)
        rx.tune_wide(f)
        want = rx.process_wide(raw)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        rx.set_capture_rate(10000000)  # through the rational state first
        rx.tune_wide(f)
        rx.process_wide(capture(83, 0, 10000000, 1))
        rx.set_capture_rate(d * rf_fs)
        assert rx.capture_decim == d and rx.capture_rate == (d * rf_fs, 1, d)
        assert rx.wide_granule == (1, d * oracle.MODES[0][0] // 2) and rx.wide_info()[2] is False
        rx.tune_wide(f)
        got = rx.process_wide(raw)
        rx.set_capture_rate(rf_fs)  # D = 1: no wide stage
        assert rx.capture_decim == 1 and rx.capture_rate == (rf_fs, 1, 1)
        rx.get_state()
        rx.set_capture_rate(10000000)
        rx.set_capture_decim(1)  # leaves the rational rate
        assert rx.capture_decim == 1 and rx.capture_rate == (rf_fs, 1, 1)
    assert np.array_equal(got, want) and np.array_equal(got, wide_compose(raw, U8, 0, 51, d, f)["pcm_mono"]) and got.any()


def test_one_context_walks_integer_rational_integer(fmrx):
    """One context through D = 2, then 6/25, then D = 10: the stage's buffers are shared, the tap buffer
    holds floats in the integer states and taps by phase in the rational one, and the rational table of
    q = 1 (N_c = 50) is longer than any integer one (at most 40).  Every step is one call of one granule,
    bit for bit the composition of its own state."""
    rf_fs, be = oracle.MODES[0][3], oracle.MODES[0][0]
    cap_fs = 10000000
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        f = rf_fs // 4 + 7000  # q = 1: N_c = 8
        assert fmrx.wide_design(rf_fs, 2, f)["N"] == 8
        raw = iqgen.make("synth:86", 2 * be, rf_fs)
        rx.set_capture_decim(2)
        assert rx.wide_info()[2] is False
        rx.tune_wide(f)
        got = rx.process_wide(raw)
        assert np.array_equal(got, wide_compose(raw, U8, 0, 51, 2, f)["pcm_mono"]) and got.any()

        f = rf_fs // 4  # q = 1: N_c = 50
        assert fmrx.rate_design(rf_fs, cap_fs, f)["N"] == 50
        raw = capture(87, 0, cap_fs, 1)
        rx.set_capture_rate(cap_fs)
        assert rx.wide_info()[2] is False and rx.capture_rate == (cap_fs, 6, 25) and rx.wide_granule[0] == 3
        rx.tune_wide(f)
        got = rx.process_wide(raw)
        assert np.array_equal(got, rate_compose(raw, U8, 0, 51, cap_fs, f)["pcm_mono"]) and got.any()

        f = rf_fs // 4 - 30000  # q = 1: N_c = 40
        assert fmrx.wide_design(rf_fs, 10, f)["N"] == 40
        raw = iqgen.make("synth:88", 10 * be, rf_fs)
        rx.set_capture_decim(10)
        assert rx.wide_info()[2] is False and rx.capture_decim == 10
        rx.tune_wide(f)
        got = rx.process_wide(raw)
        assert np.array_equal(got, wide_compose(raw, U8, 0, 51, 10, f)["pcm_mono"]) and got.any()


# ---- scan and decode ------------------------------------------------------------------------------------------

def test_scan_and_decode_stations(fmrx):
    raw = two_station_capture_10ms()[: 3 * granule(0, R_CAP_FS)[1]]
    found = sorted(f for _, f in R_STATIONS)
    with receiver(fmrx, S16, R_CAP_FS) as rx:
        assert [s.offset_hz for s in rx.scan_wide(raw, **Q_SCAN)] == found
    stations, pcm = fmrx.decode_stations(raw, capture_rate=R_CAP_FS, **Q_SCAN)
    assert [s.offset_hz for s in stations] == found
    for row, f in zip(pcm, found):
        assert np.array_equal(row, rate_compose(raw, S16, 0, 51, R_CAP_FS, f)["pcm_mono"]), f
    with pytest.raises(ValueError):
        fmrx.decode_stations(raw, capture_rate=R_CAP_FS, capture_decim=4)


# ---- CLI ---------------------------------------------------------------------------------------------------------

def cli(fm, args, data):
    exe = os.path.join(os.path.dirname(fm.LIB_PATH), "bin", "fmrx")
    return subprocess.run([exe] + args, input=data, capture_output=True, timeout=120)


def test_cli_capture_rate(fmrx):
    cap_fs, f = 10000000, -(600000 + 150000)
    raw = capture(85, 0, cap_fs, 2)
    tail = raw[: granule(0, cap_fs)[1] // 3].tobytes()  # a trailing part of a granule is dropped
    r = cli(fmrx, ["0", "1", "--mono-product", "--capture-rate", str(cap_fs), "--offset-hz", str(f)], raw.tobytes() + tail)
    assert r.returncode == 0, r.stderr
    want = rate_compose(raw, U8, 0, 51, cap_fs, f)["pcm_mono"]
    assert np.array_equal(np.frombuffer(r.stdout, np.int16), want) and want.any()
    for args, word in ((["--capture-rate", "25200000"], b"capture-rate"), (["--capture-rate", "0"], b"capture-rate"),
                       (["--capture-rate", str(cap_fs), "--capture-decim", "4"], b"exclude")):
        rb = cli(fmrx, ["0", "1"] + args, b"")
        assert rb.returncode == 1 and word in rb.stderr
