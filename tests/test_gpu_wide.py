"""GPU tests of wide captures (csrc/wide.hip; fmrx_set_capture_decim, fmrx_tune_wide,
fmrx_process_wide, fmrx_scan_wide): every output is compared bit for bit with the composition of
tests/test_wide_host.py -- the format's normalisation and the coarse rotation in numpy float32, the
oracle's resample of I' and Q' with the oracle's taps, then the narrow composition of an f32 stream
tuned to the fine offset.  No tolerance anywhere."""
from __future__ import annotations

import functools
import os
import subprocess

import numpy as np
import pytest

import iqgen
import oracle
from test_formats_host import F32, S8, S16, U8, identity_map
from test_wide_host import Q_D, Q_MODE, Q_SCAN, Q_STATIONS, two_station_capture, wide_compose

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAMES = {U8: "u8", S8: "s8", S16: "s16", F32: "f32"}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def block_elems(mode, d):
    """Array elements (two a pair) of one wide block, the same in every format."""
    return oracle.MODES[mode][0] * d


@functools.lru_cache(maxsize=None)
def capture(seed, mode, d, n_blocks, fmt=U8):
    """Deterministic u8 I/Q (the synthetic station's bytes, read at the capture's rate) carried into
    fmt with the same normalised samples; read-only."""
    a = identity_map(iqgen.make(f"synth:{seed}", n_blocks * block_elems(mode, d), oracle.MODES[mode][3]), fmt)
    a.setflags(write=False)
    return a


def receiver(fm, fmt, d, mode=0, channels=None, **kw):
    rx = fm.Receiver(mode, fm.MONO if channels is None else channels, **kw)
    if fmt != U8:
        rx.set_input_format(fmt)
    rx.set_capture_decim(d)
    assert (rx.input_format, rx.capture_decim) == (fmt, d)
    return rx


def in_calls(fn, raw, be, calls):
    out, b = [], 0
    for nb in calls:
        out.append(fn(raw[..., b * be:(b + nb) * be]))
        b += nb
    return np.concatenate(out, axis=-1)


def mode0_offsets(d):
    rf_fs = oracle.MODES[0][3]
    return [0, rf_fs // 4, rf_fs // 8, -125000 + 2 * (rf_fs // 4), d * rf_fs // 2 - 100000]


# ---- mode 0, mono, u8: chunk edges, call edges, the history; N_c of 1, 2 and 4 D ----------------------------

@pytest.mark.parametrize("rf_taps", [51, 101])
@pytest.mark.parametrize("d", [2, 3, 8])
def test_mode0_u8_matches_composition(fmrx, d, rf_taps):
    be, calls = block_elems(0, d), [1, 2, 3]
    raw = capture(40 + d, 0, d, sum(calls))
    with receiver(fmrx, U8, d, rf_taps=rf_taps) as rx:
        for f in mode0_offsets(d):
            want = wide_compose(raw, U8, 0, rf_taps, d, f)["pcm_mono"]
            rx.reset()
            rx.tune_wide(f)
            got = in_calls(rx.process_wide, raw, be, calls)
            assert rx.wide_info() == ([f], sum(calls) * be // 2, True)
            assert rx.tuner_info()[1] == sum(calls) * be // (2 * d)
            assert np.array_equal(got, want) and got.any(), f
            rx.reset()  # the same blocks in one call (and after a reset: the same PCM again)
            assert rx.wide_info() == ([f], 0, True)
            assert np.array_equal(rx.process_wide(raw), want), f


def test_mode0_decim10(fmrx):
    d, f = 10, 3 * 600000 + 37000  # N_c = 40
    raw = capture(50, 0, d, 3)
    with receiver(fmrx, U8, d) as rx:
        rx.tune_wide(f)
        got = in_calls(rx.process_wide, raw, block_elems(0, d), [1, 2])
    assert np.array_equal(got, wide_compose(raw, U8, 0, 51, d, f)["pcm_mono"]) and got.any()


# ---- formats ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("fmt", [S8, S16, F32], ids=NAMES.get)
def test_formats(fmrx, fmt, d):
    f = -(600000 + 200000)
    raw = capture(60 + d, 0, d, 3, fmt)
    if fmt == S16:  # not only multiples of 256
        raw = (raw.astype(np.int32) + (np.arange(raw.size) * 7919) % 251 - 125).clip(-32768, 32767).astype(np.int16)
    elif fmt == F32:  # inside the promised range: 0 or [2^-20, 4]
        raw = (raw * np.float32(1.7)).astype(np.float32)
        assert np.abs(raw).max() <= 4.0 and np.all((raw == 0) | (np.abs(raw) >= 2.0 ** -20))
    with receiver(fmrx, fmt, d) as rx:
        rx.tune_wide(f)
        got = in_calls(rx.process_wide, raw, block_elems(0, d), [1, 2])
    assert np.array_equal(got, wide_compose(raw, fmt, 0, 51, d, f)["pcm_mono"]) and got.any()


def test_format_set_after_decim(fmrx):
    """fmrx_set_input_format keeps the decimation and re-makes the wide history at the new pair size."""
    d, f = 3, 1200000 + 100000
    raw = capture(66, 0, d, 2, S16)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        rx.set_capture_decim(d)
        rx.tune_wide(f)
        rx.process_wide(capture(67, 0, d, 1))  # u8 history behind it
        rx.set_input_format(S16)
        assert rx.capture_decim == d and rx.wide_info() == ([f], 0, True)
        got = rx.process_wide(raw)
    assert np.array_equal(got, wide_compose(raw, S16, 0, 51, d, f)["pcm_mono"]) and got.any()


# ---- the other modes ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,d,calls,f", [(1, 3, [1, 2], 288000 + 50000), (2, 2, [1], -(1200000 + 100000)),
                                            (3, 2, [1], 576000 - 30000)])
def test_other_modes(fmrx, mode, d, calls, f):
    raw = capture(70 + mode, mode, d, sum(calls))
    with receiver(fmrx, U8, d, mode) as rx:
        rx.tune_wide(f)
        got = in_calls(rx.process_wide, raw, block_elems(mode, d), calls)
    assert np.array_equal(got, wide_compose(raw, U8, mode, 51, d, f)["pcm_mono"]) and got.any()


def test_internal_pieces(fmrx):
    """Nine mode-2 streams make 74 MB of cf32 rows a block, more than half the 128 MiB a piece may
    hold: a call of two blocks runs as two pieces, and gives the bits of the composition in one piece."""
    mode, d, ns = 2, 2, 9
    offsets = [300000 + 100000 * s for s in range(ns)]
    raw = capture(75, mode, d, 2)
    with receiver(fmrx, U8, d, mode, n_streams=ns) as rx:
        rx.tune_wide(offsets)
        got = rx.process_wide(raw)
        assert rx.wide_info() == (offsets, raw.size // 2, True)
    for s in (0, ns - 1):
        assert np.array_equal(got[s], wide_compose(raw, U8, mode, 51, d, offsets[s])["pcm_mono"]) and got[s].any(), s
    assert len({row.tobytes() for row in got}) == ns


# ---- stereo: two stations of one capture -------------------------------------------------------------------------

def test_stereo_two_streams(fmrx):
    d, offsets = 4, [1700000, -3100000]
    raw = two_station_capture()[: 4 * block_elems(0, d)]
    want = np.stack([wide_compose(raw, S16, 0, 51, d, f, fields=("pcm",))["pcm"] for f in offsets])
    with receiver(fmrx, S16, d, channels=fmrx.STEREO, n_streams=2) as rx:
        rx.tune_wide(offsets)
        got = in_calls(rx.process_wide, raw, block_elems(0, d), [2, 2])
    assert np.array_equal(got, want) and got[0].any() and got[1].any()
    assert not np.array_equal(got[0], got[1])


# ---- position: the 64-bit reduction --------------------------------------------------------------------------

def test_far_position(fmrx):
    d, f = 4, 600000 + 7000  # N_c = 16, and a fine period of 2400 pairs at rf_fs
    first = 2 ** 33 + 6 * d
    raw = capture(80, 0, d, 2)
    with receiver(fmrx, U8, d) as rx:
        rx.tune_wide(f, first)
        got = rx.process_wide(raw)
        assert rx.wide_info() == ([f], first + raw.size // 2, True)
    assert np.array_equal(got, wide_compose(raw, U8, 0, 51, d, f, first)["pcm_mono"]) and got.any()
    assert not np.array_equal(got, wide_compose(raw, U8, 0, 51, d, f, 0)["pcm_mono"])


# ---- isolation ------------------------------------------------------------------------------------------------

def test_scan_between_calls_and_reset(fmrx):
    d, f = 2, 600000 + 100000
    be = block_elems(0, d)
    raw = capture(81, 0, d, 4)
    with receiver(fmrx, U8, d) as rx:
        rx.tune_wide(f)
        whole = rx.process_wide(raw)
        rx.reset()
        a = rx.process_wide(raw[: 2 * be])
        rx.scan_wide(raw)
        b = rx.process_wide(raw[2 * be:])
    assert np.array_equal(np.concatenate([a, b]), whole) and whole.any()


def test_decim1_is_untouched(fmrx):
    iq = capture(82, 0, 1, 4)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        want = rx.process(iq)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        rx.set_capture_decim(1)
        with pytest.raises(fmrx.FmrxError) as e:
            rx.tune_wide(0)
        assert e.value.code == fmrx.FMRX_ESTATE
        assert rx.capture_decim == 1 and rx.tuner_info() == ([0], 0, False)
        rx.set_capture_decim(2)  # through the wide state and back
        rx.tune_wide(700000)
        rx.process_wide(capture(83, 0, 2, 1))
        rx.set_capture_decim(1)
        rx.tune(None)
        got = rx.process(iq)
        rx.get_state()
    assert np.array_equal(got, want)


# ---- scan and decode ------------------------------------------------------------------------------------------

def test_scan_and_decode_stations(fmrx):
    raw = two_station_capture()[: 8 * block_elems(Q_MODE, Q_D)]
    found = sorted(f for _, f in Q_STATIONS)
    with receiver(fmrx, S16, Q_D) as rx:
        assert [s.offset_hz for s in rx.scan_wide(raw, **Q_SCAN)] == found
    stations, pcm = fmrx.decode_stations(raw, capture_decim=Q_D, **Q_SCAN)
    assert [s.offset_hz for s in stations] == found
    for row, f in zip(pcm, found):
        assert np.array_equal(row, wide_compose(raw, S16, Q_MODE, 51, Q_D, f)["pcm_mono"]), f


# ---- errors: the code, no launch, no state change -------------------------------------------------------------

def test_refused_calls(fmrx):
    d, na = 2, oracle.MODES[0][2]
    raw = capture(84, 0, d, 2)
    d_iq = torch.from_numpy(np.array(raw)).cuda()
    d_pcm = torch.zeros(na, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        for bad in (0, -1, 11):
            with pytest.raises(fmrx.FmrxError) as e:
                rx.set_capture_decim(bad)
            assert e.value.code == fmrx.FMRX_EINVAL and rx.capture_decim == 1
        for call in (lambda: rx.tune_wide(0), lambda: rx.scan_wide(raw),
                     lambda: rx.process_wide_device(d_iq.data_ptr(), 1, d_pcm.data_ptr())):
            with pytest.raises(fmrx.FmrxError) as e:
                call()
            assert e.value.code == fmrx.FMRX_ESTATE
    with receiver(fmrx, U8, d) as rx:
        with pytest.raises(fmrx.FmrxError) as e:  # process_wide before tune_wide
            rx.process_wide_device(d_iq.data_ptr(), 1, d_pcm.data_ptr())
        assert e.value.code == fmrx.FMRX_ESTATE
        rx.tune_wide(700000, 4)
        for offsets, first in ((700000, 5), (2400000, 4), (600001, 4)):  # position, range, fine part
            with pytest.raises(fmrx.FmrxError) as e:
                rx.tune_wide(offsets, first)
            assert e.value.code == fmrx.FMRX_EINVAL
        assert rx.wide_info() == ([700000], 4, True) and rx.tuner_info() == ([100000], 2, True)
        with pytest.raises(fmrx.FmrxError) as e:  # one pair off: half a staging unit
            rx.process_wide_device(d_iq.data_ptr() + 2, 1, d_pcm.data_ptr())
        assert e.value.code == fmrx.FMRX_EINVAL
        for call in (rx.get_state, lambda: rx.set_state(b"\0" * 64), lambda: rx.seek(raw[:64])):
            with pytest.raises(fmrx.FmrxError) as e:
                call()
            assert e.value.code == fmrx.FMRX_ESTATE
        rx.synchronize()
        assert rx.wide_info() == ([700000], 4, True)
    assert not d_pcm.cpu().numpy().any()  # no launch


# ---- CLI ---------------------------------------------------------------------------------------------------------

def cli(fm, args, data):
    exe = os.path.join(os.path.dirname(fm.LIB_PATH), "bin", "fmrx")
    return subprocess.run([exe] + args, input=data, capture_output=True, timeout=120)


def test_cli_capture_decim(fmrx):
    d, f = 2, -(600000 + 150000)
    raw = capture(85, 0, d, 4)
    r = cli(fmrx, ["0", "1", "--mono-product", "--capture-decim", str(d), "--offset-hz", str(f)], raw.tobytes())
    assert r.returncode == 0, r.stderr
    want = wide_compose(raw, U8, 0, 51, d, f)["pcm_mono"]
    assert np.array_equal(np.frombuffer(r.stdout, np.int16), want) and want.any()
    r0 = cli(fmrx, ["0", "1", "--mono-product", "--capture-decim", str(d)], raw.tobytes())  # offset 0
    assert r0.returncode == 0 and np.array_equal(np.frombuffer(r0.stdout, np.int16),
                                                 wide_compose(raw, U8, 0, 51, d, 0)["pcm_mono"])
    for bad in ("0", "11"):
        rb = cli(fmrx, ["0", "1", "--capture-decim", bad], b"")
        assert rb.returncode == 1 and b"capture-decim" in rb.stderr
