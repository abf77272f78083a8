"""GPU tests of the raw I/Q formats (fmrx_set_input_format: u8, s8, s16, f32) through the tuned
front end (csrc/tuner.hip), the band scan (csrc/scan.hip), the state and seek entry points and the
CLI.  Expected demod and PCM come from the pinned oracle composed around a float32 rotation exactly
as tests/test_gpu_tuner.py::compose does, with the first step replaced by the format's normalisation
in numpy float32 (tests/test_formats_host.py::normalise); everything is compared bit for bit.

The one tolerance, 0.01 dB a bin of the spectrum against numpy float64, is tests/test_gpu_scan.py's
BIN_TOL_DB (the float32 transform on inputs whose bins all sit far above float32's rounding floor,
which test_scan_real_data_against_float64 asserts of its input first).

Float32 captures built here hold no sample of magnitude in (0, 2^-20): fmrx.h promises the bits for
samples that are 0 or in [2^-20, 4], so smaller ones are set to 0 when the capture is made."""
from __future__ import annotations

import functools
import os
import subprocess

import numpy as np
import pytest

import iqgen
import oracle
from test_formats_host import F32, PAIR_BYTES, S8, S16, U8, identity_map, normalise

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BIN_TOL_DB = 0.01
NAMES = {U8: "u8", S8: "s8", S16: "s16", F32: "f32"}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


_ORC = None


def _orc():
    global _ORC
    if _ORC is None:
        _ORC = oracle.Oracle()
    return _ORC


def compose(raw, fmt, mode, rf_taps, offset, first_pair=0, fields=("pcm_mono",)):
    """The expected demod and audio outputs of one stream of format fmt tuned to `offset`, from
    position first_pair, over the whole of raw in one piece."""
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


def block_elems(mode):
    """Array elements (two a pair) of one block, the same in every format."""
    return oracle.MODES[mode][0]


@functools.lru_cache(maxsize=None)
def synth(seed, mode, n_blocks):
    a = iqgen.make(f"synth:{seed}", n_blocks * block_elems(mode), oracle.MODES[mode][3])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def mapped(seed, mode, n_blocks, fmt):
    a = identity_map(synth(seed, mode, n_blocks), fmt)
    a.setflags(write=False)
    return a


def rotated(iq, rf_fs, f, amp=1.0):
    """iq moved to +f Hz in float64 (times amp), as complex samples."""
    z = (iq[0::2].astype(np.float64) - 128.0) / 128.0 + 1j * (iq[1::2].astype(np.float64) - 128.0) / 128.0
    n = np.arange(z.size, dtype=np.float64)
    return amp * z * np.exp(2j * np.pi * (f / rf_fs) * n)


def interleave(z):
    out = np.empty(2 * z.size, np.float64)
    out[0::2], out[1::2] = z.real, z.imag
    return out


def as_s16(z):
    return np.clip(np.rint(interleave(z) * 32768.0), -32768, 32767).astype(np.int16)


def as_f32(z, scale=1.0):
    f = (interleave(z) * scale).astype(np.float32)
    f[np.abs(f) < np.float32(2.0 ** -20)] = 0.0  # the promised range: 0 or [2^-20, 4]
    assert np.abs(f).max() <= 4.0
    return f


OFFSETS = (-300000, 300000)


@functools.lru_cache(maxsize=None)
def real_capture(mode, n_blocks, fmt, scale=1.0):
    """Two stations at -+300 kHz, total amplitude 0.9, built in float64: int16 by rint(z * 32768)
    with clipping and the extreme values planted at a block's first and last pairs; float32
    unquantised (times scale)."""
    rf_fs, be = oracle.MODES[mode][3], block_elems(mode)
    z = (rotated(synth(21, mode, n_blocks), rf_fs, OFFSETS[0], 0.45) +
         rotated(synth(22, mode, n_blocks), rf_fs, OFFSETS[1], 0.45))
    if fmt == S16:
        a = as_s16(z)
        b = be * (n_blocks - 1)  # the last block; (n_blocks 1: the only one)
        a[b: b + 2] = (-32768, 32767)
        a[b + be - 2: b + be] = (0, -32768)
        a[0:2] = (32767, 0)
    else:
        a = as_f32(z, scale)
    a.setflags(write=False)
    return a


def receiver(fm, fmt, mode=0, channels=None, **kw):
    rx = fm.Receiver(mode, fm.MONO if channels is None else channels, **kw)
    if fmt != U8:
        rx.set_input_format(fmt)
    assert rx.input_format == fmt
    return rx


def in_calls(fn, raw, be, calls):
    """fn over consecutive calls of `calls` blocks each, concatenated along the last axis."""
    out, b = [], 0
    for nb in calls:
        out.append(fn(raw[..., b * be:(b + nb) * be]))
        b += nb
    return np.concatenate(out, axis=-1)


def position(rx):
    return rx.tuner_info()[1]


def demod_and_pcm(fm, fmt, raw, mode, rf_taps, offset, calls):
    be = block_elems(mode)
    with receiver(fm, fmt, mode, rf_taps=rf_taps) as rx:
        rx.tune(offset)
        demod = in_calls(rx.rf_block, raw, be, calls)
        assert position(rx) == sum(calls) * be // 2
    with receiver(fm, fmt, mode, rf_taps=rf_taps) as rx:
        rx.tune(offset)
        pcm = in_calls(rx.process, raw, be, calls)
        assert position(rx) == sum(calls) * be // 2
    return demod, pcm


# ---- 1. identity: a u8 capture carried into the other formats ---------------------------------------

@functools.lru_cache(maxsize=None)
def u8_tuned(rf_taps, offset):
    return demod_and_pcm(iqgen.load_fmrx(), U8, synth(5, 0, 4), 0, rf_taps, offset, [1, 3])


@pytest.mark.parametrize("offset", [0, 300000])
@pytest.mark.parametrize("rf_taps", [51, 101])
@pytest.mark.parametrize("fmt", [S8, S16, F32], ids=NAMES.get)
def test_identity_mode0(fmrx, fmt, rf_taps, offset):
    raw = mapped(5, 0, 4, fmt)
    want = compose(raw, fmt, 0, rf_taps, offset)
    demod, pcm = demod_and_pcm(fmrx, fmt, raw, 0, rf_taps, offset, [1, 3])
    assert same(demod, want["demod"]) and np.array_equal(pcm, want["pcm_mono"])
    u8_demod, u8_pcm = u8_tuned(rf_taps, offset)
    assert same(demod, u8_demod) and np.array_equal(pcm, u8_pcm)


@pytest.mark.parametrize("mode,fmt,rf_taps,offset,blocks", [(1, S16, 51, 200000, 4), (2, F32, 51, -400000, 1),
                                                            (3, S8, 101, 96000, 1)],
                         ids=["mode1-s16", "mode2-f32", "mode3-s8"])
def test_identity_other_modes(fmrx, mode, fmt, rf_taps, offset, blocks):
    calls = [1, 3] if blocks == 4 else [blocks]
    raw = mapped(6 + mode, mode, blocks, fmt)
    want = compose(raw, fmt, mode, rf_taps, offset)
    demod, pcm = demod_and_pcm(fmrx, fmt, raw, mode, rf_taps, offset, calls)
    assert same(demod, want["demod"]) and np.array_equal(pcm, want["pcm_mono"])
    u8_demod, u8_pcm = demod_and_pcm(fmrx, U8, synth(6 + mode, mode, blocks), mode, rf_taps, offset, calls)
    assert same(demod, u8_demod) and np.array_equal(pcm, u8_pcm)


# ---- 2. real 16-bit and float data ---------------------------------------------------------------------

@pytest.mark.parametrize("mode,fmt,scale", [(0, S16, 1.0), (2, S16, 1.0), (0, F32, 1.0), (2, F32, 1.0),
                                            (0, F32, 2.0 ** -12)],
                         ids=["mode0-s16", "mode2-s16", "mode0-f32", "mode2-f32", "mode0-f32-2^-12"])
def test_real_data_matches_oracle(fmrx, mode, fmt, scale):
    blocks = 4 if mode == 0 else 1
    calls = [1, 3] if mode == 0 else [1]
    raw = real_capture(mode, blocks, fmt, scale)
    if fmt == S16:  # the planted extremes are there
        assert raw.min() == -32768 and raw.max() == 32767
    else:
        nz = np.abs(raw[raw != 0])
        assert nz.min() >= 2.0 ** -20 and nz.max() <= 4.0
    want = compose(raw, fmt, mode, 51, OFFSETS[1])
    demod, pcm = demod_and_pcm(fmrx, fmt, raw, mode, 51, OFFSETS[1], calls)
    assert same(demod, want["demod"])
    assert np.array_equal(pcm, want["pcm_mono"]) and pcm.any()


# ---- 3. seams --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [S16, F32], ids=NAMES.get)
def test_call_seams(fmrx, fmt):
    be, pairs = block_elems(0), block_elems(0) // 2
    raw = real_capture(0, 6, fmt)
    with receiver(fmrx, fmt, rf_taps=101) as rx:
        rx.tune(OFFSETS[0])
        whole = rx.process(raw)
        assert position(rx) == 6 * pairs
    with receiver(fmrx, fmt, rf_taps=101) as rx:
        rx.tune(OFFSETS[0])
        parts, b = [], 0
        for nb in (1, 3, 2):
            parts.append(rx.process(raw[b * be:(b + nb) * be]))
            b += nb
            assert position(rx) == b * pairs  # the position counts pairs, not bytes
    assert np.array_equal(np.concatenate(parts), whole) and whole.any()


# ---- 4. one capture, several stations ----------------------------------------------------------------------

def test_shared_capture_s16(fmrx):
    be = block_elems(0)
    offsets = [-300000, 0, 300000]
    raw = real_capture(0, 4, S16)
    want = np.stack([compose(raw, S16, 0, 51, f)["pcm_mono"] for f in offsets])
    with receiver(fmrx, S16, n_streams=3) as rx:
        rx.tune(offsets)
        got = in_calls(rx.process_shared, raw, be, [1, 3])
        assert rx.tuner_info() == (offsets, 4 * be // 2, True)
    assert np.array_equal(got, want)
    assert not np.array_equal(got[0], got[2])


def test_stereo_s16(fmrx):
    be, rf_fs = block_elems(0), oracle.MODES[0][3]
    raw = as_s16(rotated(synth(13, 0, 4), rf_fs, 200000, 0.9))  # the pilot is real, 200 kHz up
    want = compose(raw, S16, 0, 51, 200000, fields=("pcm",))["pcm"]
    with receiver(fmrx, S16, channels=fmrx.STEREO) as rx:
        rx.tune(200000)
        pcm = in_calls(rx.process, raw, be, [1, 3])
    assert np.array_equal(pcm, want) and pcm.any()


# ---- 5. time shard -----------------------------------------------------------------------------------------

def test_time_shard_s16(fmrx):
    be, na = block_elems(0), oracle.MODES[0][2]
    raw = real_capture(0, 6, S16)
    with receiver(fmrx, S16) as rx:
        rx.tune(OFFSETS[1])
        whole = rx.process(raw)
        hist = rx.history_bytes()
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        assert hist == 2 * rx.history_bytes()  # the same pairs, twice the bytes a pair
    assert hist % 4 == 0 and hist // 2 <= 3 * be
    with receiver(fmrx, S16) as rx:
        rx.tune(OFFSETS[1], first_pair=3 * be // 2)
        rx.seek(raw[3 * be - hist // 2: 3 * be])  # history_bytes() bytes = hist / 2 int16
        shard = rx.process(raw[3 * be:])
        assert position(rx) == 6 * be // 2
        with pytest.raises(fmrx.FmrxError) as e:  # 2 * 1001 bytes: no whole number of 4-byte pairs
            rx.seek(raw[:1001])
        assert e.value.code == fmrx.FMRX_EINVAL
    assert np.array_equal(shard, whole[3 * na:])


# ---- 6. state ------------------------------------------------------------------------------------------------

def state_size(rx):
    return len(rx.get_state())


def test_state_round_trip_and_format_check(fmrx):
    be = block_elems(0)
    raw = real_capture(0, 4, F32)
    with receiver(fmrx, F32) as rx:
        rx.tune(OFFSETS[0])
        whole = in_calls(rx.process, raw, be, [1, 3])
    with receiver(fmrx, F32) as rx:
        rx.tune(OFFSETS[0])
        head = rx.process(raw[:be])
        blob, (off, pos, on) = rx.get_state(), rx.tuner_info()
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        u8_blob = rx.get_state()
    assert len(blob) != len(u8_blob)  # the halo is raw bytes: 8 a pair against 2
    with receiver(fmrx, F32) as rx:
        rx.set_state(blob)
        rx.tune(off, first_pair=pos)
        tail = rx.process(raw[be:])
    assert np.array_equal(np.concatenate([head, tail]), whole)
    assert np.array_equal(whole, compose(raw, F32, 0, 51, OFFSETS[0])["pcm_mono"])
    for fmt in (S16, S8):  # s8: the same size as u8, told apart by the header's format word
        with receiver(fmrx, fmt) as rx:
            padded = u8_blob + bytes(max(0, state_size(rx) - len(u8_blob)))
            with pytest.raises(fmrx.FmrxError) as e:
                rx.set_state(padded)
            assert e.value.code == fmrx.FMRX_ESTATE
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        with pytest.raises(fmrx.FmrxError) as e:
            rx.set_state(blob)
        assert e.value.code == fmrx.FMRX_ESTATE


# ---- 7. switching formats ------------------------------------------------------------------------------------

def test_set_input_format_resets(fmrx):
    u8, s16 = synth(14, 0, 3), mapped(15, 0, 3, S16)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        want_u8 = rx.process(u8)
    with receiver(fmrx, S16) as rx:
        rx.tune(300000)
        want_s16 = rx.process(s16)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        assert rx.input_format == U8
        assert np.array_equal(rx.process(u8), want_u8)
        rx.set_input_format(S16)
        assert rx.input_format == S16 and rx.tuner_info() == ([0], 0, False)
        rx.tune(300000)
        assert np.array_equal(rx.process(s16), want_s16)
        rx.set_input_format(S16)  # the same format again: a reset; the offsets stay
        assert rx.tuner_info() == ([300000], 0, True)
        assert np.array_equal(rx.process(s16), want_s16)
        rx.set_input_format(U8)
        rx.tune(None)
        assert np.array_equal(rx.process(u8), want_u8)  # back on the untuned kernels


@pytest.mark.parametrize("fmt", [S8, S16, F32], ids=NAMES.get)
def test_tuning_off_is_offset_zero(fmrx, fmt):
    """No untuned kernel reads these formats: tuning off (never tuned, or fmrx_tune(NULL)) runs the
    tuned front end at offset 0, whose bits are the untuned u8 receiver's on the same samples."""
    be = block_elems(0)
    with fmrx.Receiver(0, fmrx.MONO, rf_taps=101) as rx:
        want = in_calls(rx.process, synth(16, 0, 4), be, [1, 3])
    raw = mapped(16, 0, 4, fmt)
    with receiver(fmrx, fmt, rf_taps=101) as rx:
        got = in_calls(rx.process, raw, be, [1, 3])
        assert rx.tuner_info() == ([0], 4 * be // 2, False)
        rx.tune(300000)
        assert not np.array_equal(rx.process(raw), want)
        rx.reset()
        rx.tune(None)
        again = in_calls(rx.process, raw, be, [1, 3])
    assert np.array_equal(got, want) and np.array_equal(again, want)


# ---- 8. errors -------------------------------------------------------------------------------------------------

def test_refused_calls(fmrx):
    be, na = block_elems(0), oracle.MODES[0][2]
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        for bad in (-1, 4, 17):
            with pytest.raises(fmrx.FmrxError) as e:
                rx.set_input_format(bad)
            assert e.value.code == fmrx.FMRX_EINVAL and rx.input_format == U8
        with pytest.raises(fmrx.FmrxError) as e:  # a u8 context takes no int16 array
            rx.process(mapped(16, 0, 4, S16))
        assert e.value.code == fmrx.FMRX_EINVAL
    for fmt in (S16, F32):
        raw = mapped(16, 0, 4, fmt)
        d_iq = torch.from_numpy(np.array(raw)).cuda()
        d_pcm = torch.zeros(2 * na, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        with receiver(fmrx, fmt, n_streams=2) as rx:
            for call in (rx.process_device, rx.process_shared_device):
                if call == rx.process_shared_device:
                    rx.tune([0, 300000])
                with pytest.raises(fmrx.FmrxError) as e:  # one element off: half a pair
                    call(d_iq.data_ptr() + raw.itemsize, 1, d_pcm.data_ptr())
                assert e.value.code == fmrx.FMRX_EINVAL
                with pytest.raises(fmrx.FmrxError) as e:  # one pair off: half a staging unit
                    call(d_iq.data_ptr() + 2 * raw.itemsize, 1, d_pcm.data_ptr())
                assert e.value.code == fmrx.FMRX_EINVAL
            d_p = torch.zeros(256, dtype=torch.float32, device="cuda")
            with pytest.raises(fmrx.FmrxError) as e:
                rx.scan_spectrum_device(d_iq.data_ptr() + raw.itemsize, 1024, 256, d_p.data_ptr())
            assert e.value.code == fmrx.FMRX_EINVAL
            rx.synchronize()
            assert position(rx) == 0
        assert not d_pcm.cpu().numpy().any() and not d_p.cpu().numpy().any()  # no launch
    with receiver(fmrx, S16, n_streams=2) as rx:
        for wrong in (synth(16, 0, 4), mapped(16, 0, 4, F32), mapped(16, 0, 4, S8)):
            for fn in (rx.process, rx.rf_block, rx.process_shared, rx.seek, rx.scan, rx.scan_spectrum):
                with pytest.raises(fmrx.FmrxError) as e:
                    fn(wrong)
                assert e.value.code == fmrx.FMRX_EINVAL
        with pytest.raises(fmrx.FmrxError) as e:  # shared calls still need an explicit tune
            rx.process_shared(mapped(16, 0, 4, S16)[:be])
        assert e.value.code == fmrx.FMRX_ESTATE


# ---- 9. scan ---------------------------------------------------------------------------------------------------

def welch64(raw, fmt, n):
    """fmrx.h's power spectrum in float64 on the format's normalised samples (FFT-shifted)."""
    x = normalise(raw, fmt).astype(np.float64)
    z = x[0::2] + 1j * x[1::2]
    nseg = z.size // n
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)
    f = np.fft.fft(z[: nseg * n].reshape(nseg, n) * w, axis=1)
    return np.fft.fftshift(8.0 / (3.0 * n * n * nseg) * (np.abs(f) ** 2).sum(axis=0))


def device_spectrum(rx, d_iq_ptr, n_pairs, n):
    d_p = torch.zeros(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rx.scan_spectrum_device(d_iq_ptr, n_pairs, n, d_p.data_ptr())
    rx.synchronize()
    return d_p.cpu().numpy()


@pytest.mark.parametrize("n", [256, 4096, 8192])
def test_scan_identity_is_bit_identical(fmrx, n):
    """Only powers of two differ between the formats' samples, so no product or sum may round
    differently: the spectrum of an identity-mapped capture is u8's, bit for bit."""
    u8 = synth(5, 0, 4)  # 25600 pairs: 100, 6 and 3 segments
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        want, nseg = rx.scan_spectrum(u8, n)
    assert want.any()
    for fmt in (S8, S16, F32):
        with receiver(fmrx, fmt) as rx:
            got, got_seg = rx.scan_spectrum(mapped(5, 0, 4, fmt), n)
        assert got_seg == nseg and same(got, want), NAMES[fmt]


@pytest.mark.parametrize("fmt", [S16, F32], ids=NAMES.get)
def test_scan_real_data_against_float64(fmrx, fmt):
    rng = np.random.default_rng(7)
    clean = real_capture(0, 8, fmt)  # 12 segments at 8192 bins
    noise = rng.normal(0.0, 2.0 ** -8, clean.size)  # sigma 2^-8 of full scale on both rails
    if fmt == S16:
        raw = np.clip(np.rint(clean.astype(np.float64) + noise * 32768.0), -32768, 32767).astype(np.int16)
    else:
        raw = (clean.astype(np.float64) + noise).astype(np.float32)
    with receiver(fmrx, fmt) as rx:
        for n in (256, 512, 1024, 2048, 4096, 8192):
            want = welch64(raw, fmt, n)
            assert want.min() >= 1e-6 * want.max()  # the input keeps every bin off float32's rounding floor
            got, _ = rx.scan_spectrum(raw, n)
            worst = float(np.max(np.abs(10.0 * np.log10(got.astype(np.float64)) - 10.0 * np.log10(want))))
            print(f"{NAMES[fmt]} bins={n}: worst bin {worst:.2e} dB")
            assert worst <= BIN_TOL_DB


@pytest.mark.parametrize("fmt", [U8, S8, S16, F32], ids=NAMES.get)
def test_scan_one_pair_into_a_buffer(fmrx, fmt):
    """d_iq one pair past a 16-byte boundary (2, 2, 4, 8 bytes), up to the buffer's last byte."""
    n = 256
    raw = mapped(5, 0, 4, fmt)[: 2 + 2 * 5 * n]  # one pair, then exactly five segments
    d_iq = torch.from_numpy(np.array(raw)).cuda()
    assert d_iq.data_ptr() % 16 == 0
    with receiver(fmrx, fmt) as rx:
        host, nseg = rx.scan_spectrum(raw[2:], n)
        dev = device_spectrum(rx, d_iq.data_ptr() + PAIR_BYTES[fmt], 5 * n, n)
    assert nseg == 5 and same(dev, host) and host.any()


def test_decode_stations_s16(fmrx):
    raw = real_capture(0, 8, S16)
    stations, pcm = fmrx.decode_stations(raw)
    assert [s.offset_hz for s in stations] == list(OFFSETS)
    for s, f in enumerate(OFFSETS):
        assert np.array_equal(pcm[s], compose(raw, S16, 0, 51, f)["pcm_mono"]), f
    with pytest.raises(ValueError):
        fmrx.decode_stations(raw.astype(np.int32))


# ---- 10. CLI -----------------------------------------------------------------------------------------------------

def cli(fm, args, data):
    exe = os.path.join(os.path.dirname(fm.LIB_PATH), "bin", "fmrx")
    return subprocess.run([exe] + args, input=data, capture_output=True, timeout=120)


def test_cli_s16_offset(fmrx):
    raw = real_capture(0, 4, S16)
    r = cli(fmrx, ["0", "1", "--mono-product", "--iq-format", "s16", "--offset-hz", str(OFFSETS[1])], raw.tobytes())
    assert r.returncode == 0, r.stderr
    with receiver(fmrx, S16) as rx:
        rx.tune(OFFSETS[1])
        want = rx.process(raw)
    assert np.array_equal(np.frombuffer(r.stdout, np.int16), want) and want.any()
    # no --offset-hz: the station at offset 0
    r0 = cli(fmrx, ["0", "1", "--mono-product", "--iq-format", "s16"], raw.tobytes())
    with receiver(fmrx, S16) as rx:
        want0 = rx.process(raw)
    assert r0.returncode == 0 and np.array_equal(np.frombuffer(r0.stdout, np.int16), want0)
    bad = cli(fmrx, ["0", "1", "--iq-format", "s12"], b"")
    assert bad.returncode == 1 and b"iq-format" in bad.stderr


def test_cli_scan_f32(fmrx):
    raw = real_capture(0, 4, F32)
    with receiver(fmrx, F32) as rx:
        want = rx.scan(raw)
        want_half = rx.scan(raw[: raw.size // 2])
    assert [s.offset_hz for s in want] == list(OFFSETS)
    lines = [f"{s.offset_hz} {s.power_db:.2f} {s.snr_db:.2f}" for s in want]
    r = cli(fmrx, ["0", "1", "--scan", "--iq-format", "f32"], raw.tobytes())
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode().splitlines() == lines
    # --scan-bytes counts bytes of the format
    r2 = cli(fmrx, ["0", "1", "--scan", "--iq-format", "f32", "--scan-bytes", str(raw.nbytes // 2)], raw.tobytes())
    assert r2.returncode == 0
    assert r2.stdout.decode().splitlines() == [f"{s.offset_hz} {s.power_db:.2f} {s.snr_db:.2f}" for s in want_half]


def test_cli_without_the_flag_is_u8(fmrx):
    iq = synth(17, 0, 4)
    r = cli(fmrx, ["0", "1", "--mono-product"], iq.tobytes())
    assert r.returncode == 0, r.stderr
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        want = rx.process(iq)
    assert np.array_equal(np.frombuffer(r.stdout, np.int16), want)
    r8 = cli(fmrx, ["0", "1", "--mono-product", "--iq-format", "u8"], iq.tobytes())
    assert r8.returncode == 0 and r8.stdout == r.stdout
