"""The subcarrier meter on the GPU: every power it writes is compared for equality of the
float bits with meter_ref.py, the numpy restatement, run with the library's own tables; the switch, the
routing in decode_stations and the CLI flag are checked against the calls they stand for."""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

import iqgen
import oracle
import meter_ref as M
import rds_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()  # before the library's first HIP call, as the other device-pointer tests do

FRAME_PAIRS = 24 * 6400  # mode 0: an RDS granule of 24 blocks is one 64 ms frame
# capture 5: three stations at raster offsets -- pilot + L-R + RDS, pilot + L-R, mono audio alone
STATIONS = [(-600000, dict(pilot=0.05, lr=0.10, rds=0.04, audio_hz=1000.0)),
            (100000, dict(pilot=0.05, lr=0.10, rds=0.0, audio_hz=2000.0)),
            (700000, dict(pilot=0.0, lr=0.0, rds=0.0, audio_hz=3000.0))]
PI, PS = 0x4D54, "METER FM"
FLAGS = [(1, 1), (1, 0), (0, 0)]
CAPTURE_FRAMES = 20  # 1.28 s: more than the 16 frames decode_stations probes
_cache = {}


def tables(fmrx, mode):
    if ("tab", mode) not in _cache:
        _cache["tab", mode] = fmrx.meter_design(R.bp_fs(mode))[1]
    return _cache["tab", mode]


def bits_eq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def rows(mode, granules):
    """Three streams of different content, whole frames: the multiplex, wild floats, silence."""
    key = ("rows", mode, granules)
    if key not in _cache:
        n = granules * R.granule_samples(mode)
        t = np.arange(n, dtype=np.float64) / R.bp_fs(mode)
        mpx = M.multiplex(t, bits=M.station_bits(PI, PS, n / R.bp_fs(mode)), lr=0.1).astype(np.float32)
        wild = ((np.frombuffer(iqgen.rand_bytes(11 + mode, 4 * n).tobytes(), np.uint32) / 2.0 ** 32) * 3.0 - 1.5).astype(np.float32)
        wild[::97] *= np.float32(40.0)
        _cache[key] = np.stack([mpx, wild, np.zeros(n, np.float32)])
    return _cache[key]


def want_power(fmrx, mode, x):
    return np.stack([M.power(r, tables(fmrx, mode)) for r in x])


def station_iq(frames, rf_fs=None, only=None):
    """The sum of capture 5's stations (or station `only` at offset 0) as complex samples."""
    key = ("iq", frames, rf_fs, only)
    if key not in _cache:
        fs = rf_fs or oracle.MODES[0][3]
        n = frames * FRAME_PAIRS * (fs // oracle.MODES[0][3])
        bits = M.station_bits(PI, PS, frames * 0.064)
        pick = [(0, STATIONS[only][1])] if only is not None else STATIONS
        _cache[key] = sum(M.fm_signal(0, n, offset_hz=off, rf_fs=rf_fs, bits=bits, seed=k + 1, **kw)
                          for k, (off, kw) in enumerate(pick))
    return _cache[key]


def capture5(frames=CAPTURE_FRAMES):
    if ("u8", frames) not in _cache:
        _cache["u8", frames] = R.to_u8(station_iq(frames), amp=38.0, noise_lsb=2.0)
    return _cache["u8", frames]


def flags_of(fmrx, rx, n):
    return [(lv["stereo"], lv["rds"]) for lv in (fmrx.meter_detect(rx.meter_report(k)) for k in range(n))]


# ---- 1. the primitive ---------------------------------------------------------------------------

@pytest.mark.parametrize("granules", [1, 2])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_primitive_equals_the_restatement(fmrx, mode, granules):
    x = rows(mode, granules)
    want = want_power(fmrx, mode, x)
    with fmrx.Receiver(mode, fmrx.MONO, n_streams=3) as rx:
        assert rx.rds_granule == R.GRANULES[mode]
        got = rx.meter(x)
    assert got.shape == (3, x.shape[1] // M.frame_samples(mode), 7)
    assert bits_eq(got, want)
    assert np.all(got[2] == 0) and np.all(got[0, :, 1] > 10 * got[0, :, 0])  # silence; the pilot over its guard bin


def test_nan_stays_in_its_frame(fmrx):
    x = rows(0, 2).copy()
    x[1, M.frame_samples(0) + 4321] = np.nan
    want = want_power(fmrx, 0, x)
    with fmrx.Receiver(0, fmrx.MONO, n_streams=3) as rx:
        got = rx.meter(x)
    assert np.all(np.isnan(want[1, 1])) and not np.any(np.isnan(want[1, 0]))
    assert np.array_equal(np.isnan(got), np.isnan(want))
    keep = ~np.isnan(want)
    assert bits_eq(got[keep], want[keep])


def test_device_form_equals_the_host_form(fmrx):
    x = rows(0, 2)
    with fmrx.Receiver(0, fmrx.MONO, n_streams=3) as rx:
        host = rx.meter(x)
        d_x = torch.from_numpy(x).cuda()
        d_p = torch.full((3, 2, 7), -7.0, dtype=torch.float32, device="cuda")
        rx.meter_device(d_x.data_ptr(), 48, d_p.data_ptr())
        rx.synchronize()
        assert bits_eq(d_p.cpu().numpy(), host)


# ---- 2. refusal -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n_blocks", [23, 25])
def test_part_frames_are_refused_and_nothing_is_written(fmrx, n_blocks):
    x = np.ones(n_blocks * 640, np.float32)
    out = np.full((2, 7), -7.0, np.float32)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        assert fmrx.lib().fmrx_meter(rx.h, x.ctypes.data, n_blocks, out.ctypes.data) == fmrx.FMRX_EINVAL
        d_x = torch.from_numpy(x).cuda()
        d_p = torch.full((2, 7), -7.0, dtype=torch.float32, device="cuda")
        with pytest.raises(fmrx.FmrxError) as e:
            rx.meter_device(d_x.data_ptr(), n_blocks, d_p.data_ptr())
        assert e.value.code == fmrx.FMRX_EINVAL and "frames" in str(e.value)
        rx.synchronize()
        assert np.all(out == -7.0) and bool(torch.all(d_p == -7.0))
        rx.tune([0])
        rx.set_meter(True)
        with pytest.raises(fmrx.FmrxError) as e:
            rx.process(np.full(n_blocks * 12800, 128, np.uint8))
        assert e.value.code == fmrx.FMRX_EINVAL
        assert rx.meter_report().frames == 0


# ---- 3. / 4. the switch ---------------------------------------------------------------------------

def tuned_iq():
    if "tuned" not in _cache:
        _cache["tuned"] = R.to_u8(station_iq(2, only=0))
    return _cache["tuned"]


@pytest.mark.parametrize("channels", ["MONO", "STEREO"])
def test_switch_reports_the_oracle_demod_and_leaves_the_pcm(fmrx, orc, channels):
    iq = tuned_iq()
    pw = M.power(orc.run(0, 51, iq, ["demod"])["demod"], tables(fmrx, 0))
    sums, frames = M.accumulate(pw)
    assert frames == 2 and M.detect(sums, frames)["stereo"] == 1
    with fmrx.Receiver(0, getattr(fmrx, channels)) as rx:
        rx.tune([0])
        off = rx.process(iq)
        assert rx.meter_report().frames == 0  # off: nothing measured
        rx.reset()
        rx.set_meter(True)
        on = rx.process(iq)
        rep = rx.meter_report()
        assert rep.frames == 2 and bits_eq(np.array(rep.sum), sums)
        assert fmrx.meter_detect(rep) == M.detect(sums, frames)
        rx.reset()  # clears the report, keeps the switch
        assert rx.meter_report().frames == 0 and not any(rx.meter_report().sum)
        half = iq.size // 2
        parts = np.concatenate([rx.process(iq[:half]), rx.process(iq[half:])])
        rep = rx.meter_report()
        assert rep.frames == 2 and bits_eq(np.array(rep.sum), sums)
    assert np.array_equal(on, off) and np.array_equal(parts, off)


def test_switch_beside_rds_and_deemphasis(fmrx):
    iq = tuned_iq()
    with fmrx.Receiver(0, fmrx.STEREO) as rx:
        rx.tune([0])
        rx.set_rds(True)
        rx.set_deemphasis(50)
        off, info = rx.process(iq), rx.rds_info().as_dict()
        rx.reset()
        rx.set_meter(True)
        on = rx.process(iq)
        assert rx.rds_info().as_dict() == info and info["bits"] == 2 * 76
        assert rx.meter_report().frames == 2
    assert np.array_equal(on, off)


# ---- 5. / 6. three stations in one capture ----------------------------------------------------------

def test_shared_capture_flags(fmrx):
    iq = capture5()
    with fmrx.Receiver(0, fmrx.MONO, n_streams=3) as rx:
        rx.tune([s[0] for s in STATIONS])
        off = rx.process_shared(iq)
        rx.reset()
        rx.set_meter(True)
        on = rx.process_shared(iq)
        assert flags_of(fmrx, rx, 3) == FLAGS
        assert [rx.meter_report(k).frames for k in range(3)] == [CAPTURE_FRAMES] * 3
    assert np.array_equal(on, off)


def test_wide_capture_flags(fmrx):
    """The same three stations in a capture at 4 x the mode's rate, s16, two frames."""
    iq = R.to_s16(station_iq(2, rf_fs=4 * oracle.MODES[0][3]), amp=4000.0, noise_lsb=100.0)
    with fmrx.Receiver(0, fmrx.MONO, n_streams=3) as rx:
        rx.set_input_format(fmrx.IQ_S16)
        rx.set_capture_decim(4)
        rx.tune_wide([s[0] for s in STATIONS])
        off = rx.process_wide(iq)
        rx.reset()
        rx.set_meter(True)
        on = rx.process_wide(iq)
        assert flags_of(fmrx, rx, 3) == FLAGS
    assert np.array_equal(on, off)


# ---- 7. routing -------------------------------------------------------------------------------------

def test_decode_stations_probe(fmrx):
    iq = capture5()
    offs = [s[0] for s in STATIONS]
    stations, pcm, infos, levels = fmrx.decode_stations(iq, channels=fmrx.STEREO, rds=True, probe=True)
    assert [s.offset_hz for s in stations] == offs
    assert [(lv["stereo"], lv["rds"]) for lv in levels] == FLAGS
    with fmrx.Receiver(0, fmrx.STEREO, n_streams=2) as rx:  # the two piloted stations, decoded together
        rx.tune(offs[:2])
        rx.set_rds(True)
        both, info = rx.process_shared(iq), rx.rds_info(0).as_dict()
    with fmrx.Receiver(0, fmrx.MONO, n_streams=1) as rx:
        rx.tune(offs[2:])
        mono = rx.process_shared(iq)
    assert pcm.shape == (3, both.shape[1]) and np.array_equal(pcm[:2], both)
    assert np.array_equal(pcm[2], np.repeat(mono, 2))
    assert infos == [info, None, None] and (info["pi"], info["ps"]) == (PI, PS)
    # probe=False: exactly what a direct process_shared returns
    with fmrx.Receiver(0, fmrx.STEREO, n_streams=3) as rx:
        rx.tune(offs)
        rx.set_rds(True)
        direct = rx.process_shared(iq)
        named = [rx.rds_info(k).as_dict() for k in range(3)]
    plain = fmrx.decode_stations(iq, channels=fmrx.STEREO, rds=True)
    assert len(plain) == 3 and [s.offset_hz for s in plain[0]] == offs
    assert np.array_equal(plain[1], direct) and plain[2] == named


# ---- 8. the CLI -------------------------------------------------------------------------------------

def test_cli_meter_line(fmrx):
    iq = capture5()
    exe = os.path.join(os.path.dirname(fmrx.LIB_PATH), "bin", "fmrx")
    data = iq.tobytes() + bytes([128]) * (5 * 12800)  # five blocks past the last whole frame
    args = [exe, "0", "1", "--offset-hz", str(STATIONS[0][0])]
    plain = subprocess.run(args, input=data, capture_output=True, timeout=120)
    r = subprocess.run(args + ["--meter"], input=data, capture_output=True, timeout=120)
    assert r.returncode == 0 and plain.returncode == 0, r.stderr.decode()
    lines = [x for x in r.stderr.decode().splitlines() if x.startswith("meter ")]
    assert len(lines) == 1, r.stderr.decode()
    m = re.fullmatch(r"meter pilot_snr=(-?\d+\.\d) stereo=(\d) rds_snr=(-?\d+\.\d) rds=(\d) frames=(\d+)", lines[0])
    assert m, lines[0]
    assert (m.group(2), m.group(4), int(m.group(5))) == ("1", "1", CAPTURE_FRAMES)
    assert r.stdout == plain.stdout and len(r.stdout) == (CAPTURE_FRAMES * 24 + 5) * 128 * 2 * 2
    assert b"meter " not in plain.stderr
