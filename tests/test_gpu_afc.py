"""AFC on the GPU: every carrier sum the kernel writes is compared for equality of the float
bits with afc_ref.py, the numpy restatement; the switch leaves the PCM alone; tracking is compared, bit for
bit, with a second context that the test retunes by hand; and the rule lands on stations off their raster."""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

import afc_ref as A
import iqgen
import oracle
import meter_ref as M
import rds_ref as R
from afc_ref import SCAN, shifted_capture5, tracking_capture

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()  # before the library's first HIP call, as the other device-pointer tests do


PI, PS = 0x4D54, "METER FM"
_cache = {}


def bits_eq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def rows(mode, granules):
    """Three streams of different content, whole frames, as test_gpu_meter builds them: the multiplex, wild
    floats with outliers, silence."""
    key = ("rows", mode, granules)
    if key not in _cache:
        n = granules * R.granule_samples(mode)
        t = np.arange(n, dtype=np.float64) / R.bp_fs(mode)
        mpx = M.multiplex(t, bits=M.station_bits(PI, PS, n / R.bp_fs(mode)), lr=0.1).astype(np.float32)
        wild = ((np.frombuffer(iqgen.rand_bytes(11 + mode, 4 * n).tobytes(), np.uint32) / 2.0 ** 32) * 3.0 - 1.5).astype(np.float32)
        wild[::97] *= np.float32(40.0)
        _cache[key] = np.stack([mpx, wild, np.zeros(n, np.float32)])
    return _cache[key]


def want_sums(mode, x):
    return np.stack([A.sums(r, M.window(mode)) for r in x])


def status(rx, k=0):
    st = rx.afc_status(k)
    return {"sum": st.total.sum, "sumsq": st.total.sumsq, "frames": st.total.frames, "origin_hz": st.origin_hz,
            "offset_hz": st.offset_hz, "retunes": st.retunes, "refused": st.refused, "decisions": st.decisions,
            "last": st.last.as_dict()}


# ---- 1. the primitive ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode,granules", [(0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (3, 1)])
def test_primitive_equals_the_restatement(fmrx, mode, granules):
    x = rows(mode, granules)
    want = want_sums(mode, x)
    with fmrx.Receiver(mode, fmrx.MONO, n_streams=3) as rx:
        got = rx.carrier(x)
    assert got.shape == (3, x.shape[1] // M.frame_samples(mode), 2)
    assert bits_eq(got, want)
    assert np.all(got[2] == 0) and np.all(got[:2, :, 1] > 0)  # silence; a sum of squares


def test_five_frames_of_one_stream(fmrx):
    x = rows(0, 5)[1]
    want = A.sums(x, 240)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        got = rx.carrier(x)
    assert got.shape == (5, 2) and bits_eq(got, want)
    assert len({r.tobytes() for r in got}) == 5  # every frame its own


# ---- 2. special values ----------------------------------------------------------------------------

def test_nan_and_inf_stay_in_their_frame(fmrx):
    x = rows(0, 2).copy()
    clean = want_sums(0, x)
    x[1, M.frame_samples(0) + 4321] = np.nan
    x[0, 77] = np.inf
    want = want_sums(0, x)
    with fmrx.Receiver(0, fmrx.MONO, n_streams=3) as rx:
        got = rx.carrier(x)
    assert np.all(np.isnan(want[1, 1])) and np.all(np.isinf(want[0, 0])) and np.all(want[0, 0] > 0)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    keep = ~np.isnan(want)
    assert bits_eq(got[keep], want[keep])
    untouched = np.ones(got.shape, bool)
    untouched[1, 1] = untouched[0, 0] = False
    assert bits_eq(got[untouched], clean[untouched])  # that frame's two floats only


# ---- 3. the device form -----------------------------------------------------------------------------

def test_device_form_equals_the_host_form(fmrx):
    x = rows(0, 2)
    with fmrx.Receiver(0, fmrx.MONO, n_streams=3) as rx:
        host = rx.carrier(x)
        d_x = torch.from_numpy(x).cuda()
        d_s = torch.full((3, 2, 2), -7.0, dtype=torch.float32, device="cuda")
        rx.carrier_device(d_x.data_ptr(), 48, d_s.data_ptr())
        rx.synchronize()
        assert bits_eq(d_s.cpu().numpy(), host)


# ---- 4. refusals ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_blocks", [23, 25])
def test_part_frames_are_refused_and_nothing_is_written(fmrx, n_blocks):
    x = np.ones(n_blocks * 640, np.float32)
    out = np.full((2, 2), -7.0, np.float32)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        assert fmrx.lib().fmrx_carrier(rx.h, x.ctypes.data, n_blocks, out.ctypes.data) == fmrx.FMRX_EINVAL
        d_x = torch.from_numpy(x).cuda()
        d_s = torch.full((2, 2), -7.0, dtype=torch.float32, device="cuda")
        with pytest.raises(fmrx.FmrxError) as e:
            rx.carrier_device(d_x.data_ptr(), n_blocks, d_s.data_ptr())
        assert e.value.code == fmrx.FMRX_EINVAL and "frames" in str(e.value)
        rx.synchronize()
        assert np.all(out == -7.0) and bool(torch.all(d_s == -7.0))
        rx.tune([0])
        rx.set_afc(True)
        with pytest.raises(fmrx.FmrxError) as e:
            rx.process(np.full(n_blocks * 12800, 128, np.uint8))
        assert e.value.code == fmrx.FMRX_EINVAL
        assert status(rx)["frames"] == 0
        for kw in (dict(step_hz=0), dict(frames=0), dict(max_mean_square=float("nan"))):
            with pytest.raises(fmrx.FmrxError) as e:
                rx.set_afc(True, **kw)
            assert e.value.code == fmrx.FMRX_EINVAL


# ---- 5. the switch, measuring only --------------------------------------------------------------------

def tuned_iq():
    """Two frames of capture 5's first station at the capture's centre (test_gpu_meter's input)."""
    if "tuned" not in _cache:
        _cache["tuned"] = R.to_u8(A.stations_iq(2, offsets=[0], kws=[dict(pilot=0.05, lr=0.10, rds=0.04, audio_hz=1000.0)]))
    return _cache["tuned"]


@pytest.mark.parametrize("channels", ["MONO", "STEREO"])
def test_switch_reports_the_oracle_demod_and_leaves_the_pcm(fmrx, orc, channels):
    iq = tuned_iq()
    want = A.report_of(orc.run(0, 51, iq, ["demod"])["demod"], 240)
    with fmrx.Receiver(0, getattr(fmrx, channels)) as rx:
        rx.tune([0])
        off = rx.process(iq)
        assert status(rx)["frames"] == 0  # off: nothing measured
        rx.reset()
        rx.set_afc(True, track=0)
        on = rx.process(iq)
        st = rx.afc_status()
        assert st.total.frames == 2 and bits_eq(np.float64(st.total.sum), want[0]) and bits_eq(np.float64(st.total.sumsq), want[1])
        assert (st.retunes, st.decisions, st.offset_hz, st.origin_hz) == (0, 0, 0, 0)
        got, ref = fmrx.afc_decide(st.total, 240000), A.decide(want, 240000)
        assert got["correction_hz"] == ref["correction_hz"] == 0 and got["carrier"] == ref["carrier"] == 1
        rx.reset()  # clears the report, keeps the switch
        assert status(rx)["frames"] == 0 and status(rx)["sum"] == 0.0
        half = iq.size // 2
        parts = np.concatenate([rx.process(iq[:half]), rx.process(iq[half:])])
        st = rx.afc_status()
        assert st.total.frames == 2 and bits_eq(np.float64(st.total.sum), want[0]) and bits_eq(np.float64(st.total.sumsq), want[1])
    assert np.array_equal(on, off) and np.array_equal(parts, off)


def test_switch_beside_meter_rds_deemphasis_and_blend(fmrx, orc):
    iq = tuned_iq()
    want = A.report_of(orc.run(0, 51, iq, ["demod"])["demod"], 240)
    with fmrx.Receiver(0, fmrx.STEREO) as rx:
        rx.tune([0])
        rx.set_rds(True)
        rx.set_deemphasis(50)
        rx.set_meter(True)
        rx.set_stereo_blend(True)
        off, info, meter, blend = rx.process(iq), rx.rds_info().as_dict(), rx.meter_report(), rx.blend_report()
        rx.reset()
        rx.set_afc(True, track=0)
        on = rx.process(iq)
        assert rx.rds_info().as_dict() == info and info["bits"] == 2 * 76
        assert bytes(rx.meter_report()) == bytes(meter) and meter.frames == 2 and rx.blend_report() == blend
        st = rx.afc_status()
        assert st.total.frames == 2 and bits_eq(np.float64(st.total.sum), want[0]) and bits_eq(np.float64(st.total.sumsq), want[1])
    assert np.array_equal(on, off)


# ---- 6. tracking is a retune and nothing else -----------------------------------------------------------

@pytest.mark.parametrize("kind", ["streams", "shared", "decim2", "rate"])
def test_tracking_equals_retuning_by_hand(fmrx, kind):
    wide = kind in ("decim2", "rate")
    iq = tracking_capture(kind if wide else "narrow")
    calls = np.split(iq, 4)
    tuned = A.TUNED[:2]

    def setup(rx):
        if kind == "decim2":
            rx.set_capture_decim(2)
        if kind == "rate":
            rx.set_capture_rate(10000000)
        (rx.tune_wide if wide else rx.tune)(tuned)

    def run(rx, part):
        if wide:
            return rx.process_wide(part)
        return rx.process(np.concatenate([part, part])) if kind == "streams" else rx.process_shared(part)

    with fmrx.Receiver(0, fmrx.MONO, n_streams=2) as a, fmrx.Receiver(0, fmrx.MONO, n_streams=2) as b:
        setup(a)
        setup(b)
        a.set_afc(True, frames=2)
        seen = []
        for part in calls:
            pa = run(a, part)
            pb = run(b, part)
            assert np.array_equal(pa, pb) and pa.any()
            offs = [a.afc_status(k).offset_hz for k in range(2)]
            seen.append(offs)
            info = (a.wide_info if wide else a.tuner_info)()
            assert info[0] == offs and info[2] is True
            pos = (b.wide_info if wide else b.tuner_info)()[1]
            assert pos == info[1]
            (b.tune_wide if wide else b.tune)(offs, pos)  # what A did to itself
        st = [status(a, k) for k in range(2)]
    print(kind, seen, [s["last"] for s in st])
    assert seen[0] != tuned, "the first decision moved nothing: the test shows nothing"
    for k in range(2):
        assert st[k]["origin_hz"] == tuned[k] and st[k]["decisions"] == 4 and st[k]["frames"] == 8 and st[k]["refused"] == 0
        assert abs(st[k]["offset_hz"] - A.TRUE[k]) <= 1000 and 1 <= st[k]["retunes"] <= 3


# ---- 7. it lands ----------------------------------------------------------------------------------------

def test_it_lands(fmrx):
    """The inputs of test_afc_host.test_the_reference_rule_lands_on_the_test_stations, which confirms the
    bounds on the float64 rule first."""
    iq = A.landing_capture(64)
    gates = []
    with fmrx.Receiver(0, fmrx.MONO, n_streams=4) as rx:
        rx.tune(A.TUNED)
        rx.set_afc(True)
        for part in np.split(iq, 4):
            rx.process_shared(part)
            gates.append([rx.afc_status(k).last.carrier for k in range(4)])
        st = [status(rx, k) for k in range(4)]
    for k in range(4):
        print(k, st[k]["offset_hz"], st[k]["retunes"], st[k]["last"])
    for k, true in enumerate(A.TRUE):
        assert abs(st[k]["offset_hz"] - true) <= 1000 and st[k]["retunes"] <= 3, (k, st[k])
        assert st[k]["decisions"] == 4 and st[k]["frames"] == 64 and st[k]["origin_hz"] == A.TUNED[k]
    assert [g[3] for g in gates] == [0] * 4 and all(g[:3] == [1, 1, 1] for g in gates)
    assert (st[3]["retunes"], st[3]["offset_hz"], st[3]["decisions"]) == (0, A.TUNED[3], 4)


# ---- 8. / 9. the clamp, the reset ------------------------------------------------------------------------

def far_capture():
    """6 frames of the mono station alone, 70 kHz above the capture's centre."""
    if "far" not in _cache:
        _cache["far"] = R.to_u8(A.stations_iq(6, offsets=[70000], kws=A.STATION_KW[2:]))
    return _cache["far"]


def test_the_pull_is_clamped(fmrx):
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        rx.tune([0])
        rx.set_afc(True, frames=2, max_pull_hz=50000)
        seen = []
        for part in np.split(far_capture(), 3):
            rx.process(part)
            seen.append(status(rx))
    # 70 kHz is past a quarter of the IF rate's turn, where the sine folds back: the first reading falls short of
    # 50 kHz, the second asks for more than is left and is cut at the bound
    offs = [s["offset_hz"] for s in seen]
    print(offs, [s["last"] for s in seen])
    assert 0 < offs[0] <= 50000 and offs[1:] == [50000, 50000]
    assert seen[2]["retunes"] == seen[1]["retunes"] <= 2  # at the bound nothing moves any more
    assert all(s["origin_hz"] == 0 and s["last"]["carrier"] == 1 and s["refused"] == 0 for s in seen)
    assert offs[0] + seen[1]["last"]["correction_hz"] > 50000 and seen[2]["last"]["correction_hz"] > 0  # it would go on


def test_reset_restores_the_origins_and_clears_the_reports(fmrx):
    parts = np.split(far_capture(), 3)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        rx.tune([20000])
        rx.set_afc(True, frames=2)
        first = rx.process(parts[0])
        assert status(rx)["offset_hz"] != 20000 and rx.tuner_info()[0] == [status(rx)["offset_hz"]]
        rx.reset()
        st = status(rx)
        assert (st["offset_hz"], st["origin_hz"], st["retunes"], st["decisions"], st["frames"], st["sum"], st["sumsq"]) == (
            20000, 20000, 0, 0, 0, 0.0, 0.0)
        assert st["last"] == fmrx.AfcDecision().as_dict() and rx.tuner_info() == ([20000], 0, True)
        assert np.array_equal(rx.process(parts[0]), first)  # the switch stayed on, the stream starts over
        assert status(rx)["retunes"] == 1
        rx.tune([30000])  # the caller's own tune: a new origin, the window cleared
        st = status(rx)
        assert (st["offset_hz"], st["origin_hz"]) == (30000, 30000)


# ---- 10. decode_stations ---------------------------------------------------------------------------------

def test_decode_stations_afc(fmrx):
    iq = shifted_capture5()
    plain = fmrx.decode_stations(iq)
    assert len(plain) == 2 and [s.offset_hz for s in plain[0]] == SCAN
    with fmrx.Receiver(0, fmrx.MONO, n_streams=3) as rx:  # afc=False: exactly what a direct process_shared returns
        rx.tune(SCAN)
        assert np.array_equal(plain[1], rx.process_shared(iq))
    stations, pcm, pulls = fmrx.decode_stations(iq, afc=True)
    offs = [s.offset_hz for s in stations]
    print(offs, pulls)
    assert all(abs(o - (f + 7000)) <= 1000 for o, f in zip(offs, SCAN))
    assert [p["pulled_hz"] for p in pulls] == [o - f for o, f in zip(offs, SCAN)] and all(p["carrier"] == 1 for p in pulls)
    assert all(abs(p["err_hz"]) < 1000 for p in pulls)  # the last pass moved nobody
    with fmrx.Receiver(0, fmrx.MONO, n_streams=3) as rx:
        rx.tune(offs)
        assert np.array_equal(pcm, rx.process_shared(iq))
    # beside the probe: its levels come with the last pass, the tail keeps its order
    st2, pcm2, levels, pulls2 = fmrx.decode_stations(iq, probe=True, afc=True)
    assert [s.offset_hz for s in st2] == offs and pulls2 == pulls and np.array_equal(pcm2, pcm)
    assert [(lv["stereo"], lv["rds"]) for lv in levels] == [(1, 1), (1, 0), (0, 0)]
    # shorter than a frame: decoded as without afc
    short = iq[: 23 * 12800]
    s3, pcm3, pulls3 = fmrx.decode_stations(short, afc=True, fft_bins=4096)
    s4, pcm4 = fmrx.decode_stations(short, fft_bins=4096)
    assert pulls3 == [None] * len(s3) and [s.offset_hz for s in s3] == [s.offset_hz for s in s4] and np.array_equal(pcm3, pcm4)


@pytest.mark.parametrize("kind", ["decim2", "rate"])
def test_decode_stations_afc_on_wide_captures(fmrx, kind):
    """The two stations of the tracking test in a capture at twice the mode's rate and at 10 MS/s."""
    iq = tracking_capture(kind)
    kw = dict(capture_decim=2) if kind == "decim2" else dict(capture_rate=10000000)
    plain = fmrx.decode_stations(iq, **kw)
    assert [s.offset_hz for s in plain[0]] == A.TUNED[:2]
    stations, pcm, pulls = fmrx.decode_stations(iq, afc=True, **kw)
    offs = [s.offset_hz for s in stations]
    print(kind, offs, pulls)
    assert all(abs(o - t) <= 1000 for o, t in zip(offs, A.TRUE[:2]))
    assert [p["pulled_hz"] for p in pulls] == [o - f for o, f in zip(offs, A.TUNED[:2])]
    with fmrx.Receiver(0, fmrx.MONO, n_streams=2) as rx:
        if kind == "decim2":
            rx.set_capture_decim(2)
        else:
            rx.set_capture_rate(10000000)
        rx.tune_wide(offs)
        assert np.array_equal(pcm, rx.process_wide(iq))


# ---- 11. the CLI -------------------------------------------------------------------------------------------

def test_cli_afc_line(fmrx):
    iq = A.landing_capture(64)[: 20 * 2 * A.FRAME_PAIRS]
    exe = os.path.join(os.path.dirname(fmrx.LIB_PATH), "bin", "fmrx")
    data = iq.tobytes() + bytes([128]) * (5 * 12800)  # five blocks past the last whole frame
    args = [exe, "0", "1", "--offset-hz", str(A.TUNED[0])]
    plain = subprocess.run(args, input=data, capture_output=True, timeout=120)
    r = subprocess.run(args + ["--afc"], input=data, capture_output=True, timeout=120)
    assert r.returncode == 0 and plain.returncode == 0, r.stderr.decode()
    lines = [x for x in r.stderr.decode().splitlines() if x.startswith("afc ")]
    assert len(lines) == 1, r.stderr.decode()
    m = re.fullmatch(r"afc offset=([+-]\d+) err=([+-]\d+) carrier=(\d) retunes=(\d+) frames=(\d+)", lines[0])
    assert m, lines[0]
    assert abs(int(m.group(1)) - A.TRUE[0]) <= 1000 and (m.group(3), int(m.group(4)), int(m.group(5))) == ("1", 1, 20)
    assert len(r.stdout) == len(plain.stdout) == (20 * 24 + 5) * 128 * 2 * 2
    n16 = 16 * 24 * 128 * 2 * 2  # the first decision comes behind 16 frames: up to there nothing differs
    assert r.stdout[:n16] == plain.stdout[:n16] and r.stdout[n16:] != plain.stdout[n16:]
    assert b"afc " not in plain.stderr
