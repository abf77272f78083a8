"""GPU tests of soft stereo (csrc/blend.hip, fmrx_set_stereo_blend and its primitives).

Everything is compared on the bits (np.array_equal) with the numpy restatement tests/blend_ref.py run with
the library's own thresholds; the references of the context tests are the oracle's left / right / demod,
meter_ref.power, blend_ref and the oracle's quantiser.  No tolerance anywhere.  (blend_ref.canon: the one
NaN the definition leaves open.)"""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

import blend_ref as B
import iqgen
import meter_ref as M
import oracle
from conftest import case_input, load_case
from taps_ref import dev_of, reference, station
from test_meter_host import _powers, _u8

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the levels primitive --------------------------------------------------------------------------

def level_powers(F):
    """Three streams of F frames: test_meter_host's powers; stream 1 with a zero row, a NaN and an Inf; stream 2
    with the pilot's column scaled frame by frame, so that its levels visit the whole range."""
    pw = np.stack([_powers(20 + s, F) for s in range(3)])
    pw[2, :, 1] = (pw[2, :, 0] + pw[2, :, 2]) * (np.float32(0.25) * np.float32(2.0) ** (np.arange(F) % 12)).astype(np.float32)
    pw[1, F // 2] = 0.0
    pw[1, F // 3, 1] = np.nan
    pw[1, (2 * F) // 3, 0] = np.inf
    return pw


def want_levels(pw, T, carry=None):
    out = [B.levels(pw[s], T, None if carry is None else carry[s]) for s in range(pw.shape[0])]
    return np.stack([r for r, _ in out]), np.stack([c for _, c in out])


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("F", [1, 3, 4, 5, 37])
def test_levels_primitive(fmrx, F, device):
    pw, T = level_powers(F), fmrx.blend_design()
    want, want_c = want_levels(pw, T)

    def run(rx, p, carry):
        if not device:
            return rx.blend_levels(p, carry)
        d_p, d_c = _d(p), _d(carry)
        d_l = torch.full((3, p.shape[1] + 1), 99, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rx.blend_levels_device(d_p.data_ptr(), p.shape[1], d_c.data_ptr(), d_l.data_ptr())
        rx.synchronize()
        return d_l.cpu().numpy(), d_c.cpu().numpy()

    zero = np.zeros((3, B.CARRY), np.float32)
    with fmrx.Receiver(0, fmrx.STEREO, n_streams=3) as rx:
        got, got_c = run(rx, pw, zero)
        assert np.array_equal(got, want) and np.array_equal(u32(got_c), u32(want_c))
        for cut in (1, 3):
            if not 0 < cut < F:
                continue
            r1, c1 = run(rx, pw[:, :cut], zero)
            r2, c2 = run(rx, pw[:, cut:], c1)
            assert np.array_equal(r1, want[:, :cut + 1]) and np.array_equal(r2, want[:, cut:])  # r2[0]: the level carried in
            assert np.array_equal(u32(c2), u32(want_c))
    assert np.all(want[:, 0] == 0)


def test_levels_primitive_other_thresholds_and_refusals(fmrx):
    pw = level_powers(5)
    with fmrx.Receiver(0, fmrx.STEREO, n_streams=3) as rx:
        for kw in ({"lo_db": 0.0, "hi_db": 6.0}, {}, {"lo_db": 20.0, "hi_db": 50.0}):
            want, _ = want_levels(pw, fmrx.blend_design(**kw))
            assert np.array_equal(rx.blend_levels(pw, **kw)[0], want), kw
        lv = np.full((3, 6), 77, np.uint8)
        c = np.zeros((3, 8), np.float32)
        L = fmrx.lib()
        assert L.fmrx_blend_levels(rx.h, None, pw.ctypes.data, 0, c.ctypes.data, lv.ctypes.data) == fmrx.FMRX_EINVAL
        bad = fmrx.BlendConfig(22.0, 10.0)
        import ctypes as C
        assert L.fmrx_blend_levels(rx.h, C.byref(bad), pw.ctypes.data, 5, c.ctypes.data, lv.ctypes.data) == fmrx.FMRX_EINVAL
        assert np.all(lv == 77)


# ---- the apply primitive ---------------------------------------------------------------------------

def apply_rows(n, seed):
    """Two streams of n (R, L) pairs: uniform floats in +-1.5 with every 97th x 40."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.5, 1.5, 2 * 2 * n).astype(np.float32)
    x[::97] *= np.float32(40.0)
    return x.reshape(2, n, 2)


def level_rows(mode, granules):
    """Stream 0: 0, 16, single steps and 0 <-> 16 jumps (modes 2 and 3: a change at frames 19 -> 20, across the
    granule boundary); stream 1: all 16."""
    F = B.GM[mode] * granules
    if B.GM[mode] == 1:
        row = [[0, 16], [16, 15, 0]][granules - 1] if mode == 0 else [[7, 8], [16, 0, 16]][granules - 1]
    else:
        row = [0, 0, 16, 16, 15, 14, 15, 16, 0, 16, 16, 16, 1, 2, 3, 3, 16, 16, 16, 16, 5] + [5, 16, 16, 0, 0, 9] * 4
    row = np.array(row[:F + 1], np.uint8)
    assert row.size == F + 1
    return np.stack([row, np.full(F + 1, 16, np.uint8)])


@pytest.mark.parametrize("granules", [1, 2])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_apply_primitive(fmrx, orc, mode, granules):
    n = B.A[mode] * granules
    x = apply_rows(n, 3 + mode)
    rows = level_rows(mode, granules)
    x[0, n // 3, 1] = np.nan                 # blended: whatever NaN comes out is a NaN (canon)
    x[0, n // 2, 0] = np.inf                 # L - R = -Inf, L' = L + Inf, R' = Inf - Inf
    x[1, 5] = np.array([0x7FC12345, 0xFF800000], np.uint32).view(np.float32)  # passed through: payload and all
    want = np.stack([B.apply(mode, x[s], rows[s]) for s in range(2)])
    passes = np.stack([B.mix(mode, n, rows[s])[1] for s in range(2)])
    want_pcm = np.stack([B.quant(orc, want[s]) for s in range(2)])
    assert passes[1].all() and np.array_equal(u32(want[1]), u32(x[1]))  # an all-16 row returns the input bits
    assert np.array_equal(want_pcm[1], B.quant(orc, x[1]))              # ... and its PCM is the quantiser's
    if B.GM[mode] > 1 and granules == 2:
        k, _ = B.mix(mode, n, rows[0])
        assert rows[0][19] != rows[0][20] and k[B.A[mode] - 1] != k[B.A[mode] - 2822]  # a ramp ends at the granule boundary
    canon = lambda y: np.stack([B.canon(y[s], passes[s]) for s in range(2)])
    with fmrx.Receiver(mode, fmrx.STEREO, n_streams=2) as rx:
        d_x, d_l = _d(x), _d(rows)
        d_y = torch.zeros((2, n, 2), dtype=torch.float32, device="cuda")
        d_p = torch.zeros((2, 2 * n), dtype=torch.int16, device="cuda")
        d_q = torch.zeros((2, 2 * n), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        rx.blend_apply(d_x.data_ptr(), n, d_l.data_ptr(), d_y.data_ptr(), d_p.data_ptr())  # out of place, both outlets
        rx.blend_apply(d_x.data_ptr(), n, d_l.data_ptr(), None, d_q.data_ptr())            # PCM only
        rx.synchronize()
        assert np.array_equal(u32(d_x.cpu().numpy()), u32(x))
        y = d_y.cpu().numpy()
        assert np.array_equal(canon(y), canon(want))
        assert np.array_equal(u32(y[1]), u32(x[1]))
        assert np.array_equal(d_p.cpu().numpy(), want_pcm) and np.array_equal(d_q.cpu().numpy(), want_pcm)
        rx.blend_apply(d_x.data_ptr(), n, d_l.data_ptr(), d_x.data_ptr(), None)            # in place
        rx.synchronize()
        assert np.array_equal(canon(d_x.cpu().numpy()), canon(want))


def test_apply_primitive_refusals(fmrx):
    with fmrx.Receiver(0, fmrx.STEREO) as rx:
        d = torch.zeros(2 * 3072 + 8, dtype=torch.float32, device="cuda")
        l = torch.zeros(8, dtype=torch.uint8, device="cuda")
        for args in ((d.data_ptr(), 3071, l.data_ptr(), None, None), (d.data_ptr(), 3073, l.data_ptr(), None, None),
                     (None, 3072, l.data_ptr(), None, None), (d.data_ptr(), 3072, None, None, None),
                     (d.data_ptr() + 8, 3072, l.data_ptr(), None, None)):
            with pytest.raises(fmrx.FmrxError) as e:
                rx.blend_apply(*args)
            assert e.value.code == fmrx.FMRX_EINVAL
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        with pytest.raises(fmrx.FmrxError) as e:
            rx.blend_apply(1, 3072, 1, None, None)
        assert e.value.code == fmrx.FMRX_EINVAL


# ---- the switch --------------------------------------------------------------------------------------

def in_calls(fn, iq, bb, calls):
    out, b = [], 0
    for nb in calls:
        out.append(fn(iq[..., b * bb:(b + nb) * bb]))
        b += nb
    return np.concatenate(out, axis=-1)


def blended(fm, mode=0, n_streams=1, offsets=None, **kw):
    rx = fm.Receiver(mode, fm.STEREO, n_streams=n_streams)
    rx.tune([0] * n_streams if offsets is None else offsets)
    rx.set_stereo_blend(True, **kw)
    return rx


def test_switch_mode0(fmrx, orc):
    iq = station(0, 12, (2, 80, 40))
    want, row, _, _, plain = reference(orc, fmrx, 0, iq, "switch")
    lv = set(int(v) for v in row[1:])
    print("levels", list(row))
    assert 16 in lv and min(lv) <= 4 and any(4 < v < 16 for v in lv)  # a wrong ramp or frame mapping cannot hide
    assert not np.array_equal(want, plain)
    bb = oracle.MODES[0][0]
    with blended(fmrx) as rx:
        assert rx.stereo_blend() == (True, 10.0, 22.0)
        assert np.array_equal(rx.process(iq), want)
        rep = rx.blend_report()
        assert rep["frames"] == 12 and rep["level_frames"] == B.histogram([row])
        assert abs(rep["mean"] - sum(int(v) for v in row[1:]) / (16 * 12)) < 1e-12
        for calls in ([120, 168], [24] * 12):
            rx.reset()
            assert rx.blend_report()["frames"] == 0
            assert np.array_equal(in_calls(rx.process, iq, bb, calls), want), calls
            assert rx.blend_report()["level_frames"] == B.histogram([row])
        # fmrx_set_stereo_blend, with any value, clears the carry and the reports and nothing else: the receiver
        # goes on, the stage restarts from mono and is back on the stream's levels once its window is full again
        rx.reset()
        first = rx.process(iq[:144 * bb])
        rx.set_stereo_blend(True)
        assert rx.blend_report()["frames"] == 0
        again = rx.process(iq[144 * bb:])
        assert np.array_equal(first, want[:144 * 256]) and rx.blend_report()["frames"] == 6
        assert not np.array_equal(again[:2 * 3072], want[144 * 256:][:2 * 3072])
        assert np.array_equal(again[2 * 3072 * 4:], want[144 * 256 + 2 * 3072 * 4:])


def test_clean_station(fmrx, orc):
    iq = station(0, 6, (2,))
    want, row, _, _, plain = reference(orc, fmrx, 0, iq, "clean")
    assert np.all(row[1:] == 16) and row[0] == 0
    with blended(fmrx) as rx:
        got = rx.process(iq)
    assert np.array_equal(got, want)
    assert np.array_equal(got[2 * 3072:], plain[2 * 3072:])      # the blend-off PCM from its second meter frame on
    assert not np.array_equal(got[:2 * 3072], plain[:2 * 3072])  # the ramp out of mono in front of it


def test_hold_decodes_the_tail_at_the_last_level(fmrx, orc):
    iq = station(0, 12, (2, 80, 40))
    bb, tail = oracle.MODES[0][0], 5
    _, row, _, _, _ = reference(orc, fmrx, 0, iq, "switch")
    nb = 6 * 24  # frames 0 .. 5, then five blocks at frame 5's level (noise since frame 4: below 16)
    o = orc.run(0, 51, iq[:(nb + tail) * bb], ["left", "right"])
    rl = np.stack([o["right"], o["left"]], axis=1)[nb * 128:]
    want = B.quant(orc, B.apply(0, rl, np.full(2, row[6], np.uint8)))
    assert row[6] < 16
    with blended(fmrx) as rx:
        rx.process(iq[:nb * bb])
        with pytest.raises(fmrx.FmrxError) as e:
            rx.process(iq[nb * bb:(nb + tail) * bb])
        assert e.value.code == fmrx.FMRX_EINVAL
        rx.blend_hold(True)
        got = rx.process(iq[nb * bb:(nb + tail) * bb])
        assert rx.blend_report()["frames"] == 6
    assert np.array_equal(got, want)


def test_with_other_stages(fmrx, orc):
    """De-emphasis 50, RDS and the meter on as well: the PCM is deemph_ref over the blended floats; the meter
    reports and the RDS info are those of the same call with blend off."""
    iq = station(0, 12, (2, 80, 40))
    want, row, _, pw, _ = reference(orc, fmrx, 0, iq, "switch", tau=50)
    with blended(fmrx) as rx:
        rx.set_deemphasis(50)
        rx.set_rds(True)
        rx.set_meter(True)
        got = rx.process(iq)
        meter_on, info_on, rep = rx.meter_report(), rx.rds_info().as_dict(), rx.blend_report()
        rx.set_stereo_blend(False)
        rx.reset()
        rx.process(iq)
        meter_off, info_off = rx.meter_report(), rx.rds_info().as_dict()
    assert np.array_equal(got, want)
    assert rep["level_frames"] == B.histogram([row])
    assert meter_on.frames == meter_off.frames == 12 and list(meter_on.sum) == list(meter_off.sum) == list(M.accumulate(pw)[0])
    assert info_on == info_off and info_on["bits"] > 0


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_other_modes(fmrx, orc, mode):
    frames = B.GM[mode]
    iq = station(mode, frames, (2, 80, 40, 16, 2) if frames > 1 else (16,), pilot=0.1, seed=30 + mode)
    want, row, _, _, plain = reference(orc, fmrx, mode, iq, ("mode", mode))
    print("levels", list(row))
    assert not np.array_equal(want, plain)
    with blended(fmrx, mode) as rx:
        assert rx.rds_granule == B.BLOCKS[mode]
        got = rx.process(iq)
        assert rx.blend_report()["level_frames"] == B.histogram([row])
    assert np.array_equal(got, want)


# ---- several stations --------------------------------------------------------------------------------

def test_process_shared_two_stations(fmrx, orc):
    from test_gpu_tuner import compose
    n, offsets = 2 * 24 * 6400, [-300000, 325000]
    dev = dev_of(0)
    kw = dict(lr=0.2 * dev, rds=0.0, audio=0.3 * dev)
    z = 0.8 * M.fm_signal(0, n, offset_hz=offsets[0], pilot=0.1 * dev, **kw) + \
        0.1 * M.fm_signal(0, n, offset_hz=offsets[1], pilot=0.05 * dev, audio_hz=700.0, **kw)
    iq = _u8(z, 3, 9)
    T, tab = fmrx.blend_design(), fmrx.meter_design(240000)[1]
    with blended(fmrx, n_streams=2, offsets=offsets) as rx:
        got = in_calls(rx.process_shared, iq, oracle.MODES[0][0], [24, 24])
        reps = [rx.blend_report(s) for s in range(2)]
    rows = []
    for s, f in enumerate(offsets):
        o = compose(iq, 0, 51, f, fields=("left", "right"))
        row, _ = B.levels(M.power(o["demod"], tab), T)
        rows.append(list(row))
        y = B.apply(0, np.stack([o["right"], o["left"]], axis=1), row)
        assert np.array_equal(got[s], B.quant(orc, y)), f
        assert reps[s]["level_frames"] == B.histogram([row])
    print("levels", rows)
    assert rows[0] != rows[1]  # a strong and a noisy station: levels of their own


def test_process_wide_decim2_s16_three_streams(fmrx, orc):
    from test_formats_host import S16
    from test_gpu_wide import capture
    from test_wide_host import wide_compose
    d, offsets = 2, [0, 700000, -900000]
    raw = capture(61, 0, d, 24, S16)
    T, tab = fmrx.blend_design(), fmrx.meter_design(240000)[1]
    with fmrx.Receiver(0, fmrx.STEREO, n_streams=3) as rx:
        rx.set_input_format(S16)
        rx.set_capture_decim(d)
        rx.tune_wide(offsets)
        rx.set_stereo_blend(True)
        got = rx.process_wide(raw).reshape(3, -1)
    for s, f in enumerate(offsets):
        o = wide_compose(raw, S16, 0, 51, d, f, fields=("left", "right"))
        row, _ = B.levels(M.power(o["demod"], tab), T)
        y = B.apply(0, np.stack([o["right"], o["left"]], axis=1), row)
        assert np.array_equal(got[s], B.quant(orc, y)), (f, list(row))


# ---- refusals, with the output untouched ---------------------------------------------------------------

def test_refusals(fmrx):
    import ctypes as C
    L, bb = fmrx.lib(), oracle.MODES[0][0]
    iq = np.ascontiguousarray(iqgen.make("synth:71", 25 * bb, oracle.MODES[0][3]))
    out = np.full(25 * 256, 1234, np.int16)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        assert L.fmrx_set_stereo_blend(rx.h, 1, None) == fmrx.FMRX_EINVAL
        assert rx.stereo_blend()[0] is False
    with fmrx.Receiver(0, fmrx.STEREO) as rx:
        blob = rx.get_state()
        rx.set_stereo_blend(True, lo_db=8.0, hi_db=20.0)
        d_iq = _d(iq)
        d_out = torch.full((25 * 256,), 1234, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        # untuned calls, host and device, and fmrx_audio_block
        assert L.fmrx_process(rx.h, iq.ctypes.data, 24, out.ctypes.data) == fmrx.FMRX_ESTATE
        assert L.fmrx_process_device(rx.h, d_iq.data_ptr(), 24, d_out.data_ptr()) == fmrx.FMRX_ESTATE
        demod = np.zeros(24 * 640, np.float32)
        assert L.fmrx_audio_block(rx.h, demod.ctypes.data, 24, out.ctypes.data) == fmrx.FMRX_ESTATE
        for call in (rx.get_state, lambda: rx.set_state(blob), lambda: rx.seek(iq)):
            with pytest.raises(fmrx.FmrxError) as e:
                call()
            assert e.value.code == fmrx.FMRX_ESTATE
        # tuned: a granule +- 1 blocks
        rx.tune([0])
        for nb in (23, 25):
            assert L.fmrx_process(rx.h, iq.ctypes.data, nb, out.ctypes.data) == fmrx.FMRX_EINVAL
            assert L.fmrx_process_device(rx.h, d_iq.data_ptr(), nb, d_out.data_ptr()) == fmrx.FMRX_EINVAL
        rx.synchronize()
        assert np.all(out == 1234) and bool((d_out == 1234).all())
        assert rx.blend_report()["frames"] == 0
        # a bad config: the old one kept
        for lo, hi in ((22.0, 10.0), (float("nan"), 22.0), (10.0, 61.0)):
            assert L.fmrx_set_stereo_blend(rx.h, 1, C.byref(fmrx.BlendConfig(lo, hi))) == fmrx.FMRX_EINVAL
        assert rx.stereo_blend() == (True, 8.0, 20.0)
        rx.set_stereo_blend(False)
        with pytest.raises(fmrx.FmrxError) as e:
            rx.blend_hold(True)  # nothing to hold while the stage is off
        assert e.value.code == fmrx.FMRX_ESTATE


def test_off_is_off(fmrx):
    z = load_case("m0_rf51_synth")
    iq = case_input(z)
    with fmrx.Receiver(0, fmrx.STEREO) as rx:
        rx.set_stereo_blend(True)
        rx.set_stereo_blend(False)
        assert rx.stereo_blend()[0] is False
        assert np.array_equal(rx.process(iq), z["pcm"])  # an untuned call works again, and gives the golden bits
        rx.reset()
        rx.tune([0])
        assert np.array_equal(rx.process(iq), z["pcm"])
        blob = rx.get_state()
        rx.set_state(blob)


# ---- the front ends of the API ------------------------------------------------------------------------

def test_decode_stations(fmrx, orc):
    from test_scan_host import capture
    iq = capture("two", 30)[0]  # one granule and six blocks that are trimmed
    bb = oracle.MODES[0][0]
    stations, pcm, blends = fmrx.decode_stations(iq, channels=fmrx.STEREO, blend=True)
    assert [s.offset_hz for s in stations] == [-300000, 300000]
    with blended(fmrx, n_streams=2, offsets=[s.offset_hz for s in stations]) as rx:
        want = rx.process_shared(iq[:24 * bb])
        reps = [rx.blend_report(s) for s in range(2)]
    assert np.array_equal(pcm, want) and blends == reps and blends[0]["frames"] == 1
    plain = fmrx.decode_stations(iq, channels=fmrx.STEREO)  # blend=False: today's shape
    assert len(plain) == 2 and plain[1].shape == (2, 30 * 256)
    # probe: stations routed to mono stay mono and report None
    st, pcm_p, levels, blends_p = fmrx.decode_stations(iq, channels=fmrx.STEREO, probe=True, blend=True)
    assert len(levels) == len(blends_p) == 2 and pcm_p.shape == (2, 24 * 256)
    for k in range(2):
        assert (blends_p[k] is None) == (not levels[k]["stereo"])
        if blends_p[k] is None:
            assert np.array_equal(pcm_p[k][0::2], pcm_p[k][1::2])
        else:
            assert np.array_equal(pcm_p[k], want[k]) and blends_p[k] == reps[k]


def test_cli(fmrx):
    exe = os.path.join(os.path.dirname(fmrx.LIB_PATH), "bin", "fmrx")
    iq, bb = station(0, 12, (2, 80, 40)), oracle.MODES[0][0]
    data = iq[:(48 + 5) * bb]  # two granules and five blocks: the CLI's batches are a granule, the tail is held
    r = subprocess.run([exe, "0", "2", "--blend"], input=data.tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    with blended(fmrx) as rx:
        head = rx.process(data[:48 * bb])
        rep = rx.blend_report()
        rx.blend_hold(True)
        want = np.concatenate([head, rx.process(data[48 * bb:])])
    assert r.stdout == want.tobytes()
    m = re.search(rb"^blend mean=(\d\.\d\d) full=(\d+) mono=(\d+) frames=(\d+)$", r.stderr, re.M)
    assert m, r.stderr
    assert abs(float(m[1]) - rep["mean"]) <= 0.005 + 1e-9
    assert (int(m[2]), int(m[3]), int(m[4])) == (rep["level_frames"][16], rep["level_frames"][0], 2)
    for args in (["0", "1", "--blend"], ["--blend"], ["0", "2", "--blend", "--mono-product"]):
        bad = subprocess.run([exe] + args, input=b"", capture_output=True, timeout=120)
        assert bad.returncode == 1 and b"--blend" in bad.stderr and bad.stdout == b"", args
