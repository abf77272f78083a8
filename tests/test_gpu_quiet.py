"""GPU tests of quieting (csrc/quiet.hip, fmrx_set_quieting and its primitives).

Everything is compared on the bits (np.array_equal) with the numpy restatement tests/quiet_ref.py run with the
library's own design; the references of the context tests are the oracle's mono or left / right and demod,
meter_ref.power, quiet_ref (behind blend_ref, in front of deemph_ref where those stages are on) and the
oracle's quantiser.  No tolerance anywhere.  (quiet_ref.canon: the NaNs the definition leaves open.)"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import blend_ref as B
import deemph_ref as dr
import iqgen
import meter_ref as M
import oracle
import quiet_ref as Q
from conftest import case_input, load_case
from taps_ref import dev_of, station
from test_meter_host import _powers, _u8

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CHANNELS = {1: "MONO", 2: "STEREO"}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def _d(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()  # taps_ref.station's arrays are read-only


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def design_of(fm, mode, **kw):
    return fm.quiet_design(*Q.RATES[mode], **kw)


# ---- the levels primitive --------------------------------------------------------------------------

def level_powers(F):
    """Three streams of F frames.  Stream 0: test_meter_host's powers with the two noise bins spread over the
    thresholds; stream 1: the same with a zero row, a NaN and an Inf; stream 2: the 61 kHz bin chosen so that the
    four-frame sum climbs through every threshold, 0.75 dB a frame over the cut's and 0.5 dB over the mute's
    (n_f = N_f - N_{f-1} + n_{f-4} stays positive while N rises)."""
    pw = np.stack([_powers(20 + s, F) for s in range(3)])
    pw[:2, :, 5:7] = (10.0 ** np.random.default_rng(F).uniform(0.0, 4.3, (2, F, 2))).astype(np.float32)
    pw[1, F // 2] = 0.0
    pw[1, F // 3, 5] = np.nan
    pw[1, (2 * F) // 3, 6] = np.inf
    db = np.concatenate([21.5 + 0.75 * np.arange(18), 35.6 + 0.5 * np.arange(19)])[:F]  # the readings: both levels fall 16 .. 0
    N = 4.0 * 10.0 ** (db / 10.0)
    n = np.zeros(F + 4)
    for f in range(F):
        n[f + 4] = N[f] - (n[f + 1] + n[f + 2] + n[f + 3])
    assert np.all(n[4:] > 0)
    pw[2, :, 5], pw[2, :, 6] = n[4:].astype(np.float32), 0.0
    return pw


def want_levels(pw, d, carry=None):
    out = [Q.levels(pw[s], d, None if carry is None else carry[s]) for s in range(pw.shape[0])]
    return np.stack([r for r, _ in out]), np.stack([c for _, c in out])


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("F", [1, 3, 4, 5, 37])
def test_levels_primitive(fmrx, F, device):
    d = design_of(fmrx, 0)
    pw = level_powers(F)
    want, want_c = want_levels(pw, d)
    if F == 37:  # the two levels of stream 2 visit 0 .. 16
        assert set(want[2, 1:, 0]) == set(range(17)) and set(want[2, 1:, 1]) == set(range(17))
        assert len(set(want[0, :, 0])) > 4 and (want[1, 1 + F // 3] == 0).all() and (want[1, 1 + (2 * F) // 3] == 0).all()

    def run(rx, p, carry):
        if not device:
            return rx.quiet_levels(p, carry)
        d_p, d_c = _d(p), _d(carry)
        d_l = torch.full((3, p.shape[1] + 1, 2), 99, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rx.quiet_levels_device(d_p.data_ptr(), p.shape[1], d_c.data_ptr(), d_l.data_ptr())
        rx.synchronize()
        return d_l.cpu().numpy(), d_c.cpu().numpy()

    zero = np.zeros((3, Q.CARRY), np.float32)
    with fmrx.Receiver(0, fmrx.MONO, n_streams=3) as rx:
        got, got_c = run(rx, pw, zero)
        assert np.array_equal(got, want) and np.array_equal(u32(got_c), u32(want_c))
        for cut in (1, 3):
            if not 0 < cut < F:
                continue
            r1, c1 = run(rx, pw[:, :cut], zero)
            r2, c2 = run(rx, pw[:, cut:], c1)
            assert np.array_equal(r1, want[:, :cut + 1]) and np.array_equal(r2, want[:, cut:])  # r2[0]: the pair carried in
            assert np.array_equal(u32(c2), u32(want_c))
    assert np.all(want[:, 0] == 0)


def test_levels_primitive_other_config_and_refusals(fmrx):
    kws = (dict(cut_lo_db=10.0, cut_hi_db=20.0, mute_lo_db=15.0, mute_hi_db=40.0), {}, dict(cut_lo_db=30.0, cut_hi_db=50.0))
    pw = level_powers(5)
    with fmrx.Receiver(1, fmrx.STEREO, n_streams=3) as rx:  # mode 1: P = 288 scales the thresholds
        seen = []
        for kw in kws:
            want, _ = want_levels(pw, design_of(fmrx, 1, **kw))
            assert np.array_equal(rx.quiet_levels(pw, **kw)[0], want), kw
            seen.append(want.tobytes())
        assert len(set(seen)) == 3
        # a carried pair outside 0 .. 16 counts as 0
        carry = np.zeros((3, 8), np.float32)
        carry[0, 3:5], carry[1, 3:5], carry[2, 3:5] = (17.0, -1.0), (16.0, 3.0), (np.nan, 2.5)
        got, _ = rx.quiet_levels(pw, carry)
        assert got[:, 0].tolist() == [[0, 0], [16, 3], [0, 2]] and np.array_equal(got, want_levels(pw, design_of(fmrx, 1), carry)[0])
        lv = np.full((3, 6, 2), 77, np.uint8)
        c = np.zeros((3, 8), np.float32)
        L = fmrx.lib()
        assert L.fmrx_quiet_levels(rx.h, None, pw.ctypes.data, 0, c.ctypes.data, lv.ctypes.data) == fmrx.FMRX_EINVAL
        bad = fmrx.quiet_config(cut_lo_db=40.0)
        assert L.fmrx_quiet_levels(rx.h, C.byref(bad), pw.ctypes.data, 5, c.ctypes.data, lv.ctypes.data) == fmrx.FMRX_EINVAL
        assert np.all(lv == 77)


# ---- the apply primitive ---------------------------------------------------------------------------

def apply_input(n, nch, seed):
    """Two streams of n frames of nch channels: uniform floats in +-1.5 with every 97th x 40."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.5, 1.5, 2 * n * nch).astype(np.float32)
    x[::97] *= np.float32(40.0)
    return x.reshape(2, n, nch)


def level_variants(mode, granules):
    """Lists of (c, m) pairs for stream 0 (stream 1 is all 16 throughout): all 0; single steps; 0 <-> 16 jumps; cut
    and mute differing; in modes 2 and 3 one long row with all of these and a change at frames 19 -> 20, across
    the granule boundary."""
    E = Q.GM[mode] * granules + 1
    if Q.GM[mode] == 1:
        rows = [[(0, 0)] * 3, [(7, 9), (8, 8), (7, 9)], [(0, 16), (16, 0), (0, 16)], [(16, 0), (16, 5), (3, 16)], [(16, 16), (15, 16), (16, 16)]]
    else:
        c = [0, 0, 16, 16, 15, 14, 15, 16, 0, 16, 16, 16, 1, 2, 3, 3, 16, 16, 16, 16, 5] + [5, 16, 16, 0, 0, 9] * 4
        m = [16, 0, 0, 16, 16, 16, 7, 8, 9, 16, 16, 0, 16, 16, 4, 4, 4, 16, 16, 12, 2] + [2, 16, 0, 16, 11, 16] * 4
        rows = [[(0, 0)] * E, list(zip(c, m))]
    return [np.stack([np.array(r[:E], np.uint8), np.full((E, 2), 16, np.uint8)]) for r in rows]


@pytest.mark.parametrize("nch", [1, 2], ids=["mono", "stereo"])
@pytest.mark.parametrize("granules", [1, 2])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_apply_primitive(fmrx, orc, mode, granules, nch):
    """3072 frames are three whole chunks; 56448 are 55 chunks and a partial one: both workgroup edges."""
    n = Q.A[mode] * granules
    d = design_of(fmrx, mode)
    x = apply_input(n, nch, 3 + mode)
    x[0, n // 3, nch - 1] = np.nan
    x[0, n // 2, 0] = np.inf
    x[1, 5] = np.array([0x7FC12345, 0xFF800000], np.uint32).view(np.float32)[:nch]  # passed through: payload and all
    hist = apply_input(Q.HIST, nch, 50)[:, :, :].transpose(0, 2, 1).copy()  # (2, nch, 63): a history that is not zeros
    with fmrx.Receiver(mode, getattr(fmrx, CHANNELS[nch]), n_streams=2) as rx:
        d_x = _d(x)
        for v, rows in enumerate(level_variants(mode, granules)):
            out = [Q.apply_rows(mode, x[s], rows[s], d, hist[s]) for s in range(2)]
            want, want_h, touched = (np.stack([o[k] for o in out]) for k in range(3))
            want_pcm = np.stack([Q.quant(orc, want[s]) for s in range(2)])
            assert not touched[1].any() and np.array_equal(u32(want[1]), u32(x[1]))  # all 16 returns the input bits
            assert np.array_equal(want_pcm[1], Q.quant(orc, x[1]))                   # ... and the quantiser's PCM
            canon = lambda y: np.stack([Q.canon(y[s], touched[s]) for s in range(2)])
            d_l = _d(rows)
            d_y = torch.zeros((2, n, nch), dtype=torch.float32, device="cuda")
            d_p, d_q = (torch.zeros((2, n * nch), dtype=torch.int16, device="cuda") for _ in range(2))
            d_z = torch.zeros((2, n, nch), dtype=torch.float32, device="cuda")
            d_h = [_d(hist) for _ in range(3)]
            torch.cuda.synchronize()
            rx.quiet_apply(d_x.data_ptr(), n, d_l.data_ptr(), d_h[0].data_ptr(), d_y.data_ptr(), d_p.data_ptr())  # both outlets
            rx.quiet_apply(d_x.data_ptr(), n, d_l.data_ptr(), d_h[1].data_ptr(), None, d_q.data_ptr())            # PCM only
            rx.quiet_apply(d_x.data_ptr(), n, d_l.data_ptr(), d_h[2].data_ptr(), d_z.data_ptr(), None)            # floats only
            rx.synchronize()
            y = d_y.cpu().numpy()
            assert np.array_equal(canon(y), canon(want)), v
            assert np.array_equal(u32(y[1]), u32(x[1]))
            assert np.array_equal(u32(d_z.cpu().numpy()), u32(y))
            assert np.array_equal(d_p.cpu().numpy(), want_pcm) and np.array_equal(d_q.cpu().numpy(), want_pcm), v
            for h in d_h:
                assert np.array_equal(u32(h.cpu().numpy()), u32(want_h))
        assert np.array_equal(u32(d_x.cpu().numpy()), u32(x))  # the input is never written
        if granules == 2:  # one call against two, the history's bits carried between them
            rows = level_variants(mode, 2)[-1]
            Am, Gm = Q.A[mode], Q.GM[mode]
            zero = np.zeros((2, nch, Q.HIST), np.float32)
            whole = [Q.apply_rows(mode, x[s], rows[s], d, zero[s]) for s in range(2)]
            d_h, d_y = _d(zero), torch.zeros((2, n, nch), dtype=torch.float32, device="cuda")
            halves = []
            for g in range(2):
                d_part = _d(x[:, g * Am:(g + 1) * Am])
                d_l = _d(rows[:, g * Gm: (g + 1) * Gm + 1])
                d_o = torch.zeros((2, Am, nch), dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                rx.quiet_apply(d_part.data_ptr(), Am, d_l.data_ptr(), d_h.data_ptr(), d_o.data_ptr(), None)
                rx.synchronize()
                halves.append(d_o.cpu().numpy())
                if g == 0:
                    assert np.array_equal(u32(d_h.cpu().numpy()), u32(x[:, Am - Q.HIST:Am].transpose(0, 2, 1)))
            got = np.concatenate(halves, axis=1)
            for s in range(2):
                assert np.array_equal(Q.canon(got[s], whole[s][2]), Q.canon(whole[s][0], whole[s][2])), s
                assert np.array_equal(u32(d_h.cpu().numpy()[s]), u32(whole[s][1]))


def test_apply_primitive_uses_the_context_config(fmrx, orc):
    kw = dict(mute_depth_db=6.0, corner_hz=4000)
    n, rows = Q.A[0], level_variants(0, 1)[1]
    x = apply_input(n, 1, 8)
    with fmrx.Receiver(0, fmrx.MONO, n_streams=2) as rx:
        rx.set_quieting(False, **kw)  # the config alone; the switch stays off
        on, cfg = rx.quieting()
        assert not on and (cfg.mute_depth_db, cfg.corner_hz) == (6.0, 4000)
        d_x, d_l, d_h = _d(x), _d(rows), _d(np.zeros((2, 1, Q.HIST), np.float32))
        d_y = torch.zeros((2, n, 1), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rx.quiet_apply(d_x.data_ptr(), n, d_l.data_ptr(), d_h.data_ptr(), d_y.data_ptr(), None)
        rx.synchronize()
    want = np.stack([Q.apply_rows(0, x[s], rows[s], design_of(fmrx, 0, **kw))[0] for s in range(2)])
    other = np.stack([Q.apply_rows(0, x[s], rows[s], design_of(fmrx, 0))[0] for s in range(2)])
    assert np.array_equal(u32(d_y.cpu().numpy()), u32(want)) and not np.array_equal(want, other)


def test_apply_primitive_refusals(fmrx):
    for channels, nch in ((fmrx.MONO, 1), (fmrx.STEREO, 2)):
        with fmrx.Receiver(0, channels) as rx:
            d = torch.zeros(2 * nch * 3072 + 8, dtype=torch.float32, device="cuda")
            o = torch.full((nch * 3072,), 5.0, dtype=torch.float32, device="cuda")
            l = torch.zeros(8, dtype=torch.uint8, device="cuda")
            h = torch.zeros(nch * 63, dtype=torch.float32, device="cuda")
            p, lp, hp, op = d.data_ptr(), l.data_ptr(), h.data_ptr(), o.data_ptr()
            for args in ((p, 3071, lp, hp, op, None), (p, 3073, lp, hp, op, None), (None, 3072, lp, hp, op, None),
                         (p, 3072, None, hp, op, None), (p, 3072, lp, None, op, None), (p, 3072, lp, hp, None, None),
                         (p, 3072, lp, hp, p, None),             # in place
                         (p, 3072, lp, hp, p + 4 * 1000, None),  # overlapping
                         (p + 4 * 100, 3072, lp, hp, p, None)):
                with pytest.raises(fmrx.FmrxError) as e:
                    rx.quiet_apply(*args)
                assert e.value.code == fmrx.FMRX_EINVAL, args
            rx.synchronize()
            assert bool((o == 5.0).all()) and bool((d == 0).all())


# ---- the switch --------------------------------------------------------------------------------------

_cache: dict = {}


def reference(orc, fm, mode, iq, nch, key, tau=0, blend=False, **cfg):
    """(pcm, level pairs with pair 0, powers, the stage-off PCM, the mono floats or None) of one stream over the
    whole of iq from the reset."""
    k = (key, nch, tau, blend, tuple(sorted(cfg.items())))
    if k not in _cache:
        o = orc.run(mode, 51, iq, ["left", "right", "demod"] if nch == 2 else ["mono_indep", "demod"])
        pw = M.power(o["demod"], fm.meter_design(oracle.MODES[mode][5])[1])
        rows, _ = Q.levels(pw, design_of(fm, mode, **cfg))
        x = np.stack([o["right"], o["left"]], axis=1) if nch == 2 else o["mono_indep"].reshape(-1, 1)
        plain = orc.quant(x.reshape(-1))
        if blend:
            x = B.apply(mode, x, B.levels(pw, fm.blend_design())[0])
        z = Q.apply_rows(mode, x, rows, design_of(fm, mode, **cfg))[0]
        if tau:
            h = fm.deemph_design(Q.RATES[mode][0], tau)
            pcm = dr.pcm_stereo(orc, z[:, 1], z[:, 0], h) if nch == 2 else dr.pcm(orc, z[:, 0], h)
        else:
            pcm = Q.quant(orc, z)
        _cache[k] = (pcm, rows, pw, plain, None if nch == 2 else o["mono_indep"])
    return _cache[k]


def in_calls(fn, iq, bb, calls):
    out, b = [], 0
    for nb in calls:
        out.append(fn(iq[..., b * bb:(b + nb) * bb]))
        b += nb
    return np.concatenate(out, axis=-1)


def quieted(fm, mode=0, nch=1, n_streams=1, offsets=None, **kw):
    rx = fm.Receiver(mode, getattr(fm, CHANNELS[nch]), n_streams=n_streams)
    rx.tune([0] * n_streams if offsets is None else offsets)
    rx.set_quieting(True, **kw)
    return rx


def report_of(rows_of_calls):
    hc, hm = Q.histograms(rows_of_calls)
    return hc, hm, sum(hc)


@pytest.mark.parametrize("nch", [1, 2], ids=["mono", "stereo"])
def test_switch_mode0(fmrx, orc, nch):
    iq = station(0, 12, (2, 80, 200))
    want, rows, _, plain, _ = reference(orc, fmrx, 0, iq, nch, "switch")
    print("levels", rows.tolist())
    cs, ms = set(rows[1:, 0].tolist()), set(rows[1:, 1].tolist())
    assert 16 in cs and 0 in cs and 16 in ms and min(ms) < 16  # clean, hissing and below threshold: all three met
    assert not np.array_equal(want, plain)
    bb, per = oracle.MODES[0][0], 128 * nch
    with quieted(fmrx, 0, nch) as rx:
        on, cfg = rx.quieting()
        assert on and {k: getattr(cfg, k) for k in Q.DEFAULTS} == Q.DEFAULTS
        assert np.array_equal(rx.process(iq), want)
        rep = rx.quiet_report()
        hc, hm, frames = report_of([rows])
        assert (rep["frames"], rep["cut_frames"], rep["mute_frames"]) == (12, hc, hm) and frames == 12
        assert abs(rep["cut_mean"] - rows[1:, 0].sum() / (16 * 12)) < 1e-12 and abs(rep["mute_mean"] - rows[1:, 1].sum() / (16 * 12)) < 1e-12
        for calls in ([120, 168], [24] * 12):
            rx.reset()
            assert rx.quiet_report()["frames"] == 0 and rx.quieting()[0]
            assert np.array_equal(in_calls(rx.process, iq, bb, calls), want), calls
            assert rx.quiet_report()["cut_frames"] == hc and rx.quiet_report()["mute_frames"] == hm
        # fmrx_set_quieting, with any value, clears both carries and the reports and nothing else: the receiver goes
        # on, the stage restarts closed and is back on the stream's levels once its window is full again (frame 3 of
        # the restart is computed from four frames of its own; the FIR's 63 samples are long past by then)
        rx.reset()
        first = rx.process(iq[:144 * bb])
        rx.set_quieting(True)
        assert rx.quiet_report()["frames"] == 0
        again = rx.process(iq[144 * bb:])
        assert np.array_equal(first, want[:144 * per]) and rx.quiet_report()["frames"] == 6
        assert not np.array_equal(again[:3072 * nch], want[144 * per:][:3072 * nch])
        assert np.array_equal(again[4 * 3072 * nch:], want[144 * per + 4 * 3072 * nch:])


@pytest.mark.parametrize("nch", [1, 2], ids=["mono", "stereo"])
def test_clean_station(fmrx, orc, nch):
    iq = station(0, 6, (2,))
    want, rows, _, plain, _ = reference(orc, fmrx, 0, iq, nch, "clean")
    assert np.all(rows[1:] == 16) and tuple(rows[0]) == (0, 0)
    with quieted(fmrx, 0, nch) as rx:
        got = rx.process(iq)
    assert np.array_equal(got, want)
    assert np.array_equal(got[3072 * nch:], plain[3072 * nch:])      # the stage-off PCM from audio frame 3072 on
    assert not np.array_equal(got[:3072 * nch], plain[:3072 * nch])  # ... and not before: the stream fades in


def test_hold_decodes_the_tail_at_the_last_levels(fmrx, orc):
    iq = station(0, 12, (2, 80, 200))
    bb, tail, nb = oracle.MODES[0][0], 5, 6 * 24  # frames 0 .. 5, then five blocks at frame 5's levels
    _, rows, _, _, _ = reference(orc, fmrx, 0, iq, 2, "switch")
    assert tuple(rows[6]) != (16, 16)
    d = design_of(fmrx, 0)
    o = orc.run(0, 51, iq[:(nb + tail) * bb], ["left", "right"])
    rl = np.stack([o["right"], o["left"]], axis=1)
    hist = rl[nb * 128 - Q.HIST:nb * 128].T  # the FIR history still moves
    want = Q.quant(orc, Q.apply_rows(0, rl[nb * 128:], np.tile(rows[6], (2, 1)), d, hist)[0])
    with quieted(fmrx, 0, 2) as rx:
        rx.process(iq[:nb * bb])
        rep = rx.quiet_report()
        with pytest.raises(fmrx.FmrxError) as e:
            rx.process(iq[nb * bb:(nb + tail) * bb])
        assert e.value.code == fmrx.FMRX_EINVAL
        rx.quiet_hold(True)
        got = rx.process(iq[nb * bb:(nb + tail) * bb])
        assert rx.quiet_report() == rep and rep["frames"] == 6  # nothing measured, nothing counted
    assert np.array_equal(got, want)


def test_with_other_stages(fmrx, orc):
    """Soft stereo, de-emphasis 50, RDS and the meter on as well: the PCM is deemph_ref over quiet_ref over
    blend_ref; the meter, blend and RDS reports are those of the same call with quieting off."""
    iq = station(0, 12, (2, 80, 200))
    want, rows, pw, _, _ = reference(orc, fmrx, 0, iq, 2, "switch", tau=50, blend=True)
    with quieted(fmrx, 0, 2) as rx:
        rx.set_stereo_blend(True)
        rx.set_deemphasis(50)
        rx.set_rds(True)
        rx.set_meter(True)
        got = rx.process(iq)
        on = (rx.meter_report(), rx.rds_info().as_dict(), rx.blend_report(), rx.quiet_report())
        rx.set_quieting(False)
        rx.reset()
        rx.process(iq)
        off = (rx.meter_report(), rx.rds_info().as_dict(), rx.blend_report())
    assert np.array_equal(got, want)
    hc, hm, _ = report_of([rows])
    assert (on[3]["cut_frames"], on[3]["mute_frames"]) == (hc, hm)
    assert on[0].frames == off[0].frames == 12 and list(on[0].sum) == list(off[0].sum) == list(M.accumulate(pw)[0])
    assert on[1] == off[1] and on[1]["bits"] > 0
    assert on[2] == off[2] and on[2]["level_frames"] == B.histogram([B.levels(pw, fmrx.blend_design())[0]])


def test_mono_with_deemphasis_and_d_mono_stays(fmrx, orc):
    """A mono fmrx_process_device_ex with d_mono: the stage reads d_mono and never writes it."""
    iq = station(0, 12, (2, 80, 200))
    nb, na = 288, 288 * 128
    for tau in (0, 75):
        want, _, _, _, mono = reference(orc, fmrx, 0, iq, 1, "switch", tau=tau)
        with quieted(fmrx, 0, 1) as rx:
            rx.set_deemphasis(tau)
            d_iq = _d(iq)
            d_pcm = torch.zeros(na, dtype=torch.int16, device="cuda")
            d_mono = torch.zeros(na, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            rx.process_device(d_iq.data_ptr(), nb, d_pcm.data_ptr(), d_mono.data_ptr())
            rx.synchronize()
            assert np.array_equal(u32(d_mono.cpu().numpy()), u32(mono)), tau
            assert np.array_equal(d_pcm.cpu().numpy(), want), tau
            rx.reset()
            assert np.array_equal(rx.process(iq), want), tau  # without d_mono: the context's scratch


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_other_modes(fmrx, orc, mode):
    frames, nch = Q.GM[mode], 1 + mode % 2
    iq = station(mode, frames, (2, 80, 200, 16, 2) if frames > 1 else (80,), pilot=0.1, seed=30 + mode)
    want, rows, _, plain, _ = reference(orc, fmrx, mode, iq, nch, ("mode", mode))
    print("levels", rows.tolist())
    assert not np.array_equal(want, plain)
    with quieted(fmrx, mode, nch) as rx:
        assert rx.rds_granule == Q.BLOCKS[mode]
        got = rx.process(iq)
        hc, hm, _ = report_of([rows])
        assert (rx.quiet_report()["cut_frames"], rx.quiet_report()["mute_frames"]) == (hc, hm)
    assert np.array_equal(got, want)


# ---- several stations --------------------------------------------------------------------------------

def test_process_shared_two_stations(fmrx, orc):
    from test_gpu_tuner import compose
    n, offsets = 2 * 24 * 6400, [-300000, 325000]
    dev = dev_of(0)
    kw = dict(lr=0.2 * dev, rds=0.0, audio=0.3 * dev)
    z = 0.8 * M.fm_signal(0, n, offset_hz=offsets[0], pilot=0.1 * dev, **kw) + \
        0.1 * M.fm_signal(0, n, offset_hz=offsets[1], pilot=0.05 * dev, audio_hz=700.0, **kw)
    iq = _u8(z, 16, 9)  # the station at 0.8 stays untouched, the one at 0.1 is cut and begins to mute
    d, tab = design_of(fmrx, 0), fmrx.meter_design(240000)[1]
    with quieted(fmrx, 0, 1, n_streams=2, offsets=offsets) as rx:
        got = in_calls(rx.process_shared, iq, oracle.MODES[0][0], [24, 24]).reshape(2, -1)
        reps = [rx.quiet_report(s) for s in range(2)]
    all_rows = []
    for s, f in enumerate(offsets):
        o = compose(iq, 0, 51, f, fields=("mono_indep",))
        rows, _ = Q.levels(M.power(o["demod"], tab), d)
        all_rows.append(rows.tolist())
        y = Q.apply_rows(0, o["mono_indep"].reshape(-1, 1), rows, d)[0]
        assert np.array_equal(got[s], Q.quant(orc, y)), f
        assert (reps[s]["cut_frames"], reps[s]["mute_frames"]) == Q.histograms([rows])
    print("levels", all_rows)
    assert all_rows[0] != all_rows[1]  # a strong and a weak station: levels of their own


def test_process_wide_decim2_s16_three_streams(fmrx, orc):
    from test_formats_host import S16
    from test_gpu_wide import capture
    from test_wide_host import wide_compose
    dec, offsets = 2, [0, 700000, -900000]
    raw = capture(61, 0, dec, 24, S16)
    d, tab = design_of(fmrx, 0), fmrx.meter_design(240000)[1]
    with fmrx.Receiver(0, fmrx.STEREO, n_streams=3) as rx:
        rx.set_input_format(S16)
        rx.set_capture_decim(dec)
        rx.tune_wide(offsets)
        rx.set_quieting(True)
        got = rx.process_wide(raw).reshape(3, -1)
    for s, f in enumerate(offsets):
        o = wide_compose(raw, S16, 0, 51, dec, f, fields=("left", "right"))
        rows, _ = Q.levels(M.power(o["demod"], tab), d)
        y = Q.apply_rows(0, np.stack([o["right"], o["left"]], axis=1), rows, d)[0]
        assert np.array_equal(got[s], Q.quant(orc, y)), (f, rows.tolist())


# ---- refusals, with the output untouched ---------------------------------------------------------------

@pytest.mark.parametrize("nch", [1, 2], ids=["mono", "stereo"])
def test_refusals(fmrx, nch):
    L, bb = fmrx.lib(), oracle.MODES[0][0]
    iq = np.ascontiguousarray(iqgen.make("synth:71", 25 * bb, oracle.MODES[0][3]))
    out = np.full(25 * 128 * nch, 1234, np.int16)
    with fmrx.Receiver(0, getattr(fmrx, CHANNELS[nch])) as rx:
        blob = rx.get_state()
        with pytest.raises(fmrx.FmrxError) as e:
            rx.quiet_hold(True)  # nothing to hold while the stage is off
        assert e.value.code == fmrx.FMRX_ESTATE
        rx.set_quieting(True, cut_lo_db=20.0, corner_hz=3000)
        d_iq = _d(iq)
        d_out = torch.full((25 * 128 * nch,), 1234, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        # untuned calls, host and device, and fmrx_audio_block
        assert L.fmrx_process(rx.h, iq.ctypes.data, 24, out.ctypes.data) == fmrx.FMRX_ESTATE
        assert L.fmrx_process_device(rx.h, d_iq.data_ptr(), 24, d_out.data_ptr()) == fmrx.FMRX_ESTATE
        assert L.fmrx_process_device_ex(rx.h, d_iq.data_ptr(), 24, d_out.data_ptr(), None) == fmrx.FMRX_ESTATE
        demod = np.zeros(24 * 640, np.float32)
        assert L.fmrx_audio_block(rx.h, demod.ctypes.data, 24, out.ctypes.data) == fmrx.FMRX_ESTATE
        calls = [rx.get_state, lambda: rx.set_state(blob)] + ([lambda: rx.seek(iq)] if nch == 1 else [])
        for call in calls:
            with pytest.raises(fmrx.FmrxError) as e:
                call()
            assert e.value.code == fmrx.FMRX_ESTATE
        # tuned: a granule +- 1 blocks
        rx.tune([0])
        for nb in (23, 25):
            assert L.fmrx_process(rx.h, iq.ctypes.data, nb, out.ctypes.data) == fmrx.FMRX_EINVAL
            assert L.fmrx_process_device(rx.h, d_iq.data_ptr(), nb, d_out.data_ptr()) == fmrx.FMRX_EINVAL
            assert L.fmrx_process_shared(rx.h, iq.ctypes.data, nb, out.ctypes.data) == fmrx.FMRX_EINVAL
        rx.synchronize()
        assert np.all(out == 1234) and bool((d_out == 1234).all())
        assert rx.quiet_report()["frames"] == 0
        # a bad config: the old one kept
        for kw in (dict(cut_lo_db=40.0), dict(mute_depth_db=float("nan")), dict(corner_hz=2068), dict(mute_hi_db=81.0)):
            assert L.fmrx_set_quieting(rx.h, 1, C.byref(fmrx.quiet_config(**kw))) == fmrx.FMRX_EINVAL
        on, cfg = rx.quieting()
        assert on and (cfg.cut_lo_db, cfg.cut_hi_db, cfg.corner_hz) == (20.0, 34.0, 3000)


def test_corner_bound_at_44100(fmrx):
    with fmrx.Receiver(2, fmrx.MONO) as rx:
        rx.set_quieting(True, corner_hz=1901)  # refused at 48 kHz, the least at 44.1 kHz
        with pytest.raises(fmrx.FmrxError) as e:
            rx.set_quieting(True, corner_hz=1900)
        assert e.value.code == fmrx.FMRX_EINVAL and rx.quieting()[1].corner_hz == 1901


@pytest.mark.parametrize("name,channels", [("m0_rf51_synth", "STEREO"), ("m0_rf101_synth", "MONO")])
def test_off_is_off(fmrx, name, channels):
    z = load_case(name)
    iq = case_input(z)
    want = z["pcm"] if channels == "STEREO" else z["pcm_mono"]
    with fmrx.Receiver(0, getattr(fmrx, channels), rf_taps=101 if "rf101" in name else 51) as rx:
        rx.set_quieting(True)
        rx.set_quieting(False)
        assert rx.quieting()[0] is False
        assert np.array_equal(rx.process(iq), want)  # an untuned call works again, and gives the golden bits
        rx.reset()
        rx.tune([0])
        assert np.array_equal(rx.process(iq), want)
        blob = rx.get_state()
        rx.set_state(blob)


# ---- the front ends of the API ------------------------------------------------------------------------

def test_decode_stations(fmrx, orc):
    from test_scan_host import capture
    iq = capture("two", 30)[0]  # one granule and six blocks that are trimmed
    bb = oracle.MODES[0][0]
    for nch in (1, 2):
        stations, pcm, quiets = fmrx.decode_stations(iq, channels=getattr(fmrx, CHANNELS[nch]), quiet=True)
        assert [s.offset_hz for s in stations] == [-300000, 300000]
        with quieted(fmrx, 0, nch, n_streams=2, offsets=[s.offset_hz for s in stations]) as rx:
            want = rx.process_shared(iq[:24 * bb]).reshape(2, -1)
            reps = [rx.quiet_report(s) for s in range(2)]
        assert np.array_equal(pcm, want) and quiets == reps and quiets[0]["frames"] == 1
    plain = fmrx.decode_stations(iq)  # quiet=False: today's shape
    assert len(plain) == 2 and plain[1].shape == (2, 30 * 128)
    # the report comes last, behind every other product's
    out = fmrx.decode_stations(iq, channels=fmrx.STEREO, probe=True, blend=True, afc=True, quiet=True)
    assert len(out) == 6 and out[5][0].keys() == reps[0].keys() and "pulled_hz" in out[4][0]


def test_cli(fmrx):
    exe = os.path.join(os.path.dirname(fmrx.LIB_PATH), "bin", "fmrx")
    iq, bb = station(0, 12, (2, 80, 200)), oracle.MODES[0][0]
    data = iq[:(120 + 5) * bb]  # five granules and five blocks: the CLI's batches are a granule, the tail is held
    for args, nch in ((["0", "2", "--quiet"], 2), (["0", "1", "--quiet", "--mono-product"], 1)):
        r = subprocess.run([exe] + args, input=data.tobytes(), capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        with quieted(fmrx, 0, nch) as rx:
            head = rx.process(data[:120 * bb])
            rep = rx.quiet_report()
            rx.quiet_hold(True)
            want = np.concatenate([head, rx.process(data[120 * bb:])])
        assert r.stdout == want.tobytes(), args
        m = re.search(rb"^quiet cut=(\d\.\d\d) mute=(\d\.\d\d) frames=(\d+)$", r.stderr, re.M)
        assert m, r.stderr
        assert abs(float(m[1]) - rep["cut_mean"]) <= 0.005 + 1e-9 and abs(float(m[2]) - rep["mute_mean"]) <= 0.005 + 1e-9
        assert int(m[3]) == 5 and rep["cut_mean"] < 1.0
