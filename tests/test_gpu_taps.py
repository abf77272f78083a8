"""The taps on the demod rows of a tuned call, together (csrc/front.cpp: check_taps, taps_enqueue, taps_finish): the
subcarrier meter, soft stereo with de-emphasis behind it, the RDS decode with its block sync and the AFC
carrier sums, in every mode, on MONO and STEREO contexts, through process, process_shared and process_wide,
in one call, a granule at a time and small / large / small, on up to 130 streams.  Every report and every PCM
sample is compared for equality with tests/taps_ref.py, the composed reference over the oracle and the numpy
restatements; nothing is compared with a tolerance and no expected value comes from the library except its
design tables.  tests/test_taps_host.py checks, without a GPU, that the inputs are long enough to show a wrong
kernel and that MATRIX_CASES names every compiled meter and carrier kernel."""
from __future__ import annotations

import numpy as np
import pytest

import blend_ref as B
import meter_ref as M
import oracle
import rds_ref as R
import rds_sync_ref as S
import taps_ref as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()  # before the library's first HIP call, as the other device-pointer tests do


# 3a's matrix: (mode, channels, granules).  Modes 2 and 3: one granule, and two for the split (1, 1).
# tests/test_taps_host.py holds this list to the library's meter_kernel<NI> and carrier_kernel<NI>.
MATRIX_CASES = [(mode, ch, g) for mode, sizes in ((0, (6,)), (1, (24,)), (2, (1, 2)), (3, (1, 2)))
                for ch in ("MONO", "STEREO") for g in sizes]
ALONE_MODES = (1, 3)      # 3b: P = 288 and 256
STREAM_CASES = [(0, 70), (0, 130), (3, 5)]  # 3d: (mode, n_streams)


def matrix_windows(cases=None):
    """NI = P / 16 of the meter and carrier kernels each switch-path case of the matrix launches."""
    return {M.window(mode) // 16 for mode, _, _ in (MATRIX_CASES if cases is None else cases)}


def bits_eq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def switch_on(rx, switches, order=T.SWITCHES):
    """The switches in `order`; AFC measures only (tracking retunes: test_gpu_afc.py has it)."""
    setters = {"meter": lambda: rx.set_meter(True), "rds": lambda: rx.set_rds(True), "sync": lambda: rx.set_rds_sync(True),
               "afc": lambda: rx.set_afc(True, track=0), "blend": lambda: rx.set_stereo_blend(True),
               "deemph": lambda: rx.set_deemphasis(T.TAU)}
    for name in order:
        if name in switches:
            setters[name]()


def receiver(fm, mode, stereo, switches, n_streams=1, order=T.SWITCHES):
    rx = fm.Receiver(mode, fm.STEREO if stereo else fm.MONO, n_streams=n_streams)
    rx.tune([0] * n_streams)
    switch_on(rx, switches, order)
    return rx


def reports(fm, rx, stereo, s=0):
    """Everything the taps report of stream s (after rds_blocks_flush), in taps_ref's shapes."""
    rep, st = rx.meter_report(s), rx.afc_status(s)
    return {"meter": (np.array(rep.sum, np.float64), int(rep.frames)),
            "detect": fm.meter_detect(rep) if rep.frames else None,
            "afc": (np.float64(st.total.sum), np.float64(st.total.sumsq), int(st.total.frames)),
            "moves": (st.retunes, st.decisions, st.refused, st.offset_hz - st.origin_hz),
            "rds": rx.rds_info(s).as_dict(), "ext": rx.rds_ext(s).as_dict(),
            "hist": rx.blend_report(s)["level_frames"] if stereo else [0] * 17}


def same_reports(got, want, label=""):
    assert got["meter"][1] == want["meter"][1] and bits_eq(got["meter"][0], want["meter"][0]), ("meter", label)
    assert got["detect"] == want["detect"], ("meter_detect", label)
    assert got["afc"][2] == want["afc"][2] and bits_eq(got["afc"][0], want["afc"][0]) and bits_eq(got["afc"][1], want["afc"][1]), ("afc", label)
    assert got["moves"] == (0, 0, 0, 0), ("afc moved", label)
    assert got["rds"] == want["rds"], ("rds_info", label)
    assert got["ext"] == want["ext"], ("rds_ext", label)
    assert got["hist"] == want["hist"], ("blend", label)


def entry_eq(a, b):
    """One entry of reports() against another, floats on their bits."""
    if isinstance(a, tuple):
        return a[-1] == b[-1] and all(bits_eq(x, y) for x, y in zip(a[:-1], b[:-1]))
    return a == b


def in_calls(fn, iq, per_block, calls):
    out, b = [], 0
    for nb in calls:
        out.append(fn(iq[..., b * per_block:(b + nb) * per_block]))
        b += nb
    assert b * per_block == iq.shape[-1]
    return np.concatenate(out, axis=-1)


# ---- 3a. every mode, both channel counts, all taps on, every call pattern -----------------------------------

@pytest.mark.parametrize("mode,channels,granules", MATRIX_CASES)
def test_all_taps_in_every_mode_and_call_pattern(fmrx, orc, mode, channels, granules):
    stereo = channels == "STEREO"
    sw = T.ALL_STEREO if stereo else T.ALL_MONO
    iq, bb = T.capture(mode, stereo, granules), oracle.MODES[mode][0]
    pats = T.patterns(mode, granules)
    if mode >= 2 and granules == 2:
        pats = pats[1:]  # the second granule is there for the split (1, 1) alone
    with receiver(fmrx, mode, stereo, sw) as rx:
        assert rx.rds_granule == B.BLOCKS[mode]
        for k, calls in enumerate(pats):
            if k:
                rx.reset()
            want = T.expected(orc, fmrx, mode, iq, calls, sw, stereo)
            got = in_calls(rx.process, iq, bb, calls)
            rx.rds_blocks_flush()
            same_reports(reports(fmrx, rx, stereo), want, calls)
            assert np.array_equal(got, want["pcm"]), calls
            if stereo:
                assert not np.array_equal(want["pcm"], want["pcm_off"])
            else:
                assert want["pcm"] is want["pcm_off"]  # MONO: the taps-off PCM of the same calls


# ---- 3b. each tap alone equals all together ------------------------------------------------------------------

ALONE = [("meter",), ("rds",), ("sync",), ("rds", "sync"), ("afc",), ("blend",), ("deemph",)]
MINE = {"meter": ("meter", "detect"), "rds": ("rds",), "sync": (), "afc": ("afc",), "blend": ("hist",), "deemph": ()}


@pytest.mark.parametrize("mode", ALONE_MODES)
def test_each_tap_alone_equals_all_together(fmrx, orc, mode):
    iq, nb = T.capture(mode, True), T.GRANULES[mode] * B.BLOCKS[mode]
    with receiver(fmrx, mode, True, T.ALL_STEREO) as rx:
        rx.process(iq)
        rx.rds_blocks_flush()
        together = reports(fmrx, rx, True)
    same_reports(together, T.expected(orc, fmrx, mode, iq, [nb], T.ALL_STEREO, True), "together")
    for sw in ALONE:
        want = T.expected(orc, fmrx, mode, iq, [nb], frozenset(sw), True)
        with receiver(fmrx, mode, True, sw) as rx:
            pcm = rx.process(iq)
            rx.rds_blocks_flush()
            got = reports(fmrx, rx, True)
        same_reports(got, want, sw)  # the tap's own report, and the power-on values of the others
        assert np.array_equal(pcm, want["pcm"]), sw
        own = {k for name in sw for k in MINE[name]} | ({"ext"} if set(sw) == {"rds", "sync"} else set())
        for k in own:  # bit for bit what it reported with every tap on
            assert entry_eq(got[k], together[k]), (sw, k)
        if sw == ("rds",):  # the decode without the sync leaves the extended info where it started
            assert got["ext"] == S.ext_dict(S.ext_init()) and got["rds"]["bits"] > 0
        if sw == ("sync",):  # the sync without the decode decodes nothing
            assert got["ext"] == S.ext_dict(S.ext_init()) and got["rds"]["bits"] == 0


# ---- 3c. the routes, in mode 1 ---------------------------------------------------------------------------------

ROUTE_GRANULES, ROUTE_CALLS = 12, (4, 8)
ROUTE_STATIONS = [(-250000, 0x1234, "LEFT  FM"), (200000, 0xC0DE, "RIGHT-42")]
RATE_FS = 2560000  # 9/20 of mode 1's rate: a wide granule of 3 blocks, an RDS granule of 24
_routes: dict = {}


def route_capture(kind):
    """ROUTE_GRANULES granules of mode 1 holding the two stations: u8 at the mode's rate ("shared"), s16 at twice
    it ("decim2") or u8 at RATE_FS ("rate")."""
    if kind not in _routes:
        fs = {"shared": None, "decim2": 2 * oracle.MODES[1][3], "rate": RATE_FS}[kind]
        secs = ROUTE_GRANULES * R.granule_samples(1) / R.bp_fs(1)
        n = int(round(secs * (fs or oracle.MODES[1][3])))
        z = sum(R.fm_signal(1, n, R.stream_bits(R.groups(pi, ps, None, R.n_groups_for(secs))), offset_hz=off, rf_fs=fs, seed=k)
                for k, (off, pi, ps) in enumerate(ROUTE_STATIONS))
        raw = R.to_s16(z, amp=6000.0, noise_lsb=100.0) if kind == "decim2" else R.to_u8(z, amp=55.0, noise_lsb=2.0)
        raw.setflags(write=False)
        _routes[kind] = raw
    return _routes[kind]


def route_compose(kind, raw, offset):
    """The oracle's demod and mono PCM of one station of a route's capture, as the route's own tests build them."""
    from test_formats_host import S16, U8
    if kind == "shared":
        from test_gpu_tuner import compose
        return compose(raw, 1, 51, offset)
    if kind == "decim2":
        from test_wide_host import wide_compose
        return wide_compose(raw, S16, 1, 51, 2, offset)
    from test_rate_host import rate_compose
    return rate_compose(raw, U8, 1, 51, RATE_FS, offset)


def route_receiver(fm, kind, switches):
    rx = fm.Receiver(1, fm.MONO, n_streams=2)
    offsets = [s[0] for s in ROUTE_STATIONS]
    if kind == "shared":
        rx.tune(offsets)
        call = rx.process_shared
    else:
        if kind == "decim2":
            rx.set_input_format(fm.IQ_S16)
            rx.set_capture_decim(2)
        else:
            rx.set_capture_rate(RATE_FS)
        rx.tune_wide(offsets)
        call = rx.process_wide
    switch_on(rx, switches)
    return rx, call


@pytest.mark.parametrize("kind", ["shared", "decim2", "rate"])
def test_routes_in_mode_1(fmrx, orc, kind):
    raw = route_capture(kind)
    g = B.BLOCKS[1]
    calls = [k * g for k in ROUTE_CALLS]
    per_granule = raw.size // ROUTE_GRANULES  # elements: at 9/20 a block is no whole number of wide pairs
    assert per_granule * ROUTE_GRANULES == raw.size
    rx, call = route_receiver(fmrx, kind, T.ALL_MONO)
    with rx:
        wide_blocks = 1 if kind == "shared" else rx.wide_granule[0]
        assert rx.rds_granule == g and wide_blocks == (3 if kind == "rate" else 1)
        got = in_calls(call, raw, per_granule, ROUTE_CALLS)
        rx.rds_blocks_flush()
        got_reports = [reports(fmrx, rx, False, s) for s in range(2)]
        if kind == "rate":  # whole wide granules that are no whole RDS granules: refused, nothing changed
            with pytest.raises(fmrx.FmrxError) as e:
                call(raw[: 2 * rx.wide_granule[1]])
            assert e.value.code == fmrx.FMRX_EINVAL and "granule" in str(e.value)
            after = [reports(fmrx, rx, False, s) for s in range(2)]
    for s, (off, pi, ps) in enumerate(ROUTE_STATIONS):
        o = route_compose(kind, raw, off)
        want = T.demod_reports(orc, fmrx, 1, o["demod"], calls, T.ALL_MONO)
        same_reports(got_reports[s], want, (kind, off))
        assert np.array_equal(got[s], o["pcm_mono"]), (kind, off)  # the taps-off PCM
        assert (want["rds"]["pi"], want["ext"]["pi"]) == (pi, pi) and want["ext"]["ps"] == ps and want["rds"]["groups"] >= 5
        assert want["detect"]["rds"] == 1 and want["afc"][2] == ROUTE_GRANULES
        if kind == "rate":
            same_reports(after[s], want, (kind, off, "after the refusal"))


# ---- 3d. more streams than a wave --------------------------------------------------------------------------------

STREAM_GRANULES = {0: 4, 3: 1}  # mode 0: the fewest at which the reference decodes every stream's own PI
SIGMAS, PILOTS = (2, 4, 6, 8), (0.05, 0.02, 0.01, 0.005)


def stream_pi(s):
    return 0x1000 + s


def stream_capture(mode, s):
    """Stream s: its own seed, PI, noise and pilot level (so soft stereo's levels differ from stream to stream while
    the RDS decodes in every one); every fifth stream without pilot and RDS."""
    bare = s % 5 == 4
    return T.station(mode, STREAM_GRANULES[mode] * B.GM[mode], (SIGMAS[(s // 4) % 4],), pilot=0.0 if bare else PILOTS[s % 4],
                     seed=100 + s, pi=stream_pi(s), ps="STN %04d" % s, rds=0.0 if bare else 0.04)


@pytest.mark.parametrize("mode,n_streams", STREAM_CASES)
def test_more_streams_than_a_wave(fmrx, orc, mode, n_streams):
    """Meter, RDS, sync, AFC and soft stereo on per-stream rows.  Every stream's reports equal its own
    single-stream reference, built from the oracle's demod of its row.  The PCM is compared, with the full stereo
    reference, for a sample of the streams: the first, 63, 64, the last and the ones without pilot (all five in
    mode 3); for the rest the reports alone are asserted.  Mode 0 runs four granules, not one: at one granule
    (76 bits) no stream's RDS info holds anything of its own, and a kernel reading another stream's mixer, symbol
    or state row would pass; at four the reference has every stream's PI, from the plain parser and from the block
    sync, and the test asserts that it does.  (The references are the slow side: 0.1 to 0.2 s of CPU a stream, shared by the two mode-0 cases.)"""
    sw = frozenset(("meter", "rds", "sync", "afc", "blend"))
    nb = STREAM_GRANULES[mode] * B.BLOCKS[mode]
    iq = np.stack([stream_capture(mode, s) for s in range(n_streams)])
    with receiver(fmrx, mode, True, sw, n_streams=n_streams) as rx:
        pcm = rx.process(iq)
        rx.rds_blocks_flush()
        got = [reports(fmrx, rx, True, s) for s in range(n_streams)]
    sample = {0, 63, 64, n_streams - 1} | {s for s in range(n_streams) if s % 5 == 4 or mode == 3}
    seen, hists = set(), set()
    for s in range(n_streams):
        if s in sample:
            want = T.expected(orc, fmrx, mode, iq[s], [nb], sw, True)
            assert np.array_equal(pcm[s], want["pcm"]), s
        else:
            want = T.demod_reports(orc, fmrx, mode, T.oracle_demod(orc, mode, iq[s]), [nb], sw)
        same_reports(got[s], want, s)
        seen.add((want["meter"][0].tobytes(), want["afc"][0].tobytes()))
        hists.add(tuple(want["hist"]))
        if s % 5 == 4:
            assert want["detect"]["stereo"] == 0 and (want["rds"]["pi"], want["ext"]["pi"]) == (0, None)
        else:  # the stream's own PI, from both parsers: an RDS row read at another stream's stride shows
            assert (want["rds"]["pi"], want["ext"]["pi"]) == (stream_pi(s), stream_pi(s)) and want["rds"]["groups"] >= 1, s
    assert len(seen) == n_streams  # every stream's reports its own: a row read at another stream's stride shows
    assert len(hists) >= 3


# ---- 3e. reset and order ---------------------------------------------------------------------------------------------

def test_reset_and_switch_order(fmrx, orc):
    mode, sw = 1, T.ALL_STEREO
    iq, bb = T.capture(mode, True), oracle.MODES[mode][0]
    calls = [6 * 24, 18 * 24]
    want = T.expected(orc, fmrx, mode, iq, calls, sw, True)
    seen = []
    for order in (T.SWITCHES, T.SWITCHES[::-1]):
        with receiver(fmrx, mode, True, sw, order=order) as rx:
            for again in range(2 if order is T.SWITCHES else 1):
                if again:
                    rx.reset()  # the same calls give the same reports
                pcm = in_calls(rx.process, iq, bb, calls)
                rx.rds_blocks_flush()
                got = reports(fmrx, rx, True)
                same_reports(got, want, (order, again))
                assert np.array_equal(pcm, want["pcm"]), (order, again)
                seen.append((bytes(rx.meter_report()), bytes(rx.afc_status()), bytes(rx.rds_info()), bytes(rx.rds_ext()), got["hist"]))
    assert seen[0] == seen[1] == seen[2]


def test_a_tap_switched_between_calls_clears_its_own_report(fmrx, orc):
    """include/fmrx.h: fmrx_set_afc with on != 0 clears the AFC reports; fmrx_set_stereo_blend, with any value, clears
    soft stereo's carry and reports.  Neither touches the meter, the RDS info or the extended info, which go on
    over both calls.  (No rule is documented for fmrx_set_meter, fmrx_set_rds or fmrx_set_rds_sync: none is
    asserted.)"""
    mode, sw = 1, frozenset(("meter", "rds", "sync", "afc", "blend"))
    iq, bb = T.capture(mode, True), oracle.MODES[mode][0]
    calls = [4 * 24, 20 * 24]  # cut where the level carried across is 16, not 0
    cut, na = calls[0] * oracle.MODES[mode][1], calls[0] * oracle.MODES[mode][2]
    whole = T.expected(orc, fmrx, mode, iq, calls, sw, True)
    o = T.oracle_run(orc, mode, iq, True)
    second = T.demod_reports(orc, fmrx, mode, o["demod"][cut:], calls[1:], frozenset(("afc", "blend")))
    first = T.demod_reports(orc, fmrx, mode, o["demod"][:cut], calls[:1], frozenset(("blend",)))
    y = np.stack([o["right"], o["left"]], axis=1)
    want_pcm = B.quant(orc, np.concatenate([B.apply(mode, y[:na], first["row"]), B.apply(mode, y[na:], second["row"])]))
    assert second["hist"] != whole["hist"] and int(first["row"][-1]) != 0  # the carry was not empty when it was cleared
    with receiver(fmrx, mode, True, sw) as rx:
        a = rx.process(iq[: calls[0] * bb])
        rx.set_afc(True, track=0)
        rx.set_stereo_blend(False)
        rx.set_stereo_blend(True)
        assert rx.afc_status().total.frames == 0 and rx.blend_report()["frames"] == 0
        assert rx.meter_report().frames == 4 and rx.rds_info().as_dict()["bits"] == 4 * 76
        b = rx.process(iq[calls[0] * bb:])
        rx.rds_blocks_flush()
        got = reports(fmrx, rx, True)
    same_reports(got, dict(whole, afc=second["afc"], hist=second["hist"]), "switched")
    assert np.array_equal(np.concatenate([a, b]), want_pcm)
