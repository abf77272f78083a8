"""The RDS back half on the GPU: everything it writes is compared for equality with
rds_ref.py, the numpy restatement over the oracle's front half and the reference's resample."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import oracle
import rds_ref as R
from conftest import load_rds

pytestmark = pytest.mark.gpu

PI, PS, RT = 0x54A8, "RADIO 42", "HELLO FROM THE GPU RDS DECODER. "
STATIONS = [(-400000, 0x1234, "LEFT  FM"), (400000, 0xC0DE, "RIGHT-42")]  # 800 kHz apart
IQ_GRANULES = 24  # of mode 0: 1.536 s, 17 groups


def _blocks(mode, secs):
    return int(secs * R.bp_fs(mode)) // R.granule_samples(mode) * R.GRANULES[mode]


# (mode, blocks): 3 s in modes 0 and 1, 6 blocks (2 granules) in mode 2, 2 blocks in mode 3
CASES = {0: _blocks(0, 3.0), 1: _blocks(1, 3.0), 2: 6, 3: 2}
_mix, _ref = {}, {}


def mix_of(orc, mode, n_blocks, seed=3, **kw):
    """The oracle's mixer rows of the test transmitter's signal; computed once, left unchanged."""
    key = (mode, n_blocks, seed, tuple(sorted(kw.items())))
    if key not in _mix:
        n = n_blocks * oracle.MODES[mode][1]
        bits = R.stream_bits(R.groups(PI + seed, PS, RT, R.n_groups_for(n / R.bp_fs(mode))))
        _mix[key] = orc.rds(mode, R.make_demod(mode, n, bits, seed=seed, **kw))["rds"]
        _ref[key] = R.back_half(orc, mode, _mix[key])
    return _mix[key], _ref[key]


def same(got, want):
    for k in ("bits", "codes", "win"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_y_bits_codes_and_windows(fmrx, orc, mode):
    mix, want = mix_of(orc, mode, CASES[mode])
    with fmrx.Receiver(mode, fmrx.MONO) as rx:
        assert rx.rds_granule == R.GRANULES[mode]
        got = rx.rds_bits(mix, want_y=True)
    assert np.array_equal(got["y"].view(np.uint32), want["y"].view(np.uint32)), "y differs from oracle.resample"
    same(got, want)
    if mode < 2:  # 3 s: the codes carry groups
        assert R.parse(got["bits"], got["codes"])["groups"] >= 30


def test_three_streams_with_clock_errors(fmrx, orc):
    """+100, -100 and 0 ppm over 10 s: the sampling phase wraps, and the GPU follows the reference through it."""
    nb = _blocks(0, 10.0)
    rows = [mix_of(orc, 0, nb, seed=s, noise=0.02, ppm=ppm) for s, ppm in ((5, 100.0), (6, -100.0), (7, 0.0))]
    with fmrx.Receiver(0, fmrx.MONO, n_streams=3) as rx:
        got = rx.rds_bits(np.stack([m for m, _ in rows]))
    wraps = 0
    for s, (_, want) in enumerate(rows):
        same({k: got[k][s] for k in ("bits", "codes", "win")}, want)
        wraps += int(np.sum(np.abs(np.diff(got["win"][s][:, 0].astype(int))) > 8))
    assert wraps >= 1, "no phase wrap seen"


@pytest.mark.parametrize("mode", [0, 2])
def test_granule_at_a_time_and_reset(fmrx, orc, mode):
    mix, want = mix_of(orc, mode, CASES[mode])
    g = R.granule_samples(mode)
    with fmrx.Receiver(mode, fmrx.MONO) as rx:
        parts = [rx.rds_bits(mix[k: k + g], want_y=True) for k in range(0, mix.size, g)]
        cat = {k: np.concatenate([p[k] for p in parts]) for k in ("y", "bits", "codes", "win")}
        assert np.array_equal(cat["y"].view(np.uint32), want["y"].view(np.uint32))
        same(cat, want)
        rx.reset()  # back to the start: the same call gives the first result again
        same(rx.rds_bits(mix), want)


def test_state_carries_without_reset(fmrx, orc):
    """Two calls without a reset continue the stream (the second differs from a fresh start's)."""
    mix, want = mix_of(orc, 0, CASES[0])
    half = mix.size // R.granule_samples(0) // 2 * R.granule_samples(0)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        a, b = rx.rds_bits(mix[:half]), rx.rds_bits(mix[half:])
        fresh = R.back_half(oracle.Oracle(), 0, mix[half:])
    same({k: np.concatenate([a[k], b[k]]) for k in ("bits", "codes", "win")}, want)
    assert not np.array_equal(b["bits"], fresh["bits"])


def test_non_granule_call_is_refused(fmrx):
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        x = np.zeros(23 * 640, np.float32)
        with pytest.raises(fmrx.FmrxError) as e:
            rx.rds_bits(x)
        assert e.value.code == fmrx.FMRX_EINVAL and "granule" in str(e.value)
        with pytest.raises(fmrx.FmrxError) as e:
            rx.rds_decode(x)
        assert e.value.code == fmrx.FMRX_EINVAL
        rx.tune([0])
        rx.set_rds(True)
        with pytest.raises(fmrx.FmrxError) as e:
            rx.process(np.full(23 * 12800, 128, np.uint8))
        assert e.value.code == fmrx.FMRX_EINVAL and "granule" in str(e.value)
        rx.set_rds(False)
        assert rx.process(np.full(23 * 12800, 128, np.uint8)).size == 23 * 128


def test_decode_of_the_random_bit_fixture(fmrx, orc):
    """tests/golden/rds_m0_rds57.npz: random bits without checkwords, one whole granule: no group,
    and the reference's codes and counters."""
    z = load_rds("m0_rds57")
    demod = z["demod"]
    assert z["mode"] == 0 and demod.size == R.granule_samples(0)
    want = R.from_demod(orc, 0, demod)
    assert want["info"]["groups"] == 0
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        rx.rds_decode(demod)
        assert rx.rds_info().as_dict() == want["info"]
        rx.reset()
        got = rx.rds_bits(rx.rds_block(demod)["rds"])
    same(got, want)


_iq = {}


def station_iq(offset=0.0, pi=PI, ps=PS, granules=IQ_GRANULES, rf_fs=None, seed=1):
    key = (offset, pi, ps, granules, rf_fs, seed)
    if key not in _iq:
        secs = granules * R.granule_samples(0) / R.bp_fs(0)
        bits = R.stream_bits(R.groups(pi, ps, None, R.n_groups_for(secs)))
        fs = rf_fs or oracle.MODES[0][3]
        _iq[key] = R.fm_signal(0, int(round(secs * fs)), bits, offset_hz=offset, rf_fs=rf_fs, seed=seed)
    return _iq[key]


@pytest.mark.parametrize("channels", ["MONO", "STEREO"])
def test_process_with_rds_on_equals_the_reference(fmrx, orc, channels):
    """u8 I/Q at offset 0: the oracle's demod through the reference, against set_rds(1) + tuned process."""
    iq = R.to_u8(station_iq())
    want = R.from_demod(orc, 0, orc.run(0, 51, iq, ["demod"])["demod"])["info"]
    assert (want["pi"], want["ps"]) == (PI, PS) and want["groups"] >= 15
    ch = getattr(fmrx, channels)
    with fmrx.Receiver(0, ch) as rx:
        rx.tune([0])
        off = rx.process(iq)
        assert rx.rds_info().as_dict()["bits"] == 0  # off: nothing decoded
        rx.reset()
        rx.set_rds(True)
        on = rx.process(iq)
        assert rx.rds_info().as_dict() == want
        rx.reset()  # clears the info, keeps the switch
        g = IQ_GRANULES // 2 * R.GRANULES[0] * 12800
        parts = np.concatenate([rx.process(iq[:g]), rx.process(iq[g:])])
        assert rx.rds_info().as_dict() == want
    assert np.array_equal(on, off) and np.array_equal(parts, off)


def test_two_stations_shared_and_decode_stations(fmrx):
    iq = R.to_u8(sum(station_iq(off, pi, ps, seed=k) for k, (off, pi, ps) in enumerate(STATIONS)), amp=55.0, noise_lsb=2.0)
    with fmrx.Receiver(0, fmrx.MONO, n_streams=2) as rx:
        rx.tune([s[0] for s in STATIONS])
        rx.set_rds(True)
        pcm = rx.process_shared(iq)
        infos = [rx.rds_info(k).as_dict() for k in range(2)]
    for info, (_, pi, ps) in zip(infos, STATIONS):
        assert (info["pi"], info["ps"]) == (pi, ps) and info["groups"] >= 12
    stations, pcm2, named = fmrx.decode_stations(iq, rds=True)
    assert [s.offset_hz for s in stations] == [s[0] for s in STATIONS]
    assert named == infos and np.array_equal(pcm2, pcm)


def test_two_stations_wide_s16(fmrx):
    """The same through process_wide: a capture at 4 x the mode's rate in s16."""
    fs = 4 * oracle.MODES[0][3]
    z = sum(station_iq(off, pi, ps, granules=12, rf_fs=fs, seed=k) for k, (off, pi, ps) in enumerate(STATIONS))
    iq = R.to_s16(z, amp=6000.0, noise_lsb=100.0)
    with fmrx.Receiver(0, fmrx.MONO, n_streams=2) as rx:
        rx.set_input_format(fmrx.IQ_S16)
        rx.set_capture_decim(4)
        rx.tune_wide([s[0] for s in STATIONS])
        off = rx.process_wide(iq)
        rx.reset()
        rx.set_rds(True)
        on = rx.process_wide(iq)
        infos = [rx.rds_info(k).as_dict() for k in range(2)]
    assert np.array_equal(on, off)
    for info, (_, pi, ps) in zip(infos, STATIONS):
        assert (info["pi"], info["ps"]) == (pi, ps) and info["groups"] >= 6


def test_granule_with_a_capture_rate(fmrx):
    """On a context with a capture rate set: the least common multiple with the wide granule's blocks."""
    for mode, cap_fs, wide_blocks, want in ((0, 10000000, 3, 24), (2, 6000000, 1, 3)):
        with fmrx.Receiver(mode, fmrx.MONO) as rx:
            rx.set_capture_rate(cap_fs)
            assert rx.wide_granule[0] == wide_blocks and rx.rds_granule == want


def test_rate_capture_10ms(fmrx):
    """One station in a u8 capture at 10 MS/s (6/25): named through the rational down-converter, PCM unchanged."""
    iq = R.to_u8(station_iq(granules=12, rf_fs=10000000), noise_lsb=2.0)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        rx.set_capture_rate(10000000)
        rx.tune_wide([0])
        off = rx.process_wide(iq)
        rx.reset()
        rx.set_rds(True)
        on = rx.process_wide(iq)
        info = rx.rds_info().as_dict()
        with pytest.raises(fmrx.FmrxError) as e:  # whole wide granules (3 blocks), not whole RDS granules
            rx.process_wide(iq[: 2 * 80000 * 5])
        assert e.value.code == fmrx.FMRX_EINVAL and "granule" in str(e.value)
    assert on.size == 12 * 24 * 128 and np.array_equal(on, off)
    assert (info["pi"], info["ps"]) == (PI, PS) and info["groups"] >= 6


def test_cli_prints_the_station(fmrx, orc):
    iq = R.to_u8(station_iq())
    want = R.from_demod(orc, 0, orc.run(0, 51, iq, ["demod"])["demod"])["info"]
    exe = os.path.join(os.path.dirname(fmrx.LIB_PATH), "bin", "fmrx")
    data = iq.tobytes() + bytes([128]) * (5 * 12800)  # five blocks past the last whole granule
    plain = subprocess.run([exe, "0", "1"], input=data, capture_output=True, timeout=120)
    r = subprocess.run([exe, "0", "1", "--rds"], input=data, capture_output=True, timeout=120)
    assert r.returncode == 0 and plain.returncode == 0, r.stderr.decode()
    line = 'rds pi=%04X pty=5 ps="%s" groups=%d' % (PI, PS, want["groups"])
    assert line in r.stderr.decode().splitlines(), r.stderr.decode()
    assert r.stdout == plain.stdout and len(r.stdout) == (IQ_GRANULES * 24 + 5) * 128 * 2 * 2
    assert b"rds pi=" not in plain.stderr


# ---- edge inputs: the decisions a real signal never reaches ---------------------------------------------------

EDGE_GRANULES = 2  # of mode 0: two windows, so the carried sign, chip and tail see the edges too


def edge_rows(orc, which):
    """Three streams of constructed mixer rows of mode 0, one edge a stream.  "flat": all zeros (the phase
    histogram ties at bin 0, p = 8; the pairing vote ties, q = 0), all -0.0, a constant negative row.  "mixed":
    denormals of both signs; the transmitter's row with one NaN inside the second window; impulses of both
    signs so far apart that y is exactly 0.0f between them."""
    n = EDGE_GRANULES * R.granule_samples(0)
    if which == "flat":
        return np.stack([np.zeros(n, np.float32), np.full(n, -0.0, np.float32), np.full(n, -0.25, np.float32)])
    tiny = np.float32(1e-41) * np.where((np.arange(n) // 37) % 2 == 0, 1, -1).astype(np.float32)
    nan = mix_of(orc, 0, EDGE_GRANULES * R.GRANULES[0])[0].copy()
    nan[R.granule_samples(0) + 5000] = np.nan
    sparse = np.zeros(n, np.float32)
    sparse[200::400] = np.where(np.arange(sparse[200::400].size) % 2 == 0, 1.0, -1.0).astype(np.float32)
    return np.stack([tiny, nan, sparse])


def same_edges(got, want, s, y=True):
    """Stream s of a result against its reference: bits, codes and windows equal; y on the bits wherever the
    reference is a number, and a NaN wherever it is not (NaN >= 0 is false on both sides)."""
    same({k: got[k][s] for k in ("bits", "codes", "win")}, want)
    if y:
        keep = ~np.isnan(want["y"])
        assert np.array_equal(np.isnan(got["y"][s]), ~keep), s
        assert np.array_equal(got["y"][s][keep].view(np.uint32), want["y"][keep].view(np.uint32)), s


@pytest.mark.parametrize("which", ["flat", "mixed"])
def test_rds_bits_edge_rows(fmrx, orc, which):
    rows = edge_rows(orc, which)
    want = [R.back_half(orc, 0, r) for r in rows]
    if which == "flat":
        assert want[0]["win"].tolist() == want[1]["win"].tolist() == [[8, 0], [8, 0]]  # both ties, both windows
        assert int(want[0]["bits"].sum()) == 1 and not want[0]["codes"].any() and np.all(want[2]["y"][R.WIN:] < 0)
        assert np.all(want[1]["y"] == 0)
    else:
        y0, y1, y2 = (w["y"] for w in want)
        tiny = np.finfo(np.float32).tiny
        assert np.any((y0 > 0) & (y0 < tiny)) and np.any((y0 < 0) & (y0 > -tiny)) and np.all(np.abs(y0) < tiny)
        bad = np.flatnonzero(np.isnan(y1))
        assert bad.size and bad.min() >= R.WIN and np.isfinite(y1[: R.WIN]).all()  # inside the second window
        assert np.any(y2 == 0) and np.any(y2 > 0) and np.any(y2 < 0) and np.isfinite(y2).all()
        sign = np.sign(y2[y2 != 0])
        assert np.any((y2[1:-1] == 0) & (y2[:-2] != 0)) and np.any(sign[1:] != sign[:-1])  # exact zeros between signed samples
    g = R.granule_samples(0)
    with fmrx.Receiver(0, fmrx.MONO, n_streams=3) as rx:
        got = rx.rds_bits(rows, want_y=True)
        for s in range(3):
            same_edges(got, want[s], s)
        rx.reset()  # the same rows a granule at a time: the carried bytes and the tail see the edges
        parts = [rx.rds_bits(rows[:, k: k + g], want_y=True) for k in range(0, rows.shape[1], g)]
        cat = {k: np.concatenate([p[k] for p in parts], axis=1) for k in ("y", "bits", "codes", "win")}
        for s in range(3):
            same_edges(cat, want[s], s)


def front_edge_rows(n_blocks):
    """test_gpu_stereo_variants' special values in the demod of mode 0 (stereo_ref.special_demod: denormals of both
    signs, a run of -0.0, the smallest normals, +-1e30), the same with the other sign, and the same with +-1e18
    in place of +-1e30."""
    from stereo_ref import special_demod
    a = special_demod(0, n_blocks)
    c = a.copy()
    c[np.abs(c) == np.float32(1e30)] *= np.float32(1e-12)
    return np.stack([a, -a, c])


def test_rds_block_edge_rows(fmrx, orc):
    """The front half on denormals, signed zeros and huge samples.  The channel is compared over the whole row.
    +-1e30 squares to Inf in front of the 114 kHz PLL, whose outputs are NaN from there on: NaN and Inf through
    that PLL are test_pll_demoted_special_values' subject, so nco and rds of those two streams are compared up
    to the first sample the reference does not give as a number (behind every other special value), and over
    the whole row on the stream whose largest samples, +-1e18, stay finite when squared."""
    nb = R.GRANULES[0]
    rows = front_edge_rows(nb)
    want = [orc.rds(0, r) for r in rows]
    with fmrx.Receiver(0, fmrx.MONO, n_streams=3) as rx:
        got = rx.rds_block(rows, want_nco=True, want_channel=True)
    nif = oracle.MODES[0][1]
    for s in range(3):
        assert np.isfinite(want[s]["channel"]).all()
        assert np.array_equal(got["channel"][s].view(np.uint32), want[s]["channel"].view(np.uint32)), s
        ok = np.isfinite(want[s]["nco"]) & np.isfinite(want[s]["rds"])
        end = ok.size if ok.all() else int(np.flatnonzero(~ok)[0])
        if s == 2:
            assert end == ok.size
        else:  # every other special value lies in front of the first sample that is no number
            assert nif + 200 + 32 + 120 + 32 + 20 <= end < ok.size, (s, end)
        for k in ("nco", "rds"):
            assert np.array_equal(got[k][s][:end].view(np.uint32), want[s][k][:end].view(np.uint32)), (s, k)
