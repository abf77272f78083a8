"""The RDS block sync on the GPU: the records, counts and structs it gives are compared for
equality with rds_sync_ref.py, the numpy restatement, never with a tolerance."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest
import torch

import rds_ref as R
import rds_sync_ref as S
from test_gpu_rds_decode import PI, PS, STATIONS, station_iq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()  # before the library's first HIP call, as the other device-pointer tests do


GRANULE_BITS = {0: 76, 3: 1520}          # bits an RDS granule: 24 blocks of mode 0, 1 block of mode 3
FULL_VOTE = 26 * (2 * S.J + 4)           # 520: past it some position has every neighbour inside the stream
_rows = {}


def rows(n):
    """Three streams of n bits: clean groups, the same with 1 % of the bits flipped, random bits."""
    if n not in _rows:
        clean = R.stream_bits(R.groups(PI, PS, "BLOCK SYNC TEST.", n // 104 + 1))[:n]
        rng = np.random.default_rng(11)
        _rows[n] = np.stack([clean, clean ^ (rng.random(n) < 0.01).astype(np.uint8),
                             rng.integers(0, 2, n).astype(np.uint8)])
        _rows[n].setflags(write=False)
    return _rows[n]


def whole(bits):
    return [S.blocks(b) for b in bits]


def fed(rx, bits, cuts, **cfg):
    """The records of the calls cut at `cuts` and of the flush behind them, a stream."""
    parts = [rx.rds_blocks(bits[:, a:b], **cfg) for a, b in zip((0,) + cuts, cuts + (bits.shape[1],))]
    parts.append(rx.rds_blocks_flush())
    return [np.concatenate([p[s] for p in parts]) for s in range(bits.shape[0])]


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def cases():
    out = []
    for mode, g in GRANULE_BITS.items():
        for n in sorted({g, (FULL_VOTE // g + 1) * g}):
            out.append((mode, n))
    return out


@pytest.mark.parametrize("mode,n", cases())
def test_blocks_equal_numpy_for_any_split(fmrx, mode, n):
    bits, g = rows(n), GRANULE_BITS[mode]
    want = whole(bits)
    if n > FULL_VOTE:
        assert want[0].size >= n // 26 - 1 and int(want[0]["votes"].max()) == 2 * S.J and want[2].size == 0
    k = n // g
    splits = [(), (max(k // 2, 1) * g,), (max(k // 3, 1) * g, max(2 * k // 3, 1) * g)] if k >= 3 else [(), (29,), (25, 51)]
    with fmrx.Receiver(mode, fmrx.MONO, n_streams=3) as rx:
        for cuts in splits:
            same(fed(rx, bits, cuts), want)
            rx.reset()
        # nothing is judged before its lookahead has come: a call alone gives the records below n - 26 J
        first = rx.rds_blocks(bits)
        same(first, [w[w["bit"] < n - 26 * S.J] for w in want])
        same([np.concatenate([a, b]) for a, b in zip(first, rx.rds_blocks_flush())], want)
        same(rx.rds_blocks_flush(), [w[:0] for w in want])  # nothing is pending twice


def test_one_bit_at_a_time_and_other_constants(fmrx):
    bits = rows(608)[:, :300]
    with fmrx.Receiver(0, fmrx.MONO, n_streams=3) as rx:
        same(fed(rx, bits, tuple(range(1, 300))), whole(bits))
        rx.reset()
        for cfg in ({"J": 3, "V": 2, "B": 5}, {"J": 1, "V": 1, "B": 0}, {"J": 8, "V": 16, "B": 1}):
            want = [S.blocks(b, cfg["J"], cfg["V"], cfg["B"]) for b in bits]
            same(fed(rx, bits, (77, 150), **cfg), want)
            with pytest.raises(fmrx.FmrxError) as e:  # other constants inside a stream
                rx.rds_blocks(bits[:, :10], J=2, V=2, B=2)
            assert e.value.code == fmrx.FMRX_EINVAL
            rx.reset()
        for bad in ({"J": 0}, {"J": 9}, {"V": 0}, {"V": 17}, {"B": -1}, {"B": 6}):
            with pytest.raises(fmrx.FmrxError) as e:
                rx.rds_blocks(bits[:, :10], **bad)
            assert e.value.code == fmrx.FMRX_EINVAL


def test_stream_shorter_than_a_word(fmrx):
    bits = rows(76)[:, :25]
    with fmrx.Receiver(0, fmrx.MONO, n_streams=3) as rx:
        same(rx.rds_blocks_flush(), [np.zeros(0, S.BLOCK)] * 3)  # before any bit
        same(fed(rx, bits, (0, 7)), [np.zeros(0, S.BLOCK)] * 3)


def test_host_and_device_forms_agree_and_reset(fmrx):
    bits = rows(608)
    want = whole(bits)
    cap = 5  # fewer rows than blocks: the list holds the first, the count says how many there were
    with fmrx.Receiver(0, fmrx.MONO, n_streams=3) as rx:
        host = rx.rds_blocks(bits)
        rx.reset()
        d_bits = torch.from_numpy(bits.copy()).cuda()
        d_blocks = torch.zeros(3 * 608 * 16, dtype=torch.uint8, device="cuda")
        d_small = torch.full((3 * cap * 16,), 0xEE, dtype=torch.uint8, device="cuda")
        d_counts = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        rx.rds_blocks_device(d_bits.data_ptr(), 608, d_blocks.data_ptr(), 608, d_counts.data_ptr())
        rx.synchronize()
        counts = d_counts.cpu().numpy()
        dev = d_blocks.cpu().numpy().view(S.BLOCK).reshape(3, 608)
        same([dev[s, : counts[s]] for s in range(3)], host)
        same([np.concatenate([h, f]) for h, f in zip(host, rx.rds_blocks_flush())], want)
        rx.reset()  # back to the start: the same call gives the first result again
        rx.rds_blocks_device(d_bits.data_ptr(), 608, d_small.data_ptr(), cap, d_counts.data_ptr())
        rx.synchronize()
        assert np.array_equal(d_counts.cpu().numpy(), counts) and counts[0] > cap
        small = d_small.cpu().numpy().view(S.BLOCK).reshape(3, cap)
        same([small[s, : min(cap, counts[s])] for s in range(3)], [h[:cap] for h in host])
        assert np.all(d_small.cpu().numpy().reshape(3, cap * 16)[2] == 0xEE)  # the random stream: nothing written
        rx.reset()
        same(rx.rds_blocks(bits), host)


def test_bursts_at_the_tables_extreme_shifts(fmrx):
    """Two flipped bits across a block boundary (the last bit of one block, the first of the next: a single
    error at either end of a word) and at bit 0 and bit 25 of one block (a burst of 26, beyond the table)."""
    grps = R.groups(PI, PS, None, 12)
    clean = R.stream_bits(grps)
    straddle, ends, pair_lo, pair_hi = clean.copy(), clean.copy(), clean.copy(), clean.copy()
    at = 104 * 5 + 26  # group 5's block B
    straddle[[at - 1, at]] ^= 1
    ends[[at, at + 25]] ^= 1
    pair_lo[[at, at + 1]] ^= 1      # the burst 11 at the word's highest shift
    pair_hi[[at + 24, at + 25]] ^= 1  # and at its lowest
    bits = np.stack([straddle, ends, pair_lo, pair_hi])
    want = whole(bits)
    sent = {104 * g + 26 * u + 25: (u, grp[u]) for g, grp in enumerate(grps) for u in range(4)}
    for s, w in enumerate(want):
        got = {int(r["bit"]): (int(r["slot"]), int(r["info"]), int(r["corrected"])) for r in w}
        for p, (u, info) in sent.items():
            hit = p in (at - 1, at + 25) if s == 0 else p == at + 25
            if s == 1 and hit:
                assert p not in got  # two errors 25 apart are no burst of <= 2
            else:
                assert got[p] == (u, info, int(hit)), (s, p)
    with fmrx.Receiver(0, fmrx.MONO, n_streams=4) as rx:
        same(fed(rx, bits, (600,)), want)


# ---- the switch ---------------------------------------------------------------------------------

GRANULES = 6  # the fewest of mode 0 at which the block sync has the whole PS name (the plain parser: "  DIO 42")
_want = {}


def reference(orc, iq):
    """(plain info, extended dict) of the oracle's demod of a u8 capture at offset 0."""
    key = iq.tobytes()
    if key not in _want:
        out = R.from_demod(orc, 0, orc.run(0, 51, iq, ["demod"])["demod"])
        _want[key] = (out["info"], S.parse_stream(out["bits"]))
    return _want[key]


def test_switch_equals_numpy_and_leaves_the_rest_alone(fmrx, orc):
    iq = R.to_u8(station_iq(granules=GRANULES))
    info, ext = reference(orc, iq)
    assert ext["ps"] == PS and ext["pi"] == PI and info["ps"] != PS and ext["corrected_blocks"] >= 1
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        rx.tune([0])
        rx.set_rds(True)
        off = rx.process(iq)
        assert rx.rds_info().as_dict() == info and rx.rds_ext().as_dict() == S.ext_dict(S.ext_init())
        rx.reset()
        rx.set_rds_sync(True)
        on = rx.process(iq)
        assert rx.rds_info().as_dict() == info
        rx.rds_blocks_flush()
        assert rx.rds_ext().as_dict() == ext
        rx.reset()  # clears the carry and the extended info, keeps the switch
        assert rx.rds_ext().as_dict() == S.ext_dict(S.ext_init())
        g = 2 * R.GRANULES[0] * 12800
        parts = np.concatenate([rx.process(iq[:g]), rx.process(iq[g:])])
        rx.rds_blocks_flush()
        assert rx.rds_ext().as_dict() == ext and rx.rds_info().as_dict() == info
        rx.reset()  # the sync switch without the RDS switch does nothing
        rx.set_rds(False)
        alone = rx.process(iq)
        rx.rds_blocks_flush()
        assert rx.rds_ext().as_dict() == S.ext_dict(S.ext_init())
    assert np.array_equal(on, off) and np.array_equal(parts, off) and np.array_equal(alone, off)


def test_switch_with_deemphasis_and_meter(fmrx, orc):
    iq = R.to_u8(station_iq(granules=GRANULES))
    info, ext = reference(orc, iq)
    with fmrx.Receiver(0, fmrx.STEREO) as rx:
        rx.tune([0])
        rx.set_rds(True)
        rx.set_deemphasis(50)
        rx.set_meter(True)
        off = rx.process(iq)
        report = bytes(rx.meter_report())
        rx.reset()
        rx.set_rds_sync(True)
        on = rx.process(iq)
        rx.rds_blocks_flush()
        assert rx.rds_ext().as_dict() == ext and rx.rds_info().as_dict() == info
        assert bytes(rx.meter_report()) == report
    assert np.array_equal(on, off)


def test_two_stations_shared_and_decode_stations(fmrx):
    iq = R.to_u8(sum(station_iq(off, pi, ps, seed=k) for k, (off, pi, ps) in enumerate(STATIONS)), amp=55.0, noise_lsb=2.0)
    with fmrx.Receiver(0, fmrx.MONO, n_streams=2) as rx:
        rx.tune([s[0] for s in STATIONS])
        rx.set_rds(True)
        off = rx.process_shared(iq)
        plain = [rx.rds_info(k).as_dict() for k in range(2)]
        rx.reset()
        rx.set_rds_sync(True)
        on = rx.process_shared(iq)
        assert [rx.rds_info(k).as_dict() for k in range(2)] == plain
        rx.rds_blocks_flush()
        exts = [rx.rds_ext(k).as_dict() for k in range(2)]
    assert np.array_equal(on, off)
    for x, p, (_, pi, ps) in zip(exts, plain, STATIONS):
        assert (x["pi"], x["ps"], x["bits"]) == (pi, ps, p["bits"])
        assert x["groups"] + x["partial_groups"] >= p["groups"] >= 12 and x["exact_blocks"] >= 4 * p["groups"]
    stations, pcm, named = fmrx.decode_stations(iq, rds=True, rds_sync=True)
    assert [s.offset_hz for s in stations] == [s[0] for s in STATIONS]
    assert named == exts and np.array_equal(pcm, off)
    assert fmrx.decode_stations(iq, rds=True)[2] == plain  # without it, as before
    with pytest.raises(ValueError):
        fmrx.decode_stations(iq, rds_sync=True)


def test_cli_prints_the_extended_line(fmrx, orc):
    iq = R.to_u8(station_iq(granules=GRANULES))
    info, ext = reference(orc, iq)
    exe = os.path.join(os.path.dirname(fmrx.LIB_PATH), "bin", "fmrx")
    data = iq.tobytes()
    plain = subprocess.run([exe, "0", "1", "--rds"], input=data, capture_output=True, timeout=120)
    r = subprocess.run([exe, "0", "1", "--rds", "--rds-sync"], input=data, capture_output=True, timeout=120)
    assert r.returncode == 0 and plain.returncode == 0, r.stderr.decode()
    lines = r.stderr.decode().splitlines()
    first = 'rds pi=%04X pty=5 ps="%s" groups=%d' % (PI, info["ps"], info["groups"])
    second = 'rdsx pi=%04X pty=5 ps="%s" ct=- af=0 blocks=%d+%d groups=%d+%d' % (
        PI, PS, ext["exact_blocks"], ext["corrected_blocks"], ext["groups"], ext["partial_groups"])
    assert first in lines and lines.index(second) == lines.index(first) + 1, r.stderr.decode()
    assert r.stdout == plain.stdout and b"rdsx" not in plain.stderr
    alone = subprocess.run([exe, "0", "1", "--rds-sync"], input=b"", capture_output=True, timeout=120)
    assert alone.returncode == 1 and b"--rds-sync" in alone.stderr and alone.stdout == b""
