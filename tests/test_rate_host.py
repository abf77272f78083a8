"""CPU tests of captures at a rational rate (fmrx_rate_design, fmrx_scan_detect_rate; host only): the
reduction cap_fs -> L / M, the refusals, the split and the coarse rotator at the capture rate, the
low-pass and its response, a numpy emulation of the kernel's staging, layout and history copy, and --
with the pinned oracle alone -- what the definition costs in audio quality.  rate_compose() is the
expected output of the GPU path; tests/test_gpu_rate.py compares the kernels with it bit for bit."""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np
import pytest

import iqgen
import oracle
from test_formats_host import F32, S16, U8, normalise
from test_gpu_rate_sweep import RATE_SWEEP, sweep_ratio
from test_wide_host import (Q_BLOCKS, Q_D, Q_MODE, Q_SCAN, Q_SKIP, Q_STATIONS, _orc, as_complex, narrow_compose,
                            narrow_station, peak_correlation, two_station_capture, welch64, wide_compose)

# (rf_fs, cap_fs, L, M): the 13 designs of the response test
DESIGNS = [
    (2400000, 10000000, 6, 25), (2400000, 8000000, 3, 10), (2400000, 20000000, 3, 25), (2400000, 2500000, 24, 25),
    (2400000, 12500000, 24, 125), (2400000, 2560000, 15, 16), (2400000, 6000000, 2, 5),
    (1152000, 2048000, 9, 16), (1152000, 8000000, 18, 125), (1152000, 2400000, 12, 25),
    (2304000, 2560000, 9, 10), (2304000, 8000000, 36, 125), (2304000, 6000000, 48, 125),
]


# ---- the ratio ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("rf_fs,cap_fs,up,down", DESIGNS + [(2400000, 16000000, 3, 20), (2400000, 3200000, 3, 4),
                                                            (2400000, 3000000, 4, 5), (2400000, 4800000, 1, 2),
                                                            (2400000, 24000000, 1, 10)])
def test_reduction(fmrx, rf_fs, cap_fs, up, down):
    d = fmrx.rate_design(rf_fs, cap_fs, 0)
    assert (d["up"], d["down"]) == (up, down) and up * cap_fs == down * rf_fs and math.gcd(up, down) == 1
    if up == 1:  # an integer ratio answers as the wide design does
        w = fmrx.wide_design(rf_fs, down, 0)
        assert np.array_equal(d["h"], w["h"]) and d["N"] == w["N"]
    else:
        assert d["h"].shape == (16 * down + 1,) and d["table"].tolist() == [[1.0, 0.0]]


def test_integer_design_is_the_rational_design_at_up_1(fmrx):
    """fmrx_rate_design(rf_fs, D rf_fs, f) against fmrx_wide_design(rf_fs, D, f) for every D, the modes'
    three rates and every f on a 25 kHz raster inside (-cap_fs / 2, cap_fs / 2), with the edges +-cap_fs / 2
    and +-(cap_fs / 2 - 1): the same code; accepted, the same 1 / D, split, period, step, table and taps;
    refused, no output written by either.  The taps depend on (rf_fs, D) alone: compared once each."""
    lib = fmrx.lib()
    accepted = refused = 0
    for rf_fs in sorted({m[3] for m in oracle.MODES.values()}):
        for d in range(2, 11):
            cap_fs, half = d * rf_fs, d * rf_fs // 2
            raster = range(-((half - 1) // 25000) * 25000, half, 25000)
            first = True
            for f in [-half, -(half - 1), *raster, half - 1, half]:
                rv, wv = [C.c_int(-7) for _ in range(7)], [C.c_int(-7) for _ in range(5)]
                rt, wt = np.full(80, 9.0, np.float32), np.full(80, 9.0, np.float32)
                rh = wh = None
                if first and abs(f) < half - 1:  # the first offset on the raster: also the taps
                    rh, wh = np.full(16 * d + 1, 9.0, np.float32), np.full(16 * d + 1, 9.0, np.float32)
                r = [C.byref(v) for v in rv]
                w = [C.byref(v) for v in wv]
                rc_r = lib.fmrx_rate_design(rf_fs, cap_fs, f, r[0], r[1], r[2], r[3], r[4], r[5], rt.ctypes.data, r[6],
                                            None if rh is None else rh.ctypes.data)
                rc_w = lib.fmrx_wide_design(rf_fs, d, f, w[0], w[1], w[2], w[3], wt.ctypes.data, w[4],
                                            None if wh is None else wh.ctypes.data)
                assert rc_r == rc_w, (rf_fs, d, f)
                got_r, got_w = [v.value for v in rv], [v.value for v in wv]
                if rc_r != fmrx.FMRX_OK:
                    assert rc_r == fmrx.FMRX_EINVAL and got_r == [-7] * 7 and got_w == [-7] * 5, (rf_fs, d, f)
                    assert np.all(rt == 9.0) and np.all(wt == 9.0), (rf_fs, d, f)
                    assert rh is None or (np.all(rh == 9.0) and np.all(wh == 9.0)), (rf_fs, d, f)
                    refused += 1
                    continue
                assert got_r[:2] == [1, d] and got_r[2:] == got_w, (rf_fs, d, f)
                n = got_r[4]
                assert 1 <= n <= 40 and got_r[6] == 16 * d + 1, (rf_fs, d, f)
                assert np.array_equal(rt.view(np.uint32), wt.view(np.uint32)) and np.all(rt[2 * n:] == 9.0), (rf_fs, d, f)
                if rh is not None:
                    assert np.array_equal(rh.view(np.uint32), wh.view(np.uint32)) and np.all(rh != 9.0)
                    first = False
                accepted += 1
            assert not first, (rf_fs, d)
    print(f"{accepted} offsets accepted, {refused} refused by both")
    assert accepted > 1000 and refused >= 4 * 9 * 3  # the four edges of every (rf_fs, D) are refused


@pytest.mark.parametrize("rf_fs,cap_fs,f", [
    (2400000, 2400000, 0),        # D = 1: no wide stage to design
    (2400000, 2000000, 0),        # cap_fs < rf_fs
    (2400000, 0, 0), (2400000, -10000000, 0),
    (2401002, 10000000, 0),       # rf_fs % 4 != 0
    (2400000, 2448000, 0),        # 50 / 51: L above 48
    (2400000, 2400100, 0),        # 24000 / 24001
    (2400000, 25200000, 0),       # 2 / 21: M above 10 L
    (2400000, 12550000, 0),       # 48 / 251: M above 125
    (2400000, 26400000, 0),       # D = 11
    (2400000, 10000000, 5000000), (2400000, 10000000, -5000000),   # 2 |f| >= cap_fs
    (2400000, 2500000, 1250000),
    (2400000, 10000000, 600001),  # a fine part of 1 Hz: the tuner refuses it
])
def test_refusals_write_nothing(fmrx, rf_fs, cap_fs, f):
    vals = [C.c_int(-7) for _ in range(7)]
    tab, h = np.full(1000, 9.0, np.float32), np.full(2001, 9.0, np.float32)
    p = [C.byref(v) for v in vals]
    rc = fmrx.lib().fmrx_rate_design(rf_fs, cap_fs, f, p[0], p[1], p[2], p[3], p[4], p[5], tab.ctypes.data, p[6],
                                     h.ctypes.data)
    assert rc == fmrx.FMRX_EINVAL
    assert [v.value for v in vals] == [-7] * 7 and np.all(tab == 9.0) and np.all(h == 9.0)
    with pytest.raises(fmrx.FmrxError) as e:
        fmrx.rate_design(rf_fs, cap_fs, f)
    assert e.value.code == fmrx.FMRX_EINVAL


def test_all_null_outputs(fmrx):
    assert fmrx.lib().fmrx_rate_design(2400000, 10000000, 1700000, *([None] * 9)) == fmrx.FMRX_OK


@pytest.mark.parametrize("mode,cap_fs,blocks,wide", [(0, 10000000, 3, 80000), (1, 2048000, 3, 16384), (0, 6000000, 1, 16000),
                                                     (0, 2500000, 3, 20000), (0, 12500000, 3, 100000)])
def test_granule_arithmetic(fmrx, mode, cap_fs, blocks, wide):
    """B = L / gcd(L, iq_pairs) narrow blocks are B iq_pairs M / L wide pairs: whole, and no fewer blocks are."""
    ip, rf_fs = oracle.MODES[mode][0] // 2, oracle.MODES[mode][3]
    d = fmrx.rate_design(rf_fs, cap_fs, 0)
    b = d["up"] // math.gcd(d["up"], ip)
    assert b == blocks and (b * ip * d["down"]) % d["up"] == 0 and b * ip * d["down"] // d["up"] == wide
    assert all((n * ip * d["down"]) % d["up"] != 0 for n in range(1, b))


# ---- the split and the rotator -------------------------------------------------------------------------

@pytest.mark.parametrize("rf_fs,cap_fs,f,q,f_r,n_c,k_c", [
    (2400000, 10000000, 0, 0, 0, 1, 0),
    (2400000, 10000000, 299000, 0, 299000, 1, 0),
    (2400000, 10000000, 300000, 1, -300000, 50, 3),        # the tie rounds away from zero; gcd(6, 100) = 2
    (2400000, 10000000, -300000, -1, 300000, 50, 47),
    (2400000, 10000000, 600000, 1, 0, 50, 3),
    (2400000, 10000000, 4900000, 8, 100000, 25, 12),
    (2400000, 6000000, 2900000, 5, -100000, 2, 1),         # |f_c| = cap_fs / 2: N_c = 2
    (2400000, 6000000, 700000, 1, 100000, 10, 1),
    (2400000, 2500000, 600000, 1, 0, 25, 6),               # gcd(24, 100) = 4
    (2400000, 12500000, 3000000, 5, 0, 25, 6),             # gcd(120, 500) = 20
    (2400000, 2560000, 600000, 1, 0, 64, 15),              # 15 / 16, q = 1: N_c = 4 M
    (1152000, 2048000, 288000, 1, 0, 64, 9),               # N_c = 4 M
    (1152000, 2048000, -1000000, -3, -136000, 64, 37),
    (2304000, 6000000, 576000, 1, 0, 125, 12),             # 48 / 125: gcd(48, 500) = 4
    (1152000, 8000000, 288000, 1, 0, 250, 9),              # 18 / 125
    (2304000, 2560000, -576000, -1, 0, 40, 31),            # 9 / 10: N_c = 4 M
])
def test_split(fmrx, rf_fs, cap_fs, f, q, f_r, n_c, k_c):
    d = fmrx.rate_design(rf_fs, cap_fs, f)
    got_q, rem = divmod(d["coarse_hz"], rf_fs // 4)
    assert rem == 0 and (got_q, d["fine_hz"], d["N"], d["k"]) == (q, f_r, n_c, k_c)
    assert d["coarse_hz"] + d["fine_hz"] == f and 8 * abs(d["fine_hz"]) <= rf_fs
    # k_c cap_fs / N_c is f_c mod cap_fs: the rotator turns by exactly the coarse part
    assert (d["k"] * cap_fs) % d["N"] == 0 and (d["k"] * cap_fs // d["N"] - d["coarse_hz"]) % cap_fs == 0
    assert d["table"].shape == (n_c, 2) and d["N"] <= 500


def test_longest_period(fmrx):
    """N_c = 4 M = 500 needs gcd(|q| L, 500) = 1: 18 / 125 has none (L even), 3 / 125 would; among the
    accepted ratios with M = 125 the longest is 250."""
    best = 0
    for rf_fs, cap_fs, up, down in DESIGNS:
        for q in range(0, 2 * down // up):
            f = q * (rf_fs // 4)
            if 2 * f < cap_fs:
                d = fmrx.rate_design(rf_fs, cap_fs, f)
                assert d["N"] == 4 * down // math.gcd(q * up, 4 * down) if q else d["N"] == 1
                best = max(best, d["N"])
    assert best == 250


@pytest.mark.parametrize("rf_fs,cap_fs,up,down", DESIGNS)
def test_table_within_one_ulp_of_float64(fmrx, rf_fs, cap_fs, up, down):
    for q in (1, 2, -2, -1):
        d = fmrx.rate_design(rf_fs, cap_fs, q * rf_fs // 4)
        n, tab = d["N"], d["table"]
        assert n == 4 * down // math.gcd(abs(q) * up, 4 * down)
        a = 2 * np.pi * np.arange(n, dtype=np.float64) / n
        for col, ref in ((0, np.cos(a)), (1, np.sin(a))):
            r32 = ref.astype(np.float32)
            err = np.abs(tab[:, col].astype(np.float64) - r32.astype(np.float64))
            assert np.all(err <= np.spacing(np.abs(r32)).astype(np.float64)), (col, int(np.argmax(err)))


# ---- the low-pass ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("rf_fs,cap_fs,up,down", DESIGNS)
def test_taps_are_the_library_low_pass(fmrx, rf_fs, cap_fs, up, down):
    h = fmrx.rate_design(rf_fs, cap_fs, 0)["h"]
    want = fmrx.lpf(np.float32(rf_fs) * np.float32(down), 3 * rf_fs / 8, 16 * down + 1, up)
    assert h.dtype == np.float32 and np.array_equal(h.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(h, _orc().lpf(np.float32(rf_fs) * np.float32(down), 3 * rf_fs / 8, 16 * down + 1, up))


@pytest.mark.parametrize("rf_fs,cap_fs,up,down", DESIGNS)
def test_response(fmrx, rf_fs, cap_fs, up, down):
    """Float64 response of the float32 taps at the virtual rate M rf_fs, divided by L, on 2^20 points of
    [0, M rf_fs / 2]: flat over the fine offset plus a channel, and down by 65 dB over everything that
    aliases onto that band."""
    h = fmrx.rate_design(rf_fs, cap_fs, 0)["h"].astype(np.float64)
    n = 1 << 20
    mag = np.abs(np.fft.rfft(h, 2 * n)) / up
    f = np.arange(n + 1, dtype=np.float64) * (down * rf_fs / 2) / n
    db = 20 * np.log10(np.maximum(mag, 1e-30))
    passband, stopband = f <= rf_fs / 8 + 100e3, f >= 7 * rf_fs / 8 - 200e3
    assert passband.sum() > 100 and stopband.sum() > 100
    print(f"rf_fs {rf_fs} {up}/{down}: passband {db[passband].min():+.4f} .. {db[passband].max():+.4f} dB, "
          f"stopband max {db[stopband].max():.2f} dB")
    assert np.all(np.abs(db[passband]) <= 0.05)
    assert np.all(db[stopband] <= -65.0)


# ---- the expected output of the rational path ---------------------------------------------------------------

def rate_y(raw, fmt, rf_fs, cap_fs, offset, first_pair=0):
    """The cf32 stream at rf_fs the rational down-converter makes of a capture at cap_fs (interleaved
    float32), the fine offset and (L, M): normalise, rotate by the coarse table in numpy float32 (every
    product and sum rounded separately, integer phases), the oracle's resample of I' and Q' by L / M
    with the oracle's taps."""
    fm, orc = iqgen.load_fmrx(), _orc()
    d = fm.rate_design(rf_fs, cap_fs, offset)
    up, down = d["up"], d["down"]
    x = normalise(raw, fmt)
    xi, xq = x[0::2], x[1::2]
    n_per, k, tab = d["N"], d["k"], d["table"]
    n = (int(first_pair) % n_per + np.arange(xi.size, dtype=np.int64)) % n_per
    p = (k * n) % n_per
    c, s = tab[p, 0], tab[p, 1]
    assert c.dtype == np.float32 and xi.dtype == np.float32
    ri = xi * c + xq * s
    rq = xq * c - xi * s
    h = orc.lpf(np.float32(rf_fs) * np.float32(down), 3 * rf_fs / 8, 16 * down + 1, up)
    zeros = np.zeros(16 * down, np.float32)
    assert (xi.size * up) % down == 0
    y = np.empty(2 * (xi.size * up // down), np.float32)
    y[0::2], _ = orc.resample(ri, zeros, h, up, down)
    y[1::2], _ = orc.resample(rq, zeros, h, up, down)
    return y, d["fine_hz"], (up, down)


def rate_compose(raw, fmt, mode, rf_taps, cap_fs, offset, first_pair=0, fields=("pcm_mono",)):
    """The expected outputs of one station at `offset` of a capture at cap_fs, from wide position
    first_pair (a multiple of M), over the whole of raw (whole granules) in one piece."""
    y, fine, (up, down) = rate_y(raw, fmt, oracle.MODES[mode][3], cap_fs, offset, first_pair)
    assert first_pair % down == 0
    return narrow_compose(y, F32, mode, rf_taps, fine, first_pair // down * up, fields)


def test_resample_is_the_definition():
    """Oracle.resample(x, zeros, h, L, M) against the definition's sum written out in numpy float32."""
    rng = np.random.default_rng(5)
    up, down, n = 6, 25, 500
    x = rng.standard_normal(n).astype(np.float32)
    h = _orc().lpf(np.float32(2400000) * np.float32(down), 900000.0, 16 * down + 1, up)
    got, _ = _orc().resample(x, np.zeros(16 * down, np.float32), h, up, down)
    assert got.size == n * up // down
    for m in range(got.size):
        acc = np.float32(0.0)
        for k in range((m * down) % up, 16 * down + 1, up):
            j = (m * down - k) // up
            assert (m * down - k) % up == 0
            if j >= 0:
                acc = np.float32(acc + np.float32(h[k] * x[j]))
        assert acc == got[m], m


# ---- the kernel's plan in numpy -----------------------------------------------------------------------------

def taps_by_phase(h, up, down):
    """rate_taps_by_phase (csrc/wide_design.cpp) restated: the taps regrouped by output phase, L rows of
    ceil((16 M + 1) / L), and the byte offset in the LDS rows of the pair lane 0 multiplies by each."""
    hc, ts = (16 + up - 1) // up, (16 * down + 1 + up - 1) // up
    w = (64 + hc) | 1
    hp, off = np.zeros((up, ts), np.float32), np.zeros((up, ts), np.int64)
    for phi in range(up):
        e, k0 = divmod(phi * down, up)
        for i in range(ts):
            if k0 + up * i < 16 * down + 1:
                u = hc * down + e - i
                assert u >= 0
                hp[phi, i], off[phi, i] = h[k0 + up * i], 8 * ((u % down) * w + u // down)
    return hp, off


def emulate_kernel(xi, xq, n_c, k_c, tab, h, up, down, n_out, segs, first_pair=0, grouped=False):
    """rate_ddc_kernel's staging, layout, phase stepping, history copy and hand-off in numpy float32 for
    one station: workgroups of 256 threads (four waves of 64 lanes) stage chunks of 64 M wide pairs = 64 L
    outputs, the rotated pairs in M rows of W columns behind HC history columns, the taps by phase (each
    phase summed by the 64 lanes of one wave), the outputs through rows of L | 1 and out by all 256
    threads.  xi, xq: the normalised samples of the call (zeros in front of them).

    grouped: the phases in the kernel's order -- wave by wave, in groups of pg <= 4 phases side by side,
    the last one ragged -- each tap read at the byte offset taps_by_phase gives it, nmin taps for every
    phase of a group and then one more for the phases with k_0 < rem, the hand-off rows written group by
    group.  Otherwise one phase at a time, walking the rows itself."""
    nt, ns = 64, 256
    hc, ts = (16 + up - 1) // up, (16 * down + 1 + up - 1) // up
    w, ls = (nt + hc) | 1, up | 1
    hp = np.zeros((up, ts), np.float32)
    for phi in range(up):
        kk = np.arange((phi * down) % up, 16 * down + 1, up)
        hp[phi, : kk.size] = h[kk]
    nmin, rem = (16 * down + 1) // up, (16 * down + 1) % up
    cm, p_chunk = nt * up, nt * down
    n_chunks = -(-n_out // cm)
    tid, st = np.arange(nt), np.arange(ns)

    def sample(rel):  # the virtual stream: zeros ++ data ++ zeros
        ok = (rel >= 0) & (rel < xi.size)
        r = np.where(ok, rel, 0)
        return np.where(ok, xi[r], np.float32(0)), np.where(ok, xq[r], np.float32(0))

    def rotate(rel, ph):
        a, b = sample(rel)
        c, s = tab[ph, 0], tab[ph, 1]
        return (a * c + b * s).astype(np.float32), (b * c - a * s).astype(np.float32)

    n0 = first_pair % n_c
    phase_of = lambda rel: (k_c * ((n0 + rel % n_c) % n_c)) % n_c  # noqa: E731
    y = np.full((n_out, 2), np.nan, np.float32)
    for seg in range(segs):
        c0, c1 = seg * n_chunks // segs, (seg + 1) * n_chunks // segs
        if c0 >= c1:
            continue
        xb = np.full((down * w, 2), np.nan, np.float32)
        hpairs = hc * down
        hpe = (hpairs + 1) & ~1
        shift = hpe - hpairs
        for j in range(hpe // 2):  # the prologue, unit by unit
            rel = c0 * p_chunk - hpe + 2 * j + np.arange(2)
            ri, rq = rotate(rel, phase_of(rel))
            for t in range(2):
                b = 2 * j - shift + t
                if b >= 0:
                    xb[(b % down) * w + b // down] = (ri[t], rq[t])
        pc = phase_of(c0 * p_chunk)
        ph_tid, ph_ld, ph_chunk = (2 * k_c * st) % n_c, (2 * k_c * ns) % n_c, (k_c * (p_chunk % n_c)) % n_c
        for c in range(c0, c1):
            ph = (pc + ph_tid) % n_c
            col, row = hc + (2 * st) // down, (2 * st) % down
            dcol, drow = (2 * ns) // down, (2 * ns) % down
            for l in range((p_chunk // 2 + ns - 1) // ns):
                u = st + l * ns
                live = u < p_chunk // 2
                rel = c * p_chunk + 2 * u
                r0 = rotate(rel, ph)
                r1 = rotate(rel + 1, (ph + k_c) % n_c)
                a0 = row * w + col
                a1 = np.where(row + 1 == down, col + 1, (row + 1) * w + col)
                xb[a0[live], 0], xb[a0[live], 1] = r0[0][live], r0[1][live]
                xb[a1[live], 0], xb[a1[live], 1] = r1[0][live], r1[1][live]
                ph = (ph + ph_ld) % n_c
                row, col = row + drow, col + dcol
                col = np.where(row >= down, col + 1, col)
                row = np.where(row >= down, row - down, row)
            pc = (pc + ph_chunk) % n_c
            ob = np.full((nt * ls, 2), np.nan, np.float32)
            if grouped:
                tp_h, tp_off = taps_by_phase(h, up, down)
                turns = ((up + 3) // 4 + 3) // 4
                pg = (up + 4 * turns - 1) // (4 * turns)
                done = []
                for wave in range(4):
                    for phi0 in range(wave * pg, up, 4 * pg):
                        r_n = min(pg, up - phi0)
                        acc = np.zeros((r_n, nt, 2), np.float32)
                        for i in range(nmin):
                            for r in range(r_n):
                                at = tp_off[phi0 + r, i] // 8 + tid
                                acc[r] = (acc[r] + (xb[at] * tp_h[phi0 + r, i]).astype(np.float32)).astype(np.float32)
                        for r in range(r_n):
                            if ((phi0 + r) * down) % up < rem:
                                at = tp_off[phi0 + r, nmin] // 8 + tid
                                acc[r] = (acc[r] + (xb[at] * tp_h[phi0 + r, nmin]).astype(np.float32)).astype(np.float32)
                            ob[(phi0 + r) + ls * tid] = acc[r]
                            done.append(phi0 + r)
                assert sorted(done) == list(range(up))  # every phase once
            for phi in range(0 if grouped else up):
                e, k0 = divmod(phi * down, up)
                row_s, off = e, e * w + hc
                acc = np.zeros((nt, 2), np.float32)
                for i in range(nmin + (1 if k0 < rem else 0)):
                    acc = (acc + (xb[off + tid] * hp[phi, i]).astype(np.float32)).astype(np.float32)
                    if row_s == 0:
                        row_s, off = down - 1, off + (down - 1) * w - 1
                    else:
                        row_s, off = row_s - 1, off - w
                ob[phi + ls * tid] = acc
            if c + 1 < c1:  # the history copy
                for j in range(hc):
                    xb[np.arange(down) * w + j] = xb[np.arange(down) * w + nt + j]
            t_o, p_o = st // up, st % up
            for it in range((cm + ns - 1) // ns):
                j = st + ns * it
                m = c * cm + j
                ok = (j < cm) & (m < n_out)
                y[m[ok]] = ob[(p_o + ls * t_o)[ok]]
                t_o, p_o = t_o + ns // up, p_o + ns % up
                t_o = np.where(p_o >= up, t_o + 1, t_o)
                p_o = np.where(p_o >= up, p_o - up, p_o)
    return y


@pytest.mark.parametrize("cap_fs,offset,first_pair,chunks", [(10000000, 1700000, 0, 5), (6000000, 2900000, 5 * 7, 7),
                                                             (2500000, -600000, 25 * 11, 3), (12500000, 3000000, 0, 3)])
def test_kernel_plan_in_numpy(fmrx, cap_fs, offset, first_pair, chunks):
    """The emulation against the composition: a ragged tail chunk, one segment (every chunk but the first
    takes its history from the copy) and three (each rebuilds its history from the raw pairs)."""
    rf_fs = 2400000
    d = fmrx.rate_design(rf_fs, cap_fs, offset)
    up, down = d["up"], d["down"]
    n_out = (64 * chunks - 37) * up
    raw = iqgen.make("synth:9", 2 * n_out * down // up, rf_fs)
    want, _, _ = rate_y(raw, U8, rf_fs, cap_fs, offset, first_pair)
    x = normalise(raw, U8)
    for segs in (1, 3):
        got = emulate_kernel(x[0::2], x[1::2], d["N"], d["k"], d["table"], d["h"], up, down, n_out, segs, first_pair)
        assert np.array_equal(got.reshape(-1).view(np.uint32), want.view(np.uint32)), segs
    assert want.any()


SWEEP_RATIOS = sorted({(oracle.MODES[mode][3], cap_fs) + sweep_ratio(mode, cap_fs) for mode, cap_fs in RATE_SWEEP},
                      key=lambda c: c[2:])


@pytest.mark.parametrize("rf_fs,cap_fs,up,down", SWEEP_RATIOS, ids=[f"{c[2]}/{c[3]}" for c in SWEEP_RATIOS])
def test_kernel_plan_in_numpy_over_the_sweep(fmrx, rf_fs, cap_fs, up, down):
    """Every (L, M) of tests/test_gpu_rate_sweep.py through the emulation with the phases in the kernel's
    order and the taps at the byte offsets of rate_taps_by_phase: three chunks (the last one ragged) as one
    segment and as three.  HC, the row width, L | 1, the history copy and the offsets hold at every L
    before the GPU runs one; the buffers are exactly rate_lds_bytes long, so an index past them raises."""
    offset, first_pair = rf_fs // 4 + 50000, 7 * down
    d = fmrx.rate_design(rf_fs, cap_fs, offset)
    assert (d["up"], d["down"]) == (up, down)
    n_out = (64 * 3 - 37) * up
    raw = iqgen.make("synth:9", 2 * n_out * down // up, rf_fs)
    want, _, _ = rate_y(raw, U8, rf_fs, cap_fs, offset, first_pair)
    x = normalise(raw, U8)
    for segs in (1, 3):
        got = emulate_kernel(x[0::2], x[1::2], d["N"], d["k"], d["table"], d["h"], up, down, n_out, segs, first_pair,
                             grouped=True)
        assert np.array_equal(got.reshape(-1).view(np.uint32), want.view(np.uint32)), segs
    assert want.any()


# ---- quality of the definition --------------------------------------------------------------------------

R_CAP_FS = 10000000
R_STATIONS = ((31, 1700000), (32, -3100000))  # test_wide_host's two synth stations, inside +-5 MHz


@functools.lru_cache(maxsize=None)
def two_station_capture_10ms():
    """A mode-0 capture at 10 MS/s in float64: each narrow synth station FFT-interpolated by 25 / 6,
    moved to its offset, times 0.45; the sum as int16 (12 narrow blocks: 320,000 wide pairs, 4 granules)."""
    rf_fs, total = oracle.MODES[Q_MODE][3], 0
    for seed, f in R_STATIONS:
        z = as_complex(narrow_station(seed))
        n = z.size
        assert (n * 25) % 6 == 0
        nw = n * 25 // 6
        spec = np.fft.fft(z)
        wide = np.zeros(nw, np.complex128)
        wide[: n // 2], wide[-(n // 2):] = spec[: n // 2], spec[n // 2:]
        up = np.fft.ifft(wide) * (nw / n)
        total = total + 0.45 * up * np.exp(2j * np.pi * (f / R_CAP_FS) * np.arange(up.size))
    out = np.empty(2 * total.size, np.float64)
    out[0::2], out[1::2] = total.real, total.imag
    a = np.clip(np.rint(out * 32768.0), -32768, 32767).astype(np.int16)
    a.setflags(write=False)
    return a


def test_two_stations_are_found(fmrx):
    raw = two_station_capture_10ms()
    stations, _ = fmrx.scan_detect_rate(welch64(raw, 4096), oracle.MODES[Q_MODE][3], R_CAP_FS, **Q_SCAN)
    assert [s.offset_hz for s in stations] == sorted(f for _, f in R_STATIONS)
    # an integer ratio through the same call is the wide detector
    w = two_station_capture()
    rf_fs = oracle.MODES[Q_MODE][3]
    a, _ = fmrx.scan_detect_rate(welch64(w, 4096), rf_fs, Q_D * rf_fs, **Q_SCAN)
    b, _ = fmrx.scan_detect_wide(welch64(w, 4096), rf_fs, Q_D, **Q_SCAN)
    assert [(s.offset_hz, s.power_db, s.snr_db) for s in a] == [(s.offset_hz, s.power_db, s.snr_db) for s in b]
    with pytest.raises(fmrx.FmrxError) as e:
        fmrx.scan_detect_rate(welch64(raw, 4096), rf_fs, 25200000)
    assert e.value.code == fmrx.FMRX_EINVAL


def test_quality_of_the_definition(fmrx):
    """The rational path's mono PCM of each station of the 10 MS/s capture against the oracle's PCM of
    the narrow stream it was built from (peak normalised correlation, lags -2..+2, first 4 blocks
    skipped), and the same figure for the existing D = 4 composition of test_wide_host's capture.  The
    filter delays the stream by 8 narrow pairs in both, so the figures agree; the rational one may be
    lower by 0.002, which absorbs the different interpolation of the fixture.  Measured: D = 4 0.99829 /
    0.99829, 6 / 25 0.99829 / 0.99829."""
    na = oracle.MODES[Q_MODE][2]
    skip = Q_SKIP * na
    assert Q_STATIONS == R_STATIONS and Q_BLOCKS % 3 == 0
    raw_r, raw_w = two_station_capture_10ms(), two_station_capture()
    for seed, f in R_STATIONS:
        clean = _orc().run(Q_MODE, 51, narrow_station(seed), ["pcm_mono"])["pcm_mono"]
        integer = peak_correlation(wide_compose(raw_w, S16, Q_MODE, 51, Q_D, f)["pcm_mono"], clean, skip)
        rational = peak_correlation(rate_compose(raw_r, S16, Q_MODE, 51, R_CAP_FS, f)["pcm_mono"], clean, skip)
        print(f"station at {f:+d} Hz: D = 4 {integer:.5f}, 6/25 {rational:.5f}")
        assert integer > 0.99
        assert rational >= integer - 0.002
