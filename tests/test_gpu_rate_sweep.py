"""GPU sweep of the rational down-converter (csrc/rate.hip) over every L that fmrx_set_capture_rate can
reach: rate_ddc_kernel<F> picks its code path from L (how many phases a wave sums side by side, and
whether the last group of a wave is ragged) and from M (taps a phase, staging loads a thread, bytes of
LDS), and tests/test_gpu_rate.py runs L = 2, 6, 9 and 24 only.  Every output here is compared bit for
bit with rate_compose of tests/test_rate_host.py; there is no tolerance anywhere.

RATE_SWEEP is also what tests/test_variants_host.py checks on the CPU: it recomputes each case's
grouping and asserts what the list has to cover, and tests/test_rate_host.py runs the numpy emulation
of the kernel's plan at every (L, M) named here, so a mismatch on the GPU points at kernel code."""
from __future__ import annotations

import math

import numpy as np
import pytest

import oracle
from test_formats_host import F32, S8, S16, U8

pytestmark = pytest.mark.gpu

torch = None  # imported by the _gpu fixture, like gr (tests/test_gpu_rate.py): the case list imports without them
gr = None

NAMES = {U8: "u8", S8: "s8", S16: "s16", F32: "f32"}

# (mode, cap_fs): modes 0 and 1 only (blocks of 6400 and 3072 pairs; the kernel never sees the mode)
RATE_SWEEP = [
    # mode 0, rf_fs = 2.4 MS/s: every L <= 48 that divides it
    (0, 22800000),  # 2/19: M at the bound 10 L (20 is not coprime)
    (0, 3200000),   # 3/4: M = L + 1
    (0, 8000000),   # 3/10
    (0, 16000000),  # 3/20
    (0, 20000000),  # 3/25
    (0, 3000000),   # 4/5
    (0, 4320000),   # 5/9: (16 M + 1) mod L = 0, groups 2, 2, 1
    (0, 23520000),  # 5/49: the largest M of L = 5, seven staging loads a thread
    (0, 10000000),  # 6/25
    (0, 23700000),  # 8/79: ten staging loads a thread
    (0, 2640000),   # 10/11: groups 3, 3, 3, 1
    (0, 23760000),  # 10/99
    (0, 5000000),   # 12/25
    (0, 2560000),   # 15/16: groups 4, 4, 4, 3
    (0, 4640000),   # 15/29: (16 M + 1) mod L = 0
    (0, 3750000),   # 16/25: groups of four, none ragged
    (0, 2520000),   # 20/21: groups 3 x 6, 2
    (0, 4920000),   # 20/41: six staging loads a thread
    (0, 3500000),   # 24/35
    (0, 3072000),   # 25/32: groups 4 x 6, 1
    (0, 11904000),  # 25/124: the largest M of L = 25
    (0, 2480000),   # 30/31: groups 4 x 7, 2
    (0, 9375000),   # 32/125
    (0, 2940000),   # 40/49: groups 4 x 10 in three turns
    (0, 2450000),   # 48/49
    (0, 6250000),   # 48/125: the largest L and M, 94 KB of LDS
    # mode 1, rf_fs = 1.152 MS/s: the L that only it reaches, and the radio rates
    (1, 2560000),   # 9/20
    (1, 3200000),   # 9/25
    (1, 1216000),   # 18/19
    (1, 8000000),   # 18/125
    (1, 4000000),   # 36/125: 88 KB of LDS
    (1, 1177600),   # 45/46: groups 4 x 11, 1; a granule of 15 blocks
    (1, 3174400),   # 45/124
    (1, 3000000),   # 48/125
]
# the extremes the other formats meet (test_gpu_rate.py::test_formats runs them at 6/25)
FORMAT_CASES = [(fmt, cap_fs) for cap_fs in (6250000, 2560000) for fmt in (S8, S16, F32)]
# the formats of rate_ddc_kernel<F> this module launches: tests/test_variants_host.py compares them with the library
SWEEP_FORMATS = {U8} | {fmt for fmt, _ in FORMAT_CASES}


def sweep_ratio(mode, cap_fs):
    rf_fs = oracle.MODES[mode][3]
    g = math.gcd(rf_fs, cap_fs)
    return rf_fs // g, cap_fs // g


def sweep_id(case):
    mode, cap_fs = case
    up, down = sweep_ratio(mode, cap_fs)
    return f"mode{mode}-{up}/{down}"


def sweep_offset(mode):
    """q = 1 and a fine part of 50 kHz: inside cap_fs / 2 for every case (cap_fs > rf_fs)."""
    return oracle.MODES[mode][3] // 4 + 50000


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    global torch, gr
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()
    import test_gpu_rate

    gr = test_gpu_rate


def first_difference(got, want, up):
    """Where two PCM rows first differ, for the assertion's message."""
    if got.shape != want.shape:
        return f"shapes {got.shape} != {want.shape}"
    bad = np.flatnonzero(got != want)
    return "equal" if bad.size == 0 else f"L = {up}: {bad.size} of {got.size} differ, first at {int(bad[0])}"


# ---- every reachable L: u8, 51 taps, mono ------------------------------------------------------------------------

@pytest.mark.parametrize("case", RATE_SWEEP, ids=sweep_id)
def test_sweep_u8_matches_composition(fmrx, case):
    """Two granules as two calls of one granule, then after reset() as one call."""
    mode, cap_fs = case
    up, down = sweep_ratio(mode, cap_fs)
    f = sweep_offset(mode)
    assert 2 * f < cap_fs
    b, ge = gr.granule(mode, cap_fs)
    raw = gr.capture(200 + up, mode, cap_fs, 2)
    want = gr.rate_compose(raw, U8, mode, 51, cap_fs, f)["pcm_mono"]
    with gr.receiver(fmrx, U8, cap_fs, mode) as rx:
        rx.tune_wide(f)
        got = gr.in_calls(rx.process_wide, raw, ge, [1, 1])
        assert rx.wide_info() == ([f], 2 * ge // 2, True)
        assert rx.tuner_info()[1] == 2 * b * oracle.MODES[mode][0] // 2
        assert np.array_equal(got, want) and got.any(), first_difference(got, want, up)
        rx.reset()
        assert rx.wide_info() == ([f], 0, True)
        again = rx.process_wide(raw)
        assert np.array_equal(again, want), first_difference(again, want, up)


# ---- the other formats at the largest L and M and at the ragged groups of four ----------------------------------

@pytest.mark.parametrize("fmt,cap_fs", FORMAT_CASES, ids=[f"{NAMES[f]}-{sweep_id((0, c))}" for f, c in FORMAT_CASES])
def test_sweep_formats(fmrx, fmt, cap_fs):
    f = sweep_offset(0)
    raw = gr.capture(260, 0, cap_fs, 2, fmt)
    if fmt == S16:  # not only multiples of 256
        raw = (raw.astype(np.int32) + (np.arange(raw.size) * 7919) % 251 - 125).clip(-32768, 32767).astype(np.int16)
    elif fmt == F32:  # inside the promised range: 0 or [2^-20, 4]
        raw = (raw * np.float32(1.7)).astype(np.float32)
        assert np.abs(raw).max() <= 4.0 and np.all((raw == 0) | (np.abs(raw) >= 2.0 ** -20))
    with gr.receiver(fmrx, fmt, cap_fs) as rx:
        rx.tune_wide(f)
        got = gr.in_calls(rx.process_wide, raw, gr.granule(0, cap_fs)[1], [1, 1])
    want = gr.rate_compose(raw, fmt, 0, 51, cap_fs, f)["pcm_mono"]
    assert np.array_equal(got, want) and got.any(), first_difference(got, want, sweep_ratio(0, cap_fs)[0])


# ---- workgroups that walk several chunks with groups of four ----------------------------------------------------

def rate_target(up, down, cus):
    """wide_segments (csrc/wide_design.cpp) at a rational ratio: rate_lds_bytes and at most six workgroups a CU."""
    lds = 8 * (500 + down * ((64 + (16 + up - 1) // up) | 1) + 64 * (up | 1))
    return cus * min(6, max(1, 160 * 1024 // lds))


@pytest.mark.parametrize("cap_fs,granules,chunks,hc", [(6250000, 3, 19, 1), (2560000, 5, 100, 2)], ids=["48/125", "15/16"])
def test_sweep_workgroups_walk_several_chunks(fmrx, cap_fs, granules, chunks, hc):
    """16 stations on one mode-0 capture.  48/125: 3 granules are 57,600 outputs a station, 19 chunks of
    64 * 48 (the last one ragged); one workgroup of 94 KB fits a CU, so the target is one a CU and 16 * 19
    chunks exceed it on any device of fewer than 304 CUs: segments of 4 or 5 chunks, one column of history
    copied inside LDS.  15/16: 5 granules are 96,000 outputs, 100 chunks of 64 * 15; six workgroups of
    13 KB a CU: segments of 4 chunks on 256 CUs (min(1536 / 16, 100 / 4) = 25), two columns of history, and
    every wave's groups are 4, 4, 4, 3 phases."""
    ns = 16
    up, down = sweep_ratio(0, cap_fs)
    b, ge = gr.granule(0, cap_fs)
    n_out = granules * b * oracle.MODES[0][0] // 2
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    target = rate_target(up, down, cus)
    assert -(-n_out // (64 * up)) == chunks and (16 + up - 1) // up == hc
    assert ns * chunks > target, "the shape no longer makes a workgroup walk chunks"
    segs = min(max(1, target // ns), max(1, chunks // 4))
    assert chunks // segs >= 4
    # 16 stations across the capture (q from -4 to +3 at the least), every fine part a multiple of 1 kHz
    step = cap_fs // 17 // 1000 * 1000
    offsets = [(s - 8) * step + 7000 * (s % 3) for s in range(ns)]
    raw = gr.capture(270 + up, 0, cap_fs, granules)
    with gr.receiver(fmrx, U8, cap_fs, n_streams=ns) as rx:
        rx.tune_wide(offsets)
        got = rx.process_wide(raw)
        assert rx.wide_info() == (offsets, raw.size // 2, True)
    for s in (0, 7, ns - 1):
        want = gr.rate_compose(raw, U8, 0, 51, cap_fs, offsets[s])["pcm_mono"]
        assert np.array_equal(got[s], want) and got[s].any(), (s, first_difference(got[s], want, up))
    assert len({row.tobytes() for row in got}) == ns
