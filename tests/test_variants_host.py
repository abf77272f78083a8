"""CPU guard of the GPU tests' matrices: the instantiations of tuner_kernel, wide_ddc_kernel,
mono_fused_kernel (tests/test_gpu_variants.py), scan_segments_kernel (tests/test_gpu_scan.py) and
rate_ddc_kernel (tests/test_gpu_rate_sweep.py) that libfmrx.so holds, read from its symbol table
(`nm -C`: names only, never the code), are exactly what the GPU tests parametrize over.  A newly
compiled instantiation fails here until a GPU case names it; a case whose kernel is gone fails too.

rate_ddc_kernel<F> takes L and M at run time, so its matrix is a list of capture rates, RATE_SWEEP:
the guard below recomputes from the list what each case makes the kernel do and asserts what the
list has to cover.  A rate dropped from it, or an L that becomes reachable, fails here."""
from __future__ import annotations

import math
import re
import shutil
import subprocess
from collections import Counter

import pytest

import oracle
from test_gpu_rate_sweep import FORMAT_CASES, RATE_SWEEP, SWEEP_FORMATS, rate_target, sweep_offset, sweep_ratio
from test_gpu_scan import SCAN_CASES, SCAN_WALK_CASES
from test_gpu_variants import FUSED_CASES, TUNER_CASES, WIDE_CASES, fused_variants, rf_decim

KERNELS = ("tuner_kernel", "wide_ddc_kernel", "mono_fused_kernel", "scan_segments_kernel", "rate_ddc_kernel")


@pytest.fixture(scope="module")
def instantiations(fmrx):
    """kernel name -> the set of its template argument tuples in the library (a kernel shows up twice,
    as its host stub and its handle: a set)."""
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm is not on this machine")
    out = subprocess.run([nm, "-C", fmrx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    found = {name: set() for name in KERNELS}
    for name, args in re.findall(r"\b(%s)<([-0-9, ]+)>\(" % "|".join(KERNELS), out):
        found[name].add(tuple(int(a) for a in args.split(",")))
    return found


def test_symbols_were_read(instantiations):
    """The counts of a build of this tree; the tests below say what they are made of."""
    assert {k: len(v) for k, v in instantiations.items()} == {"tuner_kernel": 24, "wide_ddc_kernel": 36,
                                                             "mono_fused_kernel": 41, "scan_segments_kernel": 24,
                                                             "rate_ddc_kernel": 4}


def test_tuner_matrix_is_complete(instantiations):
    """tuner_kernel<T, D, R, PD, F>: R and PD follow from D (launch_tuner), so (T, D, F) names one."""
    compiled = {(t, d, f) for t, d, _, _, f in instantiations["tuner_kernel"]}
    assert len(compiled) == len(instantiations["tuner_kernel"])
    tested = {(rf_taps, rf_decim(mode), fmt) for mode, rf_taps, fmt in TUNER_CASES}
    assert compiled == tested, (sorted(compiled - tested), sorted(tested - compiled))


def test_wide_matrix_is_complete(instantiations):
    compiled = instantiations["wide_ddc_kernel"]  # wide_ddc_kernel<D, F>
    tested = set(WIDE_CASES)
    assert compiled == tested, (sorted(compiled - tested), sorted(tested - compiled))


def test_fused_matrix_is_complete(instantiations):
    """mono_fused_kernel<T, D, AD, NT, R, PD, ABL, TR, AU, Z0>: every (T, D, AD, AU) meets the oracle in
    its default shape.  The other workgroup shapes (NT, R, PD, TR) of one (T, D, AD, AU) are reached only
    through the tuning switch FMRX_MONO_VARIANT, which a process reads once, and ABL = 64 only through
    fmrx_debug_mono_stamps: they are not part of this matrix."""
    compiled = {(a[0], a[1], a[2], a[8]) for a in instantiations["mono_fused_kernel"]}
    tested = set().union(*(fused_variants(*case) for case in FUSED_CASES))
    assert compiled == tested, (sorted(compiled - tested), sorted(tested - compiled))
    stages = [(rf_decim(m), oracle.MODES[m][7], oracle.MODES[m][6]) for m in range(4)] + [(9, 5, 1)]
    assert tested == {(t,) + s for t in (51, 101) for s in stages} and len(tested) == 10


def test_scan_matrix_is_complete(instantiations):
    compiled = instantiations["scan_segments_kernel"]  # scan_segments_kernel<log2 N, F>
    tested = set(SCAN_CASES)
    assert compiled == tested and len(tested) == 24, (sorted(compiled - tested), sorted(tested - compiled))
    # more segments than workgroups: u8 at every size, and every (format, size) whose next segment's units do
    # not fit 16 registers (units a thread N / 512, dwords a unit 1, 1, 2, 4) and load at staging time
    walked = set(SCAN_WALK_CASES)
    assert walked <= tested and len(walked) == len(SCAN_WALK_CASES)
    assert {(l, 0) for l in range(8, 14)} <= walked and {f for _, f in walked} == {0, 1, 2, 3}
    late = {(l, f) for l, f in tested if max(1, (1 << l) // 512) * (1, 1, 2, 4)[f] > 16}
    assert late == {(13, 2), (12, 3), (13, 3)} and late <= walked


def test_rate_formats_are_complete(instantiations):
    compiled = {f for f, in instantiations["rate_ddc_kernel"]}  # rate_ddc_kernel<F>
    assert compiled == SWEEP_FORMATS and len(compiled) == 4, (compiled, SWEEP_FORMATS)


# ---- RATE_SWEEP: what each case makes rate_ddc_kernel do --------------------------------------------------------

def rate_plan(mode, cap_fs):
    """csrc/rate.hip and csrc/wide.h restated for one case: the phases in groups of pg <= 4, dealt to the
    four waves in turn (wave w takes the groups at phi = w pg, (w + 4) pg, ...), the last one ragged."""
    up, down = sweep_ratio(mode, cap_fs)
    turns = -(-(-(-up // 4)) // 4)
    pg = -(-up // (4 * turns))
    waves = [[min(pg, up - phi) for phi in range(w * pg, up, 4 * pg)] for w in range(4)]
    ip = oracle.MODES[mode][0] // 2
    b = up // math.gcd(up, ip)
    assert (b * ip * down) % up == 0
    hc = -(-16 // up)
    return {
        "up": up, "down": down, "pg": pg, "turns": turns, "waves": waves,
        "groups": sorted((g for w in waves for g in w), reverse=True),
        "rem": (16 * down + 1) % up,
        "loads": -(-down // 8),  # staging loads a thread and chunk: 32 M units over 256 threads
        "lds": 8 * (500 + down * ((64 + hc) | 1) + 64 * (up | 1)),
        "blocks": b, "wide_pairs": b * ip * down // up, "outputs": b * ip,
    }


def reachable_ups():
    """Every L in 2..48 some mode's rf_fs is a multiple of (rate_ratio: L / M in lowest terms, so L | rf_fs)."""
    return {up for m in oracle.MODES.values() for up in range(2, 49) if m[3] % up == 0}


def largest_down(up):
    return max(m for m in range(up + 1, min(125, 10 * up) + 1) if math.gcd(up, m) == 1)


def test_rate_sweep_is_inside_the_limits(fmrx):
    assert len(set(RATE_SWEEP)) == len(RATE_SWEEP)
    for mode, cap_fs in RATE_SWEEP:
        assert mode in (0, 1)
        rf_fs, p = oracle.MODES[mode][3], rate_plan(mode, cap_fs)
        d = fmrx.rate_design(rf_fs, cap_fs, sweep_offset(mode))  # the library accepts the rate and the offset
        assert (d["up"], d["down"]) == (p["up"], p["down"]) and d["coarse_hz"] == rf_fs // 4 and d["fine_hz"] == 50000
        assert 2 <= p["up"] <= 48 and p["up"] < p["down"] <= min(125, 10 * p["up"])
        assert sum(p["groups"]) == p["up"] and 1 <= p["pg"] <= 4 and max(len(w) for w in p["waves"]) == p["turns"]
        assert p["lds"] <= 8 * (500 + 125 * 65 + 64 * 49) < 160 * 1024  # 48/125 is the most there is
        assert p["wide_pairs"] < 200000 and p["outputs"] <= 15 * 3072  # a granule stays small (3/25: 160,000 pairs)
    assert all((0, cap_fs) in RATE_SWEEP for _, cap_fs in FORMAT_CASES)
    # the walking test's shapes (16 stations on 256 CUs): a target of one and of six workgroups a CU
    assert rate_target(48, 125, 256) == 256 and rate_target(15, 16, 256) == 1536


def test_rate_sweep_covers_every_reachable_up():
    """The 21 values of L, each in the mode that reaches it."""
    reachable = reachable_ups()
    assert reachable == {2, 3, 4, 5, 6, 8, 9, 10, 12, 15, 16, 18, 20, 24, 25, 30, 32, 36, 40, 45, 48}
    ups = {m: {sweep_ratio(m, c)[0] for mode, c in RATE_SWEEP if mode == m} for m in (0, 1)}
    assert ups[0] >= {2, 3, 4, 5, 6, 8, 10, 12, 15, 16, 20, 24, 25, 30, 32, 40, 48}
    assert ups[1] >= {9, 18, 36, 45}
    assert ups[0] | ups[1] == reachable


def test_rate_sweep_covers_every_grouping():
    plans = {sweep_ratio(m, c): rate_plan(m, c) for m, c in RATE_SWEEP}
    by_up = {up: p for (up, _), p in plans.items()}
    # rate_phases<1..4>, each as a whole group and 1, 2, 3 as a ragged last one
    assert {g for p in plans.values() for g in p["groups"]} == {1, 2, 3, 4}
    ragged = {up: dict(Counter(p["groups"])) for up, p in by_up.items() if len(set(p["groups"])) > 1}
    assert ragged == {5: {2: 2, 1: 1}, 10: {3: 3, 1: 1}, 15: {4: 3, 3: 1}, 20: {3: 6, 2: 1}, 25: {4: 6, 1: 1},
                      30: {4: 7, 2: 1}, 45: {4: 11, 1: 1}}
    assert {up for up, p in by_up.items() if p["pg"] == 4} == {15, 16, 25, 30, 32, 40, 45, 48}
    # one, two and three turns of the waves
    assert {p["turns"] for p in plans.values()} == {1, 2, 3}
    # a ratio without the phases of one tap more
    assert any(p["rem"] == 0 and up in (3, 5, 9, 15, 25, 45) for (up, _), p in plans.items())
    assert sum(p["rem"] != 0 for p in plans.values()) > len(plans) // 2
    # M = L + 1
    assert any(down == up + 1 for up, down in plans)
    # the largest M of L = 36 and 48, and a small L at M <= 10 L
    assert (36, 125) in plans and (48, 125) in plans and largest_down(36) == largest_down(48) == 125
    assert any(up <= 5 and down == largest_down(up) and down >= 10 * up - 1 for up, down in plans)
    assert (plans[(36, 125)]["lds"], plans[(48, 125)]["lds"]) == (87944, 94088)  # one workgroup a CU
    # staging loops of more than one batch of four loads with a ragged last batch; M even and odd
    assert any(p["loads"] > 4 and p["loads"] % 4 for p in plans.values())
    assert {1, 2, 3, 4} <= {p["loads"] for p in plans.values()}
    assert {down % 2 for up, down in plans if up >= 15} == {0, 1}


def test_rate_sweep_covers_the_radio_rates():
    """The rates of the radios the README names that reduce inside the limits."""
    want = {(0, 2560000): (15, 16), (0, 3000000): (4, 5), (0, 3200000): (3, 4), (0, 5000000): (12, 25),
            (0, 8000000): (3, 10), (0, 16000000): (3, 20), (0, 20000000): (3, 25),
            (1, 2560000): (9, 20), (1, 3200000): (9, 25), (1, 3000000): (48, 125), (1, 4000000): (36, 125),
            (1, 8000000): (18, 125)}
    for case, ratio in want.items():
        assert case in RATE_SWEEP and sweep_ratio(*case) == ratio, case
