"""CPU side of tests/test_gpu_stereo_variants.py: what the GPU matrix is compared with is right, the matrix
is complete, and its cases could fail.

  pins     stereo_ref.audio_compose at 51 taps is the pinned oracle's run_audio, field by field, and the
           reference's golden PCM; at every other length it is the same composition of the reference's own
           primitives (live where the reference build is present, and through tests/golden/stereo_bp.npz,
           which that build wrote, everywhere).
  guard    the kernels of csrc/stereo.hip in libfmrx.so's symbol table (`nm -C`: names only, never the
           code) are exactly those stereo_ref.stereo_plan names over the GPU file's case lists; the lists hold
           the tile edges and the carry transitions they are there for.  pll_fallback_test_kernel, the test hook
           of tests/test_gpu_parity.py in the same file, is no part of the chain.
  teeth    another band-pass length gives other PCM on the matrix's inputs, and a band-pass pair that
           flushed subnormals would give other PCM on the special-values input."""
from __future__ import annotations

import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle
import stereo_ref
from conftest import golden_cases, load_case
from stereo_ref import BP_TILE, BPF_TAPS, audio_compose, flush_subnormals, special_demod, stereo_plan
from test_gpu_stereo_variants import (ALL_CASES, CALLS_A, CASES_A, CASES_B, CASES_C, CASES_D, CASES_E, CASES_MONO, CASES_F,
                                      CASES_STORED, MOST_BLOCKS, STORED, demod_row, expected, plans)

import iqgen

FIELDS = ("pcm", "mono_exact", "channel", "carrier", "nco", "mixer", "stereo", "left", "right", "pll_state")
BP_RATES = (240000, 288000, 256000)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- pins ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_composition_is_run_audio(orc, mode):
    """Block by block with the shared audio_state, 51 taps: every output of Oracle.run_audio, and a run
    continued from the returned state."""
    nb = 3 if mode < 2 else 2
    nif = oracle.MODES[mode][1]
    demod = iqgen.make_rds_demod(5 + mode, nb * nif, oracle.MODES[mode][5])
    want = orc.run_audio(mode, demod)
    got = audio_compose(orc, mode, demod)
    for f in FIELDS:
        assert same(got[f], want[f]), (mode, f)
    head = audio_compose(orc, mode, demod[:nif])
    tail = audio_compose(orc, mode, demod[nif:], state=head["state"])
    for f in FIELDS:
        assert same(np.concatenate([head[f], tail[f]]), want[f]), (mode, f)


GOLDEN_WITH_DEMOD = [n for n in golden_cases() if {"demod", "pcm"} <= set(load_case(n))]


@pytest.mark.parametrize("name", GOLDEN_WITH_DEMOD)
def test_composition_is_the_golden_pcm(orc, name):
    """Fixtures the reference wrote: its PCM, and its intermediates where stored, from its demod."""
    z = load_case(name)
    got = audio_compose(orc, z["mode"], z["demod"])
    assert np.array_equal(got["pcm"], z["pcm"])
    for f in FIELDS[1:]:
        if f in z:
            assert same(got[f], z[f]), (name, f)


def test_golden_cases_were_found():
    assert len(GOLDEN_WITH_DEMOD) >= 8 and {load_case(n)["mode"] for n in GOLDEN_WITH_DEMOD} == {0, 1}


@pytest.mark.parametrize("bp_taps", BPF_TAPS)
@pytest.mark.parametrize("mode", [0, 1])
def test_composition_is_the_reference_at_every_length(ref, mode, bp_taps):
    """Live: the same composition of the reference's own resample, PLL, mixer, LRExtraction and quantiser on
    the three streams of the GPU matrix (skipped where the reference build is absent)."""
    for s in range(3):
        want = audio_compose(ref, mode, demod_row(mode, s, MOST_BLOCKS[mode]), bp_taps)
        got = expected(mode, s, MOST_BLOCKS[mode], bp_taps)
        for f in FIELDS:
            assert same(got[f], want[f]), (mode, bp_taps, s, f)


@pytest.fixture(scope="module")
def stored():
    assert os.path.getsize(STORED) <= 64 * 1024
    return np.load(STORED)


def test_stored_tables_are_the_designs(fmrx, orc, stored):
    """The reference's band-pass tables at every length and rate: the library's design and the oracle's."""
    for fs in BP_RATES:
        for t in BPF_TAPS:
            for name, (fb, fe) in (("ch", (22000.0, 54000.0)), ("ca", (18500.0, 19500.0))):
                want = stored[f"{name}_fs{fs}_bp{t}"]
                assert want.size == t and want.any()
                assert same(fmrx.bpf(float(fs), fb, fe, t), want), (fs, t, name)
                assert same(orc.bpf(float(fs), fb, fe, t), want), (fs, t, name)
    assert len(stored.files) == 2 * len(BP_RATES) * len(BPF_TAPS) + 2 + 2 * len(BPF_TAPS)


@pytest.mark.parametrize("bp_taps", BPF_TAPS)
@pytest.mark.parametrize("mode", [0, 1])
def test_stored_hashes_are_the_composition(stored, mode, bp_taps):
    """The reference-composed PCM of the stored rows, by its SHA-256, from the oracle's primitives."""
    demod = stored[f"demod_m{mode}"]
    assert demod.size == 6 * oracle.MODES[mode][1] and same(demod, demod_row(mode, 0, 6, "stored"))
    pcm = expected(mode, 0, 6, bp_taps, "stored")["pcm"]
    assert hashlib.sha256(pcm.tobytes()).hexdigest() == str(stored[f"pcm_sha256_m{mode}_bp{bp_taps}"])
    assert len({str(stored[f"pcm_sha256_m{mode}_bp{t}"]) for t in BPF_TAPS}) == len(BPF_TAPS)


# ---- guard -----------------------------------------------------------------------------------------------------

FAMILIES = ("bpf_pair_kernel", "bpf_pair_tile_kernel", "bpf_pair_generic", "stereo_audio_kernel", "stereo_audio_tile_kernel",
            "stereo_audio_small_kernel", "stereo_state_kernel", "pll_nco_kernel")


@pytest.fixture(scope="module")
def compiled(fmrx):
    """The kernels of csrc/stereo.hip in the library, as "name" or "name<arguments>"."""
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm is not on this machine")
    out = subprocess.run([nm, "-C", fmrx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    found = re.findall(r"\b(%s)(<(?:[-0-9]+|true|false)(?:, (?:[-0-9]+|true|false))*>)?\(" % "|".join(FAMILIES), out)
    return {name + args for name, args in found}


def test_matrix_names_every_kernel(compiled):
    assert compiled == stereo_ref.STEREO_KERNELS == {
        "bpf_pair_kernel<51>", "bpf_pair_tile_kernel<51, true>", "bpf_pair_tile_kernel<51, false>", "bpf_pair_generic",
        "stereo_audio_kernel", "stereo_audio_tile_kernel", "stereo_audio_small_kernel", "stereo_state_kernel",
        "pll_nco_kernel"}, sorted(compiled ^ stereo_ref.STEREO_KERNELS)
    tested = set().union(*(stereo_ref.plan_kernels(p) for c in ALL_CASES for p in plans(c)))
    assert tested == compiled, (sorted(compiled - tested), sorted(tested - compiled))
    # ... and the comparing tests alone (not the route and the stored-row tests) name them all as well
    core = CASES_A + CASES_B + CASES_C + CASES_D + CASES_E
    assert set().union(*(stereo_ref.plan_kernels(p) for c in core for p in plans(c))) == compiled


def test_case_lists_are_the_issue_s():
    assert len({c.name for c in CASES_A}) == len(CASES_A) == 2 * 2 * (len(BPF_TAPS) + 1)
    assert (len(CASES_B), len(CASES_C), len(CASES_D), len(CASES_MONO), len(CASES_E), len(CASES_F)) == (8, 20, 6, 4, 4, 4)
    assert len(CASES_STORED) == 2 * len(BPF_TAPS)
    assert all(c.ns == 3 for c in CASES_A + CASES_B + CASES_D) and all(c.ns == 2 for c in CASES_C)
    assert {(c.bp_taps, c.bpf_tile) for c in CASES_A} == {(t, 1) for t in BPF_TAPS} | {(51, 0)}
    for c in CASES_A:  # the issue's tables: IF samples of each call against the tile
        n_if = [p["bpf_n_if"] for p in plans(c)]
        assert n_if == {0: [[640], [1280], [5120], [640]], 1: [[768], [3072], [2304]]}[c.mode]
        assert c.calls == CALLS_A[c.mode]
    for c in CASES_B:
        (p,) = plans(c)
        assert p["route"] == "pipelined" and c.chunks == 3 and c.calls[0] in (6, 12)
        assert (p["bpf_n_if"], p["bpf_offset"]) == {6: ([1920, 1920], [0, 1920]), 12: ([1920, 3840, 1920], [0, 1920, 5760])}[c.calls[0]]
        assert all(off % BP_TILE for off in p["bpf_offset"][1:])


def test_plan_restates_the_host():
    """Spot values of engine.cpp's arithmetic: the small route's limit, the pinned limit, the chunk partition."""
    assert [stereo_plan(0, 51, 1, "process", 3, nb)["route"] for nb in (1, 4, 5)] == ["small", "small", "serial"]
    assert stereo_plan(2, 51, 1, "process", 2, 1)["route"] == "serial"  # modes 2 and 3 never take the small kernel
    assert stereo_plan(2, 51, 1, "process", 2, 1)["audio"] == (stereo_ref.NCO, stereo_ref.AUDIO_FRAME, stereo_ref.STATE)
    # fmrx_audio_block: 4 MiB of demod; 3 streams of mode 0 are 546 blocks, the 547th goes to the device
    assert stereo_plan(0, 51, 1, "audio_block", 3, 546)["src"] and not stereo_plan(0, 51, 1, "audio_block", 3, 547)["src"]
    assert stereo_plan(2, 51, 1, "audio_block", 2, 2)["bpf"] == stereo_ref.BPF_TILE_SRC
    p = stereo_plan(3, 51, 1, "audio_block", 2, 2)  # 5.2 MB
    assert (p["src"], p["copy"], p["bpf"]) == (False, "entry", stereo_ref.BPF_TILE)
    assert stereo_plan(0, 13, 1, "audio_block", 3, 1)["copy"] == "launch" and stereo_plan(0, 51, 0, "audio_block", 3, 1)["copy"] == "launch"
    assert stereo_plan(0, 51, 1, "audio_block", 3, 1)["copy"] is None and stereo_plan(0, 13, 1, "process", 3, 1)["copy"] is None
    # stereo_chunks: the knob, lowered while a chunk would be shorter than the halo (two blocks in modes 0 and 1,
    # one in modes 2 and 3); the default from 16 streams on
    assert [stereo_ref.halo_blocks(m) for m in range(4)] == [2, 2, 1, 1]
    assert [stereo_plan(0, 51, 1, "process", 3, nb, 3)["chunks"] for nb in (1, 3, 6, 7, 12)] == [[0, 1], [0, 3], [0, 3, 6], [0, 3, 7], [0, 3, 9, 12]]
    assert [stereo_plan(2, 51, 1, "process", 2, nb, 2)["chunks"] for nb in (1, 2, 3)] == [[0, 1], [0, 1, 2], [0, 1, 3]]
    assert stereo_plan(0, 51, 1, "process", 16, 26)["chunks"] == [0, 26] and len(stereo_plan(0, 51, 1, "process", 16, 300)["chunks"]) == 9
    assert stereo_plan(0, 51, 1, "audio_block", 3, 6, 3)["route"] == "serial"  # the split API never pipelines


def test_band_pass_launches_cover_the_tile_edges():
    """Each 51-tap kernel meets a launch under one tile, one of whole tiles and one of tiles plus a rest; the
    generic kernel too; and a pipelined chunk starts where no tile does."""
    n_if = {}
    for c in CASES_A + CASES_B + CASES_C + CASES_E:
        for p in plans(c):
            n_if.setdefault(p["bpf"], set()).update(p["bpf_n_if"])
    for k in (stereo_ref.BPF_TILE_SRC, stereo_ref.BPF_TILE, stereo_ref.BPF_51, stereo_ref.BPF_GENERIC):
        ns = n_if[k]
        assert any(n < BP_TILE for n in ns), k
        assert any(n % BP_TILE == 0 for n in ns), k
        assert any(n > BP_TILE and n % BP_TILE for n in ns), k
    for k in (stereo_ref.BPF_TILE, stereo_ref.BPF_51, stereo_ref.BPF_GENERIC):
        assert any(p["bpf"] == k and any(off % BP_TILE for off in p["bpf_offset"]) for c in CASES_B for p in plans(c)), k
    # both 2-D copies, and the src form, on distinct rows
    copies = {(p["copy"], p["bpf"]) for c in CASES_A + CASES_C for p in plans(c)}
    assert {("launch", stereo_ref.BPF_51), ("launch", stereo_ref.BPF_GENERIC), ("entry", stereo_ref.BPF_TILE),
            ("entry", stereo_ref.BPF_51), ("entry", stereo_ref.BPF_GENERIC)} <= copies


def form(case, plan):
    """The audio form of a call: the per-frame kernel (modes 2, 3), or of modes 0 and 1 the small kernel, the tile
    kernel of the serial engine, or the tile kernel chunk by chunk."""
    if stereo_ref.AUDIO_FRAME in plan["audio"]:
        return "frame"
    return {"small": "small", "serial": "tile", "pipelined": "pipelined"}[plan["route"]]


def test_every_carry_transition_occurs():
    seen = set()
    for c in CASES_C + CASES_D:
        forms = [form(c, p) for p in plans(c)]
        seen |= set(zip(forms, forms[1:]))
    assert seen >= {("small", "tile"), ("tile", "small"), ("pipelined", "small"), ("small", "pipelined"),
                    ("frame", "frame")}, seen
    # per-frame to per-frame in both modes, pipelined and through fmrx_audio_block as well
    frames = {(c.mode, c.entry, bool(c.chunks)) for c in CASES_C if len(c.calls) > 1}
    assert frames == {(2, "process", False), (2, "process", True), (2, "audio_block", False), (3, "process", False)}
    # a pipelined call cut in two and in three, and one that falls back from three chunks to two after others
    counts = [[len(p["chunks"]) - 1 for p in plans(c)] for c in CASES_D]
    assert [2, 1, 2, 1, 1] in counts and [3, 1, 3, 1, 2] in counts and all(len(c.calls) >= 5 for c in CASES_D)


# ---- teeth -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
def test_another_length_is_other_pcm(mode):
    """A kernel that ignored bp_taps, or took the 51-tap tables, could not pass: on every stream of the band-pass
    cases every other length changes most PCM samples."""
    nb = sum(CALLS_A[mode])
    n = nb * 2 * oracle.MODES[mode][2]
    for s in range(3):
        at51 = expected(mode, s, MOST_BLOCKS[mode], 51)["pcm"][:n]
        assert at51.any()
        for t in BPF_TAPS:
            if t != 51:
                other = expected(mode, s, MOST_BLOCKS[mode], t)["pcm"][:n]
                assert np.mean(other != at51) > 0.5, (mode, s, t)


@pytest.mark.parametrize("case", CASES_E, ids=[c.name for c in CASES_E])
def test_special_values_input_has_teeth(orc, case):
    """The special-values rows leave every output of the composition finite, put subnormals into the band-pass
    outputs, and a band-pass pair that flushed them gives other PCM."""
    nb = sum(case.calls)
    tiny = np.finfo(np.float32).tiny
    for s in range(case.ns):
        demod = demod_row(case.mode, s, nb, "special")
        assert np.isfinite(demod).all() and np.any((demod != 0) & (np.abs(demod) < tiny))
        assert np.count_nonzero(np.signbit(demod) & (demod == 0)) == (120 if s == 0 else 0) and np.count_nonzero(demod == 0) == 120
        assert np.abs(demod).max() == np.float32(1e30)
        got = expected(case.mode, s, nb, case.bp_taps, "special")
        for f in FIELDS[1:]:
            assert np.isfinite(got[f]).all(), (case.name, s, f)
        # every carrier window inside the run of 200 denormals (151 of them at 51 taps); the channel's pass band
        # rejects their alternating signs, and its sums there cancel to zero
        car = got["carrier"]
        assert np.count_nonzero((car != 0) & (np.abs(car) < tiny)) >= 200 - case.bp_taps + 1, (case.name, s)
        flushed = audio_compose(orc, case.mode, demod, case.bp_taps, flush=flush_subnormals)
        assert not np.array_equal(flushed["pcm"], got["pcm"]), (case.name, s)
    assert same(special_demod(case.mode, nb), demod_row(case.mode, 0, nb, "special"))
