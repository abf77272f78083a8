"""GPU tests of every stereo back-end kernel, launch route and band-pass length (csrc/stereo.hip behind
run_stereo_audio and run_stereo_pipelined of csrc/engine.cpp): the three 51-tap band-pass kernels and
bpf_pair_generic at the ends of the accepted range of bp_taps, each from the pinned staging buffer and from
the device, at calls under one tile, of whole tiles and of tiles plus a rest, and at a pipelined chunk's
offset; the three forms of the audio stage and every order in which one hands its carry to the next, with
a checkpoint into a second context after every call; the per-frame kernel of modes 2 and 3 split,
resumed and on several streams; and denormals, signed zeros and huge samples through the packed FIRs.

Expected values: stereo_ref.audio_compose, audio_thread restated from the pinned oracle's primitives at
any band-pass length (tests/test_stereo_variants_host.py pins it to the oracle's run_audio, to the
reference's fixtures and, live, to the reference's primitives), on the oracle's demod of each stream's own
I/Q.  Everything is compared bit for bit; there is no tolerance anywhere.

The case lists below are what tests/test_stereo_variants_host.py compares stereo.hip's kernels in the
library's symbol table with, through stereo_ref.stereo_plan: a kernel without a case fails the CPU suite."""
from __future__ import annotations

import functools
import hashlib
import os
from collections import namedtuple

import numpy as np
import pytest

import iqgen
import oracle
import stereo_ref
from stereo_ref import BP_R, BP_TILE, BPF_TAPS, audio_compose, special_demod, stereo_plan

pytestmark = pytest.mark.gpu

torch = None  # imported by the _gpu fixture: the case lists import without it

STEREO = 2  # fmrx.STEREO (include/fmrx.h), checked in run_case
STORED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stereo_bp.npz")

# One context and its calls.  rows: "iq" (each stream its own capture; audio_block gets the oracle's demod of
# it) or "special" (special_demod, audio_block only).  chunks: knob stereo_chunks (0: not set).
Case = namedtuple("Case", "name mode ns bp_taps bpf_tile entry chunks calls rows")

BP_FORMS = [(t, 1) for t in BPF_TAPS] + [(51, 0)]  # (bp_taps, knob bpf_tile): every length once, 51 both ways
FEW_FORMS = [(13, 1), (51, 1), (51, 0), (64, 1)]
CALLS_A = {0: (1, 2, 8, 1), 1: (1, 4, 3)}  # mode 0: 640, 1280, 5120, 640 IF samples; mode 1: 768, 3072, 2304


def _name(*parts):
    return "-".join(str(p) for p in parts)


def _form(t, tile):
    return f"bp{t}" + ("" if tile else "-notile")


# a. the band-pass forms of modes 0 and 1, from the pinned staging buffer (audio_block) and from the device
CASES_A = [Case(_name(f"mode{m}", e, _form(t, tile)), m, 3, t, tile, e, 0, CALLS_A[m], "iq")
           for m in (0, 1) for e in ("audio_block", "process") for t, tile in BP_FORMS]
# b. the band-pass forms at a pipelined chunk's offset.  One process of 6 blocks at stereo_chunks = 3: no chunk may
# be shorter than the front end's halo, two blocks in mode 0 (stereo_ref.halo_blocks), so the library makes two
# chunks of 3 blocks, the second at IF sample 1920; and one of 12 blocks, which it does cut in three: 3, 6, 3 blocks
# at IF samples 1920 and 5760.  No offset is a multiple of the tile.
CHUNKS_B = {6: [0, 3, 6], 12: [0, 3, 9, 12]}
CASES_B = [Case(_name("mode0-chunks3", f"{nb}blocks", _form(t, tile)), 0, 3, t, tile, "process", 3, (nb,), "iq")
           for nb in CHUNKS_B for t, tile in FEW_FORMS]
# c. modes 2 and 3: the per-frame audio kernel
SHAPES_C = [(2, "process", 0, (2, 1, 3)), (2, "process", 2, (3, 2)), (2, "audio_block", 0, (1, 2)),
            (3, "process", 0, (1, 2)), (3, "audio_block", 0, (2,))]
CASES_C = [Case(_name(f"mode{m}", e, f"chunks{k}", "x".join(map(str, calls)), _form(t, tile)), m, 2, t, tile, e, k, calls, "iq")
           for m, e, k, calls in SHAPES_C for t, tile in FEW_FORMS]
RESUME_C = {(3, "process"): (1,)}  # a checkpoint into a second context after these block counts
# d. the audio forms of modes 0 and 1 and their carries
# (knob stereo_chunks, calls, the route of each call, its chunks).  With the halo of two blocks the second list's
# calls of 6 and 7 blocks fall back to 2 chunks and its last, of 3 blocks, to the serial engine and so to the small
# kernel; the third list has calls that are cut in three and a last one that falls back to 2 chunks.
SHAPES_D = [(0, (1, 5, 4, 6, 2, 7), ["small", "serial", "small", "serial", "small", "serial"], [1, 1, 1, 1, 1, 1]),
            (3, (6, 1, 7, 1, 3), ["pipelined", "small", "pipelined", "small", "small"], [2, 1, 2, 1, 1]),
            (3, (12, 1, 13, 1, 6), ["pipelined", "small", "pipelined", "small", "pipelined"], [3, 1, 3, 1, 2])]
CASES_D = [Case(_name(f"mode{m}", f"chunks{k}", "x".join(map(str, calls))), m, 3, 51, 1, "process", k, calls, "iq")
           for m in (0, 1) for k, calls, _, _ in SHAPES_D]
PLAN_D = {(k, calls): (routes, counts) for k, calls, routes, counts in SHAPES_D}
# the float mono outlet, one case an audio form (and the tile form from both of its routes)
CASES_MONO = [Case("small", 0, 3, 51, 1, "process_device", 0, (2, 3), "iq"),
              Case("tile", 0, 3, 51, 1, "process_device", 0, (5, 6), "iq"),
              Case("tile-pipelined", 0, 3, 51, 1, "process_device", 3, (6, 7), "iq"),
              Case("frame", 2, 2, 51, 1, "process_device", 0, (1, 1), "iq")]
# e. special values through the packed FIRs
CASES_E = [Case(_name("mode0", _form(t, tile)), 0, 2, t, tile, "audio_block", 0, (2, 4), "special")
           for t, tile in [(51, 1), (51, 0), (13, 1)]] + [Case("mode2-bp51", 2, 2, 51, 1, "audio_block", 0, (1,), "special")]
# f. the route really taken, where Receiver.stage_timing can tell
CASES_F = [Case("small", 0, 3, 51, 1, "process", 0, (2,), "iq"), Case("serial", 0, 3, 51, 1, "process", 0, (6,), "iq"),
           Case("pipelined", 0, 3, 51, 1, "process", 3, (6,), "iq"), Case("pipelined-3", 0, 3, 51, 1, "process", 3, (12,), "iq")]
CHUNKS_F = {"small": 1, "serial": 1, "pipelined": 2, "pipelined-3": 3}
# the reference's stored rows (tests/golden/stereo_bp.npz) at every length
CASES_STORED = [Case(_name(f"mode{m}", f"bp{t}"), m, 1, t, 1, "audio_block", 0, (2, 4), "stored") for m in (0, 1) for t in BPF_TAPS]

ALL_CASES = CASES_A + CASES_B + CASES_C + CASES_D + CASES_MONO + CASES_E + CASES_F + CASES_STORED


def plans(case):
    """stereo_plan of each call of the case."""
    return [stereo_plan(case.mode, case.bp_taps, case.bpf_tile, case.entry, case.ns, nb, case.chunks) for nb in case.calls]


def ids(cases):
    return [c.name for c in cases]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    global torch
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


# ---- inputs and expected values, computed once a module ------------------------------------------------------

def recipe(mode, s):
    """Stream s's capture: a synthetic station, random bytes, another station."""
    return (f"synth:{200 + mode}", f"rand:{210 + mode}", f"synth:{220 + mode}")[s]


@functools.lru_cache(maxsize=None)
def iq_row(mode, s, n_blocks):
    a = iqgen.make(recipe(mode, s), n_blocks * oracle.MODES[mode][0], oracle.MODES[mode][3])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def demod_row(mode, s, n_blocks, rows="iq"):
    if rows == "special":  # stream 1: the same samples with the other sign
        d = special_demod(mode, n_blocks) * np.float32(1 if s == 0 else -1)
    elif rows == "stored":
        d = np.load(STORED)[f"demod_m{mode}"][: n_blocks * oracle.MODES[mode][1]]
    else:
        d = oracle.Oracle().run(mode, 51, iq_row(mode, s, n_blocks), ["demod"])["demod"]
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def expected(mode, s, n_blocks, bp_taps, rows="iq"):
    """The composition of stream s over n_blocks blocks; a shorter run of the same stream is its prefix."""
    out = audio_compose(oracle.Oracle(), mode, demod_row(mode, s, n_blocks, rows), bp_taps)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


MOST_BLOCKS = {0: 33, 1: 33, 2: 6, 3: 3}  # the longest case of each mode: shorter ones take its prefix


def blocks_of(case):
    return sum(case.calls) if case.rows != "iq" else MOST_BLOCKS[case.mode]


def want_pcm(case):
    nb, ps = sum(case.calls), 2 * oracle.MODES[case.mode][2]
    return np.stack([expected(case.mode, s, blocks_of(case), case.bp_taps, case.rows)["pcm"][: nb * ps] for s in range(case.ns)])


# ---- running a case ----------------------------------------------------------------------------------------

def receiver(fm, case):
    knobs = {"bpf_tile": case.bpf_tile}
    if case.chunks:
        knobs["stereo_chunks"] = case.chunks
    return fm.Receiver(case.mode, fm.STEREO, n_streams=case.ns, bp_taps=case.bp_taps, knobs=knobs)


def call(rx, case, b0, nb, want_mono=False):
    """Blocks [b0, b0 + nb) of every stream through the case's entry: PCM rows (ns x 2 nb frames), and the float
    mono rows where asked (process_device)."""
    be, nif, na = oracle.MODES[case.mode][:3]
    if case.entry == "audio_block":
        d = np.stack([demod_row(case.mode, s, blocks_of(case), case.rows)[b0 * nif:(b0 + nb) * nif] for s in range(case.ns)])
        return rx.audio_block(d).reshape(case.ns, -1), None
    iq = np.stack([iq_row(case.mode, s, blocks_of(case))[b0 * be:(b0 + nb) * be] for s in range(case.ns)])
    if case.entry == "process":
        return rx.process(iq).reshape(case.ns, -1), None
    d_iq = torch.from_numpy(np.ascontiguousarray(iq)).cuda()
    d_pcm = torch.zeros(case.ns * nb * 2 * na, dtype=torch.int16, device="cuda")
    d_mono = torch.zeros(case.ns * nb * na, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rx.process_device(d_iq.data_ptr(), nb, d_pcm.data_ptr(), d_mono.data_ptr() if want_mono else None)
    rx.synchronize()
    return d_pcm.cpu().numpy().reshape(case.ns, -1), d_mono.cpu().numpy().reshape(case.ns, -1)


def where(case, got, want, band_pass):
    """The first differing PCM sample of the case: stream, call, block and frame, the plan's kernels, and for a
    band-pass case the newest IF sample that frame reads as the band-pass launch's tile, thread and r."""
    if got.shape != want.shape:
        return f"{case.name}: shapes {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return "equal"
    s, i = (int(v) for v in bad[0])
    _, nif, na, _, _, _, up, down = oracle.MODES[case.mode]
    frame, b0 = i // 2, 0
    for n, (nb, plan) in enumerate(zip(case.calls, plans(case))):
        if frame < (b0 + nb) * na:
            break
        b0 += nb
    f = frame - b0 * na  # frame of the call
    msg = (f"{case.name}: {len(bad)} of {got.size} PCM samples differ, first in stream {s}, call {n} ({nb} blocks, route "
           f"{plan['route']}), block {f // na} of the call, frame {f % na}, {'RL'[i % 2]}: got {got[s, i]} want {want[s, i]}; "
           f"kernels {plan['bpf']}{' from src' if plan['src'] else ''}{' after the 2-D copy of ' + plan['copy'] if plan['copy'] else ''}"
           f", {', '.join(plan['audio'])}; chunks {plan['chunks']}")
    if band_pass:
        j = (f // na) * nif + (f % na) * down // up  # the newest IF sample of the call the frame's stereo sum reads
        k = max(c for c, off in enumerate(plan["bpf_offset"]) if off <= j)
        j -= plan["bpf_offset"][k]
        msg += (f"; IF sample {j} of band-pass launch {k} (n_if {plan['bpf_n_if'][k]}): tile {j // BP_TILE}, "
                f"thread {j % BP_TILE // BP_R}, r {j % BP_R}")
    return msg


def run_case(fm, case, band_pass, resume_at=(), want_mono=False):
    """The case's calls on one context (the first from zero history, the rest from the carried one) against the
    composition; after each block count of resume_at, the state through a second context, which runs the rest of
    the stream in one call.  Returns the float mono rows (process_device)."""
    assert fm.STEREO == STEREO
    want, ps = want_pcm(case), 2 * oracle.MODES[case.mode][2]
    parts, monos, pos = [], [], 0
    with receiver(fm, case) as rx:
        assert rx.geo.bp_taps == case.bp_taps
        for nb in case.calls:
            pcm, mono = call(rx, case, pos, nb, want_mono)
            parts.append(pcm)
            monos.append(mono)
            pos += nb
            if pos in resume_at and pos < sum(case.calls):
                blob = rx.get_state()
                rest = case._replace(name=f"{case.name}, resumed after {pos} blocks", calls=(sum(case.calls) - pos,))
                with receiver(fm, case) as rx2:
                    rx2.set_state(blob)
                    tail, _ = call(rx2, case, pos, rest.calls[0])
                assert np.array_equal(tail, want[:, pos * ps:]), where(rest, tail, want[:, pos * ps:], band_pass)
    got = np.concatenate(parts, axis=1)
    assert np.array_equal(got, want), where(case, got, want, band_pass)
    assert all(row.any() for row in got) and len({row.tobytes() for row in got}) == case.ns
    return np.concatenate(monos, axis=1) if want_mono else None


# ---- a, b. the band-pass forms ------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES_A, ids=ids(CASES_A))
def test_band_pass_forms(fmrx, case):
    """Every band-pass length on three distinct streams, from the pinned staging buffer (src set: the tile kernel
    reads it in place, the per-output kernels after launch_bpf_pair's 2-D copy) and in the serial engine; calls
    under one tile, of whole tiles and of tiles plus 256."""
    pl = plans(case)
    assert all(p["src"] == (case.entry == "audio_block") and len(p["bpf_n_if"]) == 1 for p in pl)
    run_case(fmrx, case, band_pass=True)


@pytest.mark.parametrize("case", CASES_B, ids=ids(CASES_B))
def test_band_pass_forms_at_an_offset(fmrx, case):
    """One pipelined call: the band-pass launches of the chunks past the first start at IF samples 1920 and 5760 of
    the call, neither a multiple of the tile."""
    (p,) = plans(case)
    assert p["route"] == "pipelined" and p["chunks"] == CHUNKS_B[case.calls[0]]
    assert p["bpf_offset"] == [0, 1920, 5760][: len(p["chunks"]) - 1] and all(off % BP_TILE for off in p["bpf_offset"][1:])
    run_case(fmrx, case, band_pass=True)


# ---- c. modes 2 and 3 ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES_C, ids=ids(CASES_C))
def test_per_frame_audio_kernel(fmrx, case):
    """stereo_audio_kernel on two distinct streams: calls split, pipelined (mode 2), resumed through a second
    context (mode 3), from the pinned staging buffer (mode 2) and past its limit (mode 3: 5.2 MB, the 2-D
    copy to the device on distinct rows)."""
    pl = plans(case)
    assert all(stereo_ref.AUDIO_FRAME in p["audio"] for p in pl)
    if case.entry == "audio_block":
        assert [p["copy"] == "entry" for p in pl] == [case.mode == 3] * len(pl)
    if case.chunks:
        assert [p["chunks"] for p in pl] == [[0, 1, 3], [0, 1, 2]]
    run_case(fmrx, case, band_pass=True, resume_at=RESUME_C.get((case.mode, case.entry), ()))


# ---- d. the audio forms and their carries ------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES_D, ids=ids(CASES_D))
def test_audio_forms_and_carries(fmrx, case):
    """small, tile and pipelined calls in turn: mix_tail, mono_state, the demod history and PLL slot 4 written by
    one form and read by the next; after every call the state also goes through a second context."""
    pl = plans(case)
    routes, counts = PLAN_D[case.chunks, case.calls]
    assert [p["route"] for p in pl] == routes and [len(p["chunks"]) - 1 for p in pl] == counts
    assert all(stereo_ref.AUDIO_TILE in p["audio"] for p in pl if p["route"] != "small")
    run_case(fmrx, case, band_pass=False, resume_at=tuple(np.cumsum(case.calls)))


@pytest.mark.parametrize("case", CASES_MONO, ids=ids(CASES_MONO))
def test_float_mono_outlet(fmrx, case):
    """fmrx_process_device_ex's d_mono of a stereo context: the shared-history mono of every audio form."""
    assert {p["route"] for p in plans(case)} == {{"small": "small", "tile": "serial", "tile-pipelined": "pipelined",
                                                  "frame": "serial"}[case.name]}
    assert case.name != "tile-pipelined" or [p["chunks"] for p in plans(case)] == [[0, 3, 6], [0, 3, 7]]
    mono = run_case(fmrx, case, band_pass=False, want_mono=True)
    na = oracle.MODES[case.mode][2]
    for s in range(case.ns):
        want = expected(case.mode, s, blocks_of(case), 51)["mono_exact"][: sum(case.calls) * na]
        got = mono[s]
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (f"{case.name}: mono of stream {s} differs at {bad.size} frames, first block {bad[0] // na} "
                               f"frame {bad[0] % na}: got {got[bad[0]]!r} want {want[bad[0]]!r}; {plans(case)[0]['audio']}")


# ---- e. special values -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES_E, ids=ids(CASES_E))
def test_special_values(fmrx, case):
    """Denormals, -0.0, the smallest normals and +-1e30 in the demod: the packed FIRs keep f32 denormals
    (DESIGN section 5); a flush in the band-pass pair changes the carrier, the PLL's atan2 and every later sample
    (tests/test_stereo_variants_host.py shows that it changes this PCM)."""
    run_case(fmrx, case, band_pass=True)


# ---- f. the route really taken ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES_F, ids=ids(CASES_F))
def test_route_taken(fmrx, case):
    (p,) = plans(case)
    assert p["route"] == case.name.split("-")[0] and len(p["chunks"]) - 1 == CHUNKS_F[case.name]
    want = want_pcm(case)
    with receiver(fmrx, case) as rx:
        rx.stage_timing(1)
        got, _ = call(rx, case, 0, case.calls[0])
        st = {k: int(v[1]) for k, v in rx.stage_timing(-1).items()}
    assert np.array_equal(got, want), where(case, got, want, False)
    if p["route"] == "small":  # the NCO, the audio, the carry and the history in one launch
        assert "pll_nco" not in st and st["audio"] == 1 and st["bandpass_pair"] == 1, st
    elif p["route"] == "serial":
        assert st["pll_nco"] == 1 and st["bandpass_pair"] == 1 and st["audio"] == 1, st
    else:
        assert st["bandpass_pair"] == st["audio"] == st["front_end"] == len(p["chunks"]) - 1, st


# ---- the reference's stored rows ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES_STORED, ids=ids(CASES_STORED))
def test_stored_rows_match_the_reference(fmrx, case):
    """The demod rows of tests/golden/stereo_bp.npz through audio_block at every band-pass length against the
    SHA-256 of the PCM the reference's own primitives composed (tests/golden/make_stereo_bp.py)."""
    z = np.load(STORED)
    with receiver(fmrx, case) as rx:
        parts, pos = [], 0
        for nb in case.calls:
            parts.append(call(rx, case, pos, nb)[0])
            pos += nb
    got = np.concatenate(parts, axis=1)
    want = expected(case.mode, 0, sum(case.calls), case.bp_taps, "stored")["pcm"][None, :]
    assert np.array_equal(got, want), where(case, got, want, True)
    assert hashlib.sha256(np.ascontiguousarray(got[0]).tobytes()).hexdigest() == str(z[f"pcm_sha256_m{case.mode}_bp{case.bp_taps}"])
