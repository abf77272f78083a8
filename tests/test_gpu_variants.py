"""GPU tests of every compiled front-end kernel variant and launch regime: each instantiation of
tuner_kernel<T, D, R, PD, F> (csrc/tuner.hip), wide_ddc_kernel<D, F> (csrc/wide.hip) and every
(T, D, AD, AU) of mono_fused_kernel (csrc/mono_fused.hip) is launched and compared with a
reference; so are the regimes in which a workgroup walks several chunks, the largest rotator
table, and I/Q rows that are not 16-byte aligned.

Expected values: narrow_compose and wide_compose of tests/test_wide_host.py (the format's
normalisation and the rotations in numpy float32, the oracle's resample, FMDemod and audio thread)
and the pinned oracle's run().  Everything is compared bit for bit -- np.array_equal for PCM, the
uint32 views for float rows -- and there is no tolerance anywhere.

The parameter lists below (TUNER_CASES, WIDE_CASES, FUSED_CASES) are also what
tests/test_variants_host.py compares the library's symbol table with: an instantiation compiled
without a case here fails the CPU suite."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import iqgen
import oracle
from test_formats_host import DTYPES, F32, S8, S16, U8, identity_map
from test_wide_host import narrow_compose, wide_compose

pytestmark = pytest.mark.gpu

torch = None  # imported by the _gpu fixture: the parameter lists import without it

NAMES = {U8: "u8", S8: "s8", S16: "s16", F32: "f32"}
FORMATS = (U8, S8, S16, F32)
MONO, STEREO = 1, 2  # fmrx.MONO, fmrx.STEREO (include/fmrx.h), checked in test_fused_matches_oracle

# 1a: tuner_kernel<T, D, ., ., F> -- D is the mode's RF decimation (10, 4, 9 in modes 0, 1, 3)
TUNER_CASES = [(mode, rf_taps, fmt) for mode in (0, 1, 3) for rf_taps in (51, 101) for fmt in FORMATS]
# 1c: wide_ddc_kernel<D, F>
WIDE_CASES = [(d, fmt) for d in range(2, 11) for fmt in FORMATS]
# 1e: mono_fused_kernel<T, D, AD, ..., AU, .>
FUSED_CASES = [(mode, rf_taps, ch) for mode in (0, 1, 2, 3) for rf_taps in (51, 101) for ch in (MONO, STEREO)]


def rf_decim(mode):
    return oracle.MODES[mode][3] // oracle.MODES[mode][5]


def fused_variants(mode, rf_taps, channels):
    """The (T, D, AD, AU) a FUSED_CASES case launches (launch_mono_fused): a mono `process` runs
    the mode's audio stage in the kernel; rf_block and the stereo engine take the RF-only form,
    which in modes 2 and 3 (AU > 1) is compiled with the placeholder AD = 5."""
    up, down = oracle.MODES[mode][6], oracle.MODES[mode][7]
    rf_only = (rf_taps, rf_decim(mode), down if up == 1 else 5, 1)
    return {rf_only} if channels == STEREO else {rf_only, (rf_taps, rf_decim(mode), down, up)}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    global torch
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def first_difference(got, want, per_chunk, per_lane):
    """Where two rows first differ: the index, and the chunk and lane of the kernel it falls in."""
    got, want = bits(got).reshape(-1), bits(want).reshape(-1)
    if got.size != want.size:
        return f"sizes {got.size} != {want.size}"
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return "equal"
    i = int(bad[0])
    return (f"{bad.size} of {got.size} differ, first at {i} (chunk {i // per_chunk}, lane {i % per_chunk // per_lane}): "
            f"got {got[i]} want {want[i]}")


@functools.lru_cache(maxsize=None)
def synth(seed, mode, n_elems):
    a = iqgen.make(f"synth:{seed}", n_elems, oracle.MODES[mode][3])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def capture(seed, mode, n_elems, fmt):
    """The synthetic station's bytes carried into fmt, then moved off the identity map as
    test_gpu_wide.py::test_formats does: s16 gets low bits (not only multiples of 256), f32 is scaled by
    1.7 (a full mantissa) and stays inside the promised range, 0 or [2^-20, 4]."""
    raw = identity_map(synth(seed, mode, n_elems), fmt)
    if fmt == S16:
        raw = (raw.astype(np.int32) + (np.arange(raw.size) * 7919) % 251 - 125).clip(-32768, 32767).astype(np.int16)
    elif fmt == F32:
        raw = (raw * np.float32(1.7)).astype(np.float32)
        assert np.abs(raw).max() <= 4.0 and np.all((raw == 0) | (np.abs(raw) >= 2.0 ** -20))
    assert raw.dtype == DTYPES[fmt]
    raw.setflags(write=False)
    return raw


def receiver(fm, fmt, mode, channels=MONO, decim=1, **kw):
    rx = fm.Receiver(mode, channels, **kw)
    if fmt != U8:
        rx.set_input_format(fmt)
    if decim != 1:
        rx.set_capture_decim(decim)
    assert (rx.input_format, rx.capture_decim) == (fmt, decim)
    return rx


def in_calls(fn, raw, be, calls):
    """fn over consecutive calls of `calls` blocks of be elements each, concatenated along the last axis."""
    out, b = [], 0
    for nb in calls:
        out.append(fn(raw[..., b * be:(b + nb) * be]))
        b += nb
    return np.concatenate(out, axis=-1)


def tuner_chunk(mode):
    """(IF samples a chunk, a lane) of tuner_kernel and of mono_fused_kernel's default variant:
    one wave, R = 3 outputs a lane (2 at the odd decimation 9)."""
    r = 2 if rf_decim(mode) == 9 else 3
    return 64 * r, r


# ---- 1a. the tuner matrix: every (taps, decimation, format) -----------------------------------------------

@pytest.mark.parametrize("mode,rf_taps,fmt", TUNER_CASES,
                         ids=[f"mode{m}-rf{t}-{NAMES[f]}" for m, t, f in TUNER_CASES])
def test_tuner_matrix(fmrx, mode, rf_taps, fmt):
    offset = 100000  # table periods 24, 288 and 576 pairs in modes 0, 1 and 3
    assert fmrx.tuner_design(oracle.MODES[mode][3], offset)[0] > 1
    be = oracle.MODES[mode][0]
    calls = [1] if mode == 3 else [1, 1]
    raw = capture(100 + mode, mode, sum(calls) * be, fmt)
    want = narrow_compose(raw, fmt, mode, rf_taps, offset, 0)
    with receiver(fmrx, fmt, mode, rf_taps=rf_taps) as rx:
        rx.tune(offset)
        demod = in_calls(rx.rf_block, raw, be, calls)
    with receiver(fmrx, fmt, mode, rf_taps=rf_taps) as rx:
        rx.tune(offset)
        pcm = in_calls(rx.process, raw, be, calls)
        assert rx.tuner_info() == ([offset], sum(calls) * be // 2, True)
    assert same(demod, want["demod"]), first_difference(demod, want["demod"], *tuner_chunk(mode))
    assert np.array_equal(pcm, want["pcm_mono"]) and pcm.any()


# ---- 1b. the largest rotator table: N = 4000 of kTunerMaxN = 4096 -------------------------------------------

@pytest.mark.parametrize("sign", [1, -1], ids=["up", "down"])
@pytest.mark.parametrize("mode,hz", [(0, 600), (1, 288), (3, 576)])
def test_largest_table(fmrx, mode, hz, sign):
    """The largest period an accepted offset gives: 32,000 B of dynamic LDS beside the staged pairs."""
    offset = sign * hz
    n_per, k, tab = fmrx.tuner_design(oracle.MODES[mode][3], offset)
    assert n_per == 4000 and tab.shape == (4000, 2) and k == (1 if sign > 0 else 3999)
    be = oracle.MODES[mode][0]
    calls = [1] if mode == 3 else [1, 1]
    raw = capture(110 + mode, mode, sum(calls) * be, U8)
    want = narrow_compose(raw, U8, mode, 51, offset, 0)["pcm_mono"]
    with receiver(fmrx, U8, mode) as rx:
        rx.tune(offset)
        got = in_calls(rx.process, raw, be, calls)
    assert np.array_equal(got, want) and got.any()
    # the rotation is used: the discriminator sees the offset as a constant, which the audio low-pass keeps
    assert not np.array_equal(got, narrow_compose(raw, U8, mode, 51, 0, 0)["pcm_mono"])


# ---- 1c. the integer down-converter matrix: every (D, format) -----------------------------------------------

def wide_offset(d):
    """A coarse part with q = 2 (q != 0) and a fine part of 37 kHz where that lies inside the capture,
    otherwise q = 1."""
    rf_fs = oracle.MODES[0][3]
    f = 2 * (rf_fs // 4) + 37000
    return f if 2 * f < d * rf_fs else rf_fs // 4 + 37000


@pytest.mark.parametrize("d,fmt", WIDE_CASES, ids=[f"D{d}-{NAMES[f]}" for d, f in WIDE_CASES])
def test_wide_matrix(fmrx, d, fmt):
    f = wide_offset(d)
    w = fmrx.wide_design(oracle.MODES[0][3], d, f)
    assert w["coarse_hz"] != 0 and w["fine_hz"] == 37000 and w["N"] > 1
    be = oracle.MODES[0][0] * d
    raw = capture(120 + d, 0, 2 * be, fmt)
    want = wide_compose(raw, fmt, 0, 51, d, f)["pcm_mono"]
    with receiver(fmrx, fmt, 0, decim=d) as rx:
        rx.tune_wide(f)
        got = in_calls(rx.process_wide, raw, be, [1, 1])
        assert rx.wide_info() == ([f], raw.size // 2, True)
    assert np.array_equal(got, want) and got.any()


# ---- 1d. walks: workgroups that take several chunks each ------------------------------------------------------

def compute_units():
    return torch.cuda.get_device_properties(0).multi_processor_count


def tuner_target(rf_taps, decim, max_n, cus):
    """tuner_segments (csrc/tuner.hip): the workgroups of one wave of the grid, from variant_lds (the
    staged pairs with their pads) plus the largest rotator table.  A stream's chunks are split one a
    workgroup up to this many, and into runs of at least four past it."""
    r = 2 if decim == 9 else 3
    pairs = (rf_taps - 1) + 64 * r * decim
    lds = 8 * (pairs + pairs // (r * decim) * 2 + 8) + 8 * max_n
    return cus * min(8, max(1, 160 * 1024 // lds))


def wide_target(d, cus):
    """wide_segments (csrc/wide_design.cpp) at an integer ratio: D polyphase rows of 16 + 256 + 1
    pairs and the coarse table of kWideMaxN = 40 entries."""
    lds = 8 * (d * (16 + 256 + 1) + 40)
    return cus * min(8, max(1, 160 * 1024 // lds))


@pytest.mark.parametrize("mode,blocks,rf_taps,fmt", [(0, 40, 51, S16), (0, 40, 101, U8), (1, 36, 51, S8), (1, 36, 101, F32)],
                         ids=["51x10-s16", "101x10-u8", "51x4-s8", "101x4-f32"])
def test_tuner_walks_several_chunks(fmrx, mode, blocks, rf_taps, fmt):
    """16 streams on one shared capture: 134 chunks a stream in mode 0 (40 blocks), 144 in mode 1 (36
    blocks), above tuner_segments' 2048 workgroups on 256 CUs.  Segments are then runs of at least four
    chunks: hist[], carry, the stepped phase and a prefetch clamped at the last whole chunk are used
    again and again inside one workgroup."""
    ns = 16
    rf_fs, be, n_if = oracle.MODES[mode][3], oracle.MODES[mode][0], oracle.MODES[mode][1]
    step = 100000 if mode == 0 else 36000  # periods of at most 24 and 32 pairs
    offsets = [(s - 8) * step for s in range(ns)]
    max_n = max(fmrx.tuner_design(rf_fs, f)[0] for f in offsets)
    cif, per_lane = tuner_chunk(mode)
    chunks = -(-blocks * n_if // cif)
    target = tuner_target(rf_taps, rf_decim(mode), max_n, compute_units())
    assert chunks == (134 if mode == 0 else 144)
    assert ns * chunks > target, "the shape no longer makes a workgroup walk chunks"
    raw = capture(130 + mode, mode, blocks * be, fmt)
    with receiver(fmrx, fmt, mode, rf_taps=rf_taps, n_streams=ns) as rx:
        rx.tune(offsets)
        got = rx.process_shared(raw)
        assert rx.tuner_info() == (offsets, blocks * be // 2, True)
    for s in (0, 7, ns - 1):
        want = narrow_compose(raw, fmt, mode, rf_taps, offsets[s], 0)["pcm_mono"]
        assert np.array_equal(got[s], want) and got[s].any(), (s, first_difference(got[s], want, 1, 1))
    assert len({row.tobytes() for row in got}) == ns


@pytest.mark.parametrize("d,fmt", [(3, U8), (5, S16), (7, S8), (10, F32)], ids=["D3-u8", "D5-s16", "D7-s8", "D10-f32"])
def test_wide_walks_several_chunks(fmrx, d, fmt):
    """16 stations on six wide blocks of mode 0: 150 chunks of 256 outputs a station, 2400 in all, above
    wide_segments' target (2048 workgroups on 256 CUs; 7 a CU = 1792 at D = 10).  Every chunk of a
    workgroup past its first takes its history from the copy inside LDS: 16 D pairs, which is one partial
    pass of the 64 lanes at D = 3, two passes at D = 5 and 7 and three at D = 10."""
    ns, blocks = 16, 6
    rf_fs, be = oracle.MODES[0][3], oracle.MODES[0][0] * d
    chunks = -(-blocks * (oracle.MODES[0][0] // 2) // 256)
    target = wide_target(d, compute_units())
    assert chunks == 150
    assert ns * chunks > target, "the shape no longer makes a workgroup walk chunks"
    step = d * rf_fs // 17 // 1000 * 1000  # 16 stations across the capture, every fine part a multiple of 1 kHz
    offsets = [(s - 8) * step + 7000 * (s % 3) for s in range(ns)]
    raw = capture(140 + d, 0, blocks * be, fmt)
    with receiver(fmrx, fmt, 0, decim=d, n_streams=ns) as rx:
        rx.tune_wide(offsets)
        got = rx.process_wide(raw)
        assert rx.wide_info() == (offsets, raw.size // 2, True)
    for s in (0, 7, ns - 1):
        want = wide_compose(raw, fmt, 0, 51, d, offsets[s])["pcm_mono"]
        assert np.array_equal(got[s], want) and got[s].any(), (s, first_difference(got[s], want, 1, 1))
    assert len({row.tobytes() for row in got}) == ns


# ---- 1e. the fused kernel: every (T, D, AD, AU), 101 taps included ---------------------------------------

@pytest.mark.parametrize("mode,rf_taps,channels", FUSED_CASES,
                         ids=[f"mode{m}-rf{t}-{'mono' if c == MONO else 'stereo'}" for m, t, c in FUSED_CASES])
def test_fused_matches_oracle(fmrx, orc, mode, rf_taps, channels):
    assert (fmrx.MONO, fmrx.STEREO) == (MONO, STEREO)
    be = oracle.MODES[mode][0]
    calls = {0: [1, 2], 1: [1, 2], 2: [1, 1], 3: [1]}[mode]
    iq = synth(150 + mode, mode, sum(calls) * be)
    field = "pcm_mono" if channels == MONO else "pcm"
    want = orc.run(mode, rf_taps, iq, [field, "demod"])
    with fmrx.Receiver(mode, channels, rf_taps=rf_taps) as rx:
        pcm = in_calls(rx.process, iq, be, calls)
    assert np.array_equal(pcm, want[field]) and pcm.any()
    if channels == MONO:  # the RF-only form: in modes 2 and 3 another instantiation than `process` runs
        with fmrx.Receiver(mode, channels, rf_taps=rf_taps) as rx:
            demod = in_calls(rx.rf_block, iq, be, calls)
        assert same(demod, want["demod"]), first_difference(demod, want["demod"], *tuner_chunk(mode))
        assert demod.any()


# ---- 1f. rows that are not 16-byte aligned: the dword loads from odd addresses and halo_kernel --------------

@functools.lru_cache(maxsize=None)
def two_stream_reference(rf_taps, channels, blocks):
    """The oracle's outputs of the two streams of test_misaligned_rows, computed once a configuration."""
    orc, be = oracle.Oracle(), oracle.MODES[0][0]
    fields = ["pcm_mono", "mono_indep"] if channels == MONO else ["pcm"]
    return [orc.run(0, rf_taps, synth(160 + s, 0, blocks * be), fields) for s in range(2)]


@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("rf_taps,channels", [(51, MONO), (101, MONO), (51, STEREO)],
                         ids=["rf51-mono", "rf101-mono", "rf51-stereo"])
def test_misaligned_rows(fmrx, rf_taps, channels, k):
    """fmrx_process_device and fmrx_process_device_ex with d_iq k bytes and d_pcm two bytes into their
    buffers: the fused kernel's dword loads start at addresses that are no multiple of 4 (k = 1, 2) or of
    16, and run_fused leaves the halo to halo_kernel.  The second call reads the halo that kernel wrote.
    The oracle's PCM is also what the aligned calls give (tests/test_gpu_parity.py)."""
    ns, calls = 2, [2, 3]
    be, na = oracle.MODES[0][0], oracle.MODES[0][2] * (1 if channels == MONO else 2)
    ref = two_stream_reference(rf_taps, channels, sum(calls))
    field = "pcm_mono" if channels == MONO else "pcm"
    want = np.stack([r[field] for r in ref])
    iq = np.stack([synth(160 + s, 0, sum(calls) * be) for s in range(ns)])
    for ex in (False, True):
        float_out = ex and channels == MONO  # the mono product's float outlet: MONO contexts
        parts, mono_parts, b = [], [], 0
        with fmrx.Receiver(0, channels, rf_taps=rf_taps, n_streams=ns) as rx:
            for nb in calls:
                rows = np.ascontiguousarray(iq[:, b * be:(b + nb) * be])
                base = torch.zeros(k + rows.size, dtype=torch.uint8, device="cuda")
                base[k:] = torch.from_numpy(rows.reshape(-1)).cuda()
                d_pcm = torch.zeros(1 + ns * nb * na, dtype=torch.int16, device="cuda")
                d_mono = torch.zeros(ns * nb * na, dtype=torch.float32, device="cuda")
                assert base.data_ptr() % 16 == 0 and d_pcm.data_ptr() % 16 == 0
                torch.cuda.synchronize()
                if ex:
                    rx.process_device(base.data_ptr() + k, nb, d_pcm.data_ptr() + 2, d_mono.data_ptr() if float_out else None)
                else:
                    rc = fmrx.lib().fmrx_process_device(rx.h, base.data_ptr() + k, nb, d_pcm.data_ptr() + 2)
                    assert rc == fmrx.FMRX_OK
                rx.synchronize()
                out = d_pcm.cpu().numpy()
                assert out[0] == 0  # nothing in front of d_pcm is written
                parts.append(out[1:].reshape(ns, nb * na))
                mono_parts.append(d_mono.cpu().numpy().reshape(ns, nb * na))
                b += nb
        got = np.concatenate(parts, axis=1)
        assert np.array_equal(got, want) and got[0].any() and got[1].any(), (ex, first_difference(got, want, 1, 1))
        if float_out:
            assert same(np.concatenate(mono_parts, axis=1), np.stack([r["mono_indep"] for r in ref])), ex
    assert not np.array_equal(want[0], want[1])
