"""CPU guard of tests/test_gpu_taps.py, the matrix over the taps on the demod rows.

a. tests/taps_ref.py, the composed reference, gives exactly what meter_ref, afc_ref, blend_ref, deemph_ref,
   rds_ref and rds_sync_ref give when called one by one on the same demod, and a report accumulated over the
   calls (1, 2, 1 granules) equals the whole call's wherever the restatements say it must.
b. The matrix's inputs, checked on the reference alone, are long enough that a wrong kernel cannot hide behind
   an empty result: the stations are named, the subcarriers detected, soft stereo's levels visit the range,
   and the constructed rows of tests/test_gpu_rds_decode.py reach the ties.
c. The instantiations of meter_kernel<NI> and carrier_kernel<NI> in libfmrx.so (`nm -C`: names only) are the
   windows the switch-path cases of the matrix name."""
from __future__ import annotations

import re
import shutil
import subprocess

import numpy as np
import pytest

import afc_ref as A
import blend_ref as B
import deemph_ref as dr
import meter_ref as M
import rds_ref as R
import rds_sync_ref as S
import taps_ref as T
from test_gpu_taps import ALONE_MODES, MATRIX_CASES, STREAM_CASES, entry_eq, matrix_windows


def demod_row(mode, granules):
    """A multiplex with pilot, L-R and RDS at the demod rate: whole granules of one stream."""
    n = granules * R.granule_samples(mode)
    t = np.arange(n, dtype=np.float64) / R.bp_fs(mode)
    return M.multiplex(t, bits=M.station_bits(T.PI, T.PS, n / R.bp_fs(mode)), lr=0.1, seed=5 + mode).astype(np.float32)


# ---- a. the composed reference is its parts ------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_demod_reports_are_the_parts(fmrx, orc, mode):
    demod, g = demod_row(mode, 1), B.BLOCKS[mode]
    got = T.demod_reports(orc, fmrx, mode, demod, [g], T.ALL_STEREO)
    pw = M.power(demod, fmrx.meter_design(R.bp_fs(mode))[1])
    assert entry_eq(got["meter"], M.accumulate(pw)) and got["detect"] == M.detect(*M.accumulate(pw))
    assert entry_eq(got["afc"], A.report_of(demod, M.window(mode)))
    dec = R.from_demod(orc, mode, demod)
    assert got["rds"] == dec["info"] and got["ext"] == S.parse_stream(dec["bits"]) and dec["info"]["bits"] > 0
    row, _ = B.levels(pw, fmrx.blend_design())
    assert np.array_equal(got["row"], row) and got["hist"] == B.histogram([row]) and sum(got["hist"]) == B.GM[mode]
    off = T.demod_reports(orc, fmrx, mode, demod, [g], frozenset())
    assert off["meter"][1] == off["afc"][2] == off["rds"]["bits"] == off["ext"]["bits"] == 0 and off["hist"] == [0] * 17


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_calls_accumulate_to_the_whole(fmrx, orc, mode):
    """(1, 2, 1) granules against one call of four: every report is defined on the stream, not on the calls."""
    demod, g = demod_row(mode, 4), B.BLOCKS[mode]
    whole = T.demod_reports(orc, fmrx, mode, demod, [4 * g], T.ALL_STEREO)
    parts = T.demod_reports(orc, fmrx, mode, demod, [g, 2 * g, g], T.ALL_STEREO)
    for k in ("meter", "detect", "afc", "rds", "ext", "hist"):
        assert entry_eq(parts[k], whole[k]), k
    assert np.array_equal(parts["row"], whole["row"]) and len(parts["rows"]) == 3
    assert whole["meter"][1] == whole["afc"][2] == 4 * B.GM[mode]


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_expected_pcm_is_the_parts(fmrx, orc, mode):
    iq, nb = T.capture(mode, True), T.GRANULES[mode] * B.BLOCKS[mode]
    o = orc.run(mode, 51, iq, ["demod", "pcm", "left", "right"])
    rl = np.stack([o["right"], o["left"]], axis=1)
    h = fmrx.deemph_design(T.audio_fs(mode), T.TAU)
    both = T.expected(orc, fmrx, mode, iq, [nb], T.ALL_STEREO, True)
    y = B.apply(mode, rl, both["row"])
    assert np.array_equal(both["pcm"], dr.pcm_stereo(orc, y[:, 1], y[:, 0], h)) and np.array_equal(both["pcm_off"], o["pcm"])
    blend = T.expected(orc, fmrx, mode, iq, [nb], frozenset(("blend",)), True)
    assert np.array_equal(blend["pcm"], B.quant(orc, y)) and np.array_equal(blend["row"], both["row"])
    de = T.expected(orc, fmrx, mode, iq, [nb], frozenset(("deemph",)), True)
    assert np.array_equal(de["pcm"], dr.pcm_stereo(orc, o["left"], o["right"], h))
    assert np.array_equal(T.expected(orc, fmrx, mode, iq, [nb], frozenset(("meter", "rds", "afc")), True)["pcm"], o["pcm"])
    assert len({x["pcm"].tobytes() for x in (both, blend, de)} | {o["pcm"].tobytes()}) == 4
    if mode < 2:  # tests/test_gpu_blend.py's reference(), which moved to taps_ref with station(): the same PCM
        pcm, row, _, _, plain = T.reference(orc, fmrx, mode, iq, ("host", mode), tau=T.TAU)
        assert np.array_equal(pcm, both["pcm"]) and np.array_equal(row, both["row"]) and np.array_equal(plain, o["pcm"])


# ---- b. the inputs can show a wrong kernel ---------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_mono_capture_names_the_station(fmrx, orc, mode):
    g = T.GRANULES[mode]
    want = T.expected(orc, fmrx, mode, T.capture(mode, False), [g * B.BLOCKS[mode]], T.ALL_MONO, False)
    info, ext = want["rds"], want["ext"]
    print(mode, info["groups"], repr(info["ps"]), ext["groups"], ext["corrected_blocks"], want["detect"])
    assert want["detect"]["stereo"] == 1 and want["detect"]["rds"] == 1
    assert info["pi"] == ext["pi"] == T.PI and ext["ps"] == T.PS and ext["corrected_blocks"] >= 1
    if mode == 0:  # test_gpu_rds_sync's 6 granules: the plain parser has part of the name, the block sync all of it
        assert (info["ps"], info["groups"]) == ("  DIO 42", 3)
    else:
        assert info["ps"] == T.PS and info["groups"] >= 10
        assert info["groups"] == {1: 16, 2: 13, 3: 13}[mode]  # as measured when the captures were chosen


@pytest.mark.parametrize("mode,granules", sorted({(m, g) for m, _, g in MATRIX_CASES}))
def test_stereo_capture_visits_the_levels(fmrx, orc, mode, granules):
    iq = T.capture(mode, True, granules)
    want = T.expected(orc, fmrx, mode, iq, [granules * B.BLOCKS[mode]], T.ALL_STEREO, True)
    lv = set(int(v) for v in want["row"][1:])
    print(mode, granules, [int(v) for v in want["row"]])
    assert 16 in lv and min(lv) <= 4 and any(4 < v < 16 for v in lv)
    windows = granules * R.granule_samples(mode) * R.UP // (R.bp_fs(mode) // 2000) // R.WIN
    assert want["rds"]["bits"] == windows * R.SYMS and windows == granules * B.GM[mode]
    print(mode, granules, hex(want["rds"]["pi"]), want["rds"]["groups"], want["ext"]["pi"])
    assert want["rds"]["pi"] == want["ext"]["pi"] == 0x1234 and want["rds"]["groups"] >= 1  # station()'s PI: the RDS decodes here too
    assert not np.array_equal(want["pcm"], want["pcm_off"])


def test_edge_rows_reach_the_ties(orc):
    """tests/test_gpu_rds_decode.py's constructed rows: an all-zero phase histogram (np.argmax gives bin 0, p = 8)
    and v0 == v1 (q = 0) in both windows of zeros and of -0.0, one set bit and no code."""
    from test_gpu_rds_decode import edge_rows
    rows = edge_rows(orc, "flat")
    for r in rows[:2]:
        y, _ = R.resample(orc, 0, r)
        assert np.all(y == 0)
        s = np.concatenate(([1], (y >= np.float32(0.0)).astype(np.uint8)))
        assert s.all()  # no sign change anywhere: an all-zero histogram in both windows
        e = s[: R.CHIPS + 1]  # every chip 1 at any phase, the chip carried in too
        assert int(np.sum(e[0:152:2] == e[1:153:2])) == int(np.sum(e[1:153:2] == e[2:153:2])) == R.SYMS  # v0 == v1
        out = R.bits_from_y(y)
        assert out["win"].tolist() == [[8, 0], [8, 0]] and int(out["bits"].sum()) == 1 and not out["codes"].any()
    assert R.bits_from_y(np.zeros(2 * R.WIN, np.float32))["win"].tolist() == [[8, 0], [8, 0]]


# ---- c. the matrix names every compiled window -------------------------------------------------------------------

def test_matrix_names_every_meter_and_carrier_kernel(fmrx):
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm is not on this machine")
    out = subprocess.run([nm, "-C", fmrx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    found = {"meter_kernel": set(), "carrier_kernel": set()}
    for name, arg in re.findall(r"\b(meter_kernel|carrier_kernel)<(\d+)>\(", out):
        found[name].add(int(arg))
    assert found["meter_kernel"] == found["carrier_kernel"] == {15, 16, 18}
    # every window through the switch (a demod row kDemodHist floats into a longer row), on both channel counts
    for ch in ("MONO", "STEREO"):
        named = matrix_windows([c for c in MATRIX_CASES if c[1] == ch])
        assert named == found["meter_kernel"], (ch, sorted(found["meter_kernel"] - named), sorted(named - found["meter_kernel"]))
    assert {M.window(m) for m in ALONE_MODES} == {288, 256} and {m for m, _ in STREAM_CASES} == {0, 3}
    assert T.ALL_MONO >= {"meter", "afc"} and T.ALL_STEREO >= {"meter", "afc"}  # both kernels run in every case
