"""The RDS back half's definition and the host group parser, on the CPU: the numpy
restatement in rds_ref.py over the oracle's front half and the reference's resample decodes what
the test transmitter sent, and fmrx_rds_parse equals the numpy parser bit for bit."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
import rds_ref as R

PI, PS, RT = 0x54A8, "RADIO 42", "HELLO FROM THE GPU RDS DECODER. "


def _run(orc, mode, secs, **kw):
    g = R.granule_samples(mode)
    n = int(secs * R.bp_fs(mode)) // g * g
    bits = R.stream_bits(R.groups(PI, PS, RT, R.n_groups_for(secs)))
    out = R.from_demod(orc, mode, R.make_demod(mode, n, bits, **kw))
    rate = R.BITRATE * (1.0 + kw.get("ppm", 0.0) * 1e-6)
    out["sent"] = int((n / R.bp_fs(mode) * rate - kw.get("phase", 0.0)) // 104)  # whole groups inside the signal
    return out


_clean = {}


def clean(orc, mode, phase=0.0):
    """3 s of clean signal, computed once a (mode, phase) and left unchanged."""
    if (mode, phase) not in _clean:
        _clean[mode, phase] = _run(orc, mode, 3.0, noise=0.002, phase=phase, seed=3)
    return _clean[mode, phase]


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_reference_decodes_what_was_sent(orc, mode):
    out = clean(orc, mode)
    info = out["info"]
    assert (info["pi"], info["ps"], info["rt"]) == (PI, PS, RT.ljust(64))
    assert (info["pty"], info["tp"]) == (5, 1)
    assert info["bits"] == out["bits"].size == 76 * out["win"].shape[0]
    # all groups but the first, which falls into the filters' and the PLL's settling
    assert info["groups"] >= out["sent"] - 1
    assert info["blocks"] >= 4 * info["groups"]


def test_both_pairings(orc):
    """Start phases half a bit (one chip) apart take the two pairings, and both decode."""
    a, b = clean(orc, 0, 0.0), clean(orc, 0, 0.5)
    qa, qb = a["win"][4:, 1], b["win"][4:, 1]  # past the settling
    assert len(set(qa)) == 1 and len(set(qb)) == 1 and {int(qa[0]), int(qb[0])} == {0, 1}
    for out in (a, b):
        assert (out["info"]["pi"], out["info"]["ps"], out["info"]["rt"]) == (PI, PS, RT.ljust(64))
        assert out["info"]["groups"] >= out["sent"] - 1


@pytest.mark.parametrize("mode", [1, 3])
def test_clock_error_floor(orc, mode):
    """100 ppm of symbol-clock error at noise 0.02 over 20 s: the phase wraps (each wrap may cost a
    block) and at least 90 % of the groups still decode."""
    out = _run(orc, mode, 20.0, noise=0.02, ppm=100.0, seed=3)
    p = out["win"][:, 0].astype(int)
    assert int(np.sum(np.abs(np.diff(p)) > 8)) >= 1, "no phase wrap in 20 s at 100 ppm"
    assert out["info"]["groups"] >= 0.9 * out["sent"], (out["info"]["groups"], out["sent"])
    assert (out["info"]["pi"], out["info"]["ps"]) == (PI, PS)


def test_granules(fmrx):
    """Whole windows: 24, 24, 3, 1 blocks give 2432, 2432, 48640, 48640 outputs."""
    outs = {0: 2432, 1: 2432, 2: 48640, 3: 48640}
    for mode, blocks in R.GRANULES.items():
        n_if, fs = blocks * oracle.MODES[mode][1], R.bp_fs(mode)
        assert n_if * 19 % (fs // 2000) == 0 and n_if * 19 // (fs // 2000) == outs[mode]
        assert outs[mode] % R.WIN == 0
        for fewer in range(1, blocks):
            assert (fewer * oracle.MODES[mode][1] * 19) % ((fs // 2000) * R.WIN) != 0


def test_resample_splits_at_granules(orc):
    """The reference's resample cut at granule boundaries equals one call, bit for bit."""
    for mode in range(4):
        g = R.granule_samples(mode)
        x = R.make_demod(mode, 3 * g, R.stream_bits(R.groups(PI, PS, None, 8)))  # any signal
        whole, _ = R.resample(orc, mode, x)
        st, parts = None, []
        for k in range(3):
            y, st = R.resample(orc, mode, x[k * g: (k + 1) * g], st)
            parts.append(y)
        assert np.array_equal(whole.view(np.uint32), np.concatenate(parts).view(np.uint32))


@pytest.mark.parametrize("piece", [0, 1, 25, 26, 103])
def test_parse_equals_numpy(fmrx, orc, piece):
    """fmrx_rds_parse, fed whole (0) or in pieces, equals the numpy parser."""
    out = clean(orc, 0)
    bits, codes = out["bits"], out["codes"]
    if piece == 0:
        io = fmrx.rds_parse(bits, codes)
    else:
        io = fmrx.RdsInfo()
        for k in range(0, bits.size, piece):
            fmrx.rds_parse(bits[k: k + piece], codes[k: k + piece], io)
    assert io.as_dict() == out["info"]
    assert io.tail_n == 103 and bytes(io.tail_bits) == bits[-103:].tobytes()


def _codes_of(bits):
    """Steps 5..6 of a transmitted bit stream (no signal in between)."""
    codes = np.zeros(bits.size, np.uint8)
    view = np.lib.stride_tricks.sliding_window_view(bits, 26).astype(np.int64)
    word = view @ (1 << np.arange(25, -1, -1, dtype=np.int64))
    syn = R.crc10(word >> 10) ^ (word & 0x3FF)
    for code, off in R.OFFSETS.items():
        codes[25:][syn == off] = code
    return codes


def test_new_info_is_spaces(fmrx):
    io = fmrx.RdsInfo()
    assert io.as_dict() == {"pi": 0, "pty": 0, "tp": 0, "ps": " " * 8, "rt": " " * 64, "bits": 0, "blocks": 0, "groups": 0}
    assert fmrx.rds_parse(np.zeros(0, np.uint8), np.zeros(0, np.uint8), io).as_dict()["bits"] == 0


def test_one_corrupt_bit_drops_exactly_that_group(fmrx):
    grps = R.groups(PI, PS, RT, 12)
    bits = R.stream_bits(grps)
    good = fmrx.rds_parse(bits, _codes_of(bits)).as_dict()
    assert good["groups"] == 12 and good["ps"] == PS and good["blocks"] >= 48
    assert good == R.parse(bits, _codes_of(bits))
    # group 6 is the only carrier of PS segment 3 in these 12 (0A at 0, 2, 4, 6, 8, 10: segments 0 1 2 3 0 1)
    bad = bits.copy()
    bad[6 * 104 + 26 + 7] ^= 1  # a bit of its block B
    got = fmrx.rds_parse(bad, _codes_of(bad)).as_dict()
    assert got == R.parse(bad, _codes_of(bad))
    assert got["groups"] == 11
    assert got["ps"] == PS[:6] + "  " and got["rt"] == good["rt"]


def test_c_prime_accepted(fmrx):
    """A version-B group carries offset C' in block 3: accepted like C; 0B sets PS, 2B two characters."""
    b0 = (1 << 11) | (1 << 10) | (5 << 5)
    grps = [(PI, b0 | 1, PI, (ord("A") << 8) | ord("B")), (PI, (2 << 12) | b0 | 3, PI, (ord("x") << 8) | ord("y"))]
    bits = np.array([x for g in grps for x in R.group_bits(*g, c_prime=True)], np.uint8)
    codes = _codes_of(bits)
    assert list(codes[codes != 0]) == [1, 2, 4, 5, 1, 2, 4, 5]
    got = fmrx.rds_parse(bits, codes).as_dict()
    assert got == R.parse(bits, codes)
    assert got["groups"] == 2 and got["ps"] == "  AB    " and got["rt"][:8] == "      xy"
    # the same blocks with C' replaced by a wrong offset (D's) are no group
    wrong = np.array([x for g in grps for x in (R.block_bits(g[0], 1) + R.block_bits(g[1], 2) + R.block_bits(g[2], 5)
                                                   + R.block_bits(g[3], 5))], np.uint8)
    assert fmrx.rds_parse(wrong, _codes_of(wrong)).as_dict()["groups"] == 0


def test_text_flag_toggle_clears(fmrx):
    base = (1 << 10) | (5 << 5)
    mk = lambda ab, at, s: (PI, (2 << 12) | base | (ab << 4) | at, (ord(s[0]) << 8) | ord(s[1]), (ord(s[2]) << 8) | ord(s[3]))
    bits = R.stream_bits([mk(0, 0, "abcd"), mk(0, 1, "efgh"), mk(1, 2, "ijkl")])
    got = fmrx.rds_parse(bits, _codes_of(bits)).as_dict()
    assert got == R.parse(bits, _codes_of(bits))
    assert got["rt"] == ("        ijkl").ljust(64)
