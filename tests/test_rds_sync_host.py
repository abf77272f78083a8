"""The RDS block sync's definition and its host parts, on the CPU: the burst table and
the block-wise group parser of the library equal the numpy restatement in rds_sync_ref.py, and the
restatement itself accepts what a noisy transmitter sent and rejects noise."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import rds_ref as R
import rds_sync_ref as S
from test_rds_host import PI, PS, RT, _run

BASE = (1 << 10) | (5 << 5)  # TP 1, PTY 5


# ---- the burst table and the refusals ---------------------------------------------------------

@pytest.mark.parametrize("b", [0, 1, 2, 3, 4, 5])
def test_table_equals_numpy_and_has_no_collision(fmrx, b):
    want, collisions = S.burst_table(b)
    assert collisions == 0
    got, n = fmrx.rds_sync_design(b)
    assert np.array_equal(got, want)
    assert n == len(S.burst_patterns(b)) == int(np.count_nonzero(want != S.NONE)) - 1
    assert got[0] == 0
    if b == 2:
        assert n == 51


def test_refusals(fmrx):
    L = fmrx.lib()
    for b in (-1, 6):
        assert L.fmrx_rds_sync_design(b, None, None) == fmrx.FMRX_EINVAL
    assert L.fmrx_rds_sync_design(2, None, None) == fmrx.FMRX_OK  # both outputs may be null
    assert L.fmrx_rds_sync_config_default(None) == fmrx.FMRX_EINVAL
    assert L.fmrx_rds_ext_init(None) == fmrx.FMRX_EINVAL
    ext = fmrx.RdsExt()
    assert L.fmrx_rds_parse_blocks(None, None, 0, 0, 0) == fmrx.FMRX_EINVAL
    assert L.fmrx_rds_parse_blocks(C.byref(ext), None, 1, 0, 0) == fmrx.FMRX_EINVAL
    assert L.fmrx_rds_parse_blocks(C.byref(ext), None, 0, 0, 0) == fmrx.FMRX_OK
    bad = np.zeros(1, fmrx.RDS_BLOCK)
    bad["slot"] = 4
    assert L.fmrx_rds_parse_blocks(C.byref(ext), bad.ctypes.data, 1, 0, 0) == fmrx.FMRX_EINVAL
    assert L.fmrx_set_rds_sync(None, 1) == fmrx.FMRX_EINVAL
    assert L.fmrx_rds_ext_get(None, 0, C.byref(ext)) == fmrx.FMRX_EINVAL
    assert L.fmrx_rds_blocks(None, None, None, 0, None, 0, None) == fmrx.FMRX_EINVAL
    assert L.fmrx_rds_blocks_device(None, None, None, 0, None, 0, None) == fmrx.FMRX_EINVAL
    assert L.fmrx_rds_blocks_flush(None, None, 0, None) == fmrx.FMRX_EINVAL
    cfg = fmrx.rds_sync_config()
    assert (cfg.J, cfg.V, cfg.B) == (S.J, S.V, S.B) == (8, 3, 2)


def test_new_ext_is_empty(fmrx):
    assert fmrx.RdsExt().as_dict() == S.ext_dict(S.ext_init())
    assert fmrx.RdsExt().as_dict()["pi"] is None and fmrx.RdsExt().as_dict()["ct"] is None


def test_ext_layout_matches_the_binding(fmrx):
    """fmrx_rds_ext_init writes sizeof(fmrx_rds_ext) bytes: exactly the binding's struct, not a byte more."""
    n = C.sizeof(fmrx.RdsExt)
    buf = (C.c_uint8 * (n + 64))(*([0xEE] * (n + 64)))
    assert fmrx.lib().fmrx_rds_ext_init(C.cast(buf, C.POINTER(fmrx.RdsExt))) == fmrx.FMRX_OK
    raw = bytes(buf)
    assert raw[n:] == b"\xEE" * 64 and 0xEE not in raw[:n]
    assert raw[:n] == bytes(fmrx.RdsExt())
    assert C.sizeof(fmrx._RdsBlockRec) == fmrx.RDS_BLOCK.itemsize == S.BLOCK.itemsize == 16 and fmrx.RDS_BLOCK == S.BLOCK


# ---- the block-wise parser against the restatement's ------------------------------------------

def _recs(groups, missing=(), corrected=(), start=25):
    """The records a clean reception of groups (a, b, c, d[, c_prime]) gives: four a group, 26 bits
    apart.  missing: (group, slot) pairs left out; corrected: (group, slot) pairs flagged."""
    out = []
    for g, grp in enumerate(groups):
        for u in range(4):
            if (g, u) in missing:
                continue
            r = np.zeros((), S.BLOCK)
            r["bit"], r["info"], r["slot"], r["votes"] = start + 104 * g + 26 * u, grp[u], u, 16
            r["c_prime"] = 1 if u == 2 and len(grp) > 4 and grp[4] else 0
            r["corrected"] = 1 if (g, u) in corrected else 0
            out.append(r)
    return np.array(out, S.BLOCK)


def _both(fmrx, recs, n_bits=0, flush=True, piece=0):
    """The library's parser (whole, or piece records a call) and the restatement's; asserts they agree."""
    want = S.ext_dict(S.parse_blocks(S.ext_init(), recs, n_bits, flush))
    if piece == 0:
        ext = fmrx.rds_parse_blocks(recs, n_bits, flush=flush)
    else:
        ext = fmrx.RdsExt()
        for k in range(0, recs.size, piece):
            fmrx.rds_parse_blocks(recs[k: k + piece], 0, ext)
        fmrx.rds_parse_blocks(recs[:0], n_bits, ext, flush=flush)
    assert ext.as_dict() == want
    return ext


def _two(s):
    return (ord(s[0]) << 8) | ord(s[1])


def g0a(seg, chars, af=0xE0CD, ta=0, ms=0, di=0):
    return (PI, BASE | (ta << 4) | (ms << 3) | (di << 2) | seg, af, _two(chars))


def g2a(at, s, ab=0):
    return (PI, (2 << 12) | BASE | (ab << 4) | at, _two(s[:2]), _two(s[2:]))


def test_group_0a_name_flags_and_af(fmrx):
    # AF: count 3 (227), then 87.6 (1), 98.1 (106), 107.9 (204); filler 205 and a repeat are not kept
    afs = [(227 << 8) | 1, (106 << 8) | 204, (205 << 8) | 1, (0 << 8) | 250]
    grps = [g0a(k, PS[2 * k: 2 * k + 2], afs[k], ta=1, ms=1, di=(0b1010 >> (3 - k)) & 1) for k in range(4)]
    got = _both(fmrx, _recs(grps), 416).as_dict()
    assert (got["pi"], got["ps"], got["tp"], got["pty"]) == (PI, PS, 1, 5)
    assert (got["ta"], got["ms"], got["di"]) == (1, 1, 0b1010)
    assert got["af"] == [87.6, 98.1, 107.9] and got["af_count"] == 3
    assert (got["groups"], got["partial_groups"], got["exact_blocks"], got["corrected_blocks"], got["bits"]) == (4, 0, 16, 0, 416)


def test_group_0b_and_2b_use_d_only(fmrx):
    b0 = (1 << 11) | BASE
    grps = [(PI, b0 | 1, PI, _two("AB"), True), (PI, (2 << 12) | b0 | 3, PI, _two("xy"), True)]
    got = _both(fmrx, _recs(grps)).as_dict()
    assert got["ps"] == "  AB    " and got["rt"][:8] == "      xy" and got["af"] == [] and got["groups"] == 2


def test_group_2a_text_and_flag(fmrx):
    grps = [g2a(0, "abcd"), g2a(1, "efgh"), g2a(2, "ijkl", ab=1)]
    assert _both(fmrx, _recs(grps)).as_dict()["rt"] == "        ijkl".ljust(64)
    # C missing: D still gives its two characters; D missing: C gives its two
    got = _both(fmrx, _recs([g2a(0, "abcd"), g2a(1, "efgh")], missing=[(0, 2), (1, 3)])).as_dict()
    assert got["rt"] == "  cdef  ".ljust(64) and (got["groups"], got["partial_groups"]) == (0, 2)


def test_group_4a_clock_time(fmrx):
    def g4a(mjd, hour, minute, off):
        sign, mag = (1, -off) if off < 0 else (0, off)
        return (PI, (4 << 12) | BASE | (mjd >> 15), ((mjd & 0x7FFF) << 1) | (hour >> 4),
                ((hour & 15) << 12) | (minute << 6) | (sign << 5) | mag)

    got = _both(fmrx, _recs([g4a(60604, 13, 37, 2)])).as_dict()  # MJD 60604 is 2024-10-21
    assert got["ct"] == {"mjd": 60604, "year": 2024, "month": 10, "day": 21, "hour": 13, "minute": 37, "offset": 2}
    got = _both(fmrx, _recs([g4a(51544, 0, 0, -7)])).as_dict()  # 2000-01-01
    assert got["ct"] == {"mjd": 51544, "year": 2000, "month": 1, "day": 1, "hour": 0, "minute": 0, "offset": -7}
    assert _both(fmrx, _recs([g4a(51603, 23, 59, 0)])).as_dict()["ct"]["day"] == 29  # 2000-02-29
    # without its C or its D there is no time, nor with an hour past 23
    assert _both(fmrx, _recs([g4a(60604, 13, 37, 2)], missing=[(0, 2)])).as_dict()["ct"] is None
    assert _both(fmrx, _recs([g4a(60604, 13, 37, 2)], missing=[(0, 3)])).as_dict()["ct"] is None
    assert _both(fmrx, _recs([g4a(60604, 24, 0, 0)])).as_dict()["ct"] is None


def test_mjd_dates_equal_the_calendar():
    import datetime

    for mjd in list(range(15079, 15079 + 800)) + list(range(51500, 52300)) + list(range(60000, 61500)) + [88127]:  # to 2100-02-28
        d = datetime.date(1858, 11, 17) + datetime.timedelta(days=mjd)
        assert S.mjd_date(mjd) == (d.year, d.month, d.day), mjd


def test_group_10a_ptyn(fmrx):
    g10 = lambda at, s, ab=0: (PI, (10 << 12) | BASE | (ab << 4) | at, _two(s[:2]), _two(s[2:]))
    assert _both(fmrx, _recs([g10(0, "FOOT"), g10(1, "BALL")])).as_dict()["ptyn"] == "FOOTBALL"
    assert _both(fmrx, _recs([g10(0, "FOOT"), g10(1, "NEWS", ab=1)])).as_dict()["ptyn"] == "    NEWS"


def test_missing_c_still_yields_the_name(fmrx):
    """A group whose C block was lost: no group for the plain parser, the PS pair for this one."""
    grps = [g0a(k, PS[2 * k: 2 * k + 2]) for k in range(4)]
    got = _both(fmrx, _recs(grps, missing=[(k, 2) for k in range(4)])).as_dict()
    assert got["ps"] == PS and (got["groups"], got["partial_groups"]) == (0, 4)
    # the same loss in the bits: every C block with three wrong bits spread out
    bits = R.stream_bits(grps * 6)
    for g in range(24):
        bits[104 * g + 52 + np.array([3, 11, 19])] ^= 1
    from test_rds_host import _codes_of
    assert fmrx.rds_parse(bits, _codes_of(bits)).as_dict()["groups"] == 0
    ext = S.parse_stream(bits)
    assert ext["ps"] == PS and ext["pi"] == PI and ext["groups"] == 0 and ext["partial_groups"] == 24


def test_corrected_a_block_with_a_foreign_pi_is_ignored(fmrx):
    grps = [g0a(0, "AB"), (0x1111,) + g0a(1, "CD")[1:], g0a(2, "EF")]
    got = _both(fmrx, _recs(grps, corrected=[(1, 0)])).as_dict()
    assert got["pi"] == PI and got["ps"] == "ABCDEF  " and (got["groups"], got["partial_groups"]) == (2, 1)
    # a corrected A block that equals the PI counts; in front of any exact one it does not
    assert _both(fmrx, _recs([g0a(0, "AB"), g0a(1, "CD")], corrected=[(1, 0)])).as_dict()["groups"] == 2
    first = _both(fmrx, _recs([g0a(0, "AB")], corrected=[(0, 0)])).as_dict()
    assert first["pi"] is None and (first["groups"], first["partial_groups"]) == (0, 1)


@pytest.mark.parametrize("piece", [1, 3, 5])
def test_split_feeding_gives_equal_structs(fmrx, piece):
    grps = [g0a(k % 4, PS[2 * (k % 4): 2 * (k % 4) + 2]) if k % 2 else g2a(k // 2 % 8, RT[4 * (k // 2 % 8):][:4]) for k in range(24)]
    recs = _recs(grps, missing=[(3, 2), (5, 3), (7, 0), (9, 1), (23, 3)], corrected=[(2, 0), (4, 3)])
    for flush in (False, True):
        whole = _both(fmrx, recs, 2496, flush)
        parts = _both(fmrx, recs, 2496, flush, piece)
        assert bytes(whole) == bytes(parts)
    # without a flush the last B block waits for its D; the flush closes it
    open_ = _both(fmrx, recs, 0, False).as_dict()
    closed = _both(fmrx, recs, 0, True).as_dict()
    assert closed["groups"] + closed["partial_groups"] == open_["groups"] + open_["partial_groups"] + 1


def test_more_records_than_the_tail_holds(fmrx):
    """Records denser than any transmitter sends: the oldest leave, an open B block with them, alike in both."""
    recs = np.zeros(40, S.BLOCK)
    recs["bit"] = 25 + 2 * np.arange(40)
    recs["slot"] = np.arange(40) % 4
    recs["info"] = 0x1000 + np.arange(40)
    for piece in (0, 1, 7):
        _both(fmrx, recs, 0, True, piece)


# ---- the definition's quality, on the restatement alone ---------------------------------------

def _sent(grps):
    """bit index of a block's last bit -> (slot, info16)."""
    return {104 * g + 26 * u + 25: (u, grp[u]) for g, grp in enumerate(grps) for u in range(4)}


def _score(recs, sent):
    right = sum(1 for r in recs if sent.get(int(r["bit"])) == (int(r["slot"]), int(r["info"])))
    return right, recs.size - right


def test_clean_stream_every_block(fmrx):
    grps = R.groups(PI, PS, RT, 40)
    recs = S.blocks(R.stream_bits(grps))
    sent = _sent(grps)
    inner = [p for p in sent if 26 * S.J <= p < 104 * 40 - 26 * S.J]
    got = {int(r["bit"]): (int(r["slot"]), int(r["info"])) for r in recs}
    assert all(got.get(p) == sent[p] for p in inner)
    assert _score(recs, sent)[1] == 0 and not recs["corrected"].any()


def test_ber_1_percent_over_600_groups():
    """Seed 1: 2333 of 2400 sent blocks right (97.2 %), 8 of 2341 accepted wrong (0.34 %); the plain rule
    keeps 199 of 600 groups."""
    grps = R.groups(PI, PS, RT, 600)
    bits = R.stream_bits(grps)
    flips = (np.random.default_rng(1).random(bits.size) < 0.01).astype(np.uint8)
    recs = S.blocks(bits ^ flips)
    right, wrong = _score(recs, _sent(grps))
    from test_rds_host import _codes_of
    plain = R.parse(bits ^ flips, _codes_of(bits ^ flips))["groups"]
    print("BER 0.01: right %d of 2400, wrong %d of %d accepted; the plain rule: %d of 600 groups" % (right, wrong, recs.size, plain))
    assert right >= 0.90 * 2400
    assert wrong <= 0.01 * recs.size


def test_random_bits_give_no_block():
    """Ten minutes of random bits (seed 7): 0 blocks accepted."""
    recs = S.blocks(np.random.default_rng(7).integers(0, 2, 712500).astype(np.uint8))
    print("random bits: %d accepted" % recs.size)
    assert recs.size <= 2


def test_corrected_blocks_count_for_less(fmrx):
    """A correction can be wrong: it never overwrites what uncorrected blocks wrote, never flips an A/B flag,
    and gives no AF and no clock time; where nothing better has come it does fill the text."""
    grps = [g2a(0, "abcd"), g2a(0, "WXYZ"), g2a(1, "efgh"), g2a(2, "ijkl", ab=1), g0a(0, "AB", af=(227 << 8) | 1),
            g0a(0, "QQ"), g0a(1, "CD")]
    corrected = [(1, 3), (2, 2), (3, 1), (4, 2), (5, 1), (6, 3)]
    got = _both(fmrx, _recs(grps, corrected=corrected)).as_dict()
    # group 1's corrected D may not replace "cd"; its exact C replaces "ab"; group 2's corrected C fills an empty
    # place; group 3's corrected B may not clear the text; group 4's corrected C gives no AF; group 5's corrected
    # B may not replace "AB"; group 6's corrected D fills "CD"
    assert got["rt"] == "WXcdefgh".ljust(64) and got["ps"] == "ABCD    " and got["af"] == [] and got["af_count"] == 0
    assert (got["exact_blocks"], got["corrected_blocks"]) == (28 - 6, 6)
    # and an uncorrected pair then replaces what a corrected one filled
    again = _both(fmrx, _recs(grps + [g2a(1, "EFGH")], corrected=corrected)).as_dict()
    assert again["rt"] == "WXcdEFGH".ljust(64)


# ---- end to end through the oracle's front half -----------------------------------------------

NOISE = 0.07  # of rds_ref.multiplex, against 0.04 of RDS: see the docstring below


def test_noisy_signal_superset_of_the_plain_parser(orc):
    """Mode 0, 20 s (228 groups sent), seed 3.  Up to noise 0.06 the plain parser keeps 212 groups or more, from
    0.08 on the 114 kHz PLL lets go and whole stretches are lost to both parsers (2, 56 and 1 groups at 0.08,
    0.085 and 0.09); at 0.07 the plain parser keeps 73 of 228 (32 %), the block sync 96 complete and 1 partial
    group out of 363 exact and 27 corrected blocks.  Whatever the plain parser filled the new one has filled
    too, and every character either filled is the one sent."""
    out = _run(orc, 0, 20.0, noise=NOISE, seed=3)
    plain = out["info"]
    ext = S.parse_stream(out["bits"])
    print("noise %.3f: sent %d, plain groups %d, sync groups %d + %d, blocks %d + %d" % (
        NOISE, out["sent"], plain["groups"], ext["groups"], ext["partial_groups"], ext["exact_blocks"], ext["corrected_blocks"]))
    assert 0.20 * out["sent"] <= plain["groups"] <= 0.60 * out["sent"]
    assert ext["pi"] == PI
    for name, sent in (("ps", PS), ("rt", RT.ljust(64))):
        for k, (old, new) in enumerate(zip(plain[name], ext[name])):
            assert old == " " or new != " ", (name, k)           # a superset of the places filled
            assert new == " " or new == sent[k], (name, k, new)  # and every character the one sent
            assert old == " " or old == sent[k], (name, k, old)
    assert ext["groups"] + ext["partial_groups"] >= plain["groups"]
