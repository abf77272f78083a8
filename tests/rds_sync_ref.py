"""tests/rds_sync_ref.py — helper of the RDS block sync's tests (not a test).

The numpy restatement of DESIGN §5.13: syndromes, the burst table, candidates, the vote, the
acceptance and the block-wise group parser.  Everything is integer arithmetic; whatever the GPU and
the C parser write is compared with this for equality, never with a tolerance.
"""
from __future__ import annotations

import numpy as np

import rds_ref

J, V, B = 8, 3, 2                       # the default constants (fmrx_rds_sync_config_default)
OFFS = (0x0FC, 0x198, 0x168, 0x350, 0x1B4)  # A, B, C, C', D
NONE = 0xFFFFFFFF
BLOCK = np.dtype([("bit", "<u8"), ("info", "<u2"), ("slot", "u1"), ("c_prime", "u1"), ("corrected", "u1"),
                  ("votes", "u1"), ("pad", "u1", (2,))])  # fmrx_rds_block_rec
EXT_TAIL = 16                           # FMRX_RDS_EXT_TAIL: records the parser keeps


def syndrome26(word) -> np.ndarray:
    """The remainder of a 26-bit word by the generator 0x5B9: crc10(word >> 10) ^ (word & 0x3FF)."""
    word = np.asarray(word, np.int64)
    return rds_ref.crc10(word >> 10) ^ (word & 0x3FF)


def burst_patterns(b: int) -> list:
    """Every 26-bit burst of length <= b (first and last bit of the burst set) at every shift."""
    out = []
    for length in range(1, b + 1):
        inner = 1 if length <= 2 else 1 << (length - 2)
        for mid in range(inner):
            pat = 1 if length == 1 else (1 << (length - 1)) | (mid << 1) | 1
            for shift in range(0, 26 - length + 1):
                out.append(pat << shift)
    return out


def burst_table(b: int = B):
    """(table, collisions): 1024 entries by syndrome, the burst's 26-bit pattern or NONE; entry 0
    is the empty pattern.  collisions: patterns whose syndrome another pattern took first."""
    tab = np.full(1024, NONE, np.uint32)
    tab[0] = 0
    collisions = 0
    for pat in burst_patterns(b):
        s = int(syndrome26(pat))
        if tab[s] != NONE:
            collisions += 1
            continue
        tab[s] = pat
    return tab, collisions


def words_syndromes(bits: np.ndarray):
    """(word, syn) at every bit; zeros for i < 25."""
    bits = np.asarray(bits, np.uint8)
    n = bits.size
    word = np.zeros(n, np.int64)
    syn = np.zeros(n, np.int64)
    if n >= 26:
        view = np.lib.stride_tricks.sliding_window_view(bits, 26).astype(np.int64)
        word[25:] = view @ (1 << np.arange(25, -1, -1, dtype=np.int64))
        syn[25:] = syndrome26(word[25:])
    return word, syn


def candidates(bits: np.ndarray, b: int = B):
    """exact (4 x n bool) and cand (4 x n int64: info16 | valid << 16 | corrected << 17 | C' << 18)."""
    tab, _ = burst_table(b)
    word, syn = words_syndromes(bits)
    n = word.size
    have = np.arange(n) >= 25
    exact = np.zeros((4, n), bool)
    cand = np.zeros((4, n), np.int64)
    tries = {0: [(OFFS[0], 0)], 1: [(OFFS[1], 0)], 2: [(OFFS[2], 0), (OFFS[3], 1)], 3: [(OFFS[4], 0)]}
    for u in range(4):
        done = np.zeros(n, bool)
        for off, cp in tries[u]:  # exact first, C before C'
            hit = have & (syn == off) & ~done
            exact[u] |= hit
            cand[u][hit] = (word[hit] >> 10) | (1 << 16) | (cp << 18)
            done |= hit
        for off, cp in tries[u]:  # then correctable, C before C'
            pat = tab[(syn ^ off) & 0x3FF].astype(np.int64)
            hit = have & (pat != NONE) & ~done
            cand[u][hit] = ((word[hit] ^ pat[hit]) >> 10) | (1 << 16) | (1 << 17) | (cp << 18)
            done |= hit
    return exact, cand


def blocks(bits: np.ndarray, j: int = J, v: int = V, b: int = B) -> np.ndarray:
    """The accepted block records of a whole stream (every position judged, absent neighbours no match)."""
    bits = np.asarray(bits, np.uint8)
    n = bits.size
    exact, cand = candidates(bits, b)
    votes = np.zeros((4, n), np.int64)
    for u in range(4):
        for jj in range(-j, j + 1):
            if jj == 0:
                continue
            src = np.arange(n) + 26 * jj
            ok = (src >= 0) & (src < n)
            votes[u][ok] += exact[(u + jj) % 4][src[ok]]
    best_u = np.full(n, -1, np.int64)
    best_v = np.full(n, -1, np.int64)
    for u in range(4):
        q = ((cand[u] >> 16) & 1).astype(bool) & (votes[u] >= v) & (votes[u] > best_v)
        best_u[q] = u
        best_v[q] = votes[u][q]
    at = np.nonzero(best_u >= 0)[0]
    out = np.zeros(at.size, BLOCK)
    c = cand[best_u[at], at]
    out["bit"] = at
    out["info"] = c & 0xFFFF
    out["slot"] = best_u[at]
    out["c_prime"] = (c >> 18) & 1
    out["corrected"] = (c >> 17) & 1
    out["votes"] = best_v[at]
    return out


# ---- the block-wise parser ---------------------------------------------------------------------

def _chr(b: int) -> str:
    return chr(b) if 0x20 <= b <= 0x7E else " "


def mjd_date(mjd: int):
    """(year, month, day) by the standard's formula (IEC 62106 annex G, good from 1900-03-01 to
    2100-02-28) in integers; zeros below 15079."""
    if mjd < 15079:
        return 0, 0, 0
    y = (mjd * 100 - 1507820) // 36525
    yd = (y * 1461) // 4
    m = ((mjd - yd) * 10000 - 149561000) // 306001
    d = mjd - 14956 - yd - (m * 306001) // 10000
    k = 1 if m in (14, 15) else 0
    return 1900 + y + k, m - 1 - 12 * k, d


def ext_init() -> dict:
    return {"bits": 0, "exact": 0, "corrected": 0, "groups": 0, "partial": 0, "pi": 0, "pi_set": 0, "pty": 0,
            "tp": 0, "ta": 0, "ms": 0, "di": 0, "rt_ab": 0, "ptyn_ab": 0, "ps": [" "] * 8, "rt": [" "] * 64,
            "ptyn": [" "] * 8, "ps_sure": [False] * 8, "rt_sure": [False] * 64, "ptyn_sure": [False] * 8,
            "af": [], "af_count": 0,
            "ct": None, "tail": [], "done": []}


def _group(x: dict, rec) -> None:
    """Close the B block rec with whatever of A, C*, D the tail holds."""
    at = int(rec["bit"])
    find = lambda bit, slot: next((r for r in x["tail"] if int(r["bit"]) == bit and int(r["slot"]) == slot), None)
    a, c, d = find(at - 26, 0), find(at + 26, 2), find(at + 52, 3)
    if a is not None and a["corrected"] and not (x["pi_set"] and int(a["info"]) == x["pi"]):
        a = None
    b = int(rec["info"])
    if a is not None and c is not None and d is not None:
        x["groups"] += 1
    else:
        x["partial"] += 1
    x["tp"], x["pty"] = (b >> 10) & 1, (b >> 5) & 0x1F
    typ, ver = b >> 12, (b >> 11) & 1
    cw = None if c is None else int(c["info"])
    dw = None if d is None else int(d["info"])
    c_plain = c is not None and not c["c_prime"]
    b_sure = not rec["corrected"]
    c_sure = b_sure and c is not None and not c["corrected"]
    d_sure = b_sure and d is not None and not d["corrected"]

    def put2(name, pos, w, sure):
        """Two characters: a block pair without a correction always writes and marks the places its own;
        one with a correction writes only places not so marked."""
        for k, ch in enumerate((_chr(w >> 8), _chr(w & 0xFF))):
            if sure:
                x[name][pos + k], x[name + "_sure"][pos + k] = ch, True
            elif not x[name + "_sure"][pos + k]:
                x[name][pos + k] = ch

    def flag(name, f):
        """The A/B flag rule: a change clears the text; a corrected B block may not change it (False: skip)."""
        if f != x[name + "_ab"]:
            if not b_sure:
                return False
            x[name], x[name + "_sure"] = [" "] * len(x[name]), [False] * len(x[name])
            x[name + "_ab"] = f
        return True

    if typ == 0:
        x["ta"], x["ms"] = (b >> 4) & 1, (b >> 3) & 1
        seg = b & 3
        x["di"] = (x["di"] & ~(1 << (3 - seg))) | (((b >> 2) & 1) << (3 - seg))
        if dw is not None:
            put2("ps", 2 * seg, dw, d_sure)
        if ver == 0 and c_plain and c_sure:
            for code in (cw >> 8, cw & 0xFF):
                if 1 <= code <= 204:
                    if code not in x["af"] and len(x["af"]) < 25:
                        x["af"].append(code)
                elif 224 <= code <= 249:
                    x["af_count"] = code - 224
    elif typ == 2:
        if flag("rt", (b >> 4) & 1):
            if ver == 0:
                pos = 4 * (b & 15)
                if c_plain:
                    put2("rt", pos, cw, c_sure)
                if dw is not None:
                    put2("rt", pos + 2, dw, d_sure)
            elif dw is not None:
                put2("rt", 2 * (b & 15), dw, d_sure)
    elif typ == 4 and ver == 0 and c_plain and c_sure and d_sure:
        mjd = ((b & 3) << 15) | (cw >> 1)
        hour, minute = ((cw & 1) << 4) | (dw >> 12), (dw >> 6) & 0x3F
        if hour < 24 and minute < 60:
            off = dw & 0x1F
            y, m, dd = mjd_date(mjd)
            x["ct"] = {"mjd": mjd, "year": y, "month": m, "day": dd, "hour": hour, "minute": minute,
                       "offset": -off if (dw >> 5) & 1 else off}
    elif typ == 10 and ver == 0:
        if flag("ptyn", (b >> 4) & 1):
            pos = 4 * (b & 1)
            if c_plain:
                put2("ptyn", pos, cw, c_sure)
            if dw is not None:
                put2("ptyn", pos + 2, dw, d_sure)


def _close(x: dict, before) -> None:
    """Close the open B blocks whose D position lies before `before` (None: all of them)."""
    for k, r in enumerate(x["tail"]):
        if int(r["slot"]) == 1 and not x["done"][k] and (before is None or int(r["bit"]) + 52 < before):
            x["done"][k] = True
            _group(x, r)


def parse_blocks(x: dict, recs, n_bits: int = 0, flush: bool = False) -> dict:
    """fmrx_rds_parse_blocks: the records in stream order, in pieces of any size, into x (ext_init())."""
    x["bits"] += int(n_bits)
    for r in recs:
        _close(x, int(r["bit"]))
        x["tail"].append(r)
        x["done"].append(False)
        if len(x["tail"]) > EXT_TAIL:
            x["tail"].pop(0)
            x["done"].pop(0)
        x["corrected" if r["corrected"] else "exact"] += 1
        if int(r["slot"]) == 0 and not r["corrected"]:
            x["pi"], x["pi_set"] = int(r["info"]), 1
        _close(x, int(r["bit"]) + 1)
    if flush:
        _close(x, None)
    return x


def ext_dict(x: dict) -> dict:
    """What RdsExt.as_dict() returns."""
    return {"pi": x["pi"] if x["pi_set"] else None, "pty": x["pty"], "tp": x["tp"], "ta": x["ta"], "ms": x["ms"],
            "di": x["di"], "ps": "".join(x["ps"]), "rt": "".join(x["rt"]), "ptyn": "".join(x["ptyn"]),
            "af": [round(87.5 + 0.1 * c, 1) for c in x["af"]], "af_count": x["af_count"], "ct": x["ct"],
            "bits": x["bits"], "exact_blocks": x["exact"], "corrected_blocks": x["corrected"],
            "groups": x["groups"], "partial_groups": x["partial"]}


def parse_stream(bits, j: int = J, v: int = V, b: int = B) -> dict:
    """blocks() and the parser over a whole stream, flushed."""
    bits = np.asarray(bits, np.uint8)
    return ext_dict(parse_blocks(ext_init(), blocks(bits, j, v, b), bits.size, flush=True))
