"""tests/rds_ref.py — helper of the RDS back half's tests (not a test).

The numpy restatement of DESIGN §5.10's steps 2..7 on top of the oracle's RDS front half
(``Oracle.rds``) and the reference's ``resample`` (``Oracle.resample``), an RDS transmitter (groups
with valid checkwords, differential and biphase coding on a 57 kHz subcarrier), and an FM modulator
to u8 I/Q.  Everything the GPU writes is compared with this for equality, never with a tolerance.
"""
from __future__ import annotations

import numpy as np

import iqgen
import oracle

UP, PHASE_TAPS, WIN, CHIPS, SYMS = 19, 101, 2432, 152, 76
OFFSETS = {1: 0x0FC, 2: 0x198, 3: 0x168, 4: 0x350, 5: 0x1B4}  # A, B, C, C', D
GRANULES = {0: 24, 1: 24, 2: 3, 3: 1}
BITRATE = 1187.5


def bp_fs(mode: int) -> int:
    return oracle.MODES[mode][5]


def granule_samples(mode: int) -> int:
    return GRANULES[mode] * oracle.MODES[mode][1]


# ---- steps 1..6 -------------------------------------------------------------------------------

_taps = {}


def taps(orc, mode: int) -> np.ndarray:
    if mode not in _taps:
        _taps[mode] = orc.lpf(float(bp_fs(mode) * UP), 3000.0, PHASE_TAPS * UP, UP)
    return _taps[mode]


def resample(orc, mode: int, mix: np.ndarray, state=None):
    """Step 1: (y, state) of the mixer samples, from zeros unless a state is given."""
    h = taps(orc, mode)
    if state is None:
        state = np.zeros(h.size - 1, np.float32)
    return orc.resample(mix, state, h, UP, bp_fs(mode) // 2000)


def crc10(info: np.ndarray) -> np.ndarray:
    """x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1 over 16 information bits, MSB first, zero start."""
    info = np.asarray(info, np.int64)
    reg = np.zeros_like(info)
    for k in range(15, -1, -1):
        fb = ((reg >> 9) & 1) ^ ((info >> k) & 1)
        reg = ((reg << 1) & 0x3FF) ^ (fb * 0x1B9)
    return reg


def bits_from_y(y: np.ndarray) -> dict:
    """Steps 2..6 over whole windows of y: bits, codes (76 a window), win (windows x (p, q))."""
    y = np.asarray(y, np.float32)
    nw = y.size // WIN
    assert nw * WIN == y.size, "whole windows"
    s = np.concatenate(([1], (y >= np.float32(0.0)).astype(np.uint8))).astype(np.uint8)  # s[n] at index n + 1
    win = np.zeros((nw, 2), np.uint8)
    d = np.zeros(nw * SYMS, np.uint8)
    last_chip = 1
    for w in range(nw):
        seg = s[w * WIN: (w + 1) * WIN + 1]
        change = seg[1:] != seg[:-1]
        hist = change.reshape(-1, 16).sum(axis=0)
        p = (int(np.argmax(hist)) + 8) % 16  # argmax: the lowest index of the largest
        c = seg[1:][p::16]
        assert c.size == CHIPS
        e = np.concatenate(([last_chip], c)).astype(np.uint8)
        v0 = int(np.sum(e[0:152:2] == e[1:153:2]))
        v1 = int(np.sum(e[1:153:2] == e[2:153:2]))
        q = 0 if v1 <= v0 else 1
        d[w * SYMS: (w + 1) * SYMS] = e[1:153:2] if q == 0 else e[0:152:2]
        win[w] = (p, q)
        last_chip = int(c[-1])
    bits = d ^ np.concatenate(([0], d[:-1])).astype(np.uint8)
    codes = np.zeros(bits.size, np.uint8)
    if bits.size >= 26:
        view = np.lib.stride_tricks.sliding_window_view(bits, 26).astype(np.int64)
        word = view @ (1 << np.arange(25, -1, -1, dtype=np.int64))
        syn = crc10(word >> 10) ^ (word & 0x3FF)
        tail = np.zeros(syn.size, np.uint8)
        for code, off in OFFSETS.items():
            tail[syn == off] = code
        codes[25:] = tail
    return {"bits": bits, "codes": codes, "win": win}


def back_half(orc, mode: int, mix: np.ndarray) -> dict:
    """Steps 1..6 of one stream's mixer samples (whole granules), plus y."""
    y, _ = resample(orc, mode, mix)
    out = bits_from_y(y)
    out["y"] = y
    return out


def from_demod(orc, mode: int, demod: np.ndarray) -> dict:
    """The oracle's front half, then steps 1..7."""
    out = back_half(orc, mode, orc.rds(mode, demod)["rds"])
    out["info"] = parse(out["bits"], out["codes"])
    return out


# ---- step 7 -----------------------------------------------------------------------------------

def _chr(b: int) -> str:
    return chr(b) if 0x20 <= b <= 0x7E else " "


def parse(bits, codes) -> dict:
    """The group parser over a whole stream."""
    bits = np.asarray(bits, np.uint8)
    codes = np.asarray(codes, np.uint8)
    n = bits.size
    info = {"pi": 0, "pty": 0, "tp": 0, "ps": [" "] * 8, "rt": [" "] * 64, "bits": n,
            "blocks": int(np.count_nonzero(codes)), "groups": 0}
    ab = 0
    pw = 1 << np.arange(15, -1, -1, dtype=np.int64)
    if n >= 104:
        i = np.arange(25, n - 78)
        ok = (codes[i] == 1) & (codes[i + 26] == 2) & ((codes[i + 52] == 3) | (codes[i + 52] == 4)) & (codes[i + 78] == 5)
        for a_end in i[ok]:
            start = a_end - 25
            blk = [int(bits[start + 26 * k: start + 26 * k + 16].astype(np.int64) @ pw) for k in range(4)]
            a, b, c, d = blk
            info["groups"] += 1
            info["pi"], info["tp"], info["pty"] = a, (b >> 10) & 1, (b >> 5) & 0x1F
            typ, ver = b >> 12, (b >> 11) & 1
            if typ == 0:
                at = 2 * (b & 3)
                info["ps"][at: at + 2] = [_chr(d >> 8), _chr(d & 0xFF)]
            elif typ == 2:
                flag = (b >> 4) & 1
                if flag != ab:
                    info["rt"] = [" "] * 64
                ab = flag
                if ver == 0:
                    at = 4 * (b & 15)
                    info["rt"][at: at + 4] = [_chr(c >> 8), _chr(c & 0xFF), _chr(d >> 8), _chr(d & 0xFF)]
                else:
                    at = 2 * (b & 15)
                    info["rt"][at: at + 2] = [_chr(d >> 8), _chr(d & 0xFF)]
    info["ps"] = "".join(info["ps"])
    info["rt"] = "".join(info["rt"])
    return info


# ---- transmitter ------------------------------------------------------------------------------

def block_bits(info16: int, code: int) -> list:
    word = (info16 << 10) | (int(crc10(np.array([info16]))[0]) ^ OFFSETS[code])
    return [(word >> k) & 1 for k in range(25, -1, -1)]


def group_bits(a: int, b: int, c: int, d: int, c_prime: bool = False) -> list:
    return block_bits(a, 1) + block_bits(b, 2) + block_bits(c, 4 if c_prime else 3) + block_bits(d, 5)


def groups(pi: int, ps: str, rt: str | None, n_groups: int, pty: int = 5, tp: int = 1) -> list:
    """n_groups groups as (a, b, c, d): 0A groups cycling the PS name, alternating with 2A groups
    cycling the RadioText when there is one (a multiple of 4 characters)."""
    ps = ps.ljust(8)[:8]
    out, k0, k2 = [], 0, 0
    n_rt = len(rt) // 4 if rt else 0
    for g in range(n_groups):
        base = (tp << 10) | (pty << 5)
        if n_rt and g % 2 == 1:
            at = k2 % n_rt
            k2 += 1
            ch = [ord(x) for x in rt[4 * at: 4 * at + 4]]
            out.append((pi, (2 << 12) | base | at, (ch[0] << 8) | ch[1], (ch[2] << 8) | ch[3]))
        else:
            at = k0 % 4
            k0 += 1
            out.append((pi, base | at, 0xE0CD, (ord(ps[2 * at]) << 8) | ord(ps[2 * at + 1])))
    return out


def stream_bits(grps) -> np.ndarray:
    return np.array([x for g in grps for x in group_bits(*g)], np.uint8)


def n_groups_for(seconds: float) -> int:
    return int(seconds * BITRATE / 104) + 2


def multiplex(t: np.ndarray, bits: np.ndarray, seed: int = 1, noise: float = 0.002, ppm: float = 0.0,
              phase: float = 0.0) -> np.ndarray:
    """iqgen.make_rds_demod's signal at the times t (seconds, float64) with these bits: 1 kHz tone,
    19 kHz pilot, and the differentially coded, biphase-shaped symbols on 57 kHz.  ppm: the symbol
    clock's error; phase: its start, in bits.  Runs past the last bit repeat the stream."""
    d = np.bitwise_xor.accumulate(np.asarray(bits, np.uint8))  # d[i] = bit[i] ^ d[i-1], d[-1] = 0
    sym = 2.0 * d.astype(np.float64) - 1.0
    ph = t * (BITRATE * (1.0 + ppm * 1e-6)) + phase
    k = np.floor(ph).astype(np.int64)
    half = np.where(ph - k < 0.5, 1.0, -1.0)
    rds = sym[k % sym.size] * half
    nz = (iqgen.rand_bytes(seed + 17, t.size).astype(np.float64) - 127.5) / 127.5
    return (0.30 * np.sin(2 * np.pi * 1000.0 * t) + 0.05 * np.cos(2 * np.pi * 19000.0 * t)
            + 0.04 * rds * np.cos(2 * np.pi * 57000.0 * t) + noise * nz)


def make_demod(mode: int, n: int, bits: np.ndarray, **kw) -> np.ndarray:
    """n demod-rate samples (float32) of the multiplex."""
    return multiplex(np.arange(n, dtype=np.float64) / bp_fs(mode), bits, **kw).astype(np.float32)


def fm_signal(mode: int, n_pairs: int, bits: np.ndarray, offset_hz: float = 0.0, rf_fs: int | None = None,
              **kw) -> np.ndarray:
    """The multiplex, evaluated at rf_fs, frequency-modulated: the phase is the running sum of
    multiplex / rf_decim (the discriminator then returns the multiplex at the IF rate), plus the
    offset's ramp.  Complex128, unit amplitude."""
    fs = rf_fs or oracle.MODES[mode][3]
    rf_decim = oracle.MODES[mode][3] // oracle.MODES[mode][5]
    n = np.arange(n_pairs, dtype=np.float64)
    mpx = multiplex(n / fs, bits, **kw) * (oracle.MODES[mode][3] / fs)
    phi = np.cumsum(mpx / rf_decim) + 2 * np.pi * offset_hz * n / fs
    return np.exp(1j * phi)


def _dither(n: int, lsb: float, seed: int) -> np.ndarray:
    """Uniform noise of +-lsb: a receiver's noise floor (a noiseless capture's quantisation spurs and
    near-empty channels would otherwise pass a band scan's threshold)."""
    return lsb * (iqgen.rand_bytes(seed, n).astype(np.float64) - 127.5) / 127.5 if lsb else np.zeros(n)


def to_u8(z: np.ndarray, amp: float = 100.0, noise_lsb: float = 0.0, seed: int = 99) -> np.ndarray:
    """Interleaved u8 I/Q of amp z around 128 (the format's zero); amp |z| must stay within 120."""
    assert amp * np.max(np.abs(z)) + noise_lsb <= 120.0
    out = np.empty(2 * z.size, np.float64)
    out[0::2] = 128.0 + amp * z.real
    out[1::2] = 128.0 + amp * z.imag
    return np.clip(np.round(out + _dither(out.size, noise_lsb, seed)), 0, 255).astype(np.uint8)


def to_s16(z: np.ndarray, amp: float = 12000.0, noise_lsb: float = 0.0, seed: int = 98) -> np.ndarray:
    assert amp * np.max(np.abs(z)) + noise_lsb <= 32000.0
    out = np.empty(2 * z.size, np.float64)
    out[0::2] = amp * z.real
    out[1::2] = amp * z.imag
    return np.round(out + _dither(out.size, noise_lsb, seed)).astype("<i2")
