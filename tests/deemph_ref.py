"""What de-emphasis is checked against: a numpy restatement of the tap design and the
oracle's own resample (filter.cpp:67-103 with up = down = 1) and quantiser behind it.  Shared by
tests/test_deemph_host.py and tests/test_gpu_deemph.py."""
from __future__ import annotations

import numpy as np

T = 64          # taps
HIST = T - 1    # inputs carried in front of a call
PAIRS = [(48000, 50), (48000, 75), (44100, 50), (44100, 75)]  # (audio_fs, tau_us): modes 0/1 and 2/3


def pole(audio_fs: int, tau_us: int) -> float:
    return float(np.exp(-1.0 / (audio_fs * tau_us * 1e-6)))


def design(audio_fs: int, tau_us: int) -> np.ndarray:
    """h[n] = (float32) r[n], r[0] = 1 - p, r[n] = r[n-1] p, all in float64."""
    p = pole(audio_fs, tau_us)
    r = np.empty(T, np.float64)
    r[0] = 1.0 - p
    for n in range(1, T):
        r[n] = r[n - 1] * p
    return r.astype(np.float32)


def fir(orc, x, state, h):
    """(y, next state): Oracle.resample(x, state, h, 1, 1) with the carry kept here -- the last 63 of
    state ++ x, also where x is shorter than that (the oracle's own state move reads 63 inputs back
    from the end of x, so x is handed over as the tail of a buffer that holds them)."""
    x = np.asarray(x, np.float32)
    state = np.asarray(state, np.float32)
    buf = np.ascontiguousarray(np.concatenate([state, x]))
    y, _ = orc.resample(buf[HIST:], state, h, 1, 1)
    return y, buf[-HIST:].copy()


def pcm(orc, x, h, state=None):
    """Oracle.quant(Oracle.resample(x, state, h, 1, 1)) from a zero (or the given) state."""
    y, _ = fir(orc, x, np.zeros(HIST, np.float32) if state is None else state, h)
    return orc.quant(y)


def pcm_stereo(orc, left, right, h):
    """The interleaved R, L PCM of de-emphasised left and right rows (each its own filter)."""
    out = np.empty(2 * len(left), np.int16)
    out[0::2] = pcm(orc, right, h)
    out[1::2] = pcm(orc, left, h)
    return out
