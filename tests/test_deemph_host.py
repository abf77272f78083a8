"""CPU tests of FM de-emphasis: the tap design behind fmrx_deemph_design against a numpy
restatement, what the 64-tap cut costs against the analogue 1 / (1 + j w tau), and the definition itself
-- the oracle's resample with up = down = 1 -- carried over pieces of any size."""
from __future__ import annotations

import numpy as np
import pytest

import deemph_ref as dr


@pytest.mark.parametrize("audio_fs,tau", dr.PAIRS)
def test_design_within_one_ulp_of_numpy(fmrx, audio_fs, tau):
    h = fmrx.deemph_design(audio_fs, tau)
    want = dr.design(audio_fs, tau)
    assert h.shape == (dr.T,) and h.dtype == np.float32
    err = np.abs(h.astype(np.float64) - want.astype(np.float64))
    assert np.all(err <= np.spacing(want).astype(np.float64)), int(np.argmax(err))


@pytest.mark.parametrize("audio_fs,tau", dr.PAIRS)
def test_taps_positive_decreasing_unit_sum(fmrx, audio_fs, tau):
    h = fmrx.deemph_design(audio_fs, tau)
    assert np.all(h > 0) and np.all(np.diff(h) < 0)
    assert abs(float(np.sum(h.astype(np.float64))) - 1.0) < 1e-6


@pytest.mark.parametrize("audio_fs,tau", dr.PAIRS)
def test_tail_below_half_an_ulp(audio_fs, tau):
    """What lets 64 taps stand for the one-pole filter: the response past them sums to p^64."""
    assert dr.pole(audio_fs, tau) ** dr.T < 2.0 ** -25


@pytest.mark.parametrize("audio_fs,tau", [(48000, 0), (48000, 49), (48000, 100), (0, 50), (-44100, 75)])
def test_design_refusals(fmrx, audio_fs, tau):
    with pytest.raises(fmrx.FmrxError) as e:
        fmrx.deemph_design(audio_fs, tau)
    assert e.value.code == fmrx.FMRX_EINVAL


def test_design_refuses_null_taps(fmrx):
    assert fmrx.lib().fmrx_deemph_design(48000, 50, None) == fmrx.FMRX_EINVAL


@pytest.mark.parametrize("audio_fs,tau", dr.PAIRS)
def test_response_against_the_analogue_filter(fmrx, audio_fs, tau):
    """|H| of the float32 taps, in float64, over |1 / (1 + j w tau)| in 10 Hz steps: the sampled
    one-pole filter never lies below the analogue one, and lies above it by at most 1.44 dB (48 kHz)
    or 1.71 dB (44.1 kHz) up to 15 kHz, 0.63 / 0.74 dB up to 10 kHz."""
    h = fmrx.deemph_design(audio_fs, tau).astype(np.float64)
    f = np.arange(0.0, 15000.0 + 1.0, 10.0)
    w = 2.0 * np.pi * f / audio_fs
    H = np.exp(-1j * np.outer(w, np.arange(dr.T))) @ h
    analogue = 1.0 / np.sqrt(1.0 + (2.0 * np.pi * f * tau * 1e-6) ** 2)
    dev = 20.0 * np.log10(np.abs(H) / analogue)
    print(f"{audio_fs} S/s {tau} us: deviation min {dev.min():.4f} dB, max to 15 kHz {dev.max():.4f} dB, "
          f"max to 10 kHz {dev[f <= 10000.0].max():.4f} dB")
    assert dev.min() >= -0.01 and dev.max() <= 1.8
    assert dev[f <= 10000.0].max() <= 0.8


@pytest.mark.parametrize("audio_fs,tau", dr.PAIRS)
def test_pieces_equal_one_call(fmrx, orc, audio_fs, tau):
    """Oracle.resample(x, zeros(63), h, 1, 1) over pieces of 1, 17, 63, 64 and 200 samples with the
    state carried equals one call, bit for bit (NaN and values past +-1 among the samples)."""
    h = fmrx.deemph_design(audio_fs, tau)
    rng = np.random.default_rng(1000 * tau + audio_fs)
    x = rng.uniform(-1.5, 1.5, 1 + 17 + 63 + 64 + 200).astype(np.float32)
    x[150] = np.nan
    whole, _ = orc.resample(x, np.zeros(dr.HIST, np.float32), h, 1, 1)
    state, parts, pos = np.zeros(dr.HIST, np.float32), [], 0
    for n in (1, 17, 63, 64, 200):
        y, state = dr.fir(orc, x[pos:pos + n], state, h)
        parts.append(y)
        pos += n
    got = np.concatenate(parts)
    assert np.array_equal(got.view(np.uint32), whole.view(np.uint32))
    assert np.array_equal(state.view(np.uint32), x[-dr.HIST:].view(np.uint32))
