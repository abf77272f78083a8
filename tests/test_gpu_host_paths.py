"""GPU tests of the host runtime's shared call paths (csrc/engine.cpp, front.cpp, process.cpp): the
fmrx_kernel_timing event pairs of the fused kernel and of the wide down-converter, and both sides of
the pinned staging limit of fmrx_process, fmrx_rf_block and fmrx_audio_block.  Every PCM is compared
bit for bit with the oracle's; no tolerance anywhere."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import iqgen
import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PINNED_CALL_BYTES = 4 << 20  # csrc/ctx.h kPinnedCallBytes: calls up to this many input bytes are staged pinned
STREAMS = 8


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def around_limit(bytes_per_block):
    """(n, n + 1): the block counts of the last call on the pinned route and the first past it."""
    n = PINNED_CALL_BYTES // bytes_per_block
    assert n >= 1 and n * bytes_per_block <= PINNED_CALL_BYTES < (n + 1) * bytes_per_block
    return n, n + 1


@functools.lru_cache(maxsize=None)
def mode0_run(n_blocks):
    """One mode-0 u8 capture of n_blocks blocks and the oracle's demod, mono PCM and stereo PCM of it
    (read-only; a shorter call's outputs are their prefixes: every stage is causal)."""
    iq = iqgen.make("synth:77", n_blocks * oracle.MODES[0][0])
    out = oracle.Oracle().run(0, 51, iq, ["demod", "pcm_mono", "pcm"])
    for a in (iq, out["demod"], out["pcm_mono"], out["pcm"]):
        a.setflags(write=False)
    return iq, out


def longest(fmrx):
    """Block count of the longest case below (fmrx_process, one stream, past the limit)."""
    return around_limit(fmrx.geometry(fmrx.default_config(0, fmrx.MONO)).block_bytes)[1]


def rows(a, n):
    return np.tile(a[:n], (STREAMS, 1))


# ---- fmrx_kernel_timing ------------------------------------------------------------------------------------

def test_kernel_timing_mono(fmrx):
    iq = iqgen.make("synth:5", 4 * oracle.MODES[0][0])
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        rx.kernel_timing(1)
        rx.process(iq)
        avg_ms, launches = rx.kernel_timing(0)
        print("kernel_timing mono: avg_ms", avg_ms, "launches", launches)
        assert launches == 1 and avg_ms > 0
        rx.process(iq)
        assert rx.kernel_timing(-1)[1] == 2
        rx.process(iq)
        assert rx.kernel_timing(0) == (0.0, 0)


def test_kernel_timing_wide(fmrx):
    d = 2
    raw = iqgen.make("synth:6", 4 * d * oracle.MODES[0][0], d * oracle.MODES[0][3])
    pcm = []
    for armed in (True, False):
        with fmrx.Receiver(0, fmrx.MONO) as rx:
            rx.set_capture_decim(d)
            rx.tune_wide(oracle.MODES[0][3] // 4)
            if armed:
                rx.kernel_timing(1)
            pcm.append(rx.process_wide(raw))
            avg_ms, launches = rx.kernel_timing(0)
            print("kernel_timing wide: armed", armed, "avg_ms", avg_ms, "launches", launches)
            assert launches == (1 if armed else 0)  # the down-converter, one launch a piece
            assert (avg_ms > 0) == armed
    assert np.array_equal(pcm[0], pcm[1]) and pcm[0].any()


# ---- the pinned staging limit ------------------------------------------------------------------------------

@pytest.mark.parametrize("side", [0, 1], ids=["pinned", "device"])
def test_process_limit(fmrx, side):
    iq, want = mode0_run(longest(fmrx))
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        n = around_limit(rx.geo.block_bytes)[side]
        got = rx.process(iq[: n * rx.geo.block_bytes])
        assert np.array_equal(got, want["pcm_mono"][: n * rx.geo.pcm_samples]) and got.any()


@pytest.mark.parametrize("side", [0, 1], ids=["pinned", "device"])
def test_rf_block_limit(fmrx, side):
    iq, want = mode0_run(longest(fmrx))
    with fmrx.Receiver(0, fmrx.MONO, n_streams=STREAMS) as rx:
        n = around_limit(STREAMS * rx.geo.block_bytes)[side]
        demod = rx.rf_block(rows(iq, n * rx.geo.block_bytes))
        assert np.array_equal(demod, rows(want["demod"], n * rx.geo.if_samples))
        got = rx.audio_block(demod)
        assert np.array_equal(got, rows(want["pcm_mono"], n * rx.geo.pcm_samples)) and got.any()


@pytest.mark.parametrize("side", [0, 1], ids=["pinned", "device"])
@pytest.mark.parametrize("channels", ["MONO", "STEREO"])
def test_audio_block_limit(fmrx, channels, side):
    """The limit is on the demod bytes here.  Stereo, pinned: the band-pass kernel reads the pinned
    demod in place."""
    _, want = mode0_run(longest(fmrx))
    with fmrx.Receiver(0, getattr(fmrx, channels), n_streams=STREAMS) as rx:
        n = around_limit(STREAMS * rx.geo.if_samples * 4)[side]
        got = rx.audio_block(rows(want["demod"], n * rx.geo.if_samples))
        pcm = want["pcm_mono" if channels == "MONO" else "pcm"]
        assert np.array_equal(got, rows(pcm, n * rx.geo.pcm_samples)) and got.any()
