"""GPU tests of off-centre tuning (csrc/tuner.hip, fmrx_tune / fmrx_process_shared): every output
is compared bit for bit with the pinned oracle composed around a float32 rotation -- normalize,
rotate by the table fmrx_tuner_design returns (numpy float32: every product and sum rounded
separately; integer phase arithmetic), resample I' and Q' with the RF low-pass, FMDemod, then the
audio thread.  No tolerance anywhere."""
from __future__ import annotations

import functools
import os
import subprocess

import numpy as np
import pytest

import iqgen
import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


_ORC = None


def _orc():
    global _ORC
    if _ORC is None:
        _ORC = oracle.Oracle()
    return _ORC


def compose(iq, mode, rf_taps, offset, first_pair=0, fields=("pcm_mono",)):
    """The expected demod and audio outputs of one stream tuned to `offset`, from position
    first_pair, over the whole of iq in one piece."""
    fm, orc = iqgen.load_fmrx(), _orc()
    rf_fs, bp_fs = oracle.MODES[mode][3], oracle.MODES[mode][5]
    x = orc.normalize(iq)
    xi, xq = x[0::2], x[1::2]
    n_per, k, tab = fm.tuner_design(rf_fs, offset)
    n = (int(first_pair) % n_per + np.arange(xi.size, dtype=np.int64)) % n_per
    p = (k * n) % n_per
    c, s = tab[p, 0], tab[p, 1]
    assert c.dtype == np.float32 and xi.dtype == np.float32
    ri = xi * c + xq * s
    rq = xq * c - xi * s
    h = orc.lpf(rf_fs, 100e3, rf_taps)
    zeros = np.zeros(rf_taps - 1, np.float32)
    i_ds, _ = orc.resample(ri, zeros, h, 1, rf_fs // bp_fs)
    q_ds, _ = orc.resample(rq, zeros, h, 1, rf_fs // bp_fs)
    demod, _ = orc.fmdemod(i_ds, q_ds, [0.0, 0.0])
    out = orc.run_audio(mode, demod, list(fields))
    out["demod"] = demod
    return out


@functools.lru_cache(maxsize=None)
def synth(seed, mode, n_blocks):
    bb, rf_fs = oracle.MODES[mode][0], oracle.MODES[mode][3]
    a = iqgen.make(f"synth:{seed}", n_blocks * bb, rf_fs)
    a.setflags(write=False)
    return a


def rotated(iq, rf_fs, f, amp=1.0):
    """iq moved to +f Hz in float64 (times amp), as complex samples."""
    z = (iq[0::2].astype(np.float64) - 128.0) / 128.0 + 1j * (iq[1::2].astype(np.float64) - 128.0) / 128.0
    n = np.arange(z.size, dtype=np.float64)
    return amp * z * np.exp(2j * np.pi * (f / rf_fs) * n)


def quantised(z):
    out = np.empty(2 * z.size, np.uint8)
    out[0::2] = np.clip(np.rint(z.real * 128.0) + 128.0, 0, 255).astype(np.uint8)
    out[1::2] = np.clip(np.rint(z.imag * 128.0) + 128.0, 0, 255).astype(np.uint8)
    return out


def in_calls(fn, iq, bb, calls):
    """fn over consecutive calls of `calls` blocks each, concatenated along the last axis."""
    out, b = [], 0
    for nb in calls:
        out.append(fn(iq[..., b * bb:(b + nb) * bb]))
        b += nb
    return np.concatenate(out, axis=-1)


def position(rx):
    return rx.tuner_info()[1]


# ---- zero offsets: the new kernel against the shipped one ---------------------------------------

def test_zero_offsets_equal_untuned(fmrx):
    bb, pairs = oracle.MODES[0][0], oracle.MODES[0][0] // 2
    iq = np.stack([synth(1, 0, 7), synth(2, 0, 7)])
    calls = [1, 2, 4]
    with fmrx.Receiver(0, fmrx.MONO, rf_taps=101, n_streams=2) as rx:
        want = in_calls(rx.process, iq, bb, calls)
        assert rx.tuner_info() == ([0, 0], 0, False)
    with fmrx.Receiver(0, fmrx.MONO, rf_taps=101, n_streams=2) as rx:
        rx.tune([0, 0])
        got = in_calls(rx.process, iq, bb, calls)
        assert rx.tuner_info() == ([0, 0], 7 * pairs, True)
    assert np.array_equal(got, want)


# ---- demod and mono PCM against the composed oracle ---------------------------------------------

@pytest.mark.parametrize("offset", [300000, -125000, 1000, 1199000])
@pytest.mark.parametrize("rf_taps", [51, 101])
def test_mode0_demod_and_pcm_match_oracle(fmrx, rf_taps, offset):
    bb, pairs = oracle.MODES[0][0], oracle.MODES[0][0] // 2
    calls = [1, 2, 3, 7]  # phase and history carry across calls and chunk edges
    iq = synth(5, 0, sum(calls))
    want = compose(iq, 0, rf_taps, offset)
    with fmrx.Receiver(0, fmrx.MONO, rf_taps=rf_taps) as rx:
        rx.tune(offset)
        demod = in_calls(rx.rf_block, iq, bb, calls)
        assert position(rx) == sum(calls) * pairs
    assert same(demod, want["demod"])
    with fmrx.Receiver(0, fmrx.MONO, rf_taps=rf_taps) as rx:
        rx.tune(offset)
        pcm = in_calls(rx.process, iq, bb, calls)
        assert position(rx) == sum(calls) * pairs
    assert np.array_equal(pcm, want["pcm_mono"])


def test_mode1_matches_oracle(fmrx):
    bb = oracle.MODES[1][0]
    iq = synth(6, 1, 5)
    want = compose(iq, 1, 51, 200000)
    with fmrx.Receiver(1, fmrx.MONO) as rx:
        rx.tune(200000)
        demod = in_calls(rx.rf_block, iq, bb, [3, 2])
        assert position(rx) == 5 * bb // 2
        rx.reset()
        assert rx.tuner_info() == ([200000], 0, True)  # reset keeps the offsets, rewinds
        pcm = in_calls(rx.process, iq, bb, [3, 2])
    assert same(demod, want["demod"])
    assert np.array_equal(pcm, want["pcm_mono"])


def test_mode2_matches_oracle(fmrx):
    iq = synth(7, 2, 1)
    want = compose(iq, 2, 51, -400000)
    with fmrx.Receiver(2, fmrx.MONO) as rx:
        rx.tune(-400000)
        pcm = rx.process(iq)
        assert position(rx) == iq.size // 2
    assert np.array_equal(pcm, want["pcm_mono"])


def test_mode3_demod_matches_oracle(fmrx):
    """The odd decimation's kernel variant (mode 3: 2.304 MS/s, decimation 9), 101 taps."""
    iq = synth(8, 3, 1)
    want = compose(iq, 3, 101, 96000, fields=("pcm_mono",))
    with fmrx.Receiver(3, fmrx.MONO, rf_taps=101) as rx:
        rx.tune(96000)
        demod = rx.rf_block(iq)
        assert position(rx) == iq.size // 2
    assert same(demod, want["demod"])


def test_position_past_32_bits(fmrx):
    bb, pairs = oracle.MODES[0][0], oracle.MODES[0][0] // 2
    first = 2 ** 32 - 3200  # the call crosses pair 2^32 in its first block
    iq = synth(9, 0, 2)
    want = compose(iq, 0, 51, 1000, first_pair=first)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        rx.tune([1000], first_pair=first)
        pcm = rx.process(iq)
        assert rx.tuner_info() == ([1000], first + 2 * pairs, True)
    assert np.array_equal(pcm, want["pcm_mono"])
    # the position is used: 2^32 - 3200 is 896 mod the 2400-pair period, not 0
    assert not np.array_equal(pcm, compose(iq, 0, 51, 1000)["pcm_mono"])


# ---- one capture, several stations ---------------------------------------------------------------

def test_shared_capture(fmrx):
    bb, na, pairs = oracle.MODES[0][0], oracle.MODES[0][2], oracle.MODES[0][0] // 2
    offsets = [-300000, 0, 100000, 1000]
    iq = synth(10, 0, 5)
    want = np.stack([compose(iq, 0, 51, f)["pcm_mono"] for f in offsets])
    with fmrx.Receiver(0, fmrx.MONO, n_streams=4) as rx:
        rx.tune(offsets)
        host = in_calls(rx.process_shared, iq, bb, [2, 3])
        assert rx.tuner_info() == (offsets, 5 * pairs, True)
    assert np.array_equal(host, want)
    with fmrx.Receiver(0, fmrx.MONO, n_streams=4) as rx:
        rx.tune(offsets)
        d_iq = torch.from_numpy(np.array(iq)).cuda()
        parts = []
        for b0, nb in ((0, 2), (2, 3)):
            d_pcm = torch.zeros(4, nb * na, dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            rx.process_shared_device(d_iq.data_ptr() + b0 * bb, nb, d_pcm.data_ptr())
            rx.synchronize()
            parts.append(d_pcm.cpu().numpy())
        assert position(rx) == 5 * pairs
    assert np.array_equal(np.concatenate(parts, axis=1), want)
    for s, f in enumerate(offsets):  # and a private copy of the bytes gives the same
        with fmrx.Receiver(0, fmrx.MONO) as rx:
            rx.tune(f)
            assert np.array_equal(in_calls(rx.process, iq, bb, [2, 3]), want[s]), f


def test_two_stations_in_one_capture(fmrx):
    bb, rf_fs = oracle.MODES[0][0], oracle.MODES[0][3]
    a, b = synth(11, 0, 20), synth(12, 0, 20)
    iq = quantised(rotated(a, rf_fs, -300000, 0.5) + rotated(b, rf_fs, 300000, 0.5))
    offsets = [-300000, 300000]
    with fmrx.Receiver(0, fmrx.MONO, n_streams=2) as rx:
        rx.tune(offsets)
        got = rx.process_shared(iq)
    for s, f in enumerate(offsets):
        assert np.array_equal(got[s], compose(iq, 0, 51, f)["pcm_mono"]), f
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        pa = rx.process(a).astype(np.float64)
        rx.reset()
        pb = rx.process(b).astype(np.float64)

    def corr(x, y):
        return abs(np.corrcoef(x.astype(np.float64), y)[0, 1])

    assert corr(got[0], pa) > corr(got[0], pb)
    assert corr(got[1], pb) > corr(got[1], pa)


# ---- stereo ----------------------------------------------------------------------------------------

def test_stereo_matches_oracle(fmrx):
    bb, rf_fs = oracle.MODES[0][0], oracle.MODES[0][3]
    iq = quantised(rotated(synth(13, 0, 8), rf_fs, 200000))  # the pilot is real, 200 kHz up
    want = compose(iq, 0, 51, 200000, fields=("pcm",))["pcm"]
    with fmrx.Receiver(0, fmrx.STEREO) as rx:
        rx.tune(200000)
        pcm = in_calls(rx.process, iq, bb, [3, 1, 4])
        assert position(rx) == 8 * bb // 2
    assert np.array_equal(pcm, want)


# ---- lifecycle -------------------------------------------------------------------------------------

def test_tune_off_after_reset_is_the_untuned_receiver(fmrx):
    iq = synth(14, 0, 3)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        want = rx.process(iq)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        rx.tune(300000)
        assert not np.array_equal(rx.process(iq), want)
        rx.reset()
        rx.tune(None)
        assert rx.tuner_info()[2] is False
        assert np.array_equal(rx.process(iq), want)


def test_shared_needs_tuning_and_offsets_are_checked(fmrx):
    iq = synth(14, 0, 1)
    with fmrx.Receiver(0, fmrx.MONO, n_streams=2) as rx:
        with pytest.raises(fmrx.FmrxError) as e:
            rx.process_shared(iq)
        assert e.value.code == fmrx.FMRX_ESTATE
        d = torch.zeros(iq.size, dtype=torch.uint8, device="cuda")
        with pytest.raises(fmrx.FmrxError) as e:
            rx.process_shared_device(d.data_ptr(), 1, d.data_ptr())
        assert e.value.code == fmrx.FMRX_ESTATE
        for bad in ([0, 1200000], [-1200000, 0], [1, 0], [0, 300001]):
            with pytest.raises(fmrx.FmrxError) as e:
                rx.tune(bad)
            assert e.value.code == fmrx.FMRX_EINVAL, bad
            assert rx.tuner_info() == ([0, 0], 0, False)  # a refused call changes nothing


def test_checkpoint_round_trip(fmrx):
    bb = oracle.MODES[0][0]
    iq = synth(15, 0, 4)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        rx.tune(300000)
        whole = in_calls(rx.process, iq, bb, [2, 2])
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        rx.tune(300000)
        head = rx.process(iq[: 2 * bb])
        blob, (off, pos, on) = rx.get_state(), rx.tuner_info()
    assert (off, pos, on) == ([300000], bb, True)
    with fmrx.Receiver(0, fmrx.MONO) as rx:  # the blob holds no tuning: set_state + tune
        rx.set_state(blob)
        rx.tune(off, first_pair=pos)
        tail = rx.process(iq[2 * bb:])
    assert np.array_equal(np.concatenate([head, tail]), whole)
    assert np.array_equal(whole, compose(iq, 0, 51, 300000)["pcm_mono"])


@pytest.mark.parametrize("mode,blocks", [(0, 6), (2, 2)])
def test_time_shard_when_tuned(fmrx, mode, blocks):
    """fmrx_seek + fmrx_tune(first_pair): a shard starting at a block boundary yields the PCM the
    whole recording yields there (the audio history comes from the halo's demod)."""
    bb, na = oracle.MODES[mode][0], oracle.MODES[mode][2]
    iq = synth(16, mode, blocks)
    half = blocks // 2
    with fmrx.Receiver(mode, fmrx.MONO) as rx:
        rx.tune(-125000)
        whole = rx.process(iq)
    with fmrx.Receiver(mode, fmrx.MONO) as rx:
        rx.tune(-125000, first_pair=half * bb // 2)
        rx.seek(iq[: half * bb])
        shard = rx.process(iq[half * bb:])
        assert position(rx) == blocks * bb // 2
    assert np.array_equal(shard, whole[half * na:])


# ---- CLI -------------------------------------------------------------------------------------------

def test_cli_offset(fmrx):
    exe = os.path.join(os.path.dirname(fmrx.LIB_PATH), "bin", "fmrx")
    iq = synth(17, 0, 6)
    r = subprocess.run([exe, "0", "1", "--offset-hz", "300000"], input=iq.tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    with fmrx.Receiver(0, fmrx.STEREO) as rx:  # the CLI writes project's 2-channel stream
        rx.tune(300000)
        want = rx.process(iq)
    assert np.array_equal(np.frombuffer(r.stdout, np.int16), want)
    bad = subprocess.run([exe, "0", "1", "--offset-hz", "1"], input=b"", capture_output=True, timeout=120)
    assert bad.returncode == 1 and b"offset" in bad.stderr
