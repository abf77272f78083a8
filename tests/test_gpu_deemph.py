"""GPU tests of FM de-emphasis (csrc/deemph.hip, fmrx_set_deemphasis, fmrx_deemph).

Every PCM comparison is bit for bit (np.array_equal) against the definition:
Oracle.quant(Oracle.resample(x, state, h, 1, 1)) with h from fmrx_deemph_design and x the oracle's
mono_indep (mono contexts) or its left and right (stereo contexts, each row its own filter).  No
tolerance anywhere."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import deemph_ref as dr
import iqgen
import oracle
from conftest import case_input, load_case

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


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def synth(seed, mode, n_blocks):
    return iqgen.make(f"synth:{seed}", n_blocks * oracle.MODES[mode][0], oracle.MODES[mode][3])


def taps(fm, mode, tau):
    fs = 48000 if mode < 2 else 44100
    return fm.deemph_design(fs, tau)


def want_pcm(orc, fm, mode, rf_taps, iq, tau, stereo=False):
    """The de-emphasised PCM of one stream over the whole of iq, from zero state."""
    h = taps(fm, mode, tau)
    if stereo:
        o = orc.run(mode, rf_taps, iq, ["left", "right"])
        return dr.pcm_stereo(orc, o["left"], o["right"], h)
    return dr.pcm(orc, orc.run(mode, rf_taps, iq, ["mono_indep"])["mono_indep"], h)


def in_calls(fn, iq, bb, calls):
    out, b = [], 0
    for nb in calls:
        out.append(fn(iq[..., b * bb:(b + nb) * bb]))
        b += nb
    return np.concatenate(out, axis=-1)


# ---- the primitive ---------------------------------------------------------------------------------

def prim_input(n, seed):
    """Seeded floats in (-1.5, 1.5) with a few far past +-1 and, from 3 samples on, one NaN."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.5, 1.5, n).astype(np.float32)
    x[:: 97] *= np.float32(40.0)
    if n >= 3:
        x[n // 2] = np.nan
    return x


def run_prim(rx, x, state, tau, want_float=True):
    d_x, d_st = _d(x), _d(state)
    d_y = torch.zeros(x.size, dtype=torch.float32, device="cuda")
    d_p = torch.zeros(x.size, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    rx.deemph(d_x.data_ptr(), x.size, tau, d_st.data_ptr(), d_y.data_ptr() if want_float else None, d_p.data_ptr())
    rx.synchronize()
    return d_y.cpu().numpy(), d_p.cpu().numpy(), d_st.cpu().numpy()


@pytest.mark.parametrize("n", [1, 62, 63, 64, 65, 1023, 1024, 1025, 2500])
def test_primitive_lengths(fmrx, orc, n):
    """Around the carry's length, around the kernel's chunk (DEEMPH_CHUNK outputs a workgroup) and a
    length that is no multiple of 64, from a non-zero state, both time constants."""
    assert fmrx.DEEMPH_CHUNK == 1024 and fmrx.DEEMPH_TAPS == dr.T
    x = prim_input(n, n)
    state = np.random.default_rng(7).uniform(-1, 1, dr.HIST).astype(np.float32)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        for tau in (50, 75):
            h = fmrx.deemph_design(rx.audio_fs, tau)
            y, nxt = dr.fir(orc, x, state, h)
            gy, gp, gs = run_prim(rx, x, state, tau)
            assert np.array_equal(gp, orc.quant(y)), tau
            ok = ~np.isnan(y)
            assert np.array_equal(np.isnan(gy), ~ok) and np.array_equal(bits(gy[ok]), bits(y[ok])), tau
            assert np.array_equal(bits(gs), bits(nxt)), tau


@pytest.mark.parametrize("mode", [0, 2])
def test_primitive_carry_across_calls(fmrx, orc, mode):
    """Calls of 1, 17, 63 and 200 samples (the carry shorter and longer than a call) against one
    oracle call over the sequence; mode 2: the 44.1 kHz taps."""
    x = prim_input(1 + 17 + 63 + 200, 11)
    with fmrx.Receiver(mode, fmrx.MONO) as rx:
        assert rx.audio_fs == (48000, 44100)[mode // 2]
        h = fmrx.deemph_design(rx.audio_fs, 75)
        want = dr.pcm(orc, x, h)
        state, got, pos = np.zeros(dr.HIST, np.float32), [], 0
        for n in (1, 17, 63, 200):
            _, p, state = run_prim(rx, x[pos:pos + n], state, 75, want_float=False)
            got.append(p)
            pos += n
    assert np.array_equal(np.concatenate(got), want)
    assert np.array_equal(bits(state), bits(x[-dr.HIST:]))


def test_primitive_equals_resample_and_quantize(fmrx):
    x = prim_input(2500, 3)
    state = np.random.default_rng(8).uniform(-1, 1, dr.HIST).astype(np.float32)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        h = fmrx.deemph_design(rx.audio_fs, 50)
        _, gp, gs = run_prim(rx, x, state, 50)
        d_x, d_st, d_h = _d(x), _d(state), _d(h)
        d_y = torch.zeros(x.size, dtype=torch.float32, device="cuda")
        d_p = torch.zeros(x.size, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        assert rx.resample(d_y.data_ptr(), d_st.data_ptr(), d_x.data_ptr(), x.size, d_h.data_ptr(), dr.T, 1, 1) == x.size
        rx.quantize(d_y.data_ptr(), x.size, d_p.data_ptr())
        rx.synchronize()
        assert np.array_equal(gp, d_p.cpu().numpy())
        assert np.array_equal(bits(gs), bits(d_st.cpu().numpy()))


def test_primitive_refusals(fmrx):
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        d = torch.zeros(128, dtype=torch.float32, device="cuda")
        for args in ((d.data_ptr(), 64, 60, d.data_ptr() + 256, None, None),      # tau
                     (None, 64, 50, d.data_ptr() + 256, None, None),               # no input
                     (d.data_ptr(), 64, 50, None, None, None),                     # no state
                     (d.data_ptr(), 64, 50, d.data_ptr() + 256, d.data_ptr(), None)):  # in place
            with pytest.raises(fmrx.FmrxError) as e:
                rx.deemph(*args)
            assert e.value.code == fmrx.FMRX_EINVAL


# ---- mono contexts ---------------------------------------------------------------------------------

@pytest.mark.parametrize("tau", [50, 75])
@pytest.mark.parametrize("rf_taps", [51, 101])
def test_mode0_mono_calls(fmrx, orc, rf_taps, tau):
    """The fused kernel's float outlet through the stage: one call of 6 blocks and calls of 1, 2, 3."""
    iq, bb = synth(21, 0, 6), oracle.MODES[0][0]
    want = want_pcm(orc, fmrx, 0, rf_taps, iq, tau)
    plain = orc.run(0, rf_taps, iq, ["pcm_mono"])["pcm_mono"]
    assert not np.array_equal(want, plain)
    with fmrx.Receiver(0, fmrx.MONO, rf_taps=rf_taps) as rx:
        assert rx.deemphasis() == 0
        rx.set_deemphasis(tau)
        assert rx.deemphasis() == tau
        assert np.array_equal(rx.process(iq), want)
        rx.reset()
        assert np.array_equal(in_calls(rx.process, iq, bb, [1, 2, 3]), want)


@pytest.mark.parametrize("channels", ["MONO", "STEREO"])
@pytest.mark.parametrize("mode,nb", [(1, 2), (2, 1), (3, 1)])
def test_other_modes(fmrx, orc, mode, nb, channels):
    """Mode 1 (two blocks) and the 44.1 kHz modes 2 and 3 (one block): the fused kernel's rational
    audio stage, and for stereo the per-output audio kernel's (right, left) outlet."""
    iq = synth(30 + mode, mode, nb)
    stereo = channels == "STEREO"
    with fmrx.Receiver(mode, getattr(fmrx, channels)) as rx:
        rx.set_deemphasis(50)
        got = rx.process(iq)
    assert np.array_equal(got, want_pcm(orc, fmrx, mode, 51, iq, 50, stereo))


@pytest.mark.parametrize("channels", ["MONO", "STEREO"])
def test_rf_and_audio_blocks_equal_process(fmrx, orc, channels):
    iq, stereo = synth(23, 0, 3), channels == "STEREO"
    want = want_pcm(orc, fmrx, 0, 51, iq, 75, stereo)
    with fmrx.Receiver(0, getattr(fmrx, channels)) as rx:
        rx.set_deemphasis(75)
        assert np.array_equal(rx.process(iq), want)
    with fmrx.Receiver(0, getattr(fmrx, channels)) as rx:
        rx.set_deemphasis(75)
        assert np.array_equal(rx.audio_block(rx.rf_block(iq)), want)


# ---- stereo contexts -------------------------------------------------------------------------------

@pytest.mark.parametrize("calls", [(1, 3), (6,)])
def test_mode0_stereo_two_streams(fmrx, orc, calls):
    """Two streams, left and right each with a carry of their own: 4 blocks in calls of 1 + 3 (the
    few-block audio kernel) and 6 in one (the tiled one)."""
    nb, bb = sum(calls), oracle.MODES[0][0]
    iq = np.stack([synth(41, 0, nb), synth(42, 0, nb)])
    want = np.stack([want_pcm(orc, fmrx, 0, 51, iq[s], 50, True) for s in range(2)])
    with fmrx.Receiver(0, fmrx.STEREO, n_streams=2) as rx:
        rx.set_deemphasis(50)
        got = in_calls(rx.process, iq, bb, calls)
    assert np.array_equal(got, want)


def stereo_chunks(nb, ns, knob, halo_bytes, block_bytes, if_samples, head=8, tail=8):
    """engine.cpp stereo_chunks: the chunks a stereo call takes (1: the serial engine)."""
    def begin(k, K):
        if K <= 1 or k <= 0:
            return 0 if k <= 0 else nb
        return nb if k >= K else nb * (head + 16 * (k - 1)) // (head + 16 * (K - 2) + tail)
    k = 8 if ns >= 16 else 1
    if knob > 0:
        k = knob
    else:
        while k > 1 and nb * if_samples // k < 16384:
            k -= 1
    hb = -(-halo_bytes // block_bytes)
    while k > 1 and any(begin(j + 1, k) - begin(j, k) < hb for j in range(k)):
        k -= 1
    return k


def test_stereo_pipelined_16_streams(fmrx, orc):
    """16 streams x 8 blocks through the pipelined engine.  By engine.cpp's rule that shape takes the
    serial engine on its own (a chunk would hold fewer than 2^14 samples), so the call is made with
    the knob stereo_chunks = 2, which by the same rule gives two chunks."""
    ns, nb = 16, 8
    iq = np.stack([synth(60 + s, 0, nb) for s in range(ns)])
    with fmrx.Receiver(0, fmrx.STEREO, n_streams=ns, knobs={"stereo_chunks": 2}) as rx:
        shape = (rx.history_bytes(), rx.geo.block_bytes, rx.geo.if_samples)
        assert stereo_chunks(nb, ns, 0, *shape) == 1
        assert stereo_chunks(nb, ns, 2, *shape) == 2
        rx.set_deemphasis(75)
        got = rx.process(iq)
        rx.reset()
        again = in_calls(rx.process, iq, oracle.MODES[0][0], [3, 5])  # the carry across pipelined calls
    for s in range(ns):
        assert np.array_equal(got[s], want_pcm(orc, fmrx, 0, 51, iq[s], 75, True)), s
    assert np.array_equal(again, got)


# ---- tuned, wide and rational front ends -----------------------------------------------------------

def test_process_shared_two_offsets(fmrx, orc):
    from test_gpu_tuner import compose
    iq, offsets = synth(51, 0, 3), [-300000, 125000]
    h = taps(fmrx, 0, 50)
    with fmrx.Receiver(0, fmrx.MONO, n_streams=2) as rx:
        rx.tune(offsets)
        rx.set_deemphasis(50)
        got = in_calls(rx.process_shared, iq, oracle.MODES[0][0], [1, 2])
    for s, f in enumerate(offsets):
        assert np.array_equal(got[s], dr.pcm(orc, compose(iq, 0, 51, f, fields=("mono_indep",))["mono_indep"], h)), f


def test_process_wide_decim2(fmrx, orc):
    from test_formats_host import U8
    from test_wide_host import wide_compose
    d, f, nb = 2, 700000, 3
    raw = iqgen.make("synth:52", nb * oracle.MODES[0][0] * d, oracle.MODES[0][3])
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        rx.set_capture_decim(d)
        rx.tune_wide(f)
        rx.set_deemphasis(75)
        got = rx.process_wide(raw)
    want = dr.pcm(orc, wide_compose(raw, U8, 0, 51, d, f, fields=("mono_indep",))["mono_indep"], taps(fmrx, 0, 75))
    assert np.array_equal(got, want)


def test_process_wide_rational_one_granule(fmrx, orc):
    from test_formats_host import U8
    from test_rate_host import rate_compose
    cap_fs, f = 6000000, -450000  # 2/5 of the capture's rate: a granule is one block
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        rx.set_capture_rate(cap_fs)
        blocks, pairs = rx.wide_granule
        assert blocks == 1
        raw = iqgen.make("synth:53", 2 * pairs, oracle.MODES[0][3])
        rx.tune_wide(f)
        rx.set_deemphasis(50)
        got = rx.process_wide(raw)
    want = dr.pcm(orc, rate_compose(raw, U8, 0, 51, cap_fs, f, fields=("mono_indep",))["mono_indep"], taps(fmrx, 0, 50))
    assert np.array_equal(got, want)


def test_with_rds(fmrx, orc):
    """set_rds together with de-emphasis: the PCM is the RDS-off PCM, the info the de-emphasis-off info."""
    iq = synth(54, 0, 24)  # one RDS granule of mode 0
    want = want_pcm(orc, fmrx, 0, 51, iq, 50)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        assert rx.rds_granule == 24
        rx.tune([0])
        rx.set_rds(True)
        plain = rx.process(iq)
        info_off = rx.rds_info().as_dict()
        rx.reset()
        rx.set_deemphasis(50)
        both = rx.process(iq)
        info_on = rx.rds_info().as_dict()
        rx.reset()
        rx.set_rds(False)
        deemph_only = rx.process(iq)
    assert info_off["bits"] > 0 and info_on == info_off
    assert np.array_equal(both, want) and np.array_equal(deemph_only, want)
    assert np.array_equal(plain, orc.run(0, 51, iq, ["pcm_mono"])["pcm_mono"])


# ---- state -----------------------------------------------------------------------------------------

def test_reset_and_switching_off(fmrx, orc):
    iq, bb, na = synth(55, 0, 3), oracle.MODES[0][0], oracle.MODES[0][2]
    mono = orc.run(0, 51, iq, ["mono_indep", "pcm_mono"])
    h = taps(fmrx, 0, 75)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        rx.set_deemphasis(75)
        first = rx.process(iq)
        assert np.array_equal(first, dr.pcm(orc, mono["mono_indep"], h))
        rx.process(iq)
        rx.reset()  # the carry too; the setting stays
        assert rx.deemphasis() == 75 and np.array_equal(rx.process(iq), first)
        # fmrx_set_deemphasis clears the carry and nothing else: the receiver goes on, the filter restarts
        rx.reset()
        a = rx.process(iq[:bb])
        rx.set_deemphasis(75)
        b = rx.process(iq[bb:])
        assert np.array_equal(a, first[:na])
        assert np.array_equal(b, dr.pcm(orc, mono["mono_indep"][na:], h))
        # off again: what a fresh context gives
        rx.reset()
        rx.set_deemphasis(0)
        assert rx.deemphasis() == 0 and np.array_equal(rx.process(iq), mono["pcm_mono"])
    with fmrx.Receiver(0, fmrx.MONO) as fresh:
        assert np.array_equal(fresh.process(iq), mono["pcm_mono"])


def test_checkpoint_and_seek_are_refused_while_on(fmrx):
    iq = synth(56, 0, 2)
    with fmrx.Receiver(0, fmrx.MONO) as rx:
        blob = rx.get_state()
        rx.set_deemphasis(50)
        for call in (rx.get_state, lambda: rx.set_state(blob), lambda: rx.seek(iq)):
            with pytest.raises(fmrx.FmrxError) as e:
                call()
            assert e.value.code == fmrx.FMRX_ESTATE
        with pytest.raises(fmrx.FmrxError) as e:
            rx.set_deemphasis(60)
        assert e.value.code == fmrx.FMRX_EINVAL and rx.deemphasis() == 50
        rx.set_deemphasis(0)
        assert rx.get_state() == blob
        rx.set_state(blob)
        rx.seek(iq)


def test_off_is_the_golden_fixture_and_d_mono_stays(fmrx, orc):
    """Off (the default): the golden PCM and mono floats.  On: d_mono is still the mono product, the
    PCM its de-emphasised form."""
    z = load_case("m0_rf101_synth")
    iq, nb = case_input(z), z["n_blocks"]
    with fmrx.Receiver(0, fmrx.MONO, rf_taps=101) as rx:
        na = nb * rx.geo.audio_frames
        d_iq = _d(iq)
        for tau in (0, 75):
            rx.reset()
            rx.set_deemphasis(tau)
            d_pcm = torch.zeros(na, dtype=torch.int16, device="cuda")
            d_mono = torch.zeros(na, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            rx.process_device(d_iq.data_ptr(), nb, d_pcm.data_ptr(), d_mono.data_ptr())
            rx.synchronize()
            assert np.array_equal(bits(d_mono.cpu().numpy()), bits(z["mono_indep"])), tau
            want = z["pcm_mono"] if tau == 0 else dr.pcm(orc, z["mono_indep"], taps(fmrx, 0, tau))
            assert np.array_equal(d_pcm.cpu().numpy(), want), tau


# ---- CLI and decode_stations -----------------------------------------------------------------------

def test_cli(fmrx):
    exe = os.path.join(os.path.dirname(fmrx.LIB_PATH), "bin", "fmrx")
    iq = synth(57, 0, 20)  # the CLI's batches are 16 blocks: two calls
    r = subprocess.run([exe, "0", "1", "--deemph", "75"], input=iq.tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    with fmrx.Receiver(0, fmrx.STEREO) as rx:  # the CLI writes project's 2-channel stream
        rx.set_deemphasis(75)
        want = rx.process(iq)
    assert r.stdout == want.tobytes()
    bad = subprocess.run([exe, "0", "1", "--deemph", "60"], input=b"", capture_output=True, timeout=120)
    assert bad.returncode == 1 and b"--deemph 60" in bad.stderr and bad.stdout == b""


def test_decode_stations(fmrx, orc):
    from test_gpu_tuner import compose
    from test_scan_host import capture
    iq = capture("two", 20)[0]
    stations, pcm = fmrx.decode_stations(iq, deemphasis_us=50)
    assert [s.offset_hz for s in stations] == [-300000, 300000]
    h = taps(fmrx, 0, 50)
    for row, s in zip(pcm, stations):
        want = dr.pcm(orc, compose(iq, 0, 51, s.offset_hz, fields=("mono_indep",))["mono_indep"], h)
        assert np.array_equal(row, want), s
    assert not np.array_equal(pcm, fmrx.decode_stations(iq)[1])
