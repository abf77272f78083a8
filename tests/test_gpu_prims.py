"""Every filter.h primitive of the C ABI over the shapes and values a caller may pass.

fmrx_resample, fmrx_fm_demod, fmrx_mixer, fmrx_lr_extraction, fmrx_normalize_iq, fmrx_quantize,
fmrx_fm_demod_arctan and fmrx_estimate_psd / fmrx_psd_device are the entry points that take arbitrary
shapes; everything else runs at a mode's fixed geometry.  The case lists are those of tests/prims_ref.py, at
which tests/test_prims_host.py holds the oracle to the reference build bit for bit, so the expected values
here are the reference's.

Rules of every case:
  * the expected value is the oracle called the same way (the same split into calls, the state handed on),
    compared with np.array_equal on uint32 views; where it is a NaN the result must be a NaN (payload and
    sign not compared).  Only the arctan demodulator and the PSD estimate have a tolerance.
  * every output and state buffer has 64 elements of a fixed byte pattern on both sides of the region the call
    may write, and they must be unchanged afterwards: a tail thread that writes past n shows here only.
  * each primitive has cases with every device pointer one element off its allocation (4-byte aligned only;
    the I/Q bytes of normalize_iq one byte off).
  * n = 0 returns FMRX_OK, writes nothing and leaves any state as it was.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import prims_ref as P
from prims_ref import assert_same
from test_oracle import PSD_TOL_MODEL_DB

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# fmDemodArctan against the float64 model: tests/test_gpu_parity.py's bounds (the final float rounding,
# <= 2^-24 relative, and the model's cancellation error on its growing unwrapped phase)
ARCTAN_RTOL = 2.0 ** -23
ARCTAN_ATOL = 1e-9

GUARD = 64   # elements on both sides of every region a call may write
FILL = 0xA5  # their bytes (as float -2.87e-16, no value any case produces by chance in a whole guard)
F32, F64, I16, U8 = np.float32, np.float64, np.int16, np.uint8


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


@pytest.fixture(scope="module")
def rx(fmrx):
    with fmrx.Receiver(0, fmrx.MONO) as r:
        yield r


class Buf:
    """n elements of dtype on the device between two guards; `off` moves the region (and its pointer) that
    many elements off the allocation's alignment.  A region without `init` holds the guard bytes."""

    def __init__(self, n, dtype, init=None, off=0):
        self.dt, self.n = np.dtype(dtype), int(n)
        isz = self.dt.itemsize
        self.lead, self.size = (GUARD + off) * isz, self.n * isz
        host = np.full(self.lead + self.size + GUARD * isz, FILL, np.uint8)
        if init is not None:
            init = np.ascontiguousarray(init, self.dt)
            assert init.size == self.n
            host[self.lead:self.lead + self.size] = init.reshape(-1).view(np.uint8)
        self.t = torch.from_numpy(host).cuda()
        self.ptr = self.t.data_ptr() + self.lead

    def read(self) -> np.ndarray:
        """The region; the guards must be as they were."""
        h = self.t.cpu().numpy()
        assert (h[:self.lead] == FILL).all(), "wrote in front of the buffer"
        assert (h[self.lead + self.size:] == FILL).all(), "wrote past the buffer"
        return h[self.lead:self.lead + self.size].copy().view(self.dt)

    def untouched(self) -> bool:
        """A region made without `init`: nothing at all was written."""
        return bool((self.t.cpu().numpy() == FILL).all())


def go(rx, fn, *args):
    """One primitive call: the uploads (torch's stream) are done before it, the call before the reads."""
    torch.cuda.synchronize()
    r = fn(*args)
    rx.synchronize()
    return r


def refused(fmrx, rx, fn, *args):
    with pytest.raises(fmrx.FmrxError) as e:
        go(rx, fn, *args)
    assert e.value.code == fmrx.FMRX_EINVAL, e.value


# ---- fmrx_resample -------------------------------------------------------------------------------------
def resample_call(rx, x, d_state, coeff, up, down, off=0):
    """One fmrx_resample call on guarded buffers, the state in d_state (in/out): the outputs."""
    n_out = x.size * up // down
    d_x, d_c, d_out = Buf(x.size, F32, x, off), Buf(coeff.size, F32, coeff, off), Buf(n_out, F32, None, off)
    got_n = go(rx, rx.resample, d_out.ptr, d_state.ptr, d_x.ptr, x.size, d_c.ptr, coeff.size, up, down)
    assert got_n == n_out
    assert_same(d_x.read(), x, "input changed")
    assert_same(d_c.read(), coeff, "coefficients changed")
    if n_out == 0:
        assert d_out.untouched()
    return d_out.read()


def check_resample(rx, orc, taps, up, down, n_in, off=0, inputs=None):
    x, state, coeff = inputs or P.resample_input(taps, up, down, n_in)
    want, want_state = orc.resample(x, state, coeff, up, down)
    d_state = Buf(taps - 1, F32, state, off)
    got = resample_call(rx, x, d_state, coeff, up, down, off)
    what = (taps, up, down, n_in, off)
    assert_same(got, want, what)
    got_state = d_state.read()
    assert_same(got_state, want_state, what)
    assert_same(got_state, np.ascontiguousarray(x[x.size - (taps - 1):]), what)  # the last taps - 1 inputs
    return got


@pytest.mark.parametrize("up,down", P.RESAMPLE_RATIOS)
@pytest.mark.parametrize("taps", P.RESAMPLE_TAPS)
def test_resample_matrix(rx, orc, taps, up, down):
    for n_in in P.resample_lengths(taps):
        got = check_resample(rx, orc, taps, up, down, n_in, off=int(n_in == 257))
        if taps < up and got.size:  # phases without a tap: exactly +0.0
            k0 = (np.arange(got.size, dtype=np.int64) * down) % up
            assert not P.bits(got[k0 >= taps]).any()


@pytest.mark.parametrize("taps,up,down", P.RESAMPLE_LONG)
def test_resample_long_tables(rx, orc, taps, up, down):
    """The project's own long prototypes (RDS 1919 taps at 19/120, mode 2's 7497 at 147/800), with the whole
    window in the state (n_in = taps - 1) and mostly in the input (2 taps)."""
    for n_in, off in ((taps - 1, 0), (2 * taps, 1)):
        check_resample(rx, orc, taps, up, down, n_in, off)


@pytest.mark.parametrize("ratio", sorted(P.RESAMPLE_CHAINS))
@pytest.mark.parametrize("kind", ["aligned", "ragged"])
def test_resample_chains(rx, orc, ratio, kind):
    """Three calls of unequal length, the state left on the device between them.  Cuts with cut up % down
    == 0 equal the single call as well; cuts without equal the reference called the same way only."""
    up, down = ratio
    cuts = P.RESAMPLE_CHAINS[ratio][kind]
    taps = P.RESAMPLE_CHAIN_TAPS
    x, state, coeff = P.resample_input(taps, up, down, sum(cuts))
    d_state, want_state = Buf(taps - 1, F32, state), state
    outs, at = [], 0
    for c in cuts:
        want, want_state = orc.resample(x[at:at + c], want_state, coeff, up, down)
        got = resample_call(rx, x[at:at + c], d_state, coeff, up, down)
        assert_same(got, want, (ratio, kind, at))
        assert_same(d_state.read(), want_state, (ratio, kind, at))
        outs.append(got)
        at += c
    if kind == "aligned":
        whole, _ = orc.resample(x, state, coeff, up, down)
        assert_same(np.concatenate(outs), whole)


def test_resample_special_values(rx, orc):
    """Denormals of both signs, +-0.0, +-FLT_MAX, +-Inf and one NaN in the input row, 51 taps at 1/10:
    numbers bit for bit (no denormal flushed, no product contracted), NaN by place."""
    got = check_resample(rx, orc, 51, 1, 10, 1000, inputs=P.resample_special_input())
    assert np.isnan(got).any() and np.isinf(got).any()


def test_resample_no_input_no_history(rx, orc):
    """n_in = 0 is accepted where there is no history to refill (taps = 1): FMRX_OK, nothing written."""
    d_out, d_state = Buf(0, F32), Buf(0, F32)
    d_x, d_c = Buf(0, F32), Buf(1, F32, [0.5])
    assert go(rx, rx.resample, d_out.ptr, d_state.ptr, d_x.ptr, 0, d_c.ptr, 1, 3, 7) == 0
    assert d_out.untouched() and d_state.untouched() and d_x.untouched()


# ---- fmrx_fm_demod ---------------------------------------------------------------------------------------
def demod_call(rx, i, q, d_prev, off=0):
    d_i, d_q, d_out = Buf(i.size, F32, i, off), Buf(q.size, F32, q, off), Buf(i.size, F32, None, off)
    go(rx, rx.fm_demod, d_out.ptr, d_prev.ptr, d_i.ptr, d_q.ptr, i.size)
    assert_same(d_i.read(), i, "I changed")
    assert_same(d_q.read(), q, "Q changed")
    if i.size == 0:
        assert d_out.untouched()
    return d_out.read()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", P.COMMON_N)
def test_fm_demod_shapes(rx, orc, n, off):
    i, q, prev = P.demod_input(n)
    want, want_prev = orc.fmdemod(i, q, prev)
    d_prev = Buf(2, F32, prev, off)
    assert_same(demod_call(rx, i, q, d_prev, off), want)
    assert_same(d_prev.read(), want_prev)
    if n == 0:
        assert_same(d_prev.read(), prev)


def test_fm_demod_chain(rx, orc):
    i, q, prev = P.demod_input(sum(P.DEMOD_CHAIN), 1)
    d_prev, want_prev, at, outs = Buf(2, F32, prev), prev, 0, []
    for n in P.DEMOD_CHAIN:
        want, want_prev = orc.fmdemod(i[at:at + n], q[at:at + n], want_prev)
        got = demod_call(rx, i[at:at + n], q[at:at + n], d_prev)
        assert_same(got, want, at)
        assert_same(d_prev.read(), want_prev, at)  # the carry, after each call
        outs.append(got)
        at += n
    assert_same(np.concatenate(outs), orc.fmdemod(i, q, prev)[0])


def test_fm_demod_special_grid(rx, orc):
    """The 20 x 20 grid of special (I, Q) as one row.  The denominator (double squares, rounded to float) is
    0 for 61 pairs, a float denormal for 39 and Inf for 165; the reference gives 245 numbers of 400, counted
    before the comparison so that the case cannot drift into mostly-NaN."""
    i, q, prev = P.demod_grid_input()
    den = P.demod_grid_denominator()
    assert int((den == 0).sum()) == P.DEMOD_GRID_DEN["zero"]
    assert int(((den != 0) & (np.abs(den) < P.F32_MIN)).sum()) == P.DEMOD_GRID_DEN["denormal"]
    assert int(np.isinf(den).sum()) == P.DEMOD_GRID_DEN["inf"]
    want, want_prev = orc.fmdemod(i, q, prev)
    assert int((~np.isnan(want)).sum()) == P.DEMOD_GRID_NUMBERS
    d_prev = Buf(2, F32, prev)
    assert_same(demod_call(rx, i, q, d_prev), want)
    assert_same(d_prev.read(), want_prev)


def test_fm_demod_bit_patterns(rx, orc):
    i, q, prev = P.bit_patterns(21), P.bit_patterns(22), np.array([0.25, -0.5], F32)
    d_prev, want_prev = Buf(2, F32, prev), prev
    for at in range(0, P.N_PATTERNS, P.PATTERN_CHUNK):
        s = slice(at, at + P.PATTERN_CHUNK)
        want, want_prev = orc.fmdemod(i[s], q[s], want_prev)
        assert_same(demod_call(rx, i[s], q[s], d_prev), want, at)
        assert_same(d_prev.read(), want_prev, at)


# ---- fmrx_mixer, fmrx_lr_extraction, fmrx_quantize -------------------------------------------------------------
def mixer_call(rx, a, b, off=0):
    d_a, d_b, d_out = Buf(a.size, F32, a, off), Buf(b.size, F32, b, off), Buf(a.size, F32, None, off)
    go(rx, rx.mixer, d_out.ptr, d_a.ptr, d_b.ptr, a.size)
    if a.size == 0:
        assert d_out.untouched()
    return d_out.read()


def lr_call(rx, m, s, off=0):
    d_m, d_s = Buf(m.size, F32, m, off), Buf(s.size, F32, s, off)
    d_l, d_r = Buf(m.size, F32, None, off), Buf(m.size, F32, None, off)
    go(rx, rx.lr_extraction, d_l.ptr, d_r.ptr, d_m.ptr, d_s.ptr, m.size)
    if m.size == 0:
        assert d_l.untouched() and d_r.untouched()
    return d_l.read(), d_r.read()


def quantize_call(rx, x, off=0):
    d_x, d_out = Buf(x.size, F32, x, off), Buf(x.size, I16, None, off)
    go(rx, rx.quantize, d_x.ptr, x.size, d_out.ptr)
    if x.size == 0:
        assert d_out.untouched()
    return d_out.read()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", P.COMMON_N)
def test_elementwise_shapes(rx, orc, n, off):
    a, b = P.ordinary(n, 1), P.ordinary(n, 2)
    assert_same(mixer_call(rx, a, b, off), orc.mixer(a, b))
    for got, want in zip(lr_call(rx, a, b, off), orc.lr(a, b)):
        assert_same(got, want)
    assert_same(quantize_call(rx, a, off), orc.quant(a))


def test_mixer_and_lr_bit_patterns(rx, orc):
    a, b = P.elementwise_pair(11)
    for at in range(0, a.size, P.PATTERN_CHUNK):
        s = slice(at, at + P.PATTERN_CHUNK)
        assert_same(mixer_call(rx, a[s], b[s]), orc.mixer(a[s], b[s]), ("mixer", at))
        for got, want, what in zip(lr_call(rx, a[s], b[s]), orc.lr(a[s], b[s]), ("left", "right")):
            assert_same(got, want, (what, at))


def test_quantize_bit_patterns_and_wrap_edges(rx, orc):
    """Random bit patterns, the edge list, and k/16384 one ulp either side of the 16-bit wrap (k around
    +-32768) and of the int32 range (+-2^31/16384), where a saturating conversion differs from x86's."""
    x = P.quantize_input()
    for at in range(0, x.size, P.PATTERN_CHUNK):
        s = slice(at, at + P.PATTERN_CHUNK)
        assert_same(quantize_call(rx, x[s]), orc.quant(x[s]), at)


def test_mixer_and_lr_in_place(rx, orc):
    """d_out = d_a (and d_b) for the mixer, (d_left, d_right) = (d_mono, d_stereo) for LRExtraction: each
    element depends on itself only, so these run in place (fmrx_quantize does not: its 16-bit output k lies in
    float k / 2 of the input, and is refused)."""
    a, b = P.ordinary(1000, 3), P.ordinary(1000, 4)
    for alias in (0, 1):
        bufs = [Buf(a.size, F32, a), Buf(b.size, F32, b)]
        go(rx, rx.mixer, bufs[alias].ptr, bufs[0].ptr, bufs[1].ptr, a.size)
        assert_same(bufs[alias].read(), orc.mixer(a, b))
        assert_same(bufs[1 - alias].read(), (b, a)[alias])
    want_l, want_r = orc.lr(a, b)
    d_m, d_s = Buf(a.size, F32, a), Buf(b.size, F32, b)
    go(rx, rx.lr_extraction, d_m.ptr, d_s.ptr, d_m.ptr, d_s.ptr, a.size)
    assert_same(d_m.read(), want_l)
    assert_same(d_s.read(), want_r)
    d_m, d_s = Buf(a.size, F32, a, 1), Buf(b.size, F32, b, 1)
    go(rx, rx.lr_extraction, d_s.ptr, d_m.ptr, d_m.ptr, d_s.ptr, a.size)  # crossed
    assert_same(d_s.read(), want_l)
    assert_same(d_m.read(), want_r)


# ---- fmrx_normalize_iq ------------------------------------------------------------------------------------
def normalize_call(rx, by, off=0):
    n = by.size // 2
    d_b, d_i, d_q = Buf(by.size, U8, by, off), Buf(n, F32, None, off), Buf(n, F32, None, off)
    go(rx, rx.normalize_iq, d_b.ptr, n, d_i.ptr, d_q.ptr)
    if n == 0:
        assert d_i.untouched() and d_q.untouched()
    return d_i.read(), d_q.read()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", P.COMMON_N + ("every_byte",))
def test_normalize_iq(rx, orc, n, off):
    """The common shapes, and every byte value in both positions; off = 1 puts the bytes on an odd address."""
    by = P.all_byte_pairs() if n == "every_byte" else P.byte_pairs(n)
    want = orc.normalize(by)
    got_i, got_q = normalize_call(rx, by, off)
    assert_same(got_i, want[0::2])
    assert_same(got_q, want[1::2])


# ---- fmrx_fm_demod_arctan -----------------------------------------------------------------------------------
def arctan_call(rx, i, q, d_prev, off=0):
    d_i, d_q, d_out = Buf(i.size, F32, i, off), Buf(q.size, F32, q, off), Buf(i.size, F32, None, off)
    go(rx, rx.fm_demod_arctan, d_out.ptr, d_prev.ptr, d_i.ptr, d_q.ptr, i.size)
    if i.size == 0:
        assert d_out.untouched()
    return d_out.read().astype(F64)


def same_phase(got, want) -> bool:
    """The carried phase is the principal value, the model's the unwrapped one: equal modulo 2 pi."""
    return bool(np.all(np.abs(P.wrap_2pi(np.asarray(got, F64) - want)) < ARCTAN_ATOL))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", P.COMMON_N)
def test_arctan_shapes(rx, orc, n, off):
    i, q, ph0 = P.arctan_input(n)
    want, want_ph = orc.fm_demod_arctan(i, q, ph0)
    d_prev = Buf(1, F64, [ph0], off)
    got = arctan_call(rx, i, q, d_prev, off)
    np.testing.assert_allclose(got, want, rtol=ARCTAN_RTOL, atol=ARCTAN_ATOL)
    assert same_phase(d_prev.read(), want_ph)
    if n == 0:
        assert d_prev.read()[0] == ph0


def test_arctan_chain(rx, orc):
    i, q, ph0 = P.arctan_input(sum(P.DEMOD_CHAIN), 1)
    d_prev, want_ph, at = Buf(1, F64, [ph0]), ph0, 0
    for n in P.DEMOD_CHAIN:
        want, want_ph = orc.fm_demod_arctan(i[at:at + n], q[at:at + n], want_ph)
        got = arctan_call(rx, i[at:at + n], q[at:at + n], d_prev)
        np.testing.assert_allclose(got, want, rtol=ARCTAN_RTOL, atol=ARCTAN_ATOL)
        assert same_phase(d_prev.read(), want_ph)
        at += n


def test_arctan_axis_cases(rx, orc):
    """(0, 0), (-1, +0.0) and (-1, -0.0) after (1, 0), and a step of exactly 2 pi.  +pi and -pi are the same
    step, so these are compared modulo 2 pi, within the bounds of the other cases: ARCTAN_ATOL, and
    ARCTAN_RTOL of the value for the float that stores it (float(pi) is 8.7e-8 off pi)."""
    i, q, ph0 = P.arctan_axis_input()
    want, want_ph = orc.fm_demod_arctan(i, q, ph0)
    assert np.isclose(np.abs(want), np.pi).sum() >= 3  # the steps that sit on the cut
    d_prev = Buf(1, F64, [ph0])
    got = arctan_call(rx, i, q, d_prev)
    assert np.isfinite(got).all() and np.abs(got).max() <= np.float32(np.pi)
    err = np.abs(P.wrap_2pi(got - want))
    assert (err <= ARCTAN_ATOL + ARCTAN_RTOL * np.abs(got)).all(), (got, want)
    assert same_phase(d_prev.read(), want_ph)


# ---- fmrx_estimate_psd / fmrx_psd_device ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _psd_want(bins, n):
    import oracle

    return oracle.Oracle().estimate_psd(P.psd_input(bins, n), bins, P.PSD_FS)


@pytest.mark.parametrize("bins", P.PSD_BINS)
def test_psd_every_size(rx, bins):
    """Every power of two from 2 to 8192 (the largest take more than 64 KiB of dynamic LDS), with one
    segment, three and a ragged tail that is dropped, and nine, through the host call and the device call;
    against the oracle's float64 transform within PSD_TOL_MODEL_DB on every bin, freq exactly."""
    for k, (name, n) in enumerate(P.psd_layouts(bins)):
        x = P.psd_input(bins, n)
        want_freq, want = _psd_want(bins, n)
        assert np.isfinite(want).all()
        freq, psd = rx.estimate_psd(x, bins, P.PSD_FS)
        assert_same(freq, want_freq, (bins, name))
        assert np.abs(psd - want).max() <= PSD_TOL_MODEL_DB, (bins, name)
        off = int(k == 1)
        d_x, d_psd = Buf(n, F32, x, off), Buf(bins // 2, F32, None, off)
        go(rx, rx.psd_device, d_x.ptr, n, bins, P.PSD_FS, d_psd.ptr)
        got = d_psd.read()
        assert np.abs(got - want).max() <= PSD_TOL_MODEL_DB, (bins, name, "device")
        assert_same(got, psd, (bins, name, "host and device calls differ"))


# ---- n = 0 of fmrx_pll ------------------------------------------------------------------------------------------
def test_pll_no_samples(rx):
    st0 = np.array([1e-4, 0.25, 0.6, 0.8, 1.0, 131072.0], F32)
    d_io, d_st = Buf(0, F32), Buf(6, F32, st0)
    go(rx, rx.pll, d_io.ptr, 0, 19000.0, 240000.0, 2.0, 0.0, 0.01, d_st.ptr)
    assert d_io.untouched()
    assert_same(d_st.read(), st0)


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(fmrx, rx, orc):
    """FMRX_EINVAL for an input shorter than the history, taps / up / down < 1, a negative n, a null pointer,
    a PSD size that is no power of two in [2, 8192] or longer than the input, and for the calls that would
    race in place (fmrx_resample d_out = d_in; fmrx_fm_demod and fmrx_fm_demod_arctan d_out = d_i or d_q;
    fmrx_quantize d_out = d_x).  Nothing is launched: every buffer is as it was, and the context still works."""
    x = P.ordinary(1000, 9)
    xb = x.view(U8)
    a, b, o, o2 = Buf(1000, F32, x), Buf(1000, F32, x), Buf(1000, F32), Buf(1000, F32)
    c, st = Buf(51, F32, x[:51]), Buf(50, F32, x[:50])
    pv, ph, st6 = Buf(2, F32, x[:2]), Buf(1, F64, [0.5]), Buf(6, F32, x[:6])
    by, o16 = Buf(2000, U8, xb[:2000]), Buf(1000, I16)
    no = refused

    # fmrx_resample(out, state, in, n_in, coeff, taps, up, down)
    no(fmrx, rx, rx.resample, o.ptr, st.ptr, a.ptr, 49, c.ptr, 51, 1, 10)  # n_in < taps - 1
    no(fmrx, rx, rx.resample, o.ptr, st.ptr, a.ptr, -1, c.ptr, 1, 1, 1)
    for taps, up, down in ((0, 1, 10), (-1, 1, 10), (51, 0, 10), (51, 1, 0), (51, -3, 7), (51, 3, -7)):
        no(fmrx, rx, rx.resample, o.ptr, st.ptr, a.ptr, 1000, c.ptr, taps, up, down)
    for k in range(4):
        p = [o.ptr, st.ptr, a.ptr, c.ptr]
        p[k] = None
        no(fmrx, rx, rx.resample, p[0], p[1], p[2], 1000, p[3], 51, 1, 10)
    no(fmrx, rx, rx.resample, a.ptr, st.ptr, a.ptr, 1000, c.ptr, 51, 1, 10)  # in place

    # fmrx_fm_demod / fmrx_fm_demod_arctan(out, prev, i, q, n)
    for fn, prev in ((rx.fm_demod, pv), (rx.fm_demod_arctan, ph)):
        no(fmrx, rx, fn, o.ptr, prev.ptr, a.ptr, b.ptr, -1)
        for k in range(4):
            p = [o.ptr, prev.ptr, a.ptr, b.ptr]
            p[k] = None
            no(fmrx, rx, fn, p[0], p[1], p[2], p[3], 1000)
        no(fmrx, rx, fn, a.ptr, prev.ptr, a.ptr, b.ptr, 1000)  # d_out = d_i
        no(fmrx, rx, fn, b.ptr, prev.ptr, a.ptr, b.ptr, 1000)  # d_out = d_q

    # fmrx_mixer(out, a, b, n), fmrx_lr_extraction(l, r, m, s, n), fmrx_pll(io, n, ..., st)
    no(fmrx, rx, rx.mixer, o.ptr, a.ptr, b.ptr, -1)
    for k in range(3):
        p = [o.ptr, a.ptr, b.ptr]
        p[k] = None
        no(fmrx, rx, rx.mixer, p[0], p[1], p[2], 1000)
    no(fmrx, rx, rx.lr_extraction, o.ptr, o2.ptr, a.ptr, b.ptr, -1)
    for k in range(4):
        p = [o.ptr, o2.ptr, a.ptr, b.ptr]
        p[k] = None
        no(fmrx, rx, rx.lr_extraction, p[0], p[1], p[2], p[3], 1000)
    no(fmrx, rx, rx.pll, o.ptr, -1, 19000.0, 240000.0, 2.0, 0.0, 0.01, st6.ptr)
    no(fmrx, rx, rx.pll, None, 1000, 19000.0, 240000.0, 2.0, 0.0, 0.01, st6.ptr)
    no(fmrx, rx, rx.pll, o.ptr, 1000, 19000.0, 240000.0, 2.0, 0.0, 0.01, None)

    # fmrx_normalize_iq(iq, n_pairs, i, q), fmrx_quantize(x, n, out)
    for k in range(3):
        p = [by.ptr, o.ptr, o2.ptr]
        p[k] = None
        no(fmrx, rx, rx.normalize_iq, p[0], 1000, p[1], p[2])
    no(fmrx, rx, rx.quantize, None, 1000, o16.ptr)
    no(fmrx, rx, rx.quantize, a.ptr, 1000, None)
    no(fmrx, rx, rx.quantize, a.ptr, 1000, a.ptr)  # in place

    # PSD: freq_bins no power of two in [2, 8192], fewer samples than one segment, null pointers
    for bins in (-4, 0, 1, 3, 500, 1000, 16384):
        no(fmrx, rx, rx.psd_device, a.ptr, 1000, bins, 48000.0, o.ptr)
        if bins >= 0:  # the binding sizes its outputs by bins
            no(fmrx, rx, rx.estimate_psd, x, bins, 48000.0)
    no(fmrx, rx, rx.psd_device, a.ptr, 511, 512, 48000.0, o.ptr)
    no(fmrx, rx, rx.psd_device, None, 1000, 512, 48000.0, o.ptr)
    no(fmrx, rx, rx.psd_device, a.ptr, 1000, 512, 48000.0, None)
    no(fmrx, rx, rx.estimate_psd, x[:511], 512, 48000.0)

    for buf in (o, o2, o16):
        assert buf.untouched()
    for buf, was in ((a, x), (b, x), (c, x[:51]), (st, x[:50]), (pv, x[:2]), (st6, x[:6]), (by, xb[:2000])):
        assert_same(buf.read(), np.ascontiguousarray(was))
    assert ph.read()[0] == 0.5
    assert_same(mixer_call(rx, x, x[::-1].copy()), orc.mixer(x, x[::-1].copy()))  # the context still works
