"""Case lists and inputs of the filter.h primitives' tests.

tests/test_prims_host.py (the pinned oracle against the reference build, on the CPU) and
tests/test_gpu_prims.py (the HIP primitives against the oracle) import every list from here, so both
sides run the same shapes and the same values.  Inputs are deterministic: a case's seed is made of its
own parameters.  numpy only; nothing here needs a GPU.
"""
from __future__ import annotations

import numpy as np

# ---- shapes ------------------------------------------------------------------------------------------
# n of every element-wise primitive: nothing, one thread, and both sides of a 256-thread workgroup edge
COMMON_N = (0, 1, 255, 256, 257, 1000)

RESAMPLE_TAPS = (1, 2, 3, 19, 51, 101, 257)
# taps < up (whole phases without a tap: outputs exactly 0.0), up > down, n_out = 0 when n_in up < down
RESAMPLE_RATIOS = ((1, 1), (1, 2), (1, 10), (3, 7), (7, 3), (19, 120), (24, 5), (147, 800), (300, 7))
# the project's own long prototypes: (taps, up, down), at n_in = taps - 1 and 2 taps
RESAMPLE_LONG = ((1919, 19, 120), (7497, 147, 800))
# three calls of unequal length, state carried: cuts where cut up % down == 0 (the chain equals the single
# call too) and cuts where it is not (the chain equals the reference called the same way, nothing else)
RESAMPLE_CHAINS = {
    (1, 10): {"aligned": (250, 400, 350), "ragged": (251, 398, 351)},
    (3, 7): {"aligned": (252, 399, 349), "ragged": (250, 401, 349)},
    (19, 120): {"aligned": (240, 480, 280), "ragged": (241, 479, 280)},
}
RESAMPLE_CHAIN_TAPS = 51
# three chained calls of the two demodulators
DEMOD_CHAIN = (257, 1, 742)


def resample_lengths(taps: int) -> list[int]:
    """n_in of the taps x ratio matrix: the shortest input the call accepts, the table's length and one
    more, a workgroup edge, 1000; those shorter than the history are refused and tested as refusals."""
    want = {max(taps - 1, 1), taps, taps + 1, 255, 256, 257, 1000}
    return sorted(n for n in want if n >= taps - 1)


def resample_cases():
    """(taps, up, down, n_in) of the whole matrix: 45 (taps, n_in) pairs x 9 ratios = 405."""
    return [(t, u, d, n) for t in RESAMPLE_TAPS for (u, d) in RESAMPLE_RATIOS for n in resample_lengths(t)]


def _rng(*key) -> np.random.Generator:
    return np.random.default_rng([int(k) & 0x7FFFFFFF for k in key])


def resample_input(taps: int, up: int, down: int, n_in: int):
    """(x, state, coeff): coefficients random and asymmetric (a symmetric low-pass hides a reversed tap
    order or a state read from the wrong end), the incoming state random and nonzero."""
    r = _rng(1, taps, up, down, n_in)
    x = r.standard_normal(n_in).astype(np.float32)
    state = (r.standard_normal(taps - 1) + 0.25).astype(np.float32)
    coeff = (r.standard_normal(taps) * np.linspace(0.5, 1.5, taps)).astype(np.float32)
    return x, state, coeff


F32_MAX = np.float32(3.4028234663852886e38)
F32_MIN = np.float32(1.1754943508222875e-38)  # FLT_MIN, the smallest normal
F32_DEN = np.float32(1e-45)                   # the smallest denormal


def resample_special_input(n_in: int = 1000, taps: int = 51):
    """An input row with denormals of both signs, +-0.0, +-FLT_MAX, +-Inf and one NaN among ordinary
    samples, far enough apart at 1/10 that most outputs stay numbers."""
    x, state, coeff = resample_input(taps, 1, 10, n_in)
    x = x.copy()
    specials = [F32_DEN, -F32_DEN, np.float32(1e-39), np.float32(-1e-39), np.float32(0.0), np.float32(-0.0),
                F32_MAX, -F32_MAX, np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan)]
    for k, v in enumerate(specials):
        x[37 + 83 * k] = v
    return x, state, coeff


# ---- FMDemod -------------------------------------------------------------------------------------------
def demod_input(n: int, seed: int = 0):
    r = _rng(2, n, seed)
    ph = np.cumsum(r.uniform(-1.0, 1.0, n))
    amp = 0.5 + 0.25 * r.standard_normal(n)
    i = (amp * np.cos(ph)).astype(np.float32)
    q = (amp * np.sin(ph)).astype(np.float32)
    prev = np.array([0.25, -0.5], np.float32)
    return i, q, prev


DEMOD_GRID = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, 1e-30, 1e-20, F32_MIN, 1.0, -1.0, 0.5, 3.4e38, -3.4e38,
                       1e19, 1e30, np.inf, -np.inf, np.nan, 2.0 ** -75, 2.0 ** -64], np.float32)
DEMOD_GRID_NUMBERS = 245  # results of the reference on the row below that are numbers, of 400
DEMOD_GRID_DEN = {"zero": 61, "denormal": 39, "inf": 165}  # its denominator's classes


def demod_grid_input():
    """The 20 x 20 grid of (I, Q) as one row: sample 20 a + b is (grid[a], grid[b])."""
    i = np.repeat(DEMOD_GRID, DEMOD_GRID.size)
    q = np.tile(DEMOD_GRID, DEMOD_GRID.size)
    return i.copy(), q.copy(), np.array([0.25, -0.5], np.float32)


def demod_grid_denominator():
    """The reference's denominator on the grid (filter.cpp:118-121): double squares, rounded to float."""
    i, q, _ = demod_grid_input()
    with np.errstate(all="ignore"):
        return (i.astype(np.float64) ** 2 + q.astype(np.float64) ** 2).astype(np.float32)


# ---- element-wise primitives ---------------------------------------------------------------------------
EDGES = np.array([0, 1, -1, 1.99993896484375, 2, -2, 2.5, 1e6, -1e6, 1.4e5, np.inf, -np.inf, np.nan,
                  131071.99, -131072, 3.05e-5] * 4, np.float32)
N_PATTERNS = 65536
PATTERN_CHUNK = 32768  # floats a launch of the bit-pattern cases


def bit_patterns(seed: int) -> np.ndarray:
    """65,536 random 32-bit patterns viewed as float: NaNs of every payload, denormals, both infinities."""
    return _rng(3, seed).integers(0, 2 ** 32, N_PATTERNS, dtype=np.uint64).astype(np.uint32).view(np.float32)


def elementwise_pair(seed: int):
    """(a, b) of mixer and LRExtraction: the bit patterns, then the edge list against itself reversed."""
    a = np.concatenate([bit_patterns(seed), EDGES[::-1]])
    b = np.concatenate([bit_patterns(seed + 1), np.nan_to_num(EDGES)])
    return a, b


def quantize_input() -> np.ndarray:
    """The bit patterns, the edge list, k/16384 one ulp either side for k around +-32768 (where the 16-bit
    wrap happens), and around +-2^31/16384 (where the conversion to int32 leaves its range)."""
    pts = [np.float32(s * k / 16384.0) for s in (1, -1) for k in (32766, 32767, 32768, 32769, 32770)]
    pts += [np.float32(s * 131072.0) for s in (1, -1)]
    pts = np.array(pts, np.float32)
    around = np.concatenate([np.nextafter(pts, np.float32(-np.inf)), pts, np.nextafter(pts, np.float32(np.inf))])
    return np.concatenate([bit_patterns(7), EDGES, around])


def ordinary(n: int, seed: int) -> np.ndarray:
    return _rng(4, n, seed).standard_normal(n).astype(np.float32)


def all_byte_pairs() -> np.ndarray:
    """Interleaved (I, Q) bytes with every byte value in both positions, against different partners."""
    v = np.arange(256, dtype=np.uint8)
    return np.stack([v, v[::-1] ^ 0x5A], axis=1).reshape(-1).copy()


def byte_pairs(n_pairs: int) -> np.ndarray:
    return _rng(5, n_pairs).integers(0, 256, 2 * n_pairs, dtype=np.uint8)


# ---- arctan demodulator ----------------------------------------------------------------------------------
def arctan_input(n: int, seed: int = 0):
    """Random phase steps with |step| <= 3.0 rad at a random amplitude: (i, q, first previous phase)."""
    r = _rng(6, n, seed)
    ph = 0.4 + np.cumsum(r.uniform(-3.0, 3.0, n))
    amp = r.uniform(0.2, 1.5, n)
    return (amp * np.cos(ph)).astype(np.float32), (amp * np.sin(ph)).astype(np.float32), 0.4


def arctan_axis_input():
    """The axis cases: the origin, the negative real axis from both sides of the cut after (1, 0), and a
    step of exactly 2 pi (the same point twice).  +pi and -pi are the same step: compare modulo 2 pi."""
    i = np.array([1, 0, 1, -1, 1, -1, -1, -1, 0.5, 0.5], np.float32)
    q = np.array([0, 0, 0, 0.0, 0, -0.0, 0.0, -0.0, 0.5, 0.5], np.float32)
    return i, q, 0.0


def wrap_2pi(d):
    d = np.asarray(d, np.float64)
    return d - 2 * np.pi * np.round(d / (2 * np.pi))


# ---- PSD estimate ------------------------------------------------------------------------------------------
PSD_BINS = tuple(2 ** k for k in range(1, 14))  # every size the kernel accepts: 2 .. 8192
PSD_REF_MAX_BINS = 512  # the reference build's float transform is the expected value up to here only
PSD_FS = 48000.0


def psd_layouts(bins: int):
    """(name, n): one segment, three segments plus a ragged tail that is dropped, nine segments."""
    return (("1seg", bins), ("3seg_tail", 3 * bins + max(bins // 2 - 1, 1)), ("9seg", 9 * bins))


def psd_input(bins: int, n: int) -> np.ndarray:
    """A tone plus noise, so that no bin is -Inf."""
    r = _rng(8, bins, n)
    t = np.arange(n)
    return (0.7 * np.sin(2 * np.pi * 0.1234 * t + 0.3) + 0.1 * r.standard_normal(n)).astype(np.float32)


def psd_float64(x: np.ndarray, bins: int, fs: float):
    """estimatePSD (fourier.cpp:35-117) restated in numpy: the window product in float, the transform in
    double, the per-segment dB rounded to float and averaged in float in segment order."""
    x = np.ascontiguousarray(x, np.float32)
    nseg = x.size // bins
    s = np.sin(np.arange(bins) * np.pi / bins)
    hann = (s * s).astype(np.float32)
    freq = np.arange(bins // 2, dtype=np.float32) * (np.float32(fs) / np.float32(bins))
    acc = np.zeros(bins // 2, np.float32)
    for l in range(nseg):
        w = x[l * bins:(l + 1) * bins] * hann
        X = np.fft.fft(w.astype(np.float64))[: bins // 2]
        acc = acc + (10.0 * np.log10(4.0 / (float(np.float32(fs)) * bins) * (X.real ** 2 + X.imag ** 2))).astype(np.float32)
    return freq, acc / np.float32(nseg)


# ---- filter designs ------------------------------------------------------------------------------------------
DESIGN_TAPS = (1, 2, 3, 50, 51, 101, 151)  # even counts too: the LPF and the BPF find their centre differently
LPF_DESIGNS = ((240000.0, 16000.0, 1), (2.4e6, 100000.0, 1), (35.28e6, 16000.0, 147), (48000.0, 23999.0, 3))
BPF_DESIGNS = ((240000.0, 22000.0, 54000.0), (240000.0, 18500.0, 19500.0), (250000.0, 113500.0, 114500.0))


# ---- comparison ------------------------------------------------------------------------------------------
def bits(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got: np.ndarray, want: np.ndarray, what: str = "") -> None:
    """Bit for bit; where the expected value is a NaN the result must be a NaN (payload and sign of a NaN
    are not compared)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind != "f":
        assert np.array_equal(got, want), what
        return
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN at", np.flatnonzero(gn != wn)[:8])
    diff = np.flatnonzero((bits(got) != bits(want)) & ~wn)
    assert diff.size == 0, (what, "differs at", diff[:8], got[diff[:8]], want[diff[:8]])
