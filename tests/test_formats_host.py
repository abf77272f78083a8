"""CPU tests of the raw I/Q formats (include/fmrx.h FMRX_IQ_*: u8, s8, s16, f32): the host-only
entry points and the Python helpers, plus the numpy restatements tests/test_gpu_formats.py builds
its expected values from -- each format's normalisation in float32 and the identity maps that carry
a u8 capture into the other formats without changing a single normalised sample.  No GPU, no
context."""
from __future__ import annotations

import re

import numpy as np
import pytest

import iqgen

U8, S8, S16, F32 = 0, 1, 2, 3
FORMATS = {"u8": U8, "s8": S8, "s16": S16, "f32": F32}
PAIR_BYTES = {U8: 2, S8: 2, S16: 4, F32: 8}
DTYPES = {U8: np.uint8, S8: np.int8, S16: np.int16, F32: np.float32}


@pytest.fixture(scope="module")
def fm():
    return iqgen.load_fmrx()


def normalise(raw, fmt):
    """x of fmrx.h's table as float32, interleaved as raw is: every one of them exact."""
    raw = np.ascontiguousarray(raw)
    if raw.dtype == np.complex64:
        raw = raw.view(np.float32)
    assert raw.dtype == DTYPES[fmt], (raw.dtype, fmt)
    if fmt == U8:
        return (raw.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
    if fmt == S8:
        return raw.astype(np.float32) / np.float32(128.0)
    if fmt == S16:
        return raw.astype(np.float32) / np.float32(32768.0)
    return raw.copy()


def identity_map(u8, fmt):
    """A u8 capture in another format with the same normalised samples."""
    u8 = np.ascontiguousarray(u8, np.uint8)
    if fmt == U8:
        return u8.copy()
    if fmt == S8:
        return (u8 ^ np.uint8(0x80)).view(np.int8)
    if fmt == S16:
        return ((u8.astype(np.int32) - 128) * 256).astype(np.int16)
    return ((u8.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)).astype(np.float32)


def test_pair_bytes(fm):
    assert fm.FMRX_EINVAL == -1
    assert (fm.IQ_U8, fm.IQ_S8, fm.IQ_S16, fm.IQ_F32) == (U8, S8, S16, F32)
    assert [fm.iq_pair_bytes(f) for f in (U8, S8, S16, F32)] == [2, 2, 4, 8]
    for bad in (-1, 4):
        assert fm.lib().fmrx_iq_pair_bytes(bad) == fm.FMRX_EINVAL
        with pytest.raises(fm.FmrxError) as e:
            fm.iq_pair_bytes(bad)
        assert e.value.code == fm.FMRX_EINVAL


def test_iq_format_of(fm):
    assert fm.iq_format_of(np.zeros(4, np.uint8)) == U8
    assert fm.iq_format_of(np.zeros(4, np.int8)) == S8
    assert fm.iq_format_of(np.zeros(4, np.int16)) == S16
    assert fm.iq_format_of(np.zeros(4, np.float32)) == F32
    assert fm.iq_format_of(np.zeros(4, np.complex64)) == F32
    for dt in (np.uint16, np.int32, np.int64, np.float64, np.complex128, np.float16, bool):
        with pytest.raises(ValueError):
            fm.iq_format_of(np.zeros(4, dt))


def test_new_symbols_are_in_the_header(fm):
    syms = fm.header_symbols()
    for name in ("fmrx_iq_pair_bytes", "fmrx_set_input_format", "fmrx_input_format"):
        assert name in syms and name in fm.PROTOTYPES
    txt = open(fm.HEADER).read()
    for k, v in FORMATS.items():
        assert re.search(rf"#define\s+FMRX_IQ_{k.upper()}\s+{v}\b", txt), k


def test_identity_maps_keep_every_normalised_sample():
    u8 = np.arange(256, dtype=np.uint8)  # every byte value
    want = normalise(u8, U8)
    assert want.dtype == np.float32 and want[0] == -1.0 and want[128] == 0.0 and want[255] == np.float32(127 / 128)
    # the float32 values are the exact quotients
    assert np.array_equal(want.astype(np.float64), (u8.astype(np.float64) - 128.0) / 128.0)
    for fmt in (S8, S16, F32):
        raw = identity_map(u8, fmt)
        assert raw.dtype == DTYPES[fmt]
        got = normalise(raw, fmt)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), fmt
    assert np.array_equal(identity_map(u8, S8).astype(np.int32), u8.astype(np.int32) - 128)
    assert np.array_equal(identity_map(u8, S16).astype(np.int32), (u8.astype(np.int32) - 128) * 256)
    # and on a real capture, pairs in place
    iq = iqgen.make("synth:3", 4096)
    for fmt in (S8, S16, F32):
        assert np.array_equal(normalise(identity_map(iq, fmt), fmt), normalise(iq, U8))


def test_normalisations_are_exact_in_float32():
    s16 = np.array([-32768, -32767, -1, 0, 1, 12345, 32767], np.int16)
    assert np.array_equal(normalise(s16, S16).astype(np.float64), s16.astype(np.float64) / 32768.0)
    s8 = np.arange(-128, 128).astype(np.int8)
    assert np.array_equal(normalise(s8, S8).astype(np.float64), s8.astype(np.float64) / 128.0)
    z = np.array([1 + 2j, -0.5 + 0.25j], np.complex64)
    assert np.array_equal(normalise(z, F32), np.array([1, 2, -0.5, 0.25], np.float32))
