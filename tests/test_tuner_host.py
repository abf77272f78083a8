"""CPU tests of the rotator design behind off-centre tuning (fmrx_tuner_design, host only):
period, step and table of an offset, and the offsets it refuses."""
from __future__ import annotations

import numpy as np
import pytest


@pytest.mark.parametrize("rf_fs,f,want", [
    (2400000, 0, (1, 0)),
    (2400000, 300000, (8, 1)),
    (2400000, -125000, (96, 91)),
    (1152000, 200000, (144, 25)),
    (2400000, 1199000, (2400, 1199)),
])
def test_period_and_step(fmrx, rf_fs, f, want):
    n, k, tab = fmrx.tuner_design(rf_fs, f)
    assert (n, k) == want
    assert tab.shape == (n, 2) and tab.dtype == np.float32
    if f == 0:
        assert tab.tolist() == [[1.0, 0.0]]
    # k n f_s / N is f mod f_s: the rotator turns by exactly the offset
    assert (k * rf_fs // n - f) % rf_fs == 0 and (k * rf_fs) % n == 0


@pytest.mark.parametrize("rf_fs,f", [(2400000, 300000), (2400000, -125000), (1152000, 200000),
                                     (2400000, 1199000), (2304000, 1000), (2400000, -1000)])
def test_table_within_one_ulp_of_float64(fmrx, rf_fs, f):
    n, _, tab = fmrx.tuner_design(rf_fs, f)
    a = 2 * np.pi * np.arange(n, dtype=np.float64) / n
    for col, ref in ((0, np.cos(a)), (1, np.sin(a))):
        r32 = ref.astype(np.float32)
        err = np.abs(tab[:, col].astype(np.float64) - r32.astype(np.float64))
        assert np.all(err <= np.spacing(np.abs(r32)).astype(np.float64)), (col, int(np.argmax(err)))


@pytest.mark.parametrize("mode_fs", [2400000, 1152000, 2304000])
def test_every_kilohertz_multiple_is_accepted(fmrx, mode_fs):
    for f in (1000, -7000, 99000, mode_fs // 2 - 1000, -(mode_fs // 2 - 1000)):
        n, k, _ = fmrx.tuner_design(mode_fs, f)
        assert 1 <= n <= 4096 and 0 <= k < n


@pytest.mark.parametrize("f", [1, 1200000, -1200000, 2400000])
def test_refused_offsets(fmrx, f):
    """1 Hz needs a period of 2.4 M pairs (> 4096); |f| >= rf_fs / 2 is outside the capture."""
    with pytest.raises(fmrx.FmrxError) as e:
        fmrx.tuner_design(2400000, f)
    assert e.value.code == fmrx.FMRX_EINVAL
