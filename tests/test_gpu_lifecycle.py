"""Create/destroy cycles of a context with every lazily allocated stage turned on: the device memory in
use after cycle 2 and after cycle 20 must be equal (the context's buffers and events free themselves in
fmrx_destroy; one that did not would show here as growth), and the same for 20 refused creations."""
from __future__ import annotations

import os

import numpy as np
import pytest

import iqgen

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CYCLES = 20
CAP_FS = 6000000  # mode 0: 5/2 of rf_fs, a rational rate (rate.hip) with a granule of one block


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()  # before the library's first HIP call, as the other device-pointer tests do


def in_use():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return total - free


def lazy_stages_on(fm, rx):
    """Everything a context allocates only on demand, but the wide stage: RDS work rows, the block sync,
    the meter, the de-emphasis carry, the tuner tables (a format other than u8), the scan and both kinds of
    timing events (fmrx_kernel_timing's pairs come with the down-converter's launches: cycle_wide)."""
    rx.set_rds(True)
    rx.set_rds_sync(True)
    rx.set_meter(True)
    rx.set_deemphasis(50)
    rx.set_input_format(fm.IQ_S16)
    rx.scan(np.zeros(2 * 256, np.int16), fft_bins=256)  # the smallest transform, one segment
    rx.kernel_timing(1)
    rx.stage_timing(1)


def cycle_plain(fm):
    with fm.Receiver(0, fm.STEREO, n_streams=2) as rx:
        lazy_stages_on(fm, rx)
        n = rx.rds_granule * 2 * rx.geo.iq_pairs  # elements a stream of one RDS granule
        pcm = rx.process(np.zeros((2, n), np.int16))
        assert pcm.shape == (2, rx.rds_granule * rx.geo.pcm_samples)
        assert rx.stage_timing(0) and rx.rds_info(1).bits > 0 and rx.meter_report(1).frames == 1


def cycle_wide(fm):
    with fm.Receiver(0, fm.STEREO, n_streams=2) as rx:
        lazy_stages_on(fm, rx)
        rx.set_capture_rate(CAP_FS)
        rx.tune_wide([0, 600000])
        blocks, pairs = rx.wide_granule
        assert rx.rds_granule % blocks == 0
        pcm = rx.process_wide(np.zeros(rx.rds_granule // blocks * 2 * pairs, np.int16))  # one RDS granule
        assert pcm.shape == (2, rx.rds_granule * rx.geo.pcm_samples)
        assert rx.kernel_timing()[1] > 0 and rx.rds_info(1).bits > 0 and rx.meter_report(1).frames == 1


def cycle_refused(fm):
    os.environ["FMRX_PLL_SPEC"] = "7"  # outside [0, 1]: fmrx_create refuses the context
    try:
        with pytest.raises(fm.FmrxError) as e:
            fm.Receiver(0, fm.STEREO, n_streams=2)
        assert e.value.code == fm.FMRX_EINVAL and "FMRX_PLL_SPEC" in str(e.value)
    finally:
        del os.environ["FMRX_PLL_SPEC"]


@pytest.mark.parametrize("cycle", [cycle_plain, cycle_wide, cycle_refused], ids=["plain", "wide", "refused"])
def test_cycles_leave_device_memory_as_it_was(fmrx, cycle):
    """The first cycle warms the runtime's own pools; cycles 3 .. 20 must then leave the bytes in use
    exactly where cycle 2 left them."""
    readings = []
    for k in range(1, CYCLES + 1):
        cycle(fmrx)
        if k in (2, CYCLES):
            readings.append(in_use())
    print(f"{cycle.__name__}: {readings[0]} B in use after cycle 2, {readings[1]} B after cycle {CYCLES}")
    assert readings[1] == readings[0]
