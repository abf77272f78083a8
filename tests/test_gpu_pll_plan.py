"""The PLL executor against the recorded launch table (tests/golden/pll_plan_parent.json).

The table holds, per case, the stage records (launches and serial steps per stage kind,
fmrx_debug_stage_timing) of the commit before launch_pll was split into a plan (csrc/pll_plan.cpp)
and an executor (csrc/pll.hip), recorded on an MI355X.  tests/test_pll_plan.py holds the plan to
the table on the CPU; here the executor runs each cheap case for real: its records must equal the
table's, and its PCM the plain certified launch's (knob pll_spec = 0).
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import iqgen
import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pll_plan_parent.json")
# the stage kinds launch_pll records (the NCO is the engine's: in launch_pll, in the small audio
# kernel or on the audio stream, by call length)
NOT_PLL = ("front_end", "bandpass_pair", "pll_nco", "audio")
MAX_BLOCKS = 27  # the table's longer cases are for the CPU check alone


def load_table():
    with open(TABLE) as f:
        return json.load(f)


def trig_of(case, s):
    """Stream s's trigOffset at the call's start: `trig` for every stream; "unknown": a value
    that is no integer (the host drops its bounds); `trig_hi`: streams past the first there."""
    if case["trig"] == "unknown":
        return 1000.5
    return float(case["trig_hi"]) if s > 0 and "trig_hi" in case else float(case["trig"])


_IQ = {}


def run_case(fm, case, **more_knobs):
    """One mode-0 stereo call of the case's shape from its trigOffset (set through a state blob):
    (pcm, {stage: launches}, {stage: steps}) of the PLL's stage kinds."""
    ns, nb = case["n_streams"], case["blocks"]
    bb = oracle.MODES[0][0]
    if nb not in _IQ:
        _IQ[nb] = iqgen.make("synth:91", nb * bb)
    iq = np.tile(_IQ[nb], (ns, 1)) if ns > 1 else _IQ[nb]
    with fm.Receiver(0, fm.STEREO, n_streams=ns, knobs={**case["knobs"], **more_knobs}) as rx:
        blob = bytearray(rx.get_state())
        hdr = np.frombuffer(bytes(blob[:40]), np.uint32)
        pll_off = 40 + ns * (int(hdr[6]) + 4 * int(hdr[7]) + 4 * 64)
        pll = np.frombuffer(bytes(blob[pll_off: pll_off + 32 * ns]), np.float32).copy().reshape(ns, 8)
        pll[:, 5] = [trig_of(case, s) for s in range(ns)]
        blob[pll_off: pll_off + 32 * ns] = pll.tobytes()
        rx.set_state(bytes(blob))
        rx.stage_timing(1)
        pcm = rx.process(iq)
        st = rx.stage_timing(-1)
    st = {k: v for k, v in st.items() if k not in NOT_PLL}
    return pcm, {k: int(v[1]) for k, v in st.items()}, {k: int(v[2]) for k, v in st.items() if v[2]}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


CASES = [c for c in load_table()["cases"] if c["blocks"] <= MAX_BLOCKS] if os.path.exists(TABLE) else []


def test_table_has_the_named_shapes():
    """The shapes the executor can still go wrong at are among the cases run here."""
    have = {(c["n_streams"], c["blocks"], c["trig"]) for c in CASES}
    for shape in ((1, 1, 2**22 - 320), (1, 7, 2**19), (1, 26, 2**22), (342, 27, 2**20 - 8000), (1025, 1, 0),
                  (5000, 1, 0)):
        assert shape in have, shape
    assert any(c["n_streams"] == 16 and c["blocks"] == 26 and c["knobs"].get("stereo_chunks", 0) > 1 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_executor_launches_the_recorded_plan(fmrx, case):
    n_simd = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    assert n_simd == load_table()["n_simd"], "the table was recorded at another SIMD count"
    got, launches, steps = run_case(fmrx, case)
    print(case["name"], launches, steps)
    assert launches == case["launches"]
    assert steps == case["steps"]
    want, _, _ = run_case(fmrx, case, pll_spec=0)
    assert np.array_equal(got, want)
