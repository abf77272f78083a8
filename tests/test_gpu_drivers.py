"""The two drivers against the record of their parent (tests/golden/drivers_parent.json).

fmrx.decode_stations and the fmrx executable (csrc/cli.cpp) each carry every optional product of the
receiver: RDS, the block sync, de-emphasis, the subcarrier meter, soft stereo, AFC.  The record holds what
both did, on an MI355X, at the commit before they were given one place per product: 21 decode_stations
cases (every switch alone, the pairs, all together, a capture shorter than a frame, one without stations,
both wide routes) and 6 runs of the executable.  Each case here runs again through tests/drivers_ref.py and
must give the record's canonical JSON text, character for character: every station's offset and levels,
the PCM's bytes, every further element of the tuple; the exit status, the whole stderr and stdout's bytes.
The captures' own hashes are asserted first, so a drifting generator is told apart from a drifting decode.
"""
from __future__ import annotations

import pytest

import drivers_ref as D

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()  # before the library's first HIP call, as the other device-pointer tests do


@pytest.fixture(scope="module")
def record():
    return D.load_record()


def check_capture(record, name):
    assert D.sha256(D.capture(name)) == record["captures"][name], f"capture {name} is not the recorded one: the generator drifted"


def test_the_record_holds_every_case_and_capture(record):
    assert set(record["decode"]) == set(D.DECODE_CASES) and len(D.DECODE_CASES) == 21
    assert set(record["cli"]) == set(D.CLI_CASES) and len(D.CLI_CASES) == 6
    assert len(record["commit"]) == 40
    assert D.capture_hashes() == record["captures"]


@pytest.mark.parametrize("name", list(D.DECODE_CASES))
def test_decode_stations_case(fmrx, record, name):
    check_capture(record, D.DECODE_CASES[name][0])
    got = D.decode_case(fmrx, name)
    assert D.text(got) == D.text(record["decode"][name])


@pytest.mark.parametrize("name", list(D.CLI_CASES))
def test_cli_case(fmrx, record, name):
    check_capture(record, D.CLI_CASES[name][0])
    got = D.cli_case(fmrx, name)
    assert D.text(got) == D.text(record["cli"][name])
