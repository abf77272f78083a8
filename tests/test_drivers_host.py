"""The fmrx executable's refusals that leave before a context exists, against the record of its parent
(tests/golden/drivers_parent.json, section refusals): the exit status and the exact stderr of ten argument
lists, taken from a run of the commit before csrc/cli.cpp's argument handling became a parse function.  No
GPU is needed, as for tests/test_host.py::test_cli_built_and_usage."""
from __future__ import annotations

import pytest

import drivers_ref as D


def test_the_record_holds_every_refusal():
    assert set(D.load_record()["refusals"]) == {" ".join(a) for a in D.REFUSALS} and len(D.REFUSALS) == 10


@pytest.mark.parametrize("argv", D.REFUSALS, ids=lambda a: " ".join(a))
def test_refusal(fmrx, argv):
    want = D.load_record()["refusals"][" ".join(argv)]
    got = D.refusal_case(fmrx, argv)
    assert want["status"] != 0 and D.text(got) == D.text(want)
