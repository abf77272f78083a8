"""CPU guard of tests/test_gpu_variants.py's matrices: the instantiations of tuner_kernel,
wide_ddc_kernel and mono_fused_kernel that libfmrx.so holds, read from its symbol table (`nm -C`:
names only, never the code), are exactly what the GPU tests parametrize over.  A newly compiled
instantiation fails here until a GPU case names it; a case whose kernel is gone fails too."""
from __future__ import annotations

import re
import shutil
import subprocess

import pytest

import oracle
from test_gpu_variants import FUSED_CASES, TUNER_CASES, WIDE_CASES, fused_variants, rf_decim

KERNELS = ("tuner_kernel", "wide_ddc_kernel", "mono_fused_kernel")


@pytest.fixture(scope="module")
def instantiations(fmrx):
    """kernel name -> the set of its template argument tuples in the library (a kernel shows up twice,
    as its host stub and its handle: a set)."""
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm is not on this machine")
    out = subprocess.run([nm, "-C", fmrx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    found = {name: set() for name in KERNELS}
    for name, args in re.findall(r"\b(%s)<([-0-9, ]+)>\(" % "|".join(KERNELS), out):
        found[name].add(tuple(int(a) for a in args.split(",")))
    return found


def test_symbols_were_read(instantiations):
    """The counts of a build of this tree; the three tests below say what they are made of."""
    assert {k: len(v) for k, v in instantiations.items()} == {"tuner_kernel": 24, "wide_ddc_kernel": 36,
                                                             "mono_fused_kernel": 41}


def test_tuner_matrix_is_complete(instantiations):
    """tuner_kernel<T, D, R, PD, F>: R and PD follow from D (launch_tuner), so (T, D, F) names one."""
    compiled = {(t, d, f) for t, d, _, _, f in instantiations["tuner_kernel"]}
    assert len(compiled) == len(instantiations["tuner_kernel"])
    tested = {(rf_taps, rf_decim(mode), fmt) for mode, rf_taps, fmt in TUNER_CASES}
    assert compiled == tested, (sorted(compiled - tested), sorted(tested - compiled))


def test_wide_matrix_is_complete(instantiations):
    compiled = instantiations["wide_ddc_kernel"]  # wide_ddc_kernel<D, F>
    tested = set(WIDE_CASES)
    assert compiled == tested, (sorted(compiled - tested), sorted(tested - compiled))


def test_fused_matrix_is_complete(instantiations):
    """mono_fused_kernel<T, D, AD, NT, R, PD, ABL, TR, AU, Z0>: every (T, D, AD, AU) meets the oracle in
    its default shape.  The other workgroup shapes (NT, R, PD, TR) of one (T, D, AD, AU) are reached only
    through the tuning switch FMRX_MONO_VARIANT, which a process reads once, and ABL = 64 only through
    fmrx_debug_mono_stamps: they are not part of this matrix."""
    compiled = {(a[0], a[1], a[2], a[8]) for a in instantiations["mono_fused_kernel"]}
    tested = set().union(*(fused_variants(*case) for case in FUSED_CASES))
    assert compiled == tested, (sorted(compiled - tested), sorted(tested - compiled))
    stages = [(rf_decim(m), oracle.MODES[m][7], oracle.MODES[m][6]) for m in range(4)] + [(9, 5, 1)]
    assert tested == {(t,) + s for t in (51, 101) for s in stages} and len(tested) == 10
