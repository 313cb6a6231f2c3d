"""A seeded sweep of the float ASW matchers against the oracle (tests/asw_cases.py): random frames from 1 x 1 to 40 x 160, windows
from {1, 3, 5, 7, 9, 11, 15, 17, 21, 35} (GuidedF_2 also even ones), 1 to 47 candidates, minD from {0, 1, 3, 17}, both directions
where the method serves DISPARITY_RIGHT, the method's own parameters, rows with padding.  The input kind cycles with the case index
over constant, periodic, identical periodic, row-constant, quantised, flat-rectangle and textured pairs; every twelfth case has 48 to
150 candidates on a frame of at most 24 x 96 (the 16-wide chunk and z-split boundaries); every eighth case of classic and geodesic
is forced into the domain of the xq kernels (win 15, 63 to 200 candidates, widths 64 to 300).  A fresh context every 8 cases lets
first-use paths (unallocated tables, scratch growth) run in many orders.

asw_cases.SWEEP_COUNT = 60 cases per method and seed, 2 seeds, 10 methods: 1200 cases (20 cases took 0.1 to 0.4 s per parametrised
test on an MI355X, the oracle's side included).  tests/test_asw_cases_cpu.py shows that over these seeds every method meets every
kind and direction it serves, and that the sweep holds win 1, one-row, one-column, numD > W and minD > 0 cases.  The comparison is
asw_cases.check; a failure names the call that rebuilds its case."""
import os
import sys

import pytest

import aswstereomatch_amd as asw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asw_cases as ac  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", ac.SWEEP_SEEDS)
@pytest.mark.parametrize("method", ac.METHODS)
def test_seeded_sweep(oracle, method, seed):
    ctx = None
    try:
        for i, case in enumerate(ac.cases(method, seed)):
            if i % ac.FRESH_EVERY == 0:
                if ctx is not None:
                    ctx.close()
                ctx = asw.Context(0)
            try:
                got = ac.gpu_result(ctx, case)
            except asw.AswError as e:
                raise AssertionError("%r: asw_cases.build_case(%r, %r)" % (e, method, case["tag"]))
            assert got["disp"] is not None, "status %d: asw_cases.build_case(%r, %r)" % (asw.last_status(), method, case["tag"])
            ac.check(case, got, ac.reference(oracle, case))
    finally:
        if ctx is not None:
            ctx.close()
