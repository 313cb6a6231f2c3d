"""The float ASW matchers on pairs whose aggregated costs tie (tests/asw_cases.py): periodic pairs, on which 0.44-0.95 of the
pixels have a bit-equal minimum and the winner is not the first candidate, and a row-constant pair, on which every candidate ties.

Every method resolves its winner by "strict `<` while d ascends", spread over the 16/8/4/2/1 candidate chunks of k_asw_bilateral
and its grid.z split merged by k_merge_slices; the xq forms of the classic and geodesic kernels (candidates dealt over 4 or 8
wavefronts, the inclusive last candidate finished in the workgroup, border tiles on a side stream, the tail slice merged by
k_merge_slices or k_merge_slices_cols); launch_asw_geodesic_few; the 16-candidate chunks of k_ncc; launch_wta behind the guided
family and the weighted median.  A stage that keeps the later of two equal costs, or reduces out of order, shows on these rows and on
no textured pair.  Each row of the table names what it ties across; tests/test_asw_cases_cpu.py shows on the oracle alone that the
rows tie and that the oracle's own map follows the rule.

Comparison: the rules of asw_cases.check (bit for bit, or for the guided-filter family the volume bound and a winner among the
oracle's minimisers).  Classic and geodesic at win 15 are also compared bit for bit with a context created under
ASW_BILATERAL_XQ=0 / ASW_GEODESIC_XQ=0, the weighted median at win 15 and 17 with one under ASW_WMEDIAN_TILE=0.

The bilateral grid stays out of this file: its grid coordinates depend on x, and blocky periodic pairs gave an oracle tie share of
at most 0.002.  tests/test_gpu_asw_sweep.py covers it."""
import os
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asw_cases as ac  # noqa: E402

pytestmark = pytest.mark.gpu

TABLE_METHODS = [m for m in ac.METHODS if m != "bilgrid"]
XQ_SWITCH = {"classic": "ASW_BILATERAL_XQ", "geodesic": "ASW_GEODESIC_XQ"}


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plain():
    """contexts created under a switch set to 0, by switch name (the library reads its switches once, in asw_create)"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = asw.Context(0, env={name: "0"})
        return made[name]

    yield get
    for c in made.values():
        c.close()


def _id(row):
    return "x".join(str(v) for v in row)


def _cases():
    return [pytest.param(m, row, id="%s-%s" % (m, _id(row))) for m in TABLE_METHODS for row in ac.tie_rows(m)]


def _same(a, b):
    return np.array_equal(a["vol"], b["vol"], equal_nan=True) and np.array_equal(a["disp"], b["disp"])


@pytest.mark.parametrize("method,row", _cases())
def test_tied_costs(ctx, plain, oracle, method, row):
    for dt in ac.directions(method):
        case = ac.table_case(method, row, dt)
        got = ac.gpu_result(ctx, case)
        ac.check(case, got, ac.reference(oracle, case))
        if case["win"] == 15 and method in XQ_SWITCH:
            if row in ac.XQ_ROWS and method == "classic":    # the geodesic method reports one count for both of its forms
                assert ctx.timing()["aggregate_launches"] in (2, 4), "the row did not take the xq kernels: %r" % (case["tag"],)
            assert _same(got, ac.gpu_result(plain(XQ_SWITCH[method]), case)), (XQ_SWITCH[method], case["tag"])
        if method == "wmedian" and case["win"] in (15, 17):
            assert _same(got, ac.gpu_result(plain("ASW_WMEDIAN_TILE"), case)), ("ASW_WMEDIAN_TILE", case["tag"])


@pytest.mark.parametrize("method", ["classic", "geodesic"])
def test_row_constant_pair(ctx, plain, oracle, method):
    for dt in ac.directions(method):
        case = ac.row_constant_case(method, dt)
        got = ac.gpu_result(ctx, case)
        want = ac.reference(oracle, case)
        ac.check(case, got, want)
        assert _same(got, ac.gpu_result(plain(XQ_SWITCH[method]), case)), (XQ_SWITCH[method], case["tag"])
        # every candidate ties, so every pixel whose costs are defined keeps the first: candidates that leave the image clamp to
        # its border, whose columns hold the row's value too
        sel = np.isfinite(want["vol"]).any(axis=0)
        assert (got["disp"][sel] == case["minD"]).all()
