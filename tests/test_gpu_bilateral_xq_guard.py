"""The guard of the xq kernel's scaled domain (bilateral_xq_lut_ok, asw_methods.hip): gammas whose smallest weight product falls
below 2^-68 must take the one-kernel form and still match the oracle bit for bit; gammas just above the bound stay on the xq
kernels (and match too).  Both directions."""
import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd.synth import make_pair
from tests.test_xq_scaled_domain_cpu import lut_classic, lut_ok

pytestmark = pytest.mark.gpu
LEFT, RIGHT = asw.DISPARITY_LEFT, asw.DISPARITY_RIGHT


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


# (gamma_c, gamma_g, takes the xq kernels): 10.5 / 10.6 straddle the bound at gamma_g = 20
CASES = [(10.5, 20.0, False), (7.5, 11.25, False), (10.6, 20.0, True), (30.0, 20.0, True)]


@pytest.mark.parametrize("gc,gg,xq", CASES)
@pytest.mark.parametrize("dt", [LEFT, RIGHT])
def test_guard_path_and_parity(ctx, oracle, gc, gg, xq, dt):
    assert lut_ok(lut_classic(gc, gg)) == xq
    # dark and bright blocks so that gray differences near 255 occur: the smallest weights are in play
    L, R, _ = make_pair(9, 200, 60, seed=31, block=16)
    L[:, ::3] = 0
    R[:, 1::4] = 255
    d, v = ctx.computeAdaptiveWeight(L, R, gc, gg, dt, 15, 0, 128, return_cost_volume=True)
    launches = ctx.timing()["aggregate_launches"]
    assert launches == (4 if xq else 1), (gc, gg, launches)
    rc, dw, vw = oracle.asw_classic(L, R, gc, gg, int(dt), 15, 0, 128, want_vol=True)
    assert rc == 0
    assert np.array_equal(v, vw, equal_nan=True), (gc, gg)
    assert np.array_equal(d, dw), (gc, gg)
