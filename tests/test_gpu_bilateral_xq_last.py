"""The inclusive last candidate of the xq form (k_bilateral_xq.hip, LASTC): at numDisparity 128 / 64 -- 129 / 65 candidates, the
reference's own configurations -- the interior tiles' workgroups finish candidate 128 / 64 themselves and write the disparity;
the one-kernel launch for that candidate, its winner slice and the merge shrink to the columns of the border tiles.  Volume (all
numD + 1 planes) and disparity are compared bit for bit with the oracle and with the one-kernel path, and the launch count pins
the path (4 on the xq path with a tail, 2 without, 1 on the one-kernel path)."""
import ctypes as C

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _image
from aswstereomatch_amd.synth import make_pair

pytestmark = pytest.mark.gpu
LEFT, RIGHT = asw.DISPARITY_LEFT, asw.DISPARITY_RIGHT
BOTH = (LEFT, RIGHT)


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_old():
    c = asw.Context(0, env={"ASW_BILATERAL_XQ": "0"})  # the one-kernel form only
    yield c
    c.close()


def check(ctx, ctx_old, oracle, L, R, dt, minD, numD, launches):
    d, v = ctx.computeAdaptiveWeight(L, R, 30, 20, dt, 15, minD, numD, return_cost_volume=True)
    assert ctx.timing()["aggregate_launches"] == launches
    rc, dw, vw = oracle.asw_classic(L, R, 30, 20, int(dt), 15, minD, numD, want_vol=True)
    assert rc == 0 and v.shape == vw.shape == (numD + 1,) + L.shape[:2]
    assert np.array_equal(v, vw, equal_nan=True), np.argwhere(v != vw)[:5]
    assert np.array_equal(d, dw), np.argwhere(d != dw)[:5]
    d0, v0 = ctx_old.computeAdaptiveWeight(L, R, 30, 20, dt, 15, minD, numD, return_cost_volume=True)
    assert ctx_old.timing()["aggregate_launches"] == 1
    assert np.array_equal(v, v0, equal_nan=True) and np.array_equal(d, d0)
    return dw, vw


def shifted_pair(H, W, numD):
    """R = L moved left by numD columns (the last valid column replicated): the last candidate is the true match"""
    L = make_pair(H, W, 16, seed=5, block=16)[0]
    R = L[:, np.minimum(np.arange(W) + numD, W - 1)].copy()
    return L, R


# 200: 3 interior tiles + 1 partial border tile; 136: 2 + 1
@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("H,W,numD", [(9, 200, 128), (9, 200, 64), (9, 136, 64)])
def test_last_candidate_wins_somewhere(ctx, ctx_old, oracle, H, W, numD, dt):
    L, R = shifted_pair(H, W, numD)
    rc, dw, _ = oracle.asw_classic(L, R, 30, 20, int(dt), 15, 0, numD)
    assert rc == 0 and (dw == numD).sum() > 0  # before any comparison (the oracle's count: several hundred of these pixels)
    check(ctx, ctx_old, oracle, L, R, dt, 0, numD, 4)


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("numD", [128, 64])
def test_ties_keep_the_first_minimum(ctx, ctx_old, oracle, numD, dt):
    L = np.full((9, 200, 3), 77, np.uint8)
    dw, vw = check(ctx, ctx_old, oracle, L, L.copy(), dt, 0, numD, 4)
    assert (dw == 0).all() and (vw == vw[0]).all()


# (H, W, minD, numD, directions): W = 130: 1 interior + 2 border tiles (LEFT); 135 with 65 candidates; 70: no interior tile for
# LEFT (the old sequence); 96 LEFT with 129 candidates: most positions clamp to column 0; H = 3 / 9: the window clamps
# vertically; minD: LEFT up to 48, RIGHT up to x0_last + minD = W - 1 (192 + 7 at W = 200)
GEOMETRY = [(9, 130, 0, 128, BOTH), (3, 130, 0, 128, BOTH), (9, 135, 0, 64, BOTH), (3, 70, 0, 64, BOTH), (3, 96, 0, 128, (LEFT,)),
            (9, 96, 0, 128, (LEFT,)), (3, 200, 0, 128, BOTH), (9, 200, 48, 128, (LEFT,)), (9, 200, 7, 128, (RIGHT,)),
            (3, 200, 48, 64, (LEFT,)), (3, 200, 7, 64, (RIGHT,))]


@pytest.mark.parametrize("H,W,minD,numD,dirs", GEOMETRY)
def test_tile_geometry_and_min_disparity(ctx, ctx_old, oracle, H, W, minD, numD, dirs):
    L, R, _ = make_pair(H, W, min(numD, W // 2), seed=H * 1000 + W + minD, block=16)
    for dt in dirs:
        check(ctx, ctx_old, oracle, L, R, dt, minD, numD, 4)


# one candidate fewer: no tail at all (2 launches); more than one candidate past the block: the whole-frame tail as before (4)
@pytest.mark.parametrize("numD,launches", [(127, 2), (63, 2), (129, 4), (130, 4), (160, 4), (65, 4), (66, 4), (67, 4), (68, 4),
                                           (69, 4), (70, 4)])
def test_neighbours_of_the_switch(ctx, ctx_old, oracle, numD, launches):
    L, R, _ = make_pair(3, 200, 100, seed=numD, block=16)
    for dt in BOTH:
        check(ctx, ctx_old, oracle, L, R, dt, 0, numD, launches)


@pytest.mark.parametrize("dt", BOTH)
@pytest.mark.parametrize("W,numD", [(200, 128), (130, 128), (135, 64)])
def test_every_pixel_is_written_once_through_the_c_entry_point(ctx, oracle, W, numD, dt):
    """Interior and border launches write disjoint column windows of the same buffers: sentinel-filled host outputs, and device
    buffers that still hold another pair's result, must come back as the oracle's frame -- no sentinel, no stale column, no seam."""
    H = 5
    other = make_pair(H, W, 16, seed=77, block=8)
    ctx.computeAdaptiveWeight(other[1], other[0], 30, 20, dt, 15, 0, numD, return_cost_volume=True)
    L, R = shifted_pair(H, W, numD)
    li, la = _image(L)
    ri, ra = _image(R)
    disp = np.full((H, W), -7.0, np.float32)
    di, _ = _image(disp, 5)
    vol = np.full((numD + 1, H, W), -7.0, np.float32)
    rc = ctx._lib.asw_aggregate_bilateral(ctx._h, C.byref(li), C.byref(ri), C.byref(di), 30.0, 20.0, int(dt), 15, 0, numD,
                                          vol.ctypes.data_as(C.c_void_p), vol.size)
    assert rc == 0 and ctx.timing()["aggregate_launches"] == 4
    rc, dw, vw = oracle.asw_classic(L, R, 30, 20, int(dt), 15, 0, numD, want_vol=True)
    assert rc == 0 and not (disp == -7.0).any() and not (vol == -7.0).any()
    assert np.array_equal(vol, vw, equal_nan=True), np.argwhere(vol != vw)[:5]
    assert np.array_equal(disp, dw), np.argwhere(disp != dw)[:5]


def test_call_history_does_not_matter(oracle):
    """The winner slices and their column windows are reused scratch: 129 candidates, then 161, then 129 again on one context."""
    c = asw.Context(0)
    try:
        L, R = shifted_pair(5, 200, 128)
        for dt in BOTH:
            want = {n: oracle.asw_classic(L, R, 30, 20, int(dt), 15, 0, n, want_vol=True) for n in (128, 160)}
            for n in (128, 160, 128):
                d, v = c.computeAdaptiveWeight(L, R, 30, 20, dt, 15, 0, n, return_cost_volume=True)
                assert c.timing()["aggregate_launches"] == 4
                assert np.array_equal(d, want[n][1]) and np.array_equal(v, want[n][2], equal_nan=True)
    finally:
        c.close()
