"""The step tables of k_bilateral_xq.hip (ready-made cell entries, the lane table of clamped positions and row-loop bases):
volume and disparity bit for bit against the oracle and against the one-kernel path (ASW_BILATERAL_XQ=0), both directions, on
noise images (every gray difference, so every weight class and LUT column is gathered).  The shapes are the ones at which a
wrong offset, clamp or row assignment shows:
  H = 17: window rows with and without the vertical clamp; H = 3: the clamp covers every row
  W = 330: several interior tiles, a tile whose positions partly clamp at column 0 (LEFT) / W - 1 (RIGHT), a partial border
           tile; W = 96 and W = 130: one interior tile next to a border tile, W < numD
  numD 128 / 64: the last-candidate units (8 / 4 wavefronts); 127 / 63: no tail; 130: a whole-frame tail
  minD 48 (LEFT) and x0_last + minD = W - 1 (RIGHT): the largest admissible ones, both bounds of the position clamp active"""
import numpy as np
import pytest

import aswstereomatch_amd as asw

pytestmark = pytest.mark.gpu
LEFT, RIGHT = asw.DISPARITY_LEFT, asw.DISPARITY_RIGHT


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


def noise_pair(H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W, 3)).astype(np.uint8), rng.integers(0, 256, (H, W, 3)).astype(np.uint8)


def right_max_mind(W):
    return W - 1 - (W - 1) // 64 * 64  # x0_last + minD = W - 1


# (H, W, minD, numD)
LEFT_CASES = [(17, 330, 0, 128), (17, 330, 48, 128), (3, 330, 48, 64), (17, 330, 0, 64), (3, 330, 0, 127), (17, 330, 48, 63),
              (17, 330, 5, 130), (17, 96, 0, 128), (3, 96, 48, 64), (17, 96, 48, 127), (17, 130, 48, 128), (3, 130, 0, 63),
              (17, 130, 0, 64), (3, 130, 48, 130)]
RIGHT_CASES = [(17, 330, right_max_mind(330), 128), (3, 330, right_max_mind(330), 64), (17, 330, 0, 64), (17, 330, 0, 128),
               (3, 330, 0, 63), (17, 330, right_max_mind(330), 130), (17, 330, right_max_mind(330), 127),
               (17, 96, right_max_mind(96), 128), (3, 96, right_max_mind(96), 64), (17, 96, 0, 63),
               (17, 130, right_max_mind(130), 64), (3, 130, right_max_mind(130), 127), (17, 130, 0, 128), (3, 130, 0, 130)]


def check(ctx, ctx_old, oracle, dt, H, W, minD, numD, gc=30, gg=20):
    L, R = noise_pair(H, W, seed=((H * 1000 + W) * 100 + minD) * 1000 + numD + int(dt))
    d, v = ctx.computeAdaptiveWeight(L, R, gc, gg, dt, 15, minD, numD, return_cost_volume=True)
    # the xq kernels served the call: two launches without a tail, four with one
    assert ctx.timing()["aggregate_launches"] == (2 if numD in (127, 63) else 4)
    rc, dw, vw = oracle.asw_classic(L, R, gc, gg, int(dt), 15, minD, numD, want_vol=True)
    assert rc == 0 and v.shape == vw.shape == (numD + 1, H, W)
    assert np.array_equal(v, vw, equal_nan=True), np.argwhere(v != vw)[:5]
    assert np.array_equal(d, dw), np.argwhere(d != dw)[:5]
    d0, v0 = ctx_old.computeAdaptiveWeight(L, R, gc, gg, dt, 15, minD, numD, return_cost_volume=True)
    assert np.array_equal(v, v0, equal_nan=True) and np.array_equal(d, d0)


@pytest.mark.parametrize("H,W,minD,numD", LEFT_CASES)
def test_tables_left(ctx, ctx_old, oracle, H, W, minD, numD):
    check(ctx, ctx_old, oracle, LEFT, H, W, minD, numD)


@pytest.mark.parametrize("H,W,minD,numD", RIGHT_CASES)
def test_tables_right(ctx, ctx_old, oracle, H, W, minD, numD):
    assert (W - 1) // 64 * 64 + minD <= W - 1
    check(ctx, ctx_old, oracle, RIGHT, H, W, minD, numD)


# a second gamma pair that bilateral_xq_lut_ok accepts (smallest weight product about 2^-20): other LUT contents, same classes
@pytest.mark.parametrize("dt,H,W,minD,numD", [(LEFT, 17, 330, 48, 128), (LEFT, 3, 130, 0, 64), (RIGHT, 17, 330, 9, 64),
                                              (RIGHT, 3, 96, 31, 128)])
def test_tables_second_gamma_pair(ctx, ctx_old, oracle, dt, H, W, minD, numD):
    check(ctx, ctx_old, oracle, dt, H, W, minD, numD, gc=45, gg=12)
