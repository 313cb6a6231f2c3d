"""The interior xq kernels issue a row's LDS reads ahead of their use (k_bilateral_xq.hip, run_step): the head of a row -- grays,
right weights, the first left-weight quad -- is read during the previous row's last block and carried across the rows of a loop
body, the loop's back edge and the mid-step commit, and the left-weight quads rotate one or two blocks ahead.  Volume and disparity
bit for bit against the oracle and against the one-kernel path (ASW_BILATERAL_XQ=0), both directions, at the smallest shapes at
which a carried or early read can go wrong:
  H = 3: every window row clamped; H = 17: rows with and without the clamp
  W = 96, 130: one interior tile beside a border tile; W = 330: several interior tiles
  numD 128 / 64: the unit's wavefront, 8 / 4 wavefronts; 127 / 63: no tail; 130: a tail
  minD 0 and the largest admissible (48 LEFT; x0_last + minD = W - 1 RIGHT): wave 0's wrapped second reads are live
Images: noise (every row and column differs); a row-coded pair (another ramp in every image row, in both images: a head taken a
row early or late, or a weight quad of the wrong row, changes every cost and weight of the row); a column-coded pair (gray a
function of the column alone: the tap columns' weights differ, so a quad from the wrong ring slot or right buffer shows)."""
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


def gray3(g):
    return np.repeat(g.astype(np.uint8)[:, :, None], 3, axis=2)


def noise_pair(H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W, 3)).astype(np.uint8), rng.integers(0, 256, (H, W, 3)).astype(np.uint8)


def row_coded_pair(H, W, seed):
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    return gray3(((2 * y + 1) * x + 37 * y + seed) % 256), gray3(((2 * y + 3) * x + 91 * y + 5 + seed) % 256)


def column_coded_pair(H, W, seed):
    x = np.arange(W)[None, :] + np.zeros((H, 1), dtype=np.int64)
    return gray3((x * 37 + seed) % 251), gray3((x * 53 + 11 + seed) % 241)


PAIRS = {"noise": noise_pair, "rows": row_coded_pair, "cols": column_coded_pair}


def right_max_mind(W):
    return W - 1 - (W - 1) // 64 * 64  # x0_last + minD = W - 1


# (H, W, minD, numD): every H, W, numD and both minD of the list above, in both directions
LEFT_CASES = [(17, 330, 0, 128), (17, 330, 48, 128), (3, 330, 48, 64), (17, 330, 0, 64), (3, 330, 0, 127), (17, 330, 48, 63),
              (17, 330, 5, 130), (17, 96, 0, 128), (3, 96, 48, 64), (17, 96, 48, 127), (17, 130, 48, 128), (3, 130, 0, 63),
              (17, 130, 0, 64), (3, 130, 48, 130)]
RIGHT_CASES = [(17, 330, right_max_mind(330), 128), (3, 330, right_max_mind(330), 64), (17, 330, 0, 64), (17, 330, 0, 128),
               (3, 330, 0, 63), (17, 330, right_max_mind(330), 130), (17, 330, right_max_mind(330), 127),
               (17, 96, right_max_mind(96), 128), (3, 96, right_max_mind(96), 64), (17, 96, 0, 63),
               (17, 130, right_max_mind(130), 64), (3, 130, right_max_mind(130), 127), (17, 130, 0, 128), (3, 130, 0, 130)]
# noise and the column code on the shapes with the most interior tiles and on one of each narrow width; the row code on all
SHORT = [0, 1, 2, 6, 8, 10]


def check(ctx, ctx_old, oracle, kind, dt, H, W, minD, numD):
    L, R = PAIRS[kind](H, W, ((H * 1000 + W) * 100 + minD) * 1000 + numD + int(dt))
    d, v = ctx.computeAdaptiveWeight(L, R, 30, 20, dt, 15, minD, numD, return_cost_volume=True)
    # the xq kernels served the call: two launches without a tail, four with one
    assert ctx.timing()["aggregate_launches"] == (2 if numD in (127, 63) else 4)
    rc, dw, vw = oracle.asw_classic(L, R, 30, 20, int(dt), 15, minD, numD, want_vol=True)
    assert rc == 0 and v.shape == vw.shape == (numD + 1, H, W)
    assert np.array_equal(v, vw, equal_nan=True), np.argwhere(v != vw)[:5]
    assert np.array_equal(d, dw), np.argwhere(d != dw)[:5]
    d0, v0 = ctx_old.computeAdaptiveWeight(L, R, 30, 20, dt, 15, minD, numD, return_cost_volume=True)
    assert np.array_equal(v, v0, equal_nan=True) and np.array_equal(d, d0)


@pytest.mark.parametrize("H,W,minD,numD", LEFT_CASES)
def test_prefetch_row_coded_left(ctx, ctx_old, oracle, H, W, minD, numD):
    check(ctx, ctx_old, oracle, "rows", LEFT, H, W, minD, numD)


@pytest.mark.parametrize("H,W,minD,numD", RIGHT_CASES)
def test_prefetch_row_coded_right(ctx, ctx_old, oracle, H, W, minD, numD):
    assert (W - 1) // 64 * 64 + minD <= W - 1
    check(ctx, ctx_old, oracle, "rows", RIGHT, H, W, minD, numD)


@pytest.mark.parametrize("kind", ["noise", "cols"])
@pytest.mark.parametrize("H,W,minD,numD", [LEFT_CASES[i] for i in SHORT])
def test_prefetch_left(ctx, ctx_old, oracle, kind, H, W, minD, numD):
    check(ctx, ctx_old, oracle, kind, LEFT, H, W, minD, numD)


@pytest.mark.parametrize("kind", ["noise", "cols"])
@pytest.mark.parametrize("H,W,minD,numD", [RIGHT_CASES[i] for i in SHORT])
def test_prefetch_right(ctx, ctx_old, oracle, kind, H, W, minD, numD):
    check(ctx, ctx_old, oracle, kind, RIGHT, H, W, minD, numD)
