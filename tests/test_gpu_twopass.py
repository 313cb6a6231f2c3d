"""Two-pass (separable) adaptive-support-weight aggregation on the GPU (asw_alg_twopass over selector entry 2, k_twopass.hip,
DESIGN.md section 4.16) against the restatement of tests/twopass_ref.py.  The arithmetic is fixed completely, so every comparison
is np.array_equal, on the volume and on the map.  The gray pair handed to the restatement is ctx.bgr2gray of the inputs (pinned to
the oracle by the existing tests), so the conversion is not stated a second time.

This file holds what belongs to the method's own kernel and to the entry it is encoded over; what every selector method owes its
callers (forms and paths, batch, sub-pixel, refined calls, statuses, the seeded sweep) is in
tests/test_gpu_selector_contract.py.  That the tie-dense pairs really tie, and the window limit the statuses use, are asserted on the
restatement alone in tests/test_twopass_cpu.py."""
import os
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd._lib import AswError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import twopass_ref as tp  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import asw_oracle as O  # noqa: E402

A = asw.StereoMatchingAlgorithms
LEFT, RIGHT = asw.DISPARITY_LEFT, asw.DISPARITY_RIGHT
TOP = tp.max_window()

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


def _gray(ctx, img):
    return ctx.bgr2gray(img) if img.ndim == 3 else img


def _want(ctx, L, R, gammas, dt, win, minD, numD):
    """-> E f64, the volume, the map of the restatement"""
    return tp.twopass(_gray(ctx, L), _gray(ctx, R), gammas[0], gammas[1], win, minD, numD, int(dt))


def _check(ctx, L, R, gammas, dt, win, minD, numD):
    E, vol, disp = _want(ctx, L, R, gammas, dt, win, minD, numD)
    got, gv = ctx.computeAdaptiveWeight_twopass(L, R, gammas[0], gammas[1], dt, win, minD, numD, return_cost_volume=True)
    assert gv.shape == vol.shape and np.array_equal(gv, vol), np.argwhere(gv != vol)[:5]
    assert np.array_equal(got, disp), np.argwhere(got != disp)[:5]
    # without a kept volume: the same map, and the first strict minimum of the f64 E (not of the rounded volume)
    assert np.array_equal(ctx.computeAdaptiveWeight_twopass(L, R, gammas[0], gammas[1], dt, win, minD, numD), disp)
    best, bd = np.full(E.shape[1:], np.inf), np.zeros(E.shape[1:], np.float32)
    for k in range(E.shape[0]):
        lower = E[k] < best
        best, bd = np.where(lower, E[k], best), np.where(lower, np.float32(minD + k), bd)
    assert np.array_equal(disp, bd)
    return E, vol, disp


# H, W, channels, win, minD, numD, direction, gammas.  The kernel's tile is 64 columns x 4 rows (tp.ROW_TILE), its chunks are 8
# candidates wide with remainders 4 / 2 / 1: planes 2, 3, 5, 9, 17, 18, 33, 34 meet every chunk width and remainder
CASES = [
    (1, 1, 3, 3, 0, 1, LEFT, (30, 20)),
    (1, 1, 1, 35, 3, 4, RIGHT, (1, 1)),          # min_d + num_d > cols
    (1, 40, 3, 7, 0, 4, LEFT, (7, 36)),
    (1, 40, 1, 15, 3, 16, RIGHT, (30, 20)),
    (40, 1, 3, 7, 0, 1, LEFT, (255, 255)),
    (40, 1, 1, 35, 0, 4, RIGHT, (30, 20)),       # min_d + num_d > cols
    (3, 5, 3, 15, 3, 4, LEFT, (30, 20)),         # a window larger than the frame, candidates past the image
    (3, 5, 1, 1, 0, 16, RIGHT, (30, 20)),
    (3, 63, 3, 3, 0, 2, LEFT, (30, 20)),         # one column short of a tile, a whole tile, one column more; one row short ...
    (4, 64, 3, 7, 3, 17, RIGHT, (7, 36)),
    (5, 65, 1, 15, 0, 8, LEFT, (1, 1)),
    (7, 65, 3, 35, 0, 4, RIGHT, (255, 255)),
    (8, 64, 1, 3, 0, 33, LEFT, (30, 20)),
    (9, 130, 3, 1, 0, 4, LEFT, (30, 20)),        # win 1: E = |gL - gR|
    (9, 130, 1, 1, 3, 17, RIGHT, (1, 1)),
    (37, 130, 1, 15, 3, 17, LEFT, (30, 20)),
    (37, 130, 3, 35, 0, 17, RIGHT, (7, 36)),
    (33, 130, 3, 35, 0, 1, RIGHT, (30, 20)),
    (12, 150, 1, 7, 0, 32, LEFT, (255, 255)),
    (12, 150, 3, 15, 2, 33, RIGHT, (1, 1)),
    (65, 150, 3, 3, 0, 16, RIGHT, (255, 255)),
    (65, 301, 3, 15, 3, 2, LEFT, (30, 20)),
    (20, 301, 3, 15, 0, 17, LEFT, (7, 36)),      # five tiles a row
    (20, 301, 1, 7, 3, 8, RIGHT, (7, 36)),
    (20, 301, 3, 35, 0, 33, LEFT, (30, 20)),
    (20, 301, 1, 35, 290, 16, RIGHT, (1, 1)),    # min_d + num_d > cols on a wide frame
    (20, 301, 1, 15, 290, 17, LEFT, (30, 20)),
    (9, 130, 3, 25, 0, 8, LEFT, (30, 20)),       # 25 | 27: the dynamic-LDS opt-in above 64 KB
    (9, 130, 1, 27, 3, 8, RIGHT, (30, 20)),
    (6, 90, 3, TOP, 0, 4, LEFT, (30, 20)),       # the last served window
    (9, 130, 1, TOP, 3, 8, RIGHT, (255, 255)),
]


@pytest.mark.parametrize("H,W,cn,win,minD,numD,dt,gammas", CASES)
def test_matches_restatement(ctx, H, W, cn, win, minD, numD, dt, gammas):
    L, R = tp.textured_pair(H, W, cn, 3, H * 1000 + W)
    _check(ctx, L, R, gammas, dt, win, minD, numD)


@pytest.mark.parametrize("H,W,cn,win,minD,numD,dt", [(9, 70, 3, 7, 0, 4, LEFT), (34, 129, 1, 15, 3, 17, RIGHT), (5, 64, 3, 35, 0, 4, LEFT)])
def test_padded_row_views(ctx, H, W, cn, win, minD, numD, dt):
    Lp, Rp = tp.textured_pair(H, W + 5, cn, 3, 77)
    L, R = Lp[:, :W], Rp[:, :W]  # views whose rows carry padding
    assert L.strides[0] > W * cn and not L.flags.c_contiguous
    E, vol, disp = _check(ctx, L, R, (30, 20), dt, win, minD, numD)
    assert np.array_equal(ctx.computeAdaptiveWeight_twopass(np.ascontiguousarray(L), np.ascontiguousarray(R), 30, 20, dt, win, minD, numD), disp)


@pytest.mark.parametrize("name", ["periodic", "constant"])
@pytest.mark.parametrize("dt", [LEFT, RIGHT])
def test_tie_dense_pairs(ctx, name, dt):
    L, R, win, minD, numD = tp.tie_cases()[name]
    E, vol, disp = _check(ctx, L, R, (30, 20), dt, win, minD, numD)
    if name == "constant":
        assert (disp == minD).all()


def test_entry_2_is_unchanged_and_the_flag_is_not_a_no_op(ctx):
    H, W, numD, win = 20, 90, 8, 7
    L, R = tp.textured_pair(H, W, 3, 4, 43)
    for dt in (LEFT, RIGHT):
        rc, odisp, ovol = O.asw_classic(L, R, 30.0, 20.0, int(dt), win, 0, numD, want_vol=True)
        assert rc == 0
        two = ctx.stereoMatching(L, R, dt, asw.twopass_algorithm(30, 20), win, 0, numD, return_cost_volume=True)  # the table cache is warm
        d, v = ctx.stereoMatching(L, R, dt, A.ADAPTIVE_WEIGHT, win, 0, numD, return_cost_volume=True)
        assert np.array_equal(d, odisp) and np.array_equal(v, ovol)
        assert v.shape == two[1].shape and not np.array_equal(v, two[1])
        assert np.array_equal(two[1], _want(ctx, L, R, (30, 20), dt, win, 0, numD)[1])


def test_plain_entry_2_still_refuses_a_1_channel_pair(ctx):
    """the two-pass value serves 1-channel pairs (CASES); the plain entry it is encoded over does not"""
    g = np.ascontiguousarray(tp.textured_pair(20, 70, 3, 3, 8)[0][:, :, 1])
    with pytest.raises(AswError) as e:
        ctx.stereoMatching(g, g, LEFT, A.ADAPTIVE_WEIGHT, 15, 0, 12)
    assert e.value.status == asw.ERR_UNSUPPORTED_LAYOUT
