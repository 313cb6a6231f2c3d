"""Cross-based support-region aggregation on the GPU (selector entry 12, k_cross.hip) against the
restatement of tests/cross_ref.py.  Every sum is an integer and the one division is correctly rounded: every comparison is
np.array_equal, on the volume and on the map.  The raw cost handed to the restatement is ctx.computeAD's u8 volume for the same
direction (pinned to the oracle by the existing tests), so its border rule is not stated a second time.

This file holds what belongs to the method's own kernels; what every selector method owes its callers (forms and paths, batch,
sub-pixel, refined calls, statuses, the seeded sweep) is in tests/test_gpu_selector_contract.py.  What the region_pair
cases exercise (arms of length 0, between and L, tied minima) is asserted on the restatement alone in tests/test_cross_cpu.py."""
import os
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cross_ref as cr  # noqa: E402
from selector_methods import region_views as _pair  # noqa: E402

A = asw.StereoMatchingAlgorithms
LEFT, RIGHT = asw.DISPARITY_LEFT, asw.DISPARITY_RIGHT
CROSS = A.ADAPTIVE_WEIGHT_CROSS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


def _check(ctx, L, R, dt, tau, trunc, win, minD, D):
    e = np.stack(ctx.computeAD(L, R, dt, minD, D))
    S, N, E, disp = cr.aggregate(e, cr.arms(R if int(dt) else L, tau, win // 2), trunc, minD)
    got, vol = ctx.computeAdaptiveWeight_cross(L, R, dt, tau, trunc, win, minD, D, return_cost_volume=True)
    assert vol.shape == E.shape and np.array_equal(vol, E), np.argwhere(vol != E)[:5]
    assert np.array_equal(got, disp), np.argwhere(got != disp)[:5]
    # without a kept volume the running minimum inside the kernel is the argmin of the kept volume
    assert np.array_equal(ctx.computeAdaptiveWeight_cross(L, R, dt, tau, trunc, win, minD, D), disp)
    assert np.array_equal(disp, (np.argmin(vol, axis=0) + minD).astype(np.float32))
    return E, disp


# H, W, channels, win, minD, D, direction, tau, trunc
CASES = [
    (1, 1, 3, 3, 0, 1, LEFT, 20, 20),
    (1, 1, 3, 35, 3, 5, RIGHT, 20, 20),       # min_d + num_d > cols
    (1, 40, 3, 7, 0, 5, LEFT, 20, 20),
    (1, 40, 1, 15, 3, 17, RIGHT, 20, 255),
    (40, 1, 3, 7, 0, 1, LEFT, 20, 20),
    (40, 1, 3, 35, 0, 5, RIGHT, 0, 1),        # min_d + num_d > cols
    (3, 5, 3, 15, 3, 5, LEFT, 20, 20),        # a window larger than the frame, candidates past the image
    (3, 5, 3, 1, 0, 17, RIGHT, 255, 20),
    (7, 63, 3, 3, 0, 5, LEFT, 20, 20),        # one column short of a tile, a whole tile, one column more
    (7, 64, 3, 7, 3, 17, RIGHT, 20, 20),
    (7, 65, 3, 15, 0, 17, LEFT, 20, 1),
    (7, 65, 1, 35, 0, 5, RIGHT, 255, 255),
    (37, 130, 3, 1, 0, 5, LEFT, 20, 20),      # win 1: every region is its pixel
    (37, 130, 1, 15, 3, 17, LEFT, 0, 20),
    (33, 130, 3, 35, 0, 1, RIGHT, 255, 20),   # a band and one row; one candidate
    (65, 150, 3, 35, 3, 5, LEFT, 20, 255),
    (65, 150, 3, 3, 0, 17, RIGHT, 0, 1),
    (20, 301, 3, 15, 0, 17, LEFT, 20, 20),    # five tiles a row
    (20, 301, 3, 7, 3, 5, RIGHT, 0, 20),
    (20, 301, 3, 35, 0, 17, LEFT, 255, 20),
    (20, 301, 1, 35, 290, 17, RIGHT, 20, 20), # min_d + num_d > cols on a wide frame
]


@pytest.mark.parametrize("H,W,cn,win,minD,D,dt,tau,trunc", CASES)
def test_matches_restatement(ctx, H, W, cn, win, minD, D, dt, tau, trunc):
    L, R = _pair(H, W, cn, D)
    _check(ctx, L, R, dt, tau, trunc, win, minD, D)


@pytest.mark.parametrize("H,W,D,cell,seed,amp,win", cr.REGION_CASES)
@pytest.mark.parametrize("dt", [LEFT, RIGHT])
def test_region_cases(ctx, H, W, D, cell, seed, amp, win, dt):
    L, R, _ = cr.region_pair(H, W, D, seed, cell, amp)
    _check(ctx, L, R, dt, 20, 20, win, 0, D)


@pytest.mark.parametrize("H,W,cn,win,minD,D,dt", [(9, 70, 3, 7, 0, 5, LEFT), (34, 129, 1, 15, 3, 17, RIGHT), (5, 64, 3, 35, 0, 5, LEFT)])
def test_padded_row_views(ctx, H, W, cn, win, minD, D, dt):
    L, R = _pair(H, W, cn, D, pad=5)
    assert L.strides[0] > W * cn and not L.flags.c_contiguous
    E, disp = _check(ctx, L, R, dt, 20, 20, win, minD, D)
    assert np.array_equal(ctx.computeAdaptiveWeight_cross(np.ascontiguousarray(L), np.ascontiguousarray(R), dt, 20, 20, win, minD, D), disp)


# ---------------------------------------------------------------- one mid-size frame
def test_mid_size_frame_in_both_forms(ctx):
    """270 x 480, 64 candidates, win 15: the whole volume and map against the integral form; the literal form takes a quarter of a
    minute on this frame, so it is evaluated on every ninth row and the last (the two forms are compared pixel for pixel on whole
    frames in tests/test_cross_cpu.py).  Plain 12 and the encoded value, resident, without and with the volume."""
    H, W, D, win = 270, 480, 64, 15
    L, R, _ = cr.region_pair(H, W, D, 5, (25, 40), 0.12)
    e = np.stack(ctx.computeAD(L, R, LEFT, 0, D))
    a = cr.arms(L, 20, win // 2)
    S, N, E, disp = cr.aggregate(e, a, 20)
    rows = sorted(set(range(0, H, 9)) | {H - 1})
    S2, N2, E2, disp2 = cr.aggregate_loop(e, a, 20, rows=rows)
    assert np.array_equal(E[:, rows], E2[:, rows]) and np.array_equal(disp[rows], disp2[rows])
    ctx.upload_pair(25, L, R)
    ctx.match_resident(25, LEFT, CROSS, win, 0, D, keep_volume=False)
    assert np.array_equal(ctx.download_disparity(25, (H, W)), disp)
    ctx.match_resident(25, LEFT, asw.cross_algorithm(20, 20), win, 0, D, keep_volume=True)
    got, vol = ctx.download_disparity(25, (H, W)), ctx.download_volume(25, (D, H, W))
    assert np.array_equal(vol, E) and np.array_equal(got, disp)
    assert np.array_equal(vol[:, rows], E2[:, rows]) and np.array_equal(got[rows], disp2[rows])
