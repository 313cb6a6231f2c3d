"""AD-Census matching on the GPU (k_census.hip in front of entry 12's kernels) against the restatement of
tests/adcensus_ref.py.  Every number before the one correctly rounded division is an integer: every comparison is np.array_equal,
on the two cost builders, on the aggregated volume and on the map.

This file holds what belongs to the method's own kernels; what every selector method owes its callers (forms and paths, batch,
sub-pixel, refined calls, statuses, the seeded sweep) is in tests/test_gpu_selector_contract.py.  What the pairs exercise
(Hamming distances from 0 to 62, costs above 127, winners the AD term alone would not pick) and the margin of the two tables are
asserted on the restatement alone in tests/test_adcensus_cpu.py."""
import os
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd._lib import AswError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adcensus_ref as ac  # noqa: E402
import cross_ref as cr  # noqa: E402
from selector_methods import region_views as _pair  # noqa: E402

LEFT, RIGHT = asw.DISPARITY_LEFT, asw.DISPARITY_RIGHT
ADC = asw.adcensus_algorithm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- the two cost builders
def _check_costs(ctx, L, R, dt, minD, D, la=10, lc=30):
    ham = np.stack(ctx.computeCensus(L, R, dt, minD, D))
    want = ac.hamming(L, R, dt, minD, D)
    assert ham.dtype == np.uint8 and ham.shape == want.shape and np.array_equal(ham, want), np.argwhere(ham != want)[:5]
    e = np.stack(ctx.computeADCensus(L, R, dt, la, lc, minD, D))
    want = ac.cost(L, R, dt, la, lc, minD, D)
    assert e.dtype == np.uint8 and np.array_equal(e, want), np.argwhere(e != want)[:5]
    return ham, e


SHAPES = [(1, 1), (1, 3), (2, 4), (3, 5), (4, 9), (7, 63), (7, 64), (7, 65), (9, 130), (20, 301)]
# per shape: channels, direction, minD, D -- every D of {1, 16, 17}, both minD, both directions and channel counts occur
VARIANTS = [(3, LEFT, 0, 17), (1, RIGHT, 3, 16), (3, RIGHT, 0, 1), (1, LEFT, 3, 17), (3, LEFT, 3, 16)]


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_cost_builders(ctx, i):
    H, W = SHAPES[i]
    for j in (0, 1):
        cn, dt, minD, D = VARIANTS[(i + 2 * j) % len(VARIANTS)]
        L, R = _pair(H, W, cn, D)
        _check_costs(ctx, L, R, dt, minD, D, *((10, 30), (5, 12))[j])


def test_cost_builders_repeated_reflection_padded_rows_and_flat_pair(ctx):
    for dt in (LEFT, RIGHT):
        L, R = _pair(9, 130, 3, 17)
        _check_costs(ctx, L, R, dt, 125, 17)   # min_d + num_d > cols
        L, R = _pair(3, 5, 1, 17)
        _check_costs(ctx, L, R, dt, 3, 17)     # every partner column reflected, some more than once
    L, R = _pair(7, 65, 3, 5, pad=5)
    assert L.strides[0] > 65 * 3 and not L.flags.c_contiguous
    ham, e = _check_costs(ctx, L, R, LEFT, 0, 5)
    assert np.array_equal(ham, np.stack(ctx.computeCensus(np.ascontiguousarray(L), np.ascontiguousarray(R), LEFT, 0, 5)))
    flat = np.full((9, 70, 3), 77, np.uint8)
    other = np.full((9, 70, 3), 90, np.uint8)
    ham, e = _check_costs(ctx, flat, other, RIGHT, 0, 4)
    assert not ham.any() and (e == ac.tables(10, 30)[0][13]).all()
    # the module-level bindings and their defaults
    L, R = _pair(7, 65, 3, 5)
    assert np.array_equal(np.stack(asw.computeCensus(L, R)), ac.hamming(L, R, 0, 0, 30))
    assert np.array_equal(np.stack(asw.computeADCensus(L, R)), ac.cost(L, R, 0, 10, 30, 0, 30))


def test_cost_builder_statuses(ctx):
    L, R = _pair(8, 20, 3, 4)
    for call in (lambda **k: ctx.computeCensus(L, R, **k), lambda **k: ctx.computeADCensus(L, R, **k)):
        for kw in ({"numDisparity": 0}, {"minDisparity": -1}, {"dispType": 2}):
            with pytest.raises(AswError) as e:
                call(**kw)
            assert e.value.status == asw.ERR_BAD_ARGUMENT
    for la, lc in ((0, 30), (256, 30), (10, 0), (10, 256)):
        with pytest.raises(AswError) as e:
            ctx.computeADCensus(L, R, LEFT, la, lc, 0, 4)
        assert e.value.status == asw.ERR_BAD_ARGUMENT
    # the builders travel in asw_cost_tad's threshold from bit 30 up: stray bits 16-29 or exactly one lambda are refused, and a
    # threshold below 2^30 is the TAD mask it was
    for thr in (0x40000000 | 0x20000 | (10 << 8) | 30, 0x40000000 | 0x20000000, 0x40000000 | 30, 0x40000000 | (10 << 8)):
        with pytest.raises(AswError) as e:
            ctx.computeTAD(L, R, LEFT, thr, 0, 4)
        assert e.value.status == asw.ERR_BAD_ARGUMENT
    ad = np.stack(ctx.computeAD(L, R, LEFT, 0, 4))
    for thr in (-5, 30, 255, 0x3FFFFFFF):
        assert np.array_equal(np.stack(ctx.computeTAD(L, R, LEFT, thr, 0, 4)), np.where(ad.astype(np.int64) > thr, 255, 0).astype(np.uint8))
    two = np.zeros((8, 20, 2), np.uint8)
    with pytest.raises(AswError) as e:
        ctx.computeCensus(two, two, LEFT, 0, 4)
    assert e.value.status == asw.ERR_UNSUPPORTED_LAYOUT
    assert ctx.computeADCensus(L, R[:, :19], LEFT, 10, 30, 0, 4) == [] and asw.last_status() == asw.ERR_SIZE_MISMATCH
    assert np.array_equal(np.stack(ctx.computeADCensus(L, R, LEFT, 255, 255, 0, 4)), ac.cost(L, R, 0, 255, 255, 0, 4))


# ---------------------------------------------------------------- the matcher
def _check(ctx, L, R, dt, tau, la, lc, win, minD, D):
    S, N, E, disp = ac.match(L, R, int(dt), tau, la, lc, win, minD, D)
    got, vol = ctx.computeAdaptiveWeight_adcensus(L, R, dt, tau, la, lc, win, minD, D, return_cost_volume=True)
    assert vol.shape == E.shape and np.array_equal(vol, E), np.argwhere(vol != E)[:5]
    assert np.array_equal(got, disp), np.argwhere(got != disp)[:5]
    assert np.array_equal(ctx.computeAdaptiveWeight_adcensus(L, R, dt, tau, la, lc, win, minD, D), disp)  # without the kept volume
    return E, disp


def test_win_1_volume_is_the_raw_cost(ctx):
    for cn, dt in ((3, LEFT), (1, RIGHT)):
        L, R = _pair(20, 70, cn, 9)
        d, v = ctx.computeAdaptiveWeight_adcensus(L, R, dt, 20, 10, 30, 1, 2, 9, return_cost_volume=True)
        e = np.stack(ctx.computeADCensus(L, R, dt, 10, 30, 2, 9))
        assert np.array_equal(v, e.astype(np.float32)) and np.array_equal(v, ac.cost(L, R, int(dt), 10, 30, 2, 9).astype(np.float32))
        assert np.array_equal(d, (np.argmin(e, axis=0) + 2).astype(np.float32))


@pytest.mark.parametrize("H,W,D,cell,seed,amp,win", cr.REGION_CASES)
@pytest.mark.parametrize("dt", [LEFT, RIGHT])
def test_region_cases(ctx, H, W, D, cell, seed, amp, win, dt):
    L, R, _ = cr.region_pair(H, W, D, seed, cell, amp)
    _check(ctx, L, R, dt, 20, 10, 30, win, 0, D)


# H, W, channels, win, minD, D, direction, tau, lambda_ad, lambda_census
CASES = [
    (1, 1, 3, 3, 0, 1, LEFT, 20, 10, 30),
    (1, 40, 1, 7, 3, 5, RIGHT, 20, 1, 1),
    (40, 1, 3, 15, 0, 5, LEFT, 0, 31, 255),       # min_d + num_d > cols
    (3, 5, 3, 15, 3, 5, RIGHT, 20, 10, 30),       # a window larger than the frame, candidates past the image
    (7, 65, 1, 35, 0, 17, LEFT, 255, 31, 255),
    (33, 130, 3, 35, 0, 16, RIGHT, 255, 1, 1),
    (20, 301, 3, 15, 3, 17, LEFT, 0, 10, 30),
    (20, 301, 1, 7, 290, 17, RIGHT, 20, 10, 30),  # min_d + num_d > cols on a wide frame
]


@pytest.mark.parametrize("H,W,cn,win,minD,D,dt,tau,la,lc", CASES)
def test_matches_restatement(ctx, H, W, cn, win, minD, D, dt, tau, la, lc):
    L, R = _pair(H, W, cn, D)
    _check(ctx, L, R, dt, tau, la, lc, win, minD, D)


def test_padded_row_views(ctx):
    L, R = _pair(34, 129, 3, 17, pad=5)
    assert L.strides[0] > 129 * 3 and not L.flags.c_contiguous
    E, disp = _check(ctx, L, R, RIGHT, 20, 10, 30, 15, 3, 17)
    assert np.array_equal(ctx.computeAdaptiveWeight_adcensus(np.ascontiguousarray(L), np.ascontiguousarray(R), RIGHT, 20, 10, 30, 15, 3, 17), disp)


def test_gray_bits(ctx):
    H, W, D, cell, seed, amp, win = cr.REGION_CASES[1]
    L, R, _ = cr.region_pair(H, W, D, seed, cell, amp)
    assert not np.array_equal(ac.hamming(L, R, 0, 0, D, 14), ac.hamming(L, R, 0, 0, D, 15))
    fresh = asw.Context(0)
    try:
        fresh.set_gray_bits(15)
        assert np.array_equal(np.stack(fresh.computeCensus(L, R, LEFT, 0, D)), ac.hamming(L, R, 0, 0, D, 15))
        d, v = fresh.stereoMatching(L, R, LEFT, ADC(), win, 0, D, return_cost_volume=True)
        S, N, E, disp = ac.match(L, R, 0, 20, 10, 30, win, 0, D, bits=15)
        assert np.array_equal(v, E) and np.array_equal(d, disp)
    finally:
        fresh.close()


# ---------------------------------------------------------------- one mid-size frame
def test_mid_size_frame(ctx):
    """270 x 480, 64 candidates, win 15, resident: the map without the volume, then the volume and the map"""
    H, W, D, win = 270, 480, 64, 15
    L, R, _ = cr.region_pair(H, W, D, 5, (25, 40), 0.12)
    S, N, E, disp = ac.match(L, R, 0, 20, 10, 30, win, 0, D)
    ctx.upload_pair(35, L, R)
    ctx.match_resident(35, LEFT, ADC(), win, 0, D, keep_volume=False)
    assert np.array_equal(ctx.download_disparity(35, (H, W)), disp)
    ctx.match_resident(35, LEFT, ADC(), win, 0, D, keep_volume=True)
    got, vol = ctx.download_disparity(35, (H, W)), ctx.download_volume(35, (D, H, W))
    assert np.array_equal(vol, E) and np.array_equal(got, disp)
