"""Wide rows on the GPU: k_cost_ad<C> (k_basic.hip) and k_cost_census<C> (k_census.hip) past 1024 columns -- the second and later
passes of their x4 loops -- and past 64 KB of dynamic LDS up to the 160 KB the launchers accept, the two matchers that rest on them
(entry 12 and AD-Census) at the workload's width and over 64 KB, and k_wta's three forms around 2^20 pixels.  The widths, the inputs
and the references are tests/wide_cases.py's; tests/test_wide_rows_cpu.py holds the table to its labels and the references to having
something to distinguish past column 1024.  Everything is an integer or one correctly rounded division: every comparison is
np.array_equal.

The references: the CPU oracle for computeAD / TAD / SD and winnerTakeAll, tests/adcensus_ref.py for the census builders and the
AD-Census matcher, tests/cross_ref.py over the ORACLE's AD volume for entry 12 (tests/test_gpu_cross.py feeds it ctx.computeAD by
design; here the raw cost is the thing under test).

Order: every launch that asks for at most 64 KB of LDS comes first; the launches between 64 KB and 160 KB follow: those
take the library's opt-in above 64 KB (ASW_LAUNCH); a refused launch would give status ERR_HIP, a failure here."""
import os
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd._lib import AswError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_cases as wc  # noqa: E402

LEFT, RIGHT = asw.DISPARITY_LEFT, asw.DISPARITY_RIGHT
CROSS = asw.StereoMatchingAlgorithms.ADAPTIVE_WEIGHT_CROSS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


def _same(got, want, what):
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    wide = bad[:, -1] >= wc.PASS_PIXELS
    pytest.fail("%s: %d of %d values differ, %d of them at x >= %d; the first five: %s" % (
        what, len(bad), want.size, int(wide.sum()), wc.PASS_PIXELS,
        ["%s (x %s %d) got %s want %s" % (tuple(int(v) for v in i), ">=" if w else "<", wc.PASS_PIXELS, got[tuple(i)], want[tuple(i)])
         for i, w in zip(bad[:5], wide[:5])]))


def _ids(case):
    return "-".join(map(str, case))


# ---------------------------------------------------------------- the cost builders
def _gpu_costs(ctx, kernel, L, R, dt, minD, D):
    if wc.is_ad_kernel(kernel):
        return {"AD": ctx.computeAD(L, R, dt, minD, D), "TAD": ctx.computeTAD(L, R, dt, wc.TAD_THRESHOLD, minD, D),
                "SD": ctx.computeSD(L, R, dt, minD, D)}
    out = {"Census": ctx.computeCensus(L, R, dt, minD, D)}
    if kernel != "hamming":
        out["ADCensus"] = ctx.computeADCensus(L, R, dt, wc.LAMBDA_AD, wc.LAMBDA_CENSUS, minD, D)
    return out


def _check_costs(ctx, oracle, kernel, L, R, dt, minD, D):
    want = wc.expected_costs(oracle, kernel, L, R, dt, minD, D)
    got = _gpu_costs(ctx, kernel, L, R, dt, minD, D)
    assert set(got) == set(want)
    for name in want:
        assert len(got[name]) == D
        _same(np.stack(got[name]), want[name], "compute%s %dx%d, %d channels, direction %d, min_d %d" % (
            name, L.shape[0], L.shape[1], 3 if L.ndim == 3 else 1, dt, minD))
    return got


@pytest.mark.parametrize("case", wc.COST_CASES_LOW, ids=_ids)
def test_cost_builders_passes(ctx, oracle, case):
    kernel, H, W, cn, dt, minD, D = case
    L, R = wc.cost_pair(H, W, cn, dt)
    _check_costs(ctx, oracle, kernel, L, R, dt, minD, D)


def test_cost_builders_padded_rows(ctx, oracle):
    H, W, cn, dt, minD, D, pad = wc.PADDED_CASE
    L, R = wc.cost_pair(H, W, cn, dt, pad=pad)
    assert L.strides[0] > W * cn and not L.flags.c_contiguous
    for kernel in ("ad", "census"):
        got = _check_costs(ctx, oracle, kernel, L, R, dt, minD, D)
        dense = _gpu_costs(ctx, kernel, np.ascontiguousarray(L), np.ascontiguousarray(R), dt, minD, D)
        for name in got:
            _same(np.stack(got[name]), np.stack(dense[name]), "compute%s, padded rows against dense rows" % name)


# ---------------------------------------------------------------- the matchers
def _check_adcensus(ctx, H, W, cn, win, minD, D, dt):
    L, R = wc.region_pair(H, W, cn, D)
    S, N, E, disp = wc.expected_adcensus(L, R, dt, win, minD, D)
    got, vol = ctx.computeAdaptiveWeight_adcensus(L, R, dt, wc.TAU, wc.LAMBDA_AD, wc.LAMBDA_CENSUS, win, minD, D, return_cost_volume=True)
    _same(vol, E, "AD-Census volume %dx%d" % (H, W))
    _same(got, disp, "AD-Census map %dx%d" % (H, W))
    _same(ctx.computeAdaptiveWeight_adcensus(L, R, dt, wc.TAU, wc.LAMBDA_AD, wc.LAMBDA_CENSUS, win, minD, D), disp,
          "AD-Census map without the kept volume %dx%d" % (H, W))


def _check_cross(ctx, oracle, H, W, cn, win, minD, D, dt):
    L, R = wc.region_pair(H, W, cn, D)
    S, N, E, disp = wc.expected_cross(oracle, L, R, dt, win, minD, D)
    got, vol = ctx.computeAdaptiveWeight_cross(L, R, dt, wc.TAU, wc.TRUNC, win, minD, D, return_cost_volume=True)
    _same(vol, E, "entry 12 volume %dx%d" % (H, W))
    _same(got, disp, "entry 12 map %dx%d" % (H, W))
    _same(ctx.computeAdaptiveWeight_cross(L, R, dt, wc.TAU, wc.TRUNC, win, minD, D), disp, "entry 12 map without the kept volume %dx%d" % (H, W))


@pytest.mark.parametrize("H,W,cn,win,minD,D,dt", wc.ADCENSUS_MATCH_LOW)
def test_adcensus_matcher_at_the_workload_width(ctx, H, W, cn, win, minD, D, dt):
    _check_adcensus(ctx, H, W, cn, win, minD, D, dt)


@pytest.mark.parametrize("H,W,cn,win,minD,D,dt", wc.CROSS_MATCH_LOW)
def test_cross_matcher_at_the_workload_width(ctx, oracle, H, W, cn, win, minD, D, dt):
    _check_cross(ctx, oracle, H, W, cn, win, minD, D, dt)


# ---------------------------------------------------------------- winnerTakeAll around 2^20 pixels
@pytest.mark.parametrize("H,W,form", wc.WTA_CASES)
def test_wta_forms(ctx, oracle, H, W, form):
    vol = wc.wta_volume(H, W, H)
    _same(ctx.winnerTakeAll(vol, 3), oracle.wta(vol, 3), "winnerTakeAll %dx%d (%s)" % (H, W, form))


# ---------------------------------------------------------------- launches between 64 KB and 160 KB of LDS
@pytest.mark.parametrize("case", wc.COST_CASES_HIGH, ids=_ids)
def test_cost_builders_at_the_64k_line(ctx, oracle, case):
    form, H, W, cn, dt, minD, D = case
    L, R = wc.cost_pair(H, W, cn, dt)
    _check_costs(ctx, oracle, form, L, R, dt, minD, D)


@pytest.mark.parametrize("form,H,accepted,refused,dt", wc.LIMIT_CASES)
def test_accepted_at_the_limit_refused_one_past_it(ctx, oracle, form, H, accepted, refused, dt):
    cn = wc.FORMS[form][2]
    L, R = wc.cost_pair(H, accepted, cn, dt)
    _check_costs(ctx, oracle, form, L, R, dt, wc.LIMIT_MIN_D, wc.LIMIT_NUM_D)
    L, R = wc.cost_pair(H, refused, cn, dt)
    if wc.is_ad_kernel(form):
        calls = [lambda: ctx.computeAD(L, R, dt, wc.LIMIT_MIN_D, wc.LIMIT_NUM_D), lambda: ctx.computeSD(L, R, dt, wc.LIMIT_MIN_D, wc.LIMIT_NUM_D),
                 lambda: ctx.computeTAD(L, R, dt, wc.TAD_THRESHOLD, wc.LIMIT_MIN_D, wc.LIMIT_NUM_D)]
    elif form == "hamming":
        calls = [lambda: ctx.computeCensus(L, R, dt, wc.LIMIT_MIN_D, wc.LIMIT_NUM_D)]
    else:
        calls = [lambda: ctx.computeADCensus(L, R, dt, wc.LAMBDA_AD, wc.LAMBDA_CENSUS, wc.LIMIT_MIN_D, wc.LIMIT_NUM_D)]
    for call in calls:
        with pytest.raises(AswError) as e:
            call()
        assert e.value.status == asw.ERR_BAD_ARGUMENT, (form, refused, e.value.status)
    # and the context serves the accepted width again
    L, R = wc.cost_pair(H, accepted, cn, dt)
    _check_costs(ctx, oracle, form, L, R, dt, wc.LIMIT_MIN_D, wc.LIMIT_NUM_D)


@pytest.mark.parametrize("H,W,cn,win,minD,D,dt", wc.ADCENSUS_MATCH_HIGH)
def test_adcensus_matcher_over_64k(ctx, H, W, cn, win, minD, D, dt):
    _check_adcensus(ctx, H, W, cn, win, minD, D, dt)


@pytest.mark.parametrize("H,W,cn,win,minD,D,dt", wc.CROSS_MATCH_HIGH)
def test_cross_matcher_over_64k(ctx, oracle, H, W, cn, win, minD, D, dt):
    _check_cross(ctx, oracle, H, W, cn, win, minD, D, dt)


def test_selector_refuses_past_the_limit_and_serves_the_next_call(ctx, oracle):
    ok = (6, 1028, 3, 7, 0, 5)
    for alg, form in ((asw.adcensus_algorithm(), "adcensus3"), (int(CROSS), "ad3")):
        W = wc.LINE_160K[form][1]
        assert (alg, W) in ((asw.adcensus_algorithm(), 7433), (12, 27307))
        L, R = wc.cost_pair(2, W, 3, 0)
        for dt in (LEFT, RIGHT):
            with pytest.raises(AswError) as e:
                ctx.stereoMatching(L, R, dt, alg, 7, 0, 2)
            assert e.value.status == asw.ERR_BAD_ARGUMENT, (hex(alg), W, e.value.status)
            with pytest.raises(AswError) as e:
                ctx.stereoMatching(L, R, dt, alg, 7, 0, 2, return_cost_volume=True)
            assert e.value.status == asw.ERR_BAD_ARGUMENT
        # a following valid call on the same context
        H, W, cn, win, minD, D = ok
        L, R = wc.region_pair(H, W, cn, D)
        for dt in (LEFT, RIGHT):
            if form == "ad3":
                S, N, E, disp = wc.expected_cross(oracle, L, R, int(dt), win, minD, D)
            else:
                S, N, E, disp = wc.expected_adcensus(L, R, int(dt), win, minD, D)
            got, vol = ctx.stereoMatching(L, R, dt, alg, win, minD, D, return_cost_volume=True)
            _same(vol, E, "volume after a refused call, algorithm %#x" % alg)
            _same(got, disp, "map after a refused call, algorithm %#x" % alg)
