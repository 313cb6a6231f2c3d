"""Cross-scale cost aggregation on the GPU (asw_disparity_cross_scale() in disparity_type; k_cross_scale.hip).

The expectation is built from existing entry points and the restatement of tests/cross_scale_ref.py: the pair is halved in numpy
(down2), every scale's volume comes from a plain stereoMatching call of a SECOND context on that scale's pair and candidate range,
and combine / wta give the volume and the map.  The arithmetic is fixed completely, so volume and map are compared with
np.array_equal (NaN slots, which some methods produce, must sit in the same places).

A flag that did nothing would pass wherever the combined volume happens to equal the finest one, so every comparison also asserts
that the returned volume differs from the plain finest-scale volume.  The exemptions (must_differ): a case whose EXPECTED volume
itself equals the plain one AND whose frame has at most 16 pixels (a 1x1 frame has the same pixel on every level and the weights
sum to 1) or whose plain volume has no finite entry (entry 2 at window 1 is 0 / 0 everywhere).  The seeded sweep draws frames
narrower than their candidates as well and states its own rule where it asserts."""
import os
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib
from aswstereomatch_amd._lib import AswError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asw_cases  # noqa: E402
import cross_scale_ref as cs  # noqa: E402
import subpixel_ref as sp  # noqa: E402

A = asw.StereoMatchingAlgorithms
LEFT, RIGHT = asw.DISPARITY_LEFT, asw.DISPARITY_RIGHT
P, E = asw.SUBPIXEL_PARABOLA, asw.SUBPIXEL_EQUIANGULAR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx2():
    """the context the per-scale volumes come from: it shares no call history with the context under test"""
    c = asw.Context(0)
    yield c
    c.close()


def _planes(alg, D):
    return _lib.lib().asw_volume_planes(int(alg), D)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def must_differ(L, vol, plain):
    return not same(vol, plain) or (L.shape[0] * L.shape[1] > 16 and np.isfinite(plain).any())


def expected(ctx2, L, R, dt, alg, win, minD, numD, S, q):
    """-> (combined volume, its winner-take-all map, the plain finest-scale volume)"""
    n = _planes(alg, numD)
    ranges = cs.scale_ranges(minD, n, n - numD, S)
    vols = []
    for s, (Ls, Rs) in enumerate(zip(cs.pyramid(L, S), cs.pyramid(R, S))):
        d, v = ctx2.stereoMatching(Ls, Rs, dt, alg, win, ranges[s][0], ranges[s][2], return_cost_volume=True)
        assert v.shape == (ranges[s][1],) + Ls.shape[:2]
        vols.append(v)
    vol = cs.combine(vols, minD, cs.weights(S, q))
    return vol, cs.wta(vol, minD), vols[0]


def check(ctx, ctx2, L, R, dt, alg, win, minD, numD, S=3, q=19):
    vol, disp, plain = expected(ctx2, L, R, dt, alg, win, minD, numD, S, q)
    flag = asw.cross_scale(S, q)
    d1, v1 = ctx.stereoMatching(L, R, dt, alg, win, minD, numD, return_cost_volume=True, cross_scale=flag)
    assert same(v1, vol), np.argwhere(~((v1 == vol) | (np.isnan(v1) & np.isnan(vol))))[:5]
    assert np.array_equal(d1, disp), np.argwhere(d1 != disp)[:5]
    assert np.array_equal(ctx.stereoMatching(L, R, int(dt) | flag, alg, win, minD, numD), disp)  # no kept volume: the same map
    if must_differ(L, vol, plain):
        assert not same(v1, plain)
    return vol, disp, plain


# ---- every method, both directions where it serves both ----
# name -> (selector value, DISPARITY_RIGHT served, window, minD)
METHODS = {
    "classic": (A.ADAPTIVE_WEIGHT, True, 5, 3), "direct8": (A.ADAPTIVE_WEIGHT_8DIRECT, False, 5, 1),
    "geodesic": (A.ADAPTIVE_WEIGHT_GEODESIC, True, 5, 1), "bilgrid": (A.ADAPTIVE_WEIGHT_BILATERAL_GRID, False, 1, 3),
    "blo1": (A.ADAPTIVE_WEIGHT_BLO1, True, 5, 0), "guided": (A.ADAPTIVE_WEIGHT_GUIDED_FILTER, True, 5, 3),
    "guided2": (A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2, False, 5, 6), "wmedian": (A.ADAPTIVE_WEIGHT_MEDIAN, False, 3, 1),
    "cross": (A.ADAPTIVE_WEIGHT_CROSS, True, 7, 3), "twopass": (asw.twopass_algorithm(), True, 7, 1),
    "cross_params": (asw.cross_algorithm(), True, 7, 6), "adcensus": (asw.adcensus_algorithm(), True, 7, 3),
    "permeability": (asw.permeability_algorithm(), True, 1, 1),
}


@pytest.mark.parametrize("method", list(METHODS))
def test_methods(ctx, ctx2, method):
    alg, right, win, minD = METHODS[method]
    H, W, numD = 21, 66, 13
    L, R = cs.textured_pair(H, W, 3, minD + 4, 11)
    for dt in (LEFT, RIGHT) if right else (LEFT,):
        check(ctx, ctx2, L, R, dt, alg, win, minD, numD)


@pytest.mark.parametrize("method", ["blo1", "cross", "twopass", "permeability", "bilgrid"])
def test_gray_pairs(ctx, ctx2, method):
    alg, right, win, minD = METHODS[method]
    L, R = cs.textured_pair(13, 37, 1, minD + 2, 12)
    check(ctx, ctx2, L, R, LEFT, alg, win, minD, 9, S=4, q=64)


# ---- shapes: tiny frames, odd and even sizes on every level down to one pixel, W mod 4, both sides of 64 columns (the 16-byte form
# starts there) and of a workgroup's 256 columns ----
SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 3), (16, 16), (11, 13), (7, 31), (5, 60), (5, 63), (5, 64), (5, 65), (5, 66), (5, 67),
          (5, 68), (3, 252), (3, 256), (3, 260), (2, 516)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes(ctx, ctx2, H, W):
    L, R = cs.textured_pair(H, W, 3, 5, H * 1000 + W)
    check(ctx, ctx2, L, R, LEFT, A.ADAPTIVE_WEIGHT, 3, 1, 19, S=5, q=19)       # 20 planes, 1..20: two are left on the coarsest scale
    check(ctx, ctx2, L, R, RIGHT, A.ADAPTIVE_WEIGHT_CROSS, 5, 3, 7, S=5, q=64)  # 7 planes: fewer than 2^s from s = 3 up


# ---- candidate ranges: groups that start unaligned on every scale, n no multiple of 2^s ----
@pytest.mark.parametrize("minD", [0, 1, 3, 6])
@pytest.mark.parametrize("S", [2, 3, 4, 5])
def test_ranges(ctx, ctx2, minD, S):
    L, R = cs.textured_pair(9, 68, 3, minD + 3, 40 + minD)
    for numD in (1, 5, 11, 18):
        check(ctx, ctx2, L, R, LEFT, A.ADAPTIVE_WEIGHT_CROSS, 5, minD, numD, S=S)
    check(ctx, ctx2, L[:, :37], R[:, :37], LEFT, asw.twopass_algorithm(), 5, minD, 18, S=S)  # the scalar form, an inclusive range


@pytest.mark.parametrize("S", [2, 3, 4, 5])
@pytest.mark.parametrize("minD", [0, 3])
def test_smallest_range_and_one_less(ctx, ctx2, S, minD):
    L, R = cs.textured_pair(8, 40, 3, 4, 50 + S)
    numD = 1  # entry 2 keeps numD + 1 planes: every scale must be left with two
    while cs.scale_ranges(minD, numD + 1, 1, S) is None:
        numD += 1
    # minD 0: the last candidate numD must reach 2^(S-1); minD 3: candidates 3 and 4 already sit on two planes of scales 1 and 2,
    # and from scale 3 up the last candidate 3 + numD must reach 2^(S-1)
    assert numD == ({2: 2, 3: 4, 4: 8, 5: 16}[S] if minD == 0 else {2: 1, 3: 1, 4: 5, 5: 13}[S])
    check(ctx, ctx2, L, R, LEFT, A.ADAPTIVE_WEIGHT, 3, minD, numD, S=S)
    with pytest.raises(AswError) as e:  # one less: refused by the range rule (or, at 0, as any call without candidates)
        ctx.stereoMatching(L, R, LEFT, A.ADAPTIVE_WEIGHT, 3, minD, numD - 1, cross_scale=asw.cross_scale(S))
    assert e.value.status == asw.ERR_BAD_ARGUMENT
    if numD > 1:
        assert cs.scale_ranges(minD, numD, 1, S) is None
        assert ctx.stereoMatching(L, R, LEFT, A.ADAPTIVE_WEIGHT, 3, minD, numD - 1).shape == (8, 40)  # the plain call serves that range
    check(ctx, ctx2, L, R, LEFT, A.ADAPTIVE_WEIGHT_CROSS, 3, minD, 1, S=S)  # an exclusive range: one plane is enough on every scale


# ---- parameters ----
@pytest.mark.parametrize("S", [2, 3, 4, 5])
@pytest.mark.parametrize("q", [1, 19, 64, 255])
def test_parameters(ctx, ctx2, S, q):
    L, R = cs.textured_pair(14, 72, 3, 6, 60)
    vol, disp, plain = check(ctx, ctx2, L, R, LEFT, A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2, 5, 2, 20, S=S, q=q)
    check(ctx, ctx2, L[:, :50], R[:, :50], RIGHT, A.ADAPTIVE_WEIGHT, 5, 2, 20, S=S, q=q)
    other = ctx.stereoMatching(L, R, LEFT, A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2, 5, 2, 20, return_cost_volume=True,
                               cross_scale=asw.cross_scale(S, q + 1 if q < 255 else 254))[1]
    assert not same(other, vol)  # lambda reaches the volume
    if S == 3 and q == 19:
        assert same(ctx.stereoMatching(L, R, LEFT, A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2, 5, 2, 20, return_cost_volume=True,
                                       cross_scale=asw.cross_scale())[1], vol)  # the defaults


# ---- with a sub-pixel flag: the step runs on the combined volume ----
@pytest.mark.parametrize("method", ["classic", "cross", "guided2"])
def test_subpixel_on_the_combined_volume(ctx, ctx2, method):
    alg, right, win, minD = METHODS[method]
    L, R = cs.textured_pair(20, 70, 3, minD + 5, 70)
    vol, disp, plain = expected(ctx2, L, R, LEFT, alg, win, minD, 12, 3, 19)
    flag = asw.cross_scale()
    for mode in (P, E):
        want, ok = sp.subpixel_vec(disp, vol, minD, mode)
        assert ok.mean() >= 0.2 and not np.array_equal(want, disp)
        d1, v1 = ctx.stereoMatching(L, R, LEFT, alg, win, minD, 12, return_cost_volume=True, subpixel=mode, cross_scale=flag)
        assert same(v1, vol) and not same(v1, plain)
        assert np.array_equal(d1, want), np.argwhere(d1 != want)[:5]
        assert np.array_equal(ctx.stereoMatching(L, R, int(LEFT) | mode | flag, alg, win, minD, 12), want)  # no kept volume
        assert not np.array_equal(want, sp.subpixel_vec(cs.wta(plain, minD), plain, minD, mode)[0])


# ---- call forms ----
def test_per_method_entry_points_take_the_flag(ctx, ctx2):
    H, W, D = 15, 66, 10
    L, R = cs.textured_pair(H, W, 3, 4, 80)
    calls = [
        (A.ADAPTIVE_WEIGHT, 5, lambda dt, **k: ctx.computeAdaptiveWeight(L, R, 30, 20, dt, 5, 0, D, **k)),
        (A.ADAPTIVE_WEIGHT_8DIRECT, 5, lambda dt, **k: ctx.computeAdaptiveWeight_direct8(L, R, dt, 5, 0, D, **k)),
        (A.ADAPTIVE_WEIGHT_GEODESIC, 5, lambda dt, **k: ctx.computeAdaptiveWeight_geodesic(L, R, dt, 5, 0, D, **k)),
        (A.ADAPTIVE_WEIGHT_GUIDED_FILTER, 5, lambda dt, **k: ctx.computeAdaptiveWeight_GuidedF(L, R, dt, 1e-6, 5, 0, D, **k)),
        (A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2, 5, lambda dt, **k: ctx.computeAdaptiveWeight_GuidedF_2(L, R, dt, 1e-6, 5, 0, D, **k)),
        (A.ADAPTIVE_WEIGHT_BLO1, 5, lambda dt, **k: ctx.computeAdaptiveWeight_BLO1(L, R, dt, 0.015, 5, 0, D, **k)),
        (A.ADAPTIVE_WEIGHT_BILATERAL_GRID, 1, lambda dt, **k: ctx.computeAdaptiveWeight_bilateralGrid(L, R, dt, 10, 10, 0, D, **k)),
        (A.ADAPTIVE_WEIGHT_MEDIAN, 3, lambda dt, **k: ctx.computeAdaptiveWeight_WeightedMedian(L, R, dt, 3, 10, 10, 0, D, **k)),
        (A.ADAPTIVE_WEIGHT_CROSS, 5, lambda dt, **k: ctx.computeAdaptiveWeight_cross(L, R, dt, 20, 20, 5, 0, D, **k)),
        (asw.adcensus_algorithm(), 5, lambda dt, **k: ctx.computeAdaptiveWeight_adcensus(L, R, dt, 20, 10, 30, 5, 0, D, **k)),
        (asw.twopass_algorithm(), 5, lambda dt, **k: ctx.computeAdaptiveWeight_twopass(L, R, 30, 20, dt, 5, 0, D, **k)),
        (asw.permeability_algorithm(), 0, lambda dt, **k: ctx.computeAdaptiveWeight_permeability(L, R, dt, 8, 20, 0, D, **k)),
    ]
    flag = asw.cross_scale(4, 64)
    for alg, win, call in calls:
        vol, disp, plain = expected(ctx2, L, R, LEFT, alg, win, 0, D, 4, 64)
        d1, v1 = call(int(LEFT) | flag, return_cost_volume=True)
        assert same(v1, vol) and np.array_equal(d1, disp) and not same(v1, plain), int(alg)
        assert np.array_equal(call(int(LEFT) | flag), disp)
        d0, v0 = call(LEFT, return_cost_volume=True)  # and the unflagged call afterwards is the plain one
        assert same(v0, plain)


@pytest.mark.parametrize("method", ["classic", "guided", "cross", "permeability"])
def test_resident(ctx, ctx2, method):
    alg, right, win, minD = METHODS[method]
    H, W, D = 12, 68, 11
    L, R = cs.textured_pair(H, W, 3, minD + 3, 90)
    n = _planes(alg, D)
    vol, disp, plain = expected(ctx2, L, R, LEFT, alg, win, minD, D, 3, 19)
    ctx.upload_pair(21, L, R)
    ctx.match_resident(21, LEFT, alg, win, minD, D, keep_volume=True)  # a previous, unflagged result with a volume
    assert same(ctx.download_volume(21, (n, H, W)), plain)
    ctx.match_resident(21, LEFT, alg, win, minD, D, keep_volume=False, cross_scale=asw.cross_scale())
    assert np.array_equal(ctx.download_disparity(21, (H, W)), disp)
    with pytest.raises(AswError) as e:
        ctx.download_volume(21, (n, H, W))
    assert e.value.status == asw.ERR_NO_FRAME
    t = ctx.timing()
    assert t["total_ms"] > 0 and t["total_ms"] >= t["aggregate_ms"] >= 0 and t["aggregate_launches"] >= 1
    ctx.match_resident(21, int(LEFT) | asw.cross_scale(), alg, win, minD, D, keep_volume=True)
    assert np.array_equal(ctx.download_disparity(21, (H, W)), disp)
    got = ctx.download_volume(21, (n, H, W))
    assert same(got, vol) and not same(got, plain)
    ctx.match_resident(21, LEFT, alg, win, minD, D, keep_volume=True, subpixel=P, cross_scale=asw.cross_scale())
    assert np.array_equal(ctx.download_disparity(21, (H, W)), sp.subpixel_vec(disp, vol, minD, P)[0])
    assert same(ctx.download_volume(21, (n, H, W)), vol)
    l2, r2 = ctx.download_pair(21, L.shape)
    assert np.array_equal(l2, L) and np.array_equal(r2, R)  # the pyramid is built beside the slot, not in it
    ctx.match_resident(21, LEFT, alg, win, minD, D, keep_volume=True)  # the unflagged call afterwards is the plain one again
    assert same(ctx.download_volume(21, (n, H, W)), plain)


@pytest.mark.parametrize("alg,win", [(A.ADAPTIVE_WEIGHT, 5), (A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2, 5), (asw.permeability_algorithm(), 0)])
def test_batch_of_three(ctx2, alg, win):
    H, W, D = 14, 70, 12
    pairs = [cs.textured_pair(H, W, 3, 3 + i, 100 + i) for i in range(3)]
    flag = asw.cross_scale(3, 64)
    outs = asw.stereoMatchingBatch([p[0] for p in pairs], [p[1] for p in pairs], LEFT, alg, win, 1, D, device_ids=[0], cross_scale=flag)
    plain = asw.stereoMatchingBatch([p[0] for p in pairs], [p[1] for p in pairs], LEFT, alg, win, 1, D, device_ids=[0])
    for (L, R), o, p in zip(pairs, outs, plain):
        vol, disp, v0 = expected(ctx2, L, R, LEFT, alg, win, 1, D, 3, 64)
        assert np.array_equal(o, disp) and not same(vol, v0)
        assert not np.array_equal(o, p)
    sub = asw.stereoMatchingBatch([pairs[0][0]], [pairs[0][1]], LEFT, alg, win, 1, D, device_ids=[0], subpixel=E, cross_scale=flag)
    vol, disp, v0 = expected(ctx2, pairs[0][0], pairs[0][1], LEFT, alg, win, 1, D, 3, 64)
    assert np.array_equal(sub[0], sp.subpixel_vec(disp, vol, 1, E)[0])


# ---- statuses ----
def test_statuses(ctx):
    H, W, D = 12, 40, 12
    L, R = cs.textured_pair(H, W, 3, 4, 110)
    F = asw.cross_scale()
    ctx.upload_pair(22, L, R)
    plain_d, plain_v = ctx.stereoMatching(L, R, LEFT, A.ADAPTIVE_WEIGHT, 5, 0, D, return_cost_volume=True)

    def expect(status, dt, alg, win=5, minD=0, numD=D):
        ctx.match_resident(22, LEFT, A.ADAPTIVE_WEIGHT, 5, 0, D, keep_volume=True)  # a previous result
        with pytest.raises(AswError) as e:
            ctx.match_resident(22, dt, alg, win, minD, numD, keep_volume=True)
        assert e.value.status == status, (hex(dt), alg, e.value.status)
        for fetch in (lambda: ctx.download_disparity(22, (H, W)), lambda: ctx.download_volume(22, (D + 1, H, W))):
            with pytest.raises(AswError) as e:  # a failed flagged match drops the slot's results
                fetch()
            assert e.value.status == asw.ERR_NO_FRAME
        with pytest.raises(AswError) as e:  # the host-image call answers alike
            ctx.stereoMatching(L, R, dt, alg, win, minD, numD)
        assert e.value.status == status
        d, v = ctx.stereoMatching(L, R, LEFT, A.ADAPTIVE_WEIGHT, 5, 0, D, return_cost_volume=True)  # a plain call afterwards is unaffected
        assert np.array_equal(d, plain_d) and same(v, plain_v)

    bad = asw.ERR_BAD_ARGUMENT
    for S in (0, 1, 6, 7):  # S outside 2..5
        expect(bad, 0x1000 | (S << 13) | (19 << 16), A.ADAPTIVE_WEIGHT)
        assert asw.cross_scale(S, 19) == 0x1000 | (19 << 16)
        expect(bad, asw.cross_scale(S, 19), A.ADAPTIVE_WEIGHT_CROSS)
    expect(bad, 0x1000 | (3 << 13), A.ADAPTIVE_WEIGHT)  # q = 0
    expect(bad, asw.cross_scale(3, 0), A.ADAPTIVE_WEIGHT)
    expect(bad, asw.cross_scale(3, 256), A.ADAPTIVE_WEIGHT)
    for bit in (0x2, 0x4, 0x80, 0x400, 0x800, 1 << 24, 1 << 30):  # reserved bits
        expect(bad, F | bit, A.ADAPTIVE_WEIGHT)
        expect(bad, F | bit | RIGHT, A.ADAPTIVE_WEIGHT_GUIDED_FILTER)
    expect(bad, F | (-1 << 31), A.ADAPTIVE_WEIGHT)
    expect(bad, F | P | E, A.ADAPTIVE_WEIGHT)  # both sub-pixel flags
    expect(bad, F | P | E | 1, asw.permeability_algorithm(), win=0)
    expect(bad, asw.cross_scale(5), A.ADAPTIVE_WEIGHT, numD=15)  # a scale left without its two candidates (16 is the least)
    expect(bad, asw.cross_scale(2), A.ADAPTIVE_WEIGHT_GEODESIC, numD=1)
    expect(bad, F, A.ADAPTIVE_WEIGHT, numD=0)
    expect(asw.ERR_UNSUPPORTED_METHOD, F, A.NCC)
    expect(asw.ERR_UNSUPPORTED_METHOD, F | 1 | P, A.NCC)
    expect(asw.ERR_UNSUPPORTED_METHOD, F, A.BM, numD=16)
    expect(asw.ERR_UNSUPPORTED_METHOD, F, 13)
    # with bit 12 clear nothing changes
    expect(bad, 0x400, A.ADAPTIVE_WEIGHT)
    expect(bad, P | 0x400, A.ADAPTIVE_WEIGHT)
    expect(bad, F & ~0x1000, A.ADAPTIVE_WEIGHT)  # the fields without the flag: refused by the method, as before
    # whatever a scale's runner refuses is the call's status
    for alg in (A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2, A.ADAPTIVE_WEIGHT_MEDIAN, A.ADAPTIVE_WEIGHT_8DIRECT, A.ADAPTIVE_WEIGHT_BILATERAL_GRID):
        expect(asw.ERR_UNSUPPORTED_LAYOUT, F | 1, alg)
    expect(bad, F, A.ADAPTIVE_WEIGHT_BLO1, minD=2)
    expect(bad, F, A.ADAPTIVE_WEIGHT_CROSS, win=37)
    expect(bad, F, A.ADAPTIVE_WEIGHT, win=65)
    with pytest.raises(AswError) as e:
        ctx.computeNCC(L, R, int(LEFT) | F, 5, 0, D)
    assert e.value.status == asw.ERR_UNSUPPORTED_METHOD
    assert ctx.stereoMatching(L, R, int(LEFT) | F, A.ADAPTIVE_WEIGHT, 4, 0, D) is None  # even window: the silent return, as unflagged
    assert asw.last_status() == asw.ERR_EVEN_WINDOW
    # SGBM ignores disparity_type altogether
    s0 = ctx.stereoMatching(L, R, LEFT, A.SGBM, 5, 0, 16)
    assert np.array_equal(ctx.stereoMatching(L, R, F | P | E | 0x400, A.SGBM, 5, 0, 16), s0)
    assert np.array_equal(ctx.stereoMatching(L, R, 0x1000, A.SGBM, 5, 0, 16), s0)
    # the batch call returns the same statuses
    for dt, status in ((asw.cross_scale(6), bad), (F | 0x400, bad), (asw.cross_scale(5), bad)):
        with pytest.raises(AswError) as e:
            asw.stereoMatchingBatch([L], [R], dt, A.ADAPTIVE_WEIGHT, 5, 0, 15, device_ids=[0])
        assert e.value.status == status
    # and the slot works again afterwards
    ctx.match_resident(22, LEFT, A.ADAPTIVE_WEIGHT, 5, 0, D, cross_scale=F)
    assert ctx.download_disparity(22, (H, W)).shape == (H, W)


# ---- tied combined costs: the first minimum wins ----
@pytest.mark.parametrize("alg,win", [(A.ADAPTIVE_WEIGHT, 5), (A.ADAPTIVE_WEIGHT_CROSS, 5), (asw.twopass_algorithm(), 5)])
@pytest.mark.parametrize("dt", [LEFT, RIGHT])
def test_periodic_pair_ties(ctx, ctx2, alg, win, dt):
    """period 8 at the finest scale is period 4, 2 on the next two: candidates d and d + 8 read equal costs on every scale away from
    the borders, so the combined costs tie exactly"""
    H, W, minD, numD = 12, 128, 1, 20
    L, R = asw_cases.make_input(("periodic", 8, 3), H, W, 0)
    vol, disp, plain = check(ctx, ctx2, L, R, dt, alg, win, minD, numD, S=3)
    with np.errstate(invalid="ignore"):
        tied = (vol == vol.min(axis=0)).sum(axis=0) >= 2
    print("tied share %.3f" % tied.mean())
    assert tied.mean() >= 0.3
    first = (np.argmin(vol, axis=0) + minD).astype(np.float32)
    assert np.array_equal(disp[tied], first[tied])


# ---- views whose rows carry padding ----
@pytest.mark.parametrize("W,pad", [(64, 5), (37, 3)])
def test_padded_rows(ctx, ctx2, W, pad):
    Lw, Rw = cs.textured_pair(10, W + pad, 3, 4, 130)
    L, R = Lw[:, :W], Rw[:, :W]
    assert L.strides[0] > W * 3
    vol, disp, plain = check(ctx, ctx2, L, R, LEFT, A.ADAPTIVE_WEIGHT, 5, 2, 14, S=3)
    dense = ctx.stereoMatching(np.ascontiguousarray(L), np.ascontiguousarray(R), LEFT, A.ADAPTIVE_WEIGHT, 5, 2, 14, cross_scale=asw.cross_scale())
    assert np.array_equal(dense, disp)


# ---- seeded sweep ----
def test_seeded_sweep():
    rng = np.random.default_rng(20267)
    a = b = None
    differed = 0
    try:
        for i in range(200):
            if i % 25 == 0:  # fresh contexts: no tables, scratch or pyramid levels of earlier cases
                for c in (a, b):
                    if c is not None:
                        c.close()
                a, b = asw.Context(0), asw.Context(0)
            c = cs.random_case(rng)
            tag = "case %d: %s" % (i, {k: v for k, v in c.items() if k not in ("L", "R")})
            vol, disp, plain = expected(b, c["L"], c["R"], c["dt"], c["alg"], c["win"], c["minD"], c["numD"], c["S"], c["q"])
            if c["subpixel"]:
                disp = sp.subpixel_vec(disp, vol, c["minD"], c["subpixel"])[0]
            flag = asw.cross_scale(c["S"], c["q"])
            d1, v1 = a.stereoMatching(c["L"], c["R"], c["dt"], c["alg"], c["win"], c["minD"], c["numD"], return_cost_volume=True,
                                      subpixel=c["subpixel"], cross_scale=flag)
            assert same(v1, vol), tag
            assert np.array_equal(d1, disp), tag
            assert np.array_equal(a.stereoMatching(c["L"], c["R"], c["dt"] | c["subpixel"] | flag, c["alg"], c["win"], c["minD"], c["numD"]),
                                  disp), tag
            # a drawn case may coincide with the plain volume: a frame narrower than its candidates reads one clamped column for
            # every candidate on every scale (entry 12's truncated cost is then 20 everywhere), entry 2 at window 1 is 0 / 0.  Such
            # a case still compares; from 60 columns up (the pair's shift is at most 30) a case must differ, and the sweep as a
            # whole must not be made of the others
            if c["L"].shape[1] >= 60 and np.isfinite(plain).any():
                assert not same(v1, plain), tag
            differed += not same(v1, plain)
    finally:
        for c in (a, b):
            if c is not None:
                c.close()
    print("cases whose volume differs from the plain one: %d of 200" % differed)
    # 9 of the 15 widths drawn have 60 columns or more and window 1 of entry 2 is one case in 52: about 118 of 200 cases must
    # differ, give or take the draw's spread (a standard deviation of 7)
    assert differed >= 100
