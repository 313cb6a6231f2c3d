"""The launch forms that depend on the size of the frame, on the GPU: the candidate chunk of k_similarity (8 .. 512, the short last
slice, two column blocks), the grid.z split of k_asw_bilateral's three instantiations and of k_asw_geodesic (1 .. 8 slices of 16, 32
and 48 candidates, and one slice of more than 16), k_bm_match's tile widths 4 .. 64, the segments of k_sgbm_hcost_census by the row
count, the capped grids of k_disp_to_u8 / k_norm_u8 and k_slice_minmax past their caps, and the permeability aggregation and the
weighted median on a frame each whose natural chunk count exceeds one.  tests/geometry_cases.py holds the
frames (tall and narrow: the decisions count workgroups, not pixels), the inputs and the references; tests/test_geometry_cases_cpu.py
holds every frame to the form its label names and the references to having something to tell the forms apart.

Every comparison is np.array_equal (equal_nan where a method produces NaN), on the volume and on the map, with one exception stated
where it is made: the cost volume of GuidedF_2, which its parity test compares within 1e-4 (sliding f64 sums against direct ones).
The references: the CPU oracle for computeSimilarity, the ASW matchers, the NCC cost and the u8 conversion; tests/stereobm_ref.py and
tests/sgbm_census_ref.py for the two OpenCV-style matchers."""
import os
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_cases as gc  # noqa: E402

LEFT, RIGHT = asw.DISPARITY_LEFT, asw.DISPARITY_RIGHT
A = asw.StereoMatchingAlgorithms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


def _same(got, want, what, equal_nan=False):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if np.array_equal(got, want, equal_nan=equal_nan):
        return
    ne = got != want
    if equal_nan:
        ne &= ~(np.isnan(got) & np.isnan(want))
    bad = np.argwhere(ne)
    pytest.fail("%s: %d of %d values differ; planes / rows of the first axis touched: %s; the first five: %s" % (
        what, len(bad), want.size, np.unique(bad[:, 0])[:12].tolist(),
        ["%s got %s want %s" % (tuple(int(v) for v in i), got[tuple(i)], want[tuple(i)]) for i in bad[:5]]))


# ---------------------------------------------------------------- computeSimilarity: every dch
@pytest.mark.parametrize("win", [None, gc.SIM_PAD_WIN], ids=["unpadded", "padded"])
@pytest.mark.parametrize("case", gc.sim_cases(), ids=lambda c: "dch%d-%dx%d-D%d" % (c[4], c[0], c[1], c[3]))
def test_similarity_every_chunk(ctx, oracle, case, win):
    H, W, minD, numD, dch = case
    L, R = gc.similarity_inputs(case)
    r, c, g = gc.SIM_PARAMS
    what = "computeSimilarity %dx%d, %d candidates from %d, chunks of %d, winSize %s" % (H, W, numD, minD, dch, win)
    got = ctx.computeSimilarity(L, R, r, c, g, LEFT, minD, numD) if win is None else ctx.computeSimilarity(L, R, r, c, g, LEFT, minD, numD, winSize=win)
    _same(np.stack(got), gc.expected_similarity(oracle, case, win), what)


def test_guided2_over_a_large_chunk(ctx, oracle):
    H, W, win, minD, numD, dch = gc.GUIDED2_CASE
    L, R = gc.sim_pair(H, W, numD, 3)
    rc, d_want, v_want = oracle.asw_guided2(L, R, 0, 1e-6, win, minD, numD, want_vol=True)
    d_got, v_got = ctx.computeAdaptiveWeight_GuidedF_2(L, R, LEFT, 1e-6, win, minD, numD, return_cost_volume=True)
    assert rc == 0 and v_got.shape == (numD, H, W) and len(np.unique(d_want)) > 1
    assert np.abs(v_got - v_want).max() < 1e-4   # as test_guided2_parity compares it
    _same(d_got, d_want, "GuidedF_2 map %dx%d, similarity chunks of %d" % (H, W, dch))


def test_wmedian_over_a_large_chunk(ctx, oracle):
    H, W, win, minD, numD, dch = gc.WMEDIAN_CASE
    L, R = gc.sim_pair(H, W, numD, 3)
    rc, d_want, v_want = oracle.asw_wmedian(L, R, 0, win, 10, 10, minD, numD, want_vol=True)
    d_got, v_got = ctx.computeAdaptiveWeight_WeightedMedian(L, R, LEFT, win, 10, 10, minD, numD, return_cost_volume=True)
    assert rc == 0 and len(np.unique(d_want)) > 1
    _same(v_got, v_want, "weighted-median volume %dx%d, similarity chunks of %d" % (H, W, dch))  # the median is one of the input costs
    _same(d_got, d_want, "weighted-median map")


def test_similarity_parameter_grid(ctx, oracle):
    """the integer form of `c > thresC` (tCi = floor(thresC)) and the float form of `g > thresG` (tGdn = the largest float at or
    under thresG) against the oracle's double comparisons, at the values where they could part"""
    L, R = gc.param_pair()
    H, W, minD, numD = gc.PARAM_FRAME
    for r in gc.REGULARITY:
        for c in gc.THRES_C:
            for g in gc.THRES_G:
                rc, want = oracle.compute_similarity(L, R, r, c, g, 0, minD, numD)
                assert rc == 0
                _same(np.stack(ctx.computeSimilarity(L, R, r, c, g, LEFT, minD, numD)), want,
                      "computeSimilarity regularity %r thresC %r thresG %r" % (r, c, g))


# ---------------------------------------------------------------- classic and geodesic ASW: the grid.z split
SPLIT = [(k, case, dt) for k in sorted(gc.SPLIT_KERNELS) for case in gc.SPLIT_CASES[k] for dt in (0, 1)]


@pytest.mark.parametrize("kernel,case,dt", SPLIT, ids=lambda v: v if isinstance(v, str) else (
    "%dx%d-D%d-nz%d-per%d" % (v[0], v[1], v[4], v[5], v[6]) if isinstance(v, tuple) else ("left", "right")[v]))
def test_candidate_split(ctx, oracle, kernel, case, dt):
    method, _, _ = gc.SPLIT_KERNELS[kernel]
    H, W, win, minD, numD, nz, per_z, what = case
    L, R = gc.split_inputs(case)
    d_want, v_want = gc.expected_split(oracle, kernel, case, dt)
    run = (lambda **kw: ctx.computeAdaptiveWeight(L, R, 30, 20, dt, win, minD, numD, **kw)) if method == "classic" else \
          (lambda **kw: ctx.computeAdaptiveWeight_geodesic(L, R, dt, win, minD, numD, **kw))
    d_got, v_got = run(return_cost_volume=True)
    label = "%s %dx%d win %d, %d candidates from %d, direction %d (%s)" % (method, H, W, win, numD + 1, minD, dt, what)
    _same(v_got, v_want, label + ": volume", equal_nan=True)
    _same(d_got, d_want, label + ": map")
    _same(run(), d_want, label + ": map without the kept volume")


# ---------------------------------------------------------------- StereoBM: every tile width
@pytest.mark.parametrize("TX", sorted(gc.BM_FIRST))
def test_stereo_bm_tile_widths(ctx, TX):
    case = gc.BM_FIRST[TX]
    H, W, minD, D, w = case
    L, R = gc.bm_inputs(case)
    want = gc.expected_bm(case)
    cap, tex, U, sw, sr, M = gc.BM_SETTINGS
    got, vol = ctx.stereoBM(L, R, minD, D, w, asw.PREFILTER_XSOBEL, 9, cap, tex, U, sw, sr, M, return_cost_volume=True)
    what = "stereoBM %dx%d, %d candidates, window %d, tiles of %d columns" % (H, W, D, w, TX)
    _same(vol, want["vol"], what + ": volume", equal_nan=True)
    _same(got, want["disp"], what + ": map")


# ---------------------------------------------------------------- sgbm_census: the segments of the cost stage
@pytest.mark.parametrize("what", sorted(gc.CENSUS_CASES))
def test_sgbm_census_segments(ctx, what):
    case = gc.CENSUS_CASES[what]
    H, W, minD, D, w, nseg = case
    L, R = gc.census_inputs(case)
    want = gc.expected_census(case)
    P1, P2, m12, U, sw, sr = gc.CENSUS_SETTINGS
    got, vol = ctx.sgbm_census(L, R, minD, D, w, P1, P2, m12, U, sw, sr, paths=gc.CENSUS_PATHS, return_cost_volume=True)
    label = "sgbm_census %dx%d, %d candidates, %d segment(s)" % (H, W, D, nseg)
    _same(vol, np.moveaxis(want["S"], 2, 0).astype(np.float32), label + ": volume")
    _same(got, want["disp"], label + ": map")


# ---------------------------------------------------------------- the capped grids
def test_disparity_u8_past_the_grid_cap(ctx, oracle):
    H, W = gc.DISP_U8_FRAME
    win, minD, numD = gc.DISP_U8_MATCH
    L, R = gc.disp_u8_pair()
    want = gc.expected_disp_u8_map(oracle)
    ctx.upload_pair(4, L, R)
    ctx.match_resident(4, LEFT, A.ADAPTIVE_WEIGHT, win, minD, numD)
    _same(ctx.download_disparity(4, (H, W)), want, "classic map %dx%d" % (H, W))
    for normalize in (False, True):
        _same(ctx.download_disparity_u8(4, (H, W), normalize=normalize), oracle.disparity_to_u8(want, normalize),
              "download_disparity_u8 of %d pixels, normalize %s" % (H * W, normalize))


@pytest.mark.parametrize("H,W", gc.SLICE_SCALES_FRAMES)
def test_slice_scales_past_the_grid_cap(ctx, oracle, H, W):
    win, minD, numD = gc.SLICE_SCALES_NCC
    L, R = gc.slice_scales_pair(H, W)
    rc, want = oracle.cost_ncc(L, R, 0, win, minD, numD)
    assert rc == 0
    _same(np.stack(ctx.computeNCC_costs(L, R, LEFT, win, minD, numD)), want, "normalised NCC cost %dx%d" % (H, W), equal_nan=True)


# ---------------------------------------------------------------- the natural chunk counts, no switch set
def _forced(env):
    return asw.Context(0, env=env)


def test_permeability_natural_chunks(ctx, oracle):
    """448 + 29 candidates a chunk by the 2 GiB fit, against a context forced to one candidate a chunk (the map) and against
    tests/permeability_ref.py over the oracle's AD planes (the first and the last plane of both chunks)"""
    import permeability_ref as pm
    H, W, minD, n, sigma, trunc = gc.PERM_NATURAL
    L, R = gc.perm_natural_pair()
    chunk = gc.perm_chunk(H, W, n)
    d_nat, vol = ctx.computeAdaptiveWeight_permeability(L, R, LEFT, sigma, trunc, minD, n, return_cost_volume=True)
    assert vol.shape == (n, H, W) and (d_nat - minD < chunk).any() and (d_nat - minD >= chunk).any()  # winners from both chunks
    c = _forced({"ASW_PERM_CHUNK": "1"})
    try:
        _same(c.computeAdaptiveWeight_permeability(L, R, LEFT, sigma, trunc, minD, n), d_nat, "permeability map, natural chunks against one candidate a chunk")
    finally:
        c.close()
    e = []
    for k in gc.PERM_PLANES:
        rc, ad = oracle.compute_ad(L, R, 0, minD + k, 1)
        assert rc == 0
        e.append(ad[0])
    E, want, _, _ = pm.aggregate(np.stack(e), L, sigma, trunc, minD)
    for i, k in enumerate(gc.PERM_PLANES):
        assert gc.varies(want[i])
        _same(vol[k], want[i], "permeability plane %d of %d, natural chunks of %d" % (k, n, chunk))


def test_wmedian_natural_chunks(ctx, oracle):
    """list chunks of 8 + 1 slices by the 2 GiB / 6 fit at 35x35, against a context forced to one slice a chunk (whole frame) and
    against the oracle on the first and the last rows of the frame"""
    H, W, win, minD, n = gc.WMEDIAN_NATURAL
    L, R = gc.wmedian_natural_pair()
    run = lambda c: c.computeAdaptiveWeight_WeightedMedian(L, R, LEFT, win, 10, 10, minD, n, return_cost_volume=True)
    d_nat, v_nat = run(ctx)
    c = _forced({"ASW_WMEDIAN_TILE_CHUNK": "1"})
    try:
        d_one, v_one = run(c)
    finally:
        c.close()
    _same(v_nat, v_one, "weighted-median volume, natural list chunks against one slice a chunk")
    _same(d_nat, d_one, "weighted-median map, natural list chunks against one slice a chunk")
    for rows, d_want, v_want in gc.expected_wmedian_bands(oracle):
        _same(v_nat[:, rows], v_want, "weighted-median volume, rows %d..%d" % (rows.start, rows.stop - 1))
        _same(d_nat[rows], d_want, "weighted-median map, rows %d..%d" % (rows.start, rows.stop - 1))
