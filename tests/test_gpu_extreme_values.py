"""Every exactness bound at its extreme, on the two-level pairs of tests/extreme_cases.py (the table is there; the conditions that
keep these cases from being vacuous are held by tests/test_extreme_cases_cpu.py on the restatements alone).

Every comparison is np.array_equal (NaN equal to NaN) on volumes, maps, masks and counts, against the oracle or the restatement of
the method.  The one exception is the guided-filter family, which keeps asw_cases.tolerance / asw_cases.check as they are.  Frames
are the smallest that reach the bound; widths cross the 64-column tile."""
import os
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adcensus_ref as ar  # noqa: E402
import asw_cases as ac  # noqa: E402
import cross_ref as cr  # noqa: E402
import cross_scale_ref as cs  # noqa: E402
import extreme_cases as ec  # noqa: E402
import permeability_ref as pm  # noqa: E402
import refine_ref as rr  # noqa: E402
import scanline_ref as sl  # noqa: E402
import sgbm_census_ref as scref  # noqa: E402
import sgbm_paths_ref as pref  # noqa: E402
import sgbm_ref  # noqa: E402
import subpixel_ref as sp  # noqa: E402
import twopass_ref as tp  # noqa: E402
import window_cases as wc  # noqa: E402

pytestmark = pytest.mark.gpu
LEFT, RIGHT = asw.DISPARITY_LEFT, asw.DISPARITY_RIGHT
A = asw.StereoMatchingAlgorithms


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


@pytest.fixture(scope="module")
def ctx_two_pass():
    c = asw.Context(0, env={"ASW_GUIDED_FUSED": "0"})
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_fused():
    c = asw.Context(0, env={"ASW_GUIDED_FUSED": "1"})
    yield c
    c.close()


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ---------------------------------------------------------------- refine
def _refine(ctx, G, dl, dr, minD, n, win, gc, gs):
    want = rr.refine_vec(G, dl, dr, minD, n, 1.0, win, gc, gs)
    out, nrej, nunf, mask = ctx.refineDisparity(G, dl, dr, minD, n, 1.0, win, gc, gs, return_mask=True)
    assert np.array_equal(mask, want["mask"])
    assert (nrej, nunf) == (want["n_rejected"], want["n_unfillable"])
    assert np.array_equal(out, want["out"]), np.argwhere(out != want["out"])[:5]
    return want


def _guide(H, W, cn):
    return np.full((H, W) if cn == 1 else (H, W, 3), 255, np.uint8)


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("win", ec.REFINE_T_WINDOWS)
def test_refine_total_weight_at_its_maximum(ctx, win, cn):
    H, W, minD, n, _ = ec.REFINE_T_CASE
    dl, dr = ec.refine_two_level_maps(H, W, minD, n)
    want = _refine(ctx, _guide(H, W, cn), dl, dr, minD, n, win, ec.REFINE_GAMMA, ec.REFINE_GAMMA)
    filled = want["mask"] == 1
    assert set(np.unique(want["out"][filled])) == {minD, minD + n - 1}


@pytest.mark.parametrize("cn", [1, 3])
def test_refine_votes_at_both_ends_of_the_range(ctx, cn):
    H, W, minD, n, win = ec.REFINE_ENDS_CASE
    assert n == ec.REFINE_MAX_N
    dl, dr = ec.refine_two_level_maps(H, W, minD, n)
    want = _refine(ctx, _guide(H, W, cn), dl, dr, minD, n, win, ec.REFINE_GAMMA, ec.REFINE_GAMMA)
    assert (want["out"] != want["fill"]).any()


@pytest.mark.parametrize("minD", [-ec.REFINE_MAX_MIND, ec.REFINE_MAX_MIND])
def test_refine_ends_of_min_disparity(ctx, minD):
    H, W = ec.REFINE_MIND_FRAME
    dl = ec.refine_mind_end_map(minD)
    for cn in (1, 3):
        want = _refine(ctx, _guide(H, W, cn), dl, dl.copy(), minD, ec.REFINE_MAX_N, 15, 60.0, 9.0)
        assert want["n_unfillable"] == H * W


@pytest.mark.parametrize("win", [35, 3])
def test_refine_all_equal_map(ctx, win):
    H, W = ec.REFINE_T_CASE[:2]
    dl, dr = ec.refine_equal_maps(H, W, 5)
    want = _refine(ctx, _guide(H, W, 3), dl, dr, 0, 9, win, ec.REFINE_GAMMA, ec.REFINE_GAMMA)
    assert want["n_rejected"] == 5 * H and (want["out"] == 5).all()
    # the guide at both levels (checker): the last column of the colour table on half the taps
    _refine(ctx, ec.checker(H, W, 3)[0], dl, dr, 0, 9, win, 1.0, 1.0)
    _refine(ctx, ec.checker(H, W, 1)[0], dl, dr, 0, 9, win, ec.REFINE_GAMMA, 1.0)


# ---------------------------------------------------------------- cross and AD-Census
CROSS_KINDS = {"opposed_flat": 20, "checker": 0, "complement": 255}      # kind -> tau


def _cross_check(got, E, disp):
    d, v, d2 = got
    assert same(v, E), np.argwhere(v != E)[:5]
    assert np.array_equal(d, disp) and np.array_equal(d2, disp)


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("win", ec.CROSS_WINDOWS)
@pytest.mark.parametrize("dt", [LEFT, RIGHT])
@pytest.mark.parametrize("kind", list(CROSS_KINDS))
def test_cross_entry_12(ctx, kind, dt, win, cn):
    H, W = ec.CROSS_FRAME
    tau, minD, D = CROSS_KINDS[kind], 0, 5
    for label, L, R in ec.variants(kind, H, W, cn):
        e = ar.ad(L, R, int(dt), minD, D)
        assert np.array_equal(np.stack(ctx.computeAD(L, R, dt, minD, D)), e), label
        S, N, E, disp = cr.aggregate(e, cr.arms(R if dt else L, tau, win // 2), 255, minD)
        if kind == "opposed_flat" and cn == 1 and win == 35:
            assert S.max() == ec.CROSS_S_MAX
        if kind == "checker":
            assert (N == 1).all()
        d, v = ctx.computeAdaptiveWeight_cross(L, R, dt, tau, 255, win, minD, D, return_cost_volume=True)
        d2 = ctx.computeAdaptiveWeight_cross(L, R, dt, tau, 255, win, minD, D)
        _cross_check((d, v, d2), E, disp)


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("win", ec.CROSS_WINDOWS)
@pytest.mark.parametrize("dt", [LEFT, RIGHT])
@pytest.mark.parametrize("kind", list(CROSS_KINDS))
def test_adcensus_entry(ctx, kind, dt, win, cn):
    minD, D = 0, 5
    # checker: tau 0 (every arm 0, N = 1) on the cross frame, and tau 255 on the frame whose regions stay off the clamped census border
    runs = [(0, ec.CROSS_FRAME), (255, ec.ADCENSUS_FRAME)] if kind == "checker" else [(CROSS_KINDS[kind], ec.CROSS_FRAME)]
    for tau, (H, W) in runs:
        for lambdas in (ec.ADCENSUS_LAMBDAS, (10, 30)):
            for label, L, R in ec.variants(kind, H, W, cn):
                S, N, E, disp = ar.match(L, R, int(dt), tau, lambdas[0], lambdas[1], win, minD, D)
                if kind == "checker" and tau == 0:
                    assert (N == 1).all()
                if kind == "checker" and tau == 255 and cn == 1 and win == 35 and lambdas == ec.ADCENSUS_LAMBDAS:
                    assert S.max() == ec.ADCENSUS_E_MAX * 1225
                args = (L, R, dt, tau, lambdas[0], lambdas[1], win, minD, D)
                d, v = ctx.computeAdaptiveWeight_adcensus(*args, return_cost_volume=True)
                _cross_check((d, v, ctx.computeAdaptiveWeight_adcensus(*args)), E, disp)


# ---------------------------------------------------------------- cost builders
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("dt", [LEFT, RIGHT])
@pytest.mark.parametrize("kind", ec.KINDS)
def test_cost_builders(ctx, oracle, kind, dt, cn):
    H, W, minD, D = 9, 70, 0, 6
    for label, L, R in ec.variants(kind, H, W, cn):
        msg = (kind, label)
        assert np.array_equal(np.stack(ctx.computeAD(L, R, dt, minD, D)), oracle.compute_ad(L, R, int(dt), minD, D)[1]), msg
        for T in (30, 255):
            assert np.array_equal(np.stack(ctx.computeTAD(L, R, dt, T, minD, D)), oracle.compute_tad(L, R, int(dt), T, minD, D)[1]), msg
        assert np.array_equal(np.stack(ctx.computeCensus(L, R, dt, minD, D)), ar.hamming(L, R, int(dt), minD, D)), msg
        for la, lc in (ec.ADCENSUS_LAMBDAS, (10, 30), (255, 255)):
            assert np.array_equal(np.stack(ctx.computeADCensus(L, R, dt, la, lc, minD, D)), ar.cost(L, R, int(dt), la, lc, minD, D)), msg
        # the oracle's SAD cost takes 3 channels: a gray pair is held to the oracle on its three equal channels, whose gray it is
        L3, R3 = (L, R) if cn == 3 else (np.repeat(L[:, :, None], 3, axis=2), np.repeat(R[:, :, None], 3, axis=2))
        for win in (15, 63):
            assert np.array_equal(np.stack(ctx.getCostSAD(L, R, dt, win, minD, D)), oracle.cost_sad(L3, R3, int(dt), win, minD, D)[1]), msg
        if cn == 3 and dt == LEFT:   # the only branch of computeSimilarity that can execute
            got = np.stack(ctx.computeSimilarity(L, R, *ec.SIM_PARAMS, LEFT, minD, D))
            assert np.array_equal(got, oracle.compute_similarity(L, R, *ec.SIM_PARAMS, 0, minD, D)[1]), msg
            if kind == "opposed_edges":
                assert (float(got.min()), float(got.max())) == ec.tad_cost_range()
            got = np.stack(ctx.computeSimilarity(L, R, *ec.SIM_PARAMS, LEFT, minD, D, winSize=7))
            assert np.array_equal(got, oracle.compute_similarity(L, R, *ec.SIM_PARAMS, 0, minD, D, win=7)[1]), msg


# ---------------------------------------------------------------- the bit-exact matcher group
LARGE_WINDOWS = dict(wc.derived_limits(), geodesic=wc.LIMITS["geodesic"][0], wmedian=wc.LIMITS["wmedian"][0])
DEFAULT_WINDOW = 15


def _matcher_case(method, kind, label, L, R, win, dt, params=None):
    p = ac.TABLE_PARAMS[method] if params is None else params
    return {"method": method, "tag": (kind, label, win, int(dt), p), "kind": kind, "L": L, "R": R, "win": win, "minD": 0, "numD": 4,
            "dt": dt, "params": p}


@pytest.mark.parametrize("kind", ec.KINDS)
@pytest.mark.parametrize("method", ac.BIT_EXACT)
def test_bit_exact_matchers(ctx, oracle, method, kind):
    H, W = ec.FLOAT_FRAME
    windows = (1,) if method == "bilgrid" else (DEFAULT_WINDOW, LARGE_WINDOWS[method])
    for label, L, R in ec.variants(kind, H, W, 3):
        for win in windows:
            if label != "plain" and win != windows[0]:
                continue      # the swapped and padded forms at the default window
            for dt in ac.directions(method):
                case = _matcher_case(method, kind, label, L, R, win, dt)
                ac.check(case, ac.gpu_result(ctx, case), ac.reference(oracle, case))


def test_classic_on_checker_with_zero_denominators(ctx, oracle):
    H, W = ec.FLOAT_FRAME
    L, R = ec.checker(H, W, 3)
    for gammas, nan in ((ec.CHECKER_GAMMAS_NAN, True), (ec.CHECKER_GAMMAS_FINITE, False), ((255.0, 255.0), False), ((1.0, 1.0), False)):
        for dt in (LEFT, RIGHT):
            case = _matcher_case("classic", "checker", "plain", L, R, 15, dt, gammas)
            want = ac.reference(oracle, case)
            assert bool(np.isnan(want["vol"]).all()) == nan
            ac.check(case, ac.gpu_result(ctx, case), want)


@pytest.mark.parametrize("kind", ec.KINDS)
def test_twopass(ctx, kind):
    H, W = ec.FLOAT_FRAME
    for label, L, R in ec.variants(kind, H, W, 3) + [("gray",) + ec.pair(kind, H, W, 1)]:
        for win in (DEFAULT_WINDOW, 35) if label == "plain" else (DEFAULT_WINDOW,):
            for gc, gg in ((30, 20), (255, 255), (1, 1)):
                for dt in (LEFT, RIGHT):
                    got, (vol, disp) = tp.gpu_result(ctx, {"L": L, "R": R, "gamma_c": gc, "gamma_g": gg, "win": win, "minD": 0, "numD": 4,
                                                           "dt": dt})
                    assert same(got[0], vol) and np.array_equal(got[1], disp) and np.array_equal(got[2], disp), (label, win, gc, gg, dt)
                    if kind == "opposed_flat":
                        assert (vol == np.float32(255.0)).all()


@pytest.mark.parametrize("kind", ec.KINDS)
def test_permeability(ctx, kind):
    H, W = ec.FLOAT_FRAME
    for label, L, R in ec.variants(kind, H, W, 3) + [("gray",) + ec.pair(kind, H, W, 1)]:
        for sigma in (1, 255):
            for dt in (LEFT, RIGHT):
                got, (vol, disp) = pm.gpu_result(ctx, {"L": L, "R": R, "sigma": sigma, "trunc": 255, "minD": 0, "D": 5, "dt": dt})
                assert same(got[0], vol) and np.array_equal(got[1], disp) and np.array_equal(got[2], disp), (label, sigma, dt)


# ---------------------------------------------------------------- classic on the xq form
def right_max_mind(W):
    return W - 1 - (W - 1) // 64 * 64


XQ_CASES = [(LEFT, 0), (LEFT, 48), (RIGHT, 0), (RIGHT, right_max_mind(ec.XQ_FRAME[1]))]


XQ_NO_TAIL = (63, 127)      # the inclusive range ends at the xq kernel's 64 / 128 candidates: two launches, no tail


@pytest.mark.parametrize("numD", [63, 64, 127, 128, 130])
@pytest.mark.parametrize("dt,minD", XQ_CASES)
@pytest.mark.parametrize("kind", ["opposed_edges", "checker", "complement"])
def test_classic_xq(ctx, ctx_old, oracle, kind, dt, minD, numD):
    H, W = ec.XQ_FRAME
    L, R = ec.pair(kind, H, W, 3)
    gc, gg = ec.XQ_GAMMAS
    d, v = ctx.computeAdaptiveWeight(L, R, gc, gg, dt, 15, minD, numD, return_cost_volume=True)
    assert ctx.timing()["aggregate_launches"] == (2 if numD in XQ_NO_TAIL else 4)      # the xq kernels served the call
    rc, dw, vw = oracle.asw_classic(L, R, gc, gg, int(dt), 15, minD, numD, want_vol=True)
    assert rc == 0 and v.shape == vw.shape == (numD + 1, H, W)
    assert np.array_equal(v, vw, equal_nan=True), np.argwhere(v != vw)[:5]
    assert np.array_equal(d, dw), np.argwhere(d != dw)[:5]
    d0, v0 = ctx_old.computeAdaptiveWeight(L, R, gc, gg, dt, 15, minD, numD, return_cost_volume=True)
    assert np.array_equal(v, v0, equal_nan=True) and np.array_equal(d, d0)


# ---------------------------------------------------------------- the weighted median, every form
@pytest.mark.parametrize("form", list(ec.WMEDIAN_WINDOWS))
def test_weighted_median_forms(ctx, oracle, form):
    H, W = ec.WMEDIAN_FRAME
    win = ec.WMEDIAN_WINDOWS[form]
    for label, L, R in ec.variants("opposed_edges", H, W, 3):
        case = dict(_matcher_case("wmedian", "opposed_edges", label, L, R, win, LEFT), numD=5)
        want = ac.reference(oracle, case)
        ac.check(case, ac.gpu_result(ctx, case), want)
        lo, hi = ec.tad_cost_range()
        assert float(want["vol"].max()) == hi and float(want["vol"].min()) >= lo


# ---------------------------------------------------------------- the guided-filter family
GUIDED_KINDS = ("opposed_flat", "opposed_edges", "checker")


@pytest.mark.parametrize("eps", [1e-6, 1e-8])
@pytest.mark.parametrize("kind", GUIDED_KINDS)
@pytest.mark.parametrize("method", ac.TOLERANCE)
def test_guided_family(ctx, oracle, method, kind, eps):
    H, W = ec.FLOAT_FRAME
    for label, L, R in ec.variants(kind, H, W, 3):
        for win in (DEFAULT_WINDOW, 5):
            for dt in ac.directions(method):
                case = _matcher_case(method, kind, label, L, R, win, dt, (eps,))
                ac.check(case, ac.gpu_result(ctx, case), ac.reference(oracle, case))


@pytest.mark.parametrize("eps", [1e-6, 1e-8])
@pytest.mark.parametrize("kind", GUIDED_KINDS)
def test_guided2_fused_walk_equals_two_pass(ctx_two_pass, ctx_fused, oracle, kind, eps):
    H, W = ec.FLOAT_FRAME
    L, R = ec.pair(kind, H, W, 3)
    case = _matcher_case("guided2", kind, "plain", L, R, 15, LEFT, (eps,))
    two = ac.gpu_result(ctx_two_pass, case)
    assert ctx_two_pass.timing()["aggregate_launches"] == 4
    fused = ac.gpu_result(ctx_fused, case)
    assert ctx_fused.timing()["aggregate_launches"] == 3, "the fused walk did not run"
    assert np.array_equal(fused["disp"], two["disp"]) and np.array_equal(fused["vol"], two["vol"], equal_nan=True)
    ac.check(case, two, ac.reference(oracle, case))


@pytest.mark.parametrize("eps", [1e-6, 1e-8])
@pytest.mark.parametrize("kind", GUIDED_KINDS)
def test_guided_filter_3_and_6_channels(ctx, oracle, kind, eps):
    H, W = ec.FLOAT_FRAME
    L, R = ec.pair(kind, H, W, 3)
    rc, sim = oracle.compute_similarity(L, R, *ec.SIM_PARAMS, 0, 0, 1)
    for guide in (L, np.concatenate([L, R], axis=2)):
        for P in (sim[0], np.full((H, W), 8452.0, np.float32)):
            for r in (15, 5):
                rc, want = oracle.guided_filter(guide, P, r, eps)
                got = ctx.getGuidedFilter(guide, P, r, eps)
                assert rc == 0 and got.shape == want.shape and np.array_equal(np.isfinite(got), np.isfinite(want))
                fin = np.isfinite(want)
                # q lives on the normalised [0, 1] scale of P: tolerance 1e-4 absolute there (tests/test_gpu_parity.py)
                assert not fin.any() or np.abs(got[fin] - want[fin]).max() < 1e-4, (guide.shape[2], r, np.abs(got[fin] - want[fin]).max())


# ---------------------------------------------------------------- the SGBM family
def _sgbm_compare(got, vol, want):
    assert np.array_equal(got, want["disp"]), np.argwhere(got != want["disp"])[:5]
    if vol is not None:
        assert np.array_equal(vol, np.moveaxis(want["S"], 2, 0).astype(np.float32))


@pytest.mark.parametrize("paths", ec.SGBM_MASKS)
def test_sgbm_paths_volume_near_the_f32_bound(ctx, paths):
    L, R, a = ec.sgbm_volume_args(paths)
    want = pref.sgbm_paths(L, R, *a)
    if paths == 0xFF:
        assert want["S"].max() >= 1 << 23
    got, vol = ctx.sgbm_paths(L, R, *a[:-1], paths=paths, return_cost_volume=True)
    _sgbm_compare(got, vol, want)
    # one more in P2 is refused with a volume and served without one
    with pytest.raises(asw.AswError) as e:
        ctx.sgbm_paths(L, R, a[0], a[1], a[2], a[3], a[4] + 1, *a[5:-1], paths=paths, return_cost_volume=True)
    assert e.value.status == asw.ERR_BAD_ARGUMENT
    b = a[:4] + (a[4] + 1,) + a[5:]
    _sgbm_compare(ctx.sgbm_paths(L, R, *b[:-1], paths=paths), None, pref.sgbm_paths(L, R, *b))


SGBM_FRAME = (24, 100)


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("bar", [1, 2, 20])
def test_sgbm_and_census_accept_their_largest_penalties_and_refuse_one_more(ctx, bar, cn):
    """What the host check holds, no more: on these periodic pairs S stays below 3.7e6 whatever P2 is, so a penalty of 7e8 enters no
    sum.  The calls show that the largest accepted P2 is served with the restatement's map (and S where a volume is kept) and that
    one more is refused; the int32 bound itself is reached by no frame a test can afford (tests/extreme_cases.py, TABLE)."""
    H, W = SGBM_FRAME
    L, R = ec.opposed_edges(H, W, cn, bar)
    minD, D, w, cap = 0, 16, 11, 63
    for want_volume in (False, True):
        P2 = ec.sgbm_largest_p2(cn, w, cap, 0x07, want_volume)
        want = sgbm_ref.sgbm(L, R, minD, D, w, P2 - 1, P2, 1, cap, 0, 0, 0)
        got = ctx.sgbm(L, R, minD, D, w, P2 - 1, P2, 1, cap, 0, 0, 0, return_cost_volume=want_volume)
        _sgbm_compare(*(got if want_volume else (got, None)), want)
        with pytest.raises(asw.AswError) as e:
            ctx.sgbm(L, R, minD, D, w, P2, P2 + 1, 1, cap, 0, 0, 0, return_cost_volume=want_volume)
        assert e.value.status == asw.ERR_BAD_ARGUMENT
        for paths in ec.SGBM_MASKS:
            P2 = ec.sgbm_largest_p2(cn, w, cap, paths, want_volume, census=True)
            want = scref.sgbm_census(L, R, minD, D, w, P2 - 1, P2, 1, 0, 0, 0, paths)
            got = ctx.sgbm_census(L, R, minD, D, w, P2 - 1, P2, 1, 0, 0, 0, paths=paths, return_cost_volume=want_volume)
            _sgbm_compare(*(got if want_volume else (got, None)), want)


# ---------------------------------------------------------------- StereoBM
def test_stereobm_block_sad_at_its_maximum(ctx):
    H, W, minD, D, w = ec.BM_CASE
    cap, tex, U, sw, sr, M = ec.BM_SETTINGS
    L, R = ec.bm_pair()
    want = ec.bm_reached()
    assert np.nanmax(want["vol"]) == ec.BM_SAD_MAX
    got, vol = ctx.stereoBM(L, R, minD, D, w, preFilterCap=cap, textureThreshold=tex, uniquenessRatio=U, speckleWindowSize=sw,
                            speckleRange=sr, disp12MaxDiff=M, return_cost_volume=True)
    assert np.array_equal(got, want["disp"]) and same(vol, want["vol"])
    assert np.array_equal(ctx.stereoBM(L, R, minD, D, w, preFilterCap=cap, textureThreshold=tex, uniquenessRatio=U, speckleWindowSize=sw,
                                       speckleRange=sr, disp12MaxDiff=M), want["disp"])


# ---------------------------------------------------------------- the flags over an extreme volume
FLAG_METHODS = {"classic": 5, "cross": 15}     # method -> window


def _flag_case(method, kind, dt):
    H, W = ec.FLOAT_FRAME
    L, R = ec.pair(kind, H, W, 3)
    return {"method": method, "alg": cs.algorithm(method), "extra": cs.METHODS[method][1], "dt": dt, "win": FLAG_METHODS[method], "minD": 0,
            "numD": 8, "L": L, "R": R, "tag": (method, kind, int(dt))}


def _flag_check(got, want, tag):
    (v, d, d2), (vw, dw) = got, want
    assert same(v, vw), tag
    assert np.array_equal(d, dw) and np.array_equal(d2, dw), tag


@pytest.mark.parametrize("dt", [LEFT, RIGHT])
@pytest.mark.parametrize("kind", ["opposed_flat", "checker"])
@pytest.mark.parametrize("method", list(FLAG_METHODS))
def test_scanline_with_the_largest_and_the_smallest_code(ctx, method, kind, dt):
    for code in (ec.SCANLINE_MAX, ec.SCANLINE_MIN):
        for sub in (0, asw.SUBPIXEL_PARABOLA, asw.SUBPIXEL_EQUIANGULAR):
            case = dict(_flag_case(method, kind, dt), a=code[0], u=code[1], ratio=code[2], subpixel=sub)
            got, want = sl.gpu_result(ctx, case)
            _flag_check(got, want, case["tag"] + code + (sub,))


@pytest.mark.parametrize("dt", [LEFT, RIGHT])
@pytest.mark.parametrize("kind", ["opposed_flat", "checker"])
@pytest.mark.parametrize("method", list(FLAG_METHODS))
def test_cross_scale_with_the_largest_and_the_smallest_weight(ctx, method, kind, dt):
    for q in ec.CROSS_SCALE_Q:
        for sub in (0, asw.SUBPIXEL_PARABOLA, asw.SUBPIXEL_EQUIANGULAR):
            case = dict(_flag_case(method, kind, dt), S=3, q=q, subpixel=sub)
            got, want = cs.gpu_result(ctx, case)
            _flag_check(got, want, case["tag"] + (q, sub))


@pytest.mark.parametrize("dt", [LEFT, RIGHT])
@pytest.mark.parametrize("kind", ["opposed_flat", "checker"])
@pytest.mark.parametrize("method", list(FLAG_METHODS))
def test_subpixel_with_zero_denominators(ctx, method, kind, dt):
    c = _flag_case(method, kind, dt)
    d0, v0 = ctx.stereoMatching(c["L"], c["R"], dt, c["alg"], c["win"], 0, c["numD"], return_cost_volume=True)
    if kind == "opposed_flat":
        assert (v0 == v0[0]).all()          # all planes equal: every pixel a tie, every denominator 0
    for mode in (asw.SUBPIXEL_PARABOLA, asw.SUBPIXEL_EQUIANGULAR):
        want, ok = sp.subpixel_vec(d0, v0, 0, mode)
        d1, v1 = ctx.stereoMatching(c["L"], c["R"], dt, c["alg"], c["win"], 0, c["numD"], return_cost_volume=True, subpixel=mode)
        assert v1.tobytes() == v0.tobytes()
        assert np.array_equal(d1, want), np.argwhere(d1 != want)[:5]
        if kind == "opposed_flat":
            assert d1.tobytes() == d0.tobytes()


# ---------------------------------------------------------------- the driver path
@pytest.mark.parametrize("kind", ["opposed_edges", "checker", "opposed_flat"])
def test_preprocess_match_and_u8(ctx, oracle, kind):
    sh, sw, dw, dh, minD, D = 72, 140, 70, 36, 3, 8
    L, R = ec.pair(kind, sh, sw, 3)
    for boost in (False, True):
        assert ctx.preprocess_pair(2, L, R, (dw, dh), detail_boost=boost)
        gl, gr = ctx.download_pair(2, (dh, dw, 3))
        pl, pr = oracle.preprocess(L, (dw, dh), boost), oracle.preprocess(R, (dw, dh), boost)
        assert np.array_equal(gl, pl) and np.array_equal(gr, pr), boost
    # full-size (no resize: the two levels survive) with the boost: the saturating V + 2 (V - blur)
    assert ctx.preprocess_pair(2, L, R, (sw, sh), detail_boost=True)
    gl, gr = ctx.download_pair(2, (sh, sw, 3))
    pl, pr = oracle.preprocess(L, (sw, sh), True), oracle.preprocess(R, (sw, sh), True)
    assert np.array_equal(gl, pl) and np.array_equal(gr, pr)
    ctx.match_resident(2, LEFT, A.ADAPTIVE_WEIGHT, 15, minD, D)
    d = ctx.download_disparity(2, (sh, sw))
    rc, want = oracle.stereo_matching(pl, pr, 0, int(A.ADAPTIVE_WEIGHT), 15, minD, D)
    assert rc == 0 and np.array_equal(d, want)
    if kind == "opposed_flat":
        assert (want == minD).all()         # a constant map: max == min
    for norm in (False, True):
        assert np.array_equal(ctx.download_disparity_u8(2, (sh, sw), normalize=norm), oracle.disparity_to_u8(want, norm)), norm
