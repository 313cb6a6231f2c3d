"""Left-right refinement on the GPU (asw_refine_disparity, asw_match_refined_resident, asw_stereo_match_refined, the C++ shim)
against the restatement of tests/refine_ref.py.  The rule is stated in integers: every comparison is
np.array_equal, on maps, masks and counts.

A kernel that skipped the fill or the median would pass on inputs where those stages change nothing, so every comparison on
matcher output first asserts, on the restatement alone: rejected share >= 5 % of the pixels and, for windows >= 7, the median
differs from the fill on >= 2 % of the filled pixels."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib
from aswstereomatch_amd._lib import AswError
from aswstereomatch_amd.synth import make_pair

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_ref as ref  # noqa: E402
from shim_build import build_demo  # noqa: E402

A = asw.StereoMatchingAlgorithms
NAN = np.float32(np.nan)
PAIRS = {"a": (96, 260, 24, 11, 32), "b": (60, 160, 16, 5, 16)}
SETTINGS = [(15, 60.0, 9.0), (15, 150.0, 9.0), (7, 150.0, 3.0), (35, 150.0, 20.0)]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


def _planes(alg, D):
    return _lib.lib().asw_volume_planes(int(alg), D)


def _maps(ctx, L, R, alg, win, minD, D):
    dl = ctx.stereoMatching(L, R, asw.DISPARITY_LEFT, alg, win, minD, D)
    dr = ctx.stereoMatching(L, R, asw.DISPARITY_RIGHT, alg, win, minD, D)
    return dl, dr


def _non_vacuous(want, win):
    rejected, moved = ref.vacuity_shares(want)
    print("rejected share %.4f, median != fill on %.4f of the filled pixels" % (rejected, moved))
    assert rejected >= 0.05
    if win >= 7:
        assert moved >= 0.02


def _compare(ctx, G, dl, dr, minD, n, max_diff, win, gc, gs, form=ref.refine_vec, matcher_output=False):
    want = form(G, dl, dr, minD, n, max_diff, win, gc, gs)
    if matcher_output:
        _non_vacuous(want, win)
    out, nrej, nunf, mask = ctx.refineDisparity(G, dl, dr, minD, n, max_diff, win, gc, gs, return_mask=True)
    assert np.array_equal(mask, want["mask"])
    assert (nrej, nunf) == (want["n_rejected"], want["n_unfillable"])
    assert np.array_equal(out, want["out"])
    return want


# ---- (a) the library's own classic maps of the two pairs of the table ----
@pytest.mark.parametrize("pair", ["a", "b"])
@pytest.mark.parametrize("win,gc,gs", SETTINGS)
def test_refine_classic_maps(ctx, pair, win, gc, gs):
    H, W, D, seed, block = PAIRS[pair]
    L, R, _ = make_pair(H, W, D, seed=seed, block=block)
    dl, dr = _maps(ctx, L, R, A.ADAPTIVE_WEIGHT, 15, 0, D)
    want = _compare(ctx, L, dl, dr, 0, D + 1, 1.0, win, gc, gs, matcher_output=True)
    assert want["n_unfillable"] == 0


def test_refine_literal_form_on_a_crop(ctx):
    # the literal per-pixel loop as yardstick, on matcher output small enough for it
    H, W, D, seed, block = PAIRS["b"]
    L, R, _ = make_pair(H, W, D, seed=seed, block=block)
    dl, dr = _maps(ctx, L, R, A.ADAPTIVE_WEIGHT, 15, 0, D)
    _compare(ctx, L, dl, dr, 0, D + 1, 1.0, 7, 150.0, 3.0, form=ref.refine_loop, matcher_output=True)


# ---- (b) geodesic and GuidedF maps ----
@pytest.mark.parametrize("alg", [A.ADAPTIVE_WEIGHT_GEODESIC, A.ADAPTIVE_WEIGHT_GUIDED_FILTER])
def test_refine_other_methods_maps(ctx, alg):
    H, W, D, seed, block = PAIRS["b"]
    L, R, _ = make_pair(H, W, D, seed=seed, block=block)
    dl, dr = _maps(ctx, L, R, alg, 15, 0, D)
    _compare(ctx, L, dl, dr, 0, _planes(alg, D), 1.0, 15, 150.0, 9.0, matcher_output=True)


# ---- (c) random integer maps with random rejections ----
def _random_case(rng, H, W, cn, n, minD, p_reject, dead_rows=()):
    G = rng.integers(0, 256, (H, W) if cn == 1 else (H, W, 3)).astype(np.uint8)
    if rng.random() < 0.5:
        G = (G // 64 * 64).astype(np.uint8)  # piece-wise flat: off-centre colour weights that are not negligible
    levels = min(n, 40)
    stride = (n - 1) // (levels - 1) if levels > 1 else 1
    far = rng.integers(0, levels, (H, W)) * stride       # the whole range of n: valid only where the frame is wide enough
    near = rng.integers(0, max(1, min(n, W // 3)), (H, W))  # disparities that point inside a narrow frame
    dl = (minD + np.where(rng.random((H, W)) < (0.8 if n > W // 2 else 0.0), near, far)).astype(np.float32)
    xr = np.arange(W)[None, :] - dl.astype(np.int64)
    dr = np.full((H, W), -9.0, np.float32)
    ys, xs = np.nonzero((xr >= 0) & (xr < W))
    dr[ys, xr[ys, xs]] = dl[ys, xs]  # a later writer wins: pixels that share a target disagree with it, rejected as well
    kill = rng.random((H, W)) < p_reject
    dr[kill] = np.where(rng.random(int(kill.sum())) < 0.5, NAN, np.float32(-5.0))
    for y in dead_rows:
        dr[y] = NAN
    return G, dl, dr


RANDOM_CASES = [
    # H, W, channels, win, n, minD, dead rows
    (5, 1, 1, 3, 2, 0, ()), (9, 1, 3, 35, 5, 2, (4,)), (7, 63, 3, 15, 2, 0, ()), (9, 64, 1, 35, 9, 3, (0,)),
    (11, 65, 3, 3, 30, 0, (10,)), (13, 131, 3, 1, 17, 5, (3, 4)), (37, 41, 1, 7, 40, 2, ()), (3, 200, 3, 35, 30, 0, ()),
    (40, 7, 1, 35, 4, 1, (39,)), (33, 129, 3, 7, 12, 0, (16,)), (70, 300, 1, 15, 64, 7, (1, 68)), (19, 17, 3, 15, 1025, 0, ()),
    (50, 20, 1, 35, 1025, 4, (25,)), (6, 1300, 3, 15, 1025, 0, (2,)),
]


@pytest.mark.parametrize("H,W,cn,win,n,minD,dead", RANDOM_CASES)
def test_refine_random_maps(ctx, H, W, cn, win, n, minD, dead):
    rng = np.random.default_rng(H * 1000 + W + win)
    G, dl, dr = _random_case(rng, H, W, cn, n, minD, 0.3, dead)
    want = _compare(ctx, G, dl, dr, minD, n, 1.0, win, 80.0, 6.0)
    assert want["n_rejected"] > 0
    for y in dead:
        assert (want["mask"][y] == 2).all()
    if win >= 7 and W > 1 and H * W > 500:
        assert (want["out"] != want["fill"]).any()  # the median moved something in this case
    if H * W <= 700:
        lit = ref.refine_loop(G, dl, dr, minD, n, 1.0, win, 80.0, 6.0)
        assert np.array_equal(lit["out"], want["out"]) and np.array_equal(lit["mask"], want["mask"])


def test_refine_nothing_rejected_and_everything_rejected(ctx):
    rng = np.random.default_rng(77)
    H, W = 21, 90
    G = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    zero = np.zeros((H, W), np.float32)  # disparity 0 points at itself
    out, nrej, nunf, mask = ctx.refineDisparity(G, zero + 3, zero.copy() + 3, 3, 1, 0.0, 15, 60.0, 9.0, return_mask=True)
    # x - 3 < 0 for the first three columns: rejected, filled from the right
    want = ref.refine_vec(G, zero + 3, zero + 3, 3, 1, 0.0, 15, 60.0, 9.0)
    assert nrej == 3 * H == want["n_rejected"] and np.array_equal(out, want["out"]) and (out == 3).all()
    out, nrej, nunf, mask = ctx.refineDisparity(G, zero, zero, 0, 4, 0.0, 15, 60.0, 9.0, return_mask=True)
    assert nrej == 0 and nunf == 0 and not mask.any() and np.array_equal(out, zero)
    out, nrej, nunf, mask = ctx.refineDisparity(G, zero, zero + NAN, 0, 4, 0.0, 15, 60.0, 9.0, return_mask=True)
    assert nrej == H * W == nunf and (mask == 2).all() and (out == -1).all()
    out, nrej, nunf = ctx.refineDisparity(G, zero + 7, zero + NAN, 7, 1, 5.0, 3, 60.0, 9.0)
    assert nrej == H * W == nunf and (out == 6).all()  # min_disparity - 1


def test_small_colour_gamma_median_is_the_identity(ctx):
    H, W, D, seed, block = PAIRS["b"]
    L, R, _ = make_pair(H, W, D, seed=seed, block=block)
    dl, dr = _maps(ctx, L, R, A.ADAPTIVE_WEIGHT, 15, 0, D)
    want = ref.refine_vec(L, dl, dr, 0, D + 1, 1.0, 15, 10.0, 9.0)
    rejected, moved = ref.vacuity_shares(want)
    print("gamma_c = 10: rejected share %.4f, median != fill on %.4f of the filled pixels" % (rejected, moved))
    assert rejected >= 0.05 and moved < 0.02  # the explicit "median is the identity" case: why parity cases use larger colour gammas
    out, nrej, nunf = ctx.refineDisparity(L, dl, dr, 0, D + 1, 1.0, 15, 10.0, 9.0)
    assert np.array_equal(out, want["out"]) and nrej == want["n_rejected"]


# ---- resident and host-image forms equal the building block fed with two plain matches ----
@pytest.mark.parametrize("alg,minD", [(A.ADAPTIVE_WEIGHT, 0), (A.ADAPTIVE_WEIGHT, 2), (A.ADAPTIVE_WEIGHT_GEODESIC, 0),
                                      (A.ADAPTIVE_WEIGHT_GUIDED_FILTER, 1), (A.NCC, 0), (A.ADAPTIVE_WEIGHT_GUIDED_FILTER_3, 0)])
def test_refined_calls_equal_the_building_block(ctx, alg, minD):
    H, W, D, seed, block = PAIRS["b"]
    L, R, _ = make_pair(H, W, D, seed=seed, block=block)
    win, rwin, gc, gs = 15, 15, 150.0, 9.0
    dl, dr = _maps(ctx, L, R, alg, win, minD, D)
    n = _planes(alg, D)
    want_ref = ref.refine_vec(L, dl, dr, minD, n, 1.0, rwin, gc, gs)
    _non_vacuous(want_ref, rwin)  # on the restatement alone, before any refined GPU result is looked at
    want, wrej, wunf = want_ref["out"], want_ref["n_rejected"], want_ref["n_unfillable"]
    out, nrej, nunf = ctx.refineDisparity(L, dl, dr, minD, n, 1.0, rwin, gc, gs)
    assert (nrej, nunf) == (wrej, wunf) and np.array_equal(out, want)
    # resident
    ctx.upload_pair(3, L, R)
    ctx.match_resident(3, asw.DISPARITY_LEFT, alg, win, minD, D, keep_volume=True)  # a previous result with a volume
    assert ctx.download_volume(3, (n, H, W)).shape == (n, H, W)
    nrej, nunf = ctx.match_refined_resident(3, alg, win, minD, D, 1.0, rwin, gc, gs)
    assert (nrej, nunf) == (wrej, wunf)
    got = ctx.download_disparity(3, (H, W))
    assert np.array_equal(got, want)
    t = ctx.timing()
    assert t["total_ms"] > 0 and t["total_ms"] >= t["aggregate_ms"] >= 0
    u8 = ctx.download_disparity_u8(3, (H, W), normalize=False)
    assert np.array_equal(u8, np.clip(np.rint(want), 0, 255).astype(np.uint8))
    with pytest.raises(AswError) as e:
        ctx.download_volume(3, (n, H, W))
    assert e.value.status == asw.ERR_NO_FRAME
    l2, r2 = ctx.download_pair(3, L.shape)
    assert np.array_equal(l2, L) and np.array_equal(r2, R)
    # host images; the module-level binding
    got, nrej, nunf = ctx.stereoMatchingRefined(L, R, alg, win, minD, D, 1.0, rwin, gc, gs)
    assert np.array_equal(got, want) and (nrej, nunf) == (wrej, wunf)
    # the host-image call works on the private frame: the slot still holds the resident result
    assert np.array_equal(ctx.download_disparity(3, (H, W)), want)


def test_module_level_bindings(ctx):
    H, W, D, seed, block = PAIRS["b"]
    L, R, _ = make_pair(H, W, D, seed=seed, block=block)
    dl, dr = _maps(ctx, L, R, A.ADAPTIVE_WEIGHT, 15, 0, D)
    want = ref.refine_vec(L, dl, dr, 0, D + 1, 1.0, 7, 150.0, 3.0)
    _non_vacuous(want, 7)
    got, nrej, nunf = asw.stereoMatchingRefined(L, R, A.ADAPTIVE_WEIGHT, 15, 0, D, 1.0, 7, 150.0, 3.0)
    assert np.array_equal(got, want["out"]) and (nrej, nunf) == (want["n_rejected"], want["n_unfillable"])
    assert np.array_equal(asw.refineDisparity(L, dl, dr, 0, D + 1, 1.0, 7, 150.0, 3.0)[0], want["out"])
    # the defaults are the header's: win 15, gamma_c 60, gamma_s 9
    dflt = ref.refine_vec(L, dl, dr, 0, D + 1, 1.0, 15, 60.0, 9.0)
    _non_vacuous(dflt, 15)
    assert np.array_equal(ctx.refineDisparity(L, dl, dr, 0, D + 1)[0], dflt["out"])


def test_guide_is_the_preprocessed_left_image(ctx):
    L, R, _ = make_pair(120, 320, 20, seed=21, block=32)
    ctx.preprocess_pair(5, L, R, dsize=(160, 60), detail_boost=True)
    Lp, Rp = ctx.download_pair(5, (60, 160, 3))
    assert not np.array_equal(Lp, np.ascontiguousarray(L[::2, ::2]))
    D = 10
    dl, dr = _maps(ctx, Lp, Rp, A.ADAPTIVE_WEIGHT, 15, 0, D)  # on the private frame: slot 5 keeps the processed pair
    want = ref.refine_vec(Lp, dl, dr, 0, D + 1, 1.0, 15, 150.0, 9.0)
    _non_vacuous(want, 15)
    assert not np.array_equal(want["out"], ref.refine_vec(np.ascontiguousarray(L[::2, ::2]), dl, dr, 0, D + 1, 1.0, 15, 150.0, 9.0)["out"])
    nrej, nunf = ctx.match_refined_resident(5, A.ADAPTIVE_WEIGHT, 15, 0, D, 1.0, 15, 150.0, 9.0)
    got = ctx.download_disparity(5, (60, 160))
    assert np.array_equal(got, want["out"]) and (nrej, nunf) == (want["n_rejected"], want["n_unfillable"])


# ---- one whole frame ----
def test_refined_resident_full_frame(ctx):
    H, W, D = 1080, 1920, 128
    L, R, _ = make_pair(H, W, D, seed=1234, block=48)
    ctx.upload_pair(0, L, R)
    ctx.match_resident(0, asw.DISPARITY_LEFT, A.ADAPTIVE_WEIGHT, 15, 0, D)
    dl = ctx.download_disparity(0, (H, W))
    ctx.match_resident(0, asw.DISPARITY_RIGHT, A.ADAPTIVE_WEIGHT, 15, 0, D)
    dr = ctx.download_disparity(0, (H, W))
    want = ref.refine_vec(L, dl, dr, 0, D + 1, 1.0, 15, 150.0, 9.0)
    _non_vacuous(want, 15)
    nrej, nunf = ctx.match_refined_resident(0, A.ADAPTIVE_WEIGHT, 15, 0, D, 1.0, 15, 150.0, 9.0)
    got = ctx.download_disparity(0, (H, W))
    assert (nrej, nunf) == (want["n_rejected"], want["n_unfillable"])
    assert np.array_equal(got, want["out"])
    nrej2, nunf2 = ctx.match_refined_resident(0, A.ADAPTIVE_WEIGHT, 15, 0, D, 1.0, 15, 150.0, 9.0)
    assert (nrej2, nunf2) == (nrej, nunf) and ctx.download_disparity(0, (H, W)).tobytes() == got.tobytes()


# ---- status behaviour ----
def _raw_refine(ctx, G, dl, dr, minD, n, max_diff, win, gc, gs, null=None):
    """The C-ABI call on sentinel-filled outputs -> (status, out, mask, counts)."""
    lib = _lib.lib()
    gi, ga = asw._image(G)
    dl = np.ascontiguousarray(dl, np.float32)
    dr = np.ascontiguousarray(dr, np.float32)
    out = np.full(dl.shape, -777.0, np.float32)
    mask = np.full(dl.shape, 99, np.uint8)
    nr, nu = C.c_int(-5), C.c_int(-6)
    p = {"ctx": ctx._h, "guide": C.byref(gi), "dl": dl.ctypes.data_as(C.c_void_p), "dr": dr.ctypes.data_as(C.c_void_p),
         "out": out.ctypes.data_as(C.c_void_p)}
    if null:
        p[null] = None
    rc = lib.asw_refine_disparity(p["ctx"], p["guide"], p["dl"], p["dr"], minD, n, C.c_float(max_diff), win, gc, gs, p["out"],
                                  mask.ctypes.data_as(C.c_void_p), C.byref(nr), C.byref(nu))
    return rc, out, mask, (nr.value, nu.value)


def _untouched(out, mask, counts):
    return (out == -777.0).all() and (mask == 99).all() and counts == (-5, -6)


def test_bad_arguments_leave_the_outputs_untouched(ctx):
    rng = np.random.default_rng(9)
    H, W, minD, n = 12, 70, 2, 6
    G = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    dl = (minD + rng.integers(0, n, (H, W))).astype(np.float32)
    dr = dl.copy()
    rc, out, mask, counts = _raw_refine(ctx, G, dl, dr, minD, n, 1.0, 15, 60.0, 9.0)
    assert rc == 0 and not _untouched(out, mask, counts)
    for bad in (minD + 0.5, NAN, np.float32(np.inf), np.float32(-np.inf), float(minD + n), float(minD - 1)):  # step 0
        d = dl.copy()
        d[H - 1, W - 1] = bad
        rc, out, mask, counts = _raw_refine(ctx, G, d, dr, minD, n, 1.0, 15, 60.0, 9.0)
        assert rc == asw.ERR_BAD_ARGUMENT and _untouched(out, mask, counts), bad
    for kw in (dict(win=14), dict(win=37), dict(win=0), dict(win=-3), dict(gc=0.0), dict(gc=-1.0), dict(gs=0.0), dict(gs=float("nan")),
               dict(n=0), dict(n=1026), dict(max_diff=-1.0), dict(max_diff=float("nan")), dict(null="dl"), dict(null="dr"),
               dict(null="out"), dict(null="guide"), dict(null="ctx")):
        a = dict(minD=minD, n=n, max_diff=1.0, win=15, gc=60.0, gs=9.0, null=None)
        a.update(kw)
        rc, out, mask, counts = _raw_refine(ctx, G, dl, dr, a["minD"], a["n"], a["max_diff"], a["win"], a["gc"], a["gs"], a["null"])
        assert rc == asw.ERR_BAD_ARGUMENT and _untouched(out, mask, counts), kw
    # optional outputs may be NULL; a 6-channel guide is a layout the stage does not serve
    lib = _lib.lib()
    gi, _ = asw._image(G)
    out = np.zeros((H, W), np.float32)
    rc = lib.asw_refine_disparity(ctx._h, C.byref(gi), dl.ctypes.data_as(C.c_void_p), dr.ctypes.data_as(C.c_void_p), minD, n,
                                  C.c_float(1.0), 15, 60.0, 9.0, out.ctypes.data_as(C.c_void_p), None, None, None)
    assert rc == 0 and np.array_equal(out, ref.refine_vec(G, dl, dr, minD, n, 1.0, 15, 60.0, 9.0)["out"])
    G6 = np.concatenate([G, G], axis=2)
    assert _raw_refine(ctx, G6, dl, dr, minD, n, 1.0, 15, 60.0, 9.0)[0] == asw.ERR_UNSUPPORTED_LAYOUT


def test_refined_resident_status_and_slot_state(ctx):
    H, W, D, seed, block = PAIRS["b"]
    L, R, _ = make_pair(H, W, D, seed=seed, block=block)
    ctx.upload_pair(7, L, R)

    def expect(status, alg, win=15, minD=0, numD=D, max_diff=1.0, rwin=15, gc=60.0, gs=9.0):
        ctx.match_resident(7, asw.DISPARITY_LEFT, A.ADAPTIVE_WEIGHT, 15, 0, D)  # a previous result
        assert ctx.download_disparity(7, (H, W)) is not None
        with pytest.raises(AswError) as e:
            ctx.match_refined_resident(7, alg, win, minD, numD, max_diff, rwin, gc, gs)
        assert e.value.status == status, (alg, e.value.status)
        with pytest.raises(AswError) as e:  # the slot's previous result is gone
            ctx.download_disparity(7, (H, W))
        assert e.value.status == asw.ERR_NO_FRAME
        l2, r2 = ctx.download_pair(7, L.shape)  # the pair survives
        assert np.array_equal(l2, L) and np.array_equal(r2, R)

    for alg in (A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2, A.ADAPTIVE_WEIGHT_MEDIAN, A.ADAPTIVE_WEIGHT_8DIRECT, A.ADAPTIVE_WEIGHT_BILATERAL_GRID):
        expect(asw.ERR_UNSUPPORTED_LAYOUT, alg)
    expect(asw.ERR_UNSUPPORTED_METHOD, A.SGBM, numD=16)
    expect(asw.ERR_UNSUPPORTED_METHOD, A.BM, numD=16)
    expect(asw.ERR_BAD_ARGUMENT, A.ADAPTIVE_WEIGHT, rwin=8)
    expect(asw.ERR_BAD_ARGUMENT, A.ADAPTIVE_WEIGHT, rwin=37)
    expect(asw.ERR_BAD_ARGUMENT, A.ADAPTIVE_WEIGHT, gc=0.0)
    expect(asw.ERR_BAD_ARGUMENT, A.ADAPTIVE_WEIGHT, gs=-2.0)
    expect(asw.ERR_BAD_ARGUMENT, A.ADAPTIVE_WEIGHT, max_diff=-1.0)
    # the NCC matcher leaves a pixel 0 where no candidate has a comparable cost (flat windows: 0 / 0): with min_disparity > 0 that
    # literal zero is outside the domain of the left map
    flat = np.full_like(L, 90)
    ctx.upload_pair(8, flat, flat)
    ctx.match_resident(8, asw.DISPARITY_LEFT, A.NCC, 15, 3, D)
    assert (ctx.download_disparity(8, (H, W)) == 0).all()
    with pytest.raises(AswError) as e:
        ctx.match_refined_resident(8, A.NCC, 15, 3, D)
    assert e.value.status == asw.ERR_BAD_ARGUMENT
    with pytest.raises(AswError) as e:
        ctx.download_disparity(8, (H, W))
    assert e.value.status == asw.ERR_NO_FRAME
    assert ctx.match_refined_resident(8, A.NCC, 15, 0, D) == (0, 0)  # min_disparity 0: both maps are zeros, every pixel agrees
    expect(asw.ERR_EVEN_WINDOW, A.ADAPTIVE_WEIGHT, win=14)
    expect(asw.ERR_BAD_ARGUMENT, A.ADAPTIVE_WEIGHT_GUIDED_FILTER, numD=0)  # as a plain match
    expect(asw.ERR_BAD_ARGUMENT, A.ADAPTIVE_WEIGHT, minD=-1)
    with pytest.raises(AswError) as e:
        ctx.match_refined_resident(911, A.ADAPTIVE_WEIGHT, 15, 0, D)
    assert e.value.status == asw.ERR_NO_FRAME
    # the host-image form: same statuses
    with pytest.raises(AswError) as e:
        ctx.stereoMatchingRefined(L, R, A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2, 15, 0, D)
    assert e.value.status == asw.ERR_UNSUPPORTED_LAYOUT
    with pytest.raises(AswError) as e:
        ctx.stereoMatchingRefined(L, R, A.SGBM, 15, 0, 16)
    assert e.value.status == asw.ERR_UNSUPPORTED_METHOD
    # and the slot works again afterwards
    ctx.match_refined_resident(7, A.ADAPTIVE_WEIGHT, 15, 0, D)
    assert ctx.download_disparity(7, (H, W)).shape == (H, W)


# ---- the C++ shim ----
@pytest.mark.parametrize("cv", [False, True])
def test_shim_refine(ctx, tmp_path, cv):
    exe = build_demo("refine_demo.cpp", tmp_path / "refine_demo", cv)
    H, W, D, seed, block = PAIRS["b"]
    L, R, _ = make_pair(H, W, D, seed=seed, block=block)
    L.tofile(tmp_path / "l.raw")
    R.tofile(tmp_path / "r.raw")
    dl, dr = _maps(ctx, L, R, A.ADAPTIVE_WEIGHT, 15, 0, D)
    want_ref = ref.refine_vec(L, dl, dr, 0, D + 1, 1.0, 15, 150.0, 9.0)
    _non_vacuous(want_ref, 15)
    want, nrej, nunf = want_ref["out"], want_ref["n_rejected"], want_ref["n_unfillable"]
    assert np.array_equal(ctx.stereoMatchingRefined(L, R, A.ADAPTIVE_WEIGHT, 15, 0, D, 1.0, 15, 150.0, 9.0)[0], want)
    r = subprocess.run([exe, str(H), str(W), "3", str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), "2", "15", "0", str(D), "1.0", "15",
                        "150", "9", str(tmp_path / "one.raw"), str(tmp_path / "two.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok %d %d rejected=%d,%d unfillable=%d,%d" % (H, W, nrej, nrej, nunf, nunf), \
        (r.stdout, r.stderr)
    for name in ("one.raw", "two.raw"):
        assert np.array_equal(np.fromfile(tmp_path / name, np.float32).reshape(H, W), want)
    r = subprocess.run([exe, str(H), str(W), "3", str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), "8", "15", "0", str(D), "1.0", "15",
                        "150", "9", str(tmp_path / "one.raw"), str(tmp_path / "two.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("error"), (r.stdout, r.stderr)
