"""Confidence-weighted edge-aware smoothing on the GPU (k_smooth.hip; asw_mi355x.h "Smoothing").

smoothDisparity is held to tests/smooth_ref.py bit for bit (equal f32 bit patterns: a NaN that passes through keeps its payload, +0
is not -0).  The matched forms are held to smoothDisparity applied to the two channels of a second context's 2-channel call.

The kernels' constants (k_smooth.hip): a pass puts SM_LINES = 64 neighbouring lines on a workgroup of one wavefront; it takes a
line's steps SM_TILE = 16 at a time, and the row pass stages its N / D tiles of 64 lines x 16 steps through LDS; the prep kernel
works on tiles of SM_PREP = 32 x 32 pixels (it transposes the horizontal link indices through LDS)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib
from aswstereomatch_amd._lib import AswError, AswImage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scanline_ref as sr  # noqa: E402
import smooth_ref as sm  # noqa: E402
from test_gpu_scanline import METHODS  # noqa: E402  (the method rows: selector value, RIGHT served, window, minD, scanline code)

A = asw.StereoMatchingAlgorithms
LEFT = asw.DISPARITY_LEFT
SM_LINES, SM_TILE, SM_PREP = 64, 16, 32
bits = sm.same_bits
SMOOTH = asw.REFINE_SMOOTH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx2():
    """the context the 2-channel results come from: it shares no call history with the context under test"""
    c = asw.Context(0)
    yield c
    c.close()


def check(ctx, G, d, c, sigma_c=8.0, lam=900.0, T=3):
    want = sm.smooth_vec(G, d, c, sigma_c, lam, T)
    got = ctx.smoothDisparity(G, d, c, sigma_c, lam, T)
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert bits(got, want), (G.shape, sigma_c, lam, T, int(diff.sum()), np.argwhere(diff)[:5], got[diff][:5], want[diff][:5])
    return got


def inputs(H, W, cn=3, kind="smooth", seed=0, ckind="mixed", bad=0.0, pad=0):
    rng = np.random.default_rng([H, W, cn, seed])
    return sm.make_guide(rng, H, W, cn, kind, pad), sm.make_map(rng, H, W, bad), sm.make_conf(rng, H, W, ckind)


# ---- frames: the smallest ones, lines of one pixel, and both sides of every tile constant, as rows and as columns ----
EDGES = sorted({1, 2, SM_TILE - 1, SM_TILE, SM_TILE + 1, SM_PREP - 1, SM_PREP, SM_PREP + 1, SM_LINES - 1, SM_LINES, SM_LINES + 1,
                2 * SM_LINES + 1})
SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 3), (3, 1), (1, 70), (70, 1), (3, 5)] + [(n, 37) for n in EDGES] + [(21, n) for n in EDGES] + \
         [(63, 63), (64, 64), (65, 65), (63, 65), (65, 63)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes(ctx, H, W):
    for cn, kind in ((3, "smooth"), (1, "blocks")):
        G, d, c = inputs(H, W, cn, kind, seed=1)
        check(ctx, G, d, c, 8.0, 900.0, 2)


def test_shapes_reach_both_sides_of_the_constants():
    rows, cols = {h for h, w in SHAPES}, {w for h, w in SHAPES}
    for k in (SM_TILE, SM_PREP, SM_LINES):
        assert {k - 1, k, k + 1} <= rows and {k - 1, k, k + 1} <= cols, k
    assert (1, 1) in SHAPES and (2, 2) in SHAPES and 2 * SM_LINES + 1 in rows and 2 * SM_LINES + 1 in cols  # more than one workgroup


# ---- parameters ----
@pytest.mark.parametrize("T", [1, 2, 3, 8])
@pytest.mark.parametrize("lam", [2.0 ** -10, 1.0, 900.0, 2.0 ** 20])
def test_iterations_and_lambda(ctx, T, lam):
    G, d, c = inputs(35, 70, 3, "smooth", seed=2)
    out = check(ctx, G, d, c, 8.0, lam, T)
    assert np.isfinite(out).all()


@pytest.mark.parametrize("sigma_c", [0.05, 8.0, 1000.0])
@pytest.mark.parametrize("cn", [1, 3])
def test_sigma(ctx, sigma_c, cn):
    for kind in ("smooth", "noise"):
        G, d, c = inputs(33, 66, cn, kind, seed=3, bad=0.03)
        out = check(ctx, G, d, c, sigma_c, 900.0, 3)
        if sigma_c == 0.05 and kind == "noise":
            # Wt[k] = 0 from k = 1 on (exp(-20) * 65536 < 0.5): on a noise guide next to every link is cut, lines fall apart, and an
            # untrusted pixel without a trusted one in its component keeps its input bits: the D_T = 0 fallback is reached
            assert sm.table(0.05, cn)[1] == 0.0
            hole = ~(np.isfinite(d) & np.isfinite(c) & (c > 0))
            kept = out.view(np.uint32) == d.view(np.uint32)
            assert (hole & kept).sum() > 0.5 * hole.sum() and np.isnan(out).any()


# ---- guides ----
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("pad", [1, 5])
def test_padded_guide_rows(ctx, cn, pad):
    G, d, c = inputs(19, 45, cn, "smooth", seed=4, pad=pad)
    assert not G.flags.c_contiguous
    out = check(ctx, G, d, c)
    assert bits(out, ctx.smoothDisparity(np.ascontiguousarray(G), d, c))


@pytest.mark.parametrize("cn", [1, 3])
def test_constant_guide(ctx, cn):
    G, d, c = inputs(40, 50, cn, "constant", seed=5, ckind="unit")
    out = check(ctx, G, d, c, 8.0, 2.0 ** 20, 3)  # every weight 1, a strong pull: next to the frame's weighted mean everywhere
    mean = float((d.astype(np.float64) * c).sum() / c.astype(np.float64).sum())
    assert np.abs(out - mean).max() < 0.05 * max(1.0, abs(mean))
    flat = np.full_like(d, 7.5)
    assert np.abs(check(ctx, G, flat, c) - 7.5).max() <= 7.5e-7  # the constant-map bound of tests/test_smooth_cpu.py


@pytest.mark.parametrize("cn", [1, 3])
def test_step_edges(ctx, cn):
    """one vertical and one horizontal step edge of 160 levels: Wt[160 * cn] = 0 at sigma_c = 8, four regions that do not mix"""
    H, W = 30, 44
    G = sm.make_guide(np.random.default_rng(6), H, W, cn, "edges")
    assert sm.table(8.0, cn)[160 * cn] == 0.0
    quadrant = (np.arange(H)[:, None] >= (H + 1) // 2) * 2 + (np.arange(W)[None, :] >= (W + 1) // 2)
    d = (10.0 * quadrant + 3).astype(np.float32)
    rng = np.random.default_rng(7)
    c = np.where(rng.random((H, W)) < 0.5, 0, 1).astype(np.float32)  # a validity mask
    noisy = np.where(c > 0, d, np.float32(99)).astype(np.float32)
    out = check(ctx, G, noisy, c)
    assert np.abs(out - d).max() <= 1e-5  # every region's trusted pixels hold its constant (33 at most: 33 * 2^-23 < 1e-5)


# ---- maps and confidences ----
def test_non_finite_maps_and_odd_confidences(ctx):
    G, d, c = inputs(37, 67, 3, "smooth", seed=8, ckind="mixed", bad=0.08)
    assert np.isnan(d).any() and np.isposinf(d).any() and np.isneginf(d).any()
    assert (c == 0).any() and (c < 0).any() and np.isnan(c).any() and (c > 1).any() and np.isinf(c).any()
    out = check(ctx, G, d, c)
    hole = ~(np.isfinite(d) & np.isfinite(c) & (c > 0))
    assert np.isfinite(out[hole & ~np.isfinite(d)]).any()  # non-finite pixels were filled from their neighbours
    check(ctx, G, d, sm.make_conf(np.random.default_rng(9), 37, 67, "mask"))


def test_a_frame_of_zero_confidence(ctx):
    G, d, c = inputs(18, 70, 3, "smooth", seed=10, ckind="zero", bad=0.1)
    d[0, 0] = np.frombuffer(np.uint32(0x7FC12345).tobytes(), np.float32)[0]  # a NaN with a payload
    for conf in (c, np.full_like(c, -1.0), np.full_like(c, np.nan)):
        assert bits(check(ctx, G, d, conf), d)


# ---- seeded sweep, fresh contexts ----
def test_seeded_sweep():
    rng = np.random.default_rng(20425)
    a = None
    try:
        for i in range(60):
            if i % 10 == 0:  # a fresh context: no table or scratch of earlier cases
                if a is not None:
                    a.close()
                a = asw.Context(0)
            case = sm.random_case(rng)
            want = sm.smooth_vec(case["G"], case["d"], case["c"], case["sigma_c"], case["lam"], case["T"])
            got = a.smoothDisparity(case["G"], case["d"], case["c"], case["sigma_c"], case["lam"], case["T"])
            assert bits(got, want), "case %d: %s" % (i, case["tag"])
    finally:
        if a is not None:
            a.close()


# ---- the matched forms ----
ROWS = ["classic", "direct8", "guided2", "wmedian", "cross", "bilgrid"]  # direct8, guided2, wmedian, bilgrid: no RIGHT branch, the refinement refuses them


@pytest.mark.parametrize("method", ROWS)
def test_matched_forms(ctx, ctx2, method):
    alg, right, win, minD, code = METHODS[method]
    H, W, D = 21, 66, 13
    L, R = sr.textured_pair(H, W, 3, minD + 4, 11)
    sigma_c, lam, T = 12.0, 50.0, 2
    d, conf = ctx2.stereoMatching(L, R, LEFT, alg, win, minD, D, return_confidence=True)
    want = ctx2.smoothDisparity(L, d, conf, sigma_c, lam, T)
    assert bits(want, sm.smooth_vec(L, d, conf, sigma_c, lam, T))
    assert bits(ctx.stereoMatchingSmoothed(L, R, alg, win, minD, D, sigma_c, lam, T), want)
    ctx.upload_pair(31, L, R)
    ctx.match_resident(31, LEFT, alg, win, minD, D)
    plain = ctx.timing()
    ctx.match_smoothed_resident(31, alg, win, minD, D, sigma_c, lam, T)
    t = ctx.timing()
    assert bits(ctx.download_disparity(31, (H, W)), want)
    # the slot afterwards: no volume, no confidence of its own
    for fetch in (lambda: ctx.download_volume(31, (_lib.lib().asw_volume_planes(int(alg), D), H, W)),
                  lambda: ctx.download_disparity(31, (H, W), confidence=True)):
        with pytest.raises(AswError) as e:
            fetch()
        assert e.value.status == asw.ERR_NO_FRAME
    # the timing: the match's aggregation, everything else in cost_ms
    assert t["aggregate_launches"] == plain["aggregate_launches"]
    assert t["total_ms"] > t["aggregate_ms"] >= 0 and abs(t["cost_ms"] - (t["total_ms"] - t["aggregate_ms"])) < 1e-3
    if not right:  # the refinement refuses the method; the smoothing above served it
        with pytest.raises(AswError) as e:
            ctx.match_refined_resident(31, alg, win, minD, D)
        assert e.value.status == asw.ERR_UNSUPPORTED_LAYOUT
    # defaults of the wrapper
    assert bits(ctx.stereoMatchingSmoothed(L, R, alg, win, minD, D), ctx2.smoothDisparity(L, d, conf))


def test_a_failed_smoothed_match_drops_the_slot_and_keeps_the_pair(ctx):
    L, R = sr.textured_pair(12, 40, 3, 4, 12)
    ctx.upload_pair(32, L, R)
    ctx.match_resident(32, LEFT, A.ADAPTIVE_WEIGHT_CROSS, 5, 0, 8)
    with pytest.raises(AswError) as e:
        ctx.match_smoothed_resident(32, A.SGBM, 5, 0, 16)
    assert e.value.status == asw.ERR_UNSUPPORTED_METHOD
    with pytest.raises(AswError) as e:
        ctx.download_disparity(32, (12, 40))
    assert e.value.status == asw.ERR_NO_FRAME
    gl, gr = ctx.download_pair(32, (12, 40, 3))
    assert np.array_equal(gl, L) and np.array_equal(gr, R)
    ctx.match_smoothed_resident(32, A.ADAPTIVE_WEIGHT_CROSS, 5, 0, 8)
    assert ctx.download_disparity(32, (12, 40)).shape == (12, 40)
    with pytest.raises(AswError) as e:
        ctx.match_smoothed_resident(33, A.ADAPTIVE_WEIGHT_CROSS, 5, 0, 8)  # an empty slot
    assert e.value.status == asw.ERR_NO_FRAME


# ---- statuses ----
def raw_smooth(ctx, G, d, c, out, word, sigma_c=8.0, lam=900.0, mask=None, gimg=None):
    gi = gimg if gimg is not None else asw._image(G)[0]
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return _lib.lib().asw_refine_disparity(ctx._h, C.byref(gi) if gi is not None else None, p(d), p(c), 0, 1, 0.0, word, sigma_c, lam,
                                           p(out), p(mask), None, None)


def test_statuses_of_smooth_disparity(ctx):
    H, W = 12, 40
    G, d, c = inputs(H, W, 3, "smooth", seed=13)
    bad, layout = asw.ERR_BAD_ARGUMENT, asw.ERR_UNSUPPORTED_LAYOUT
    good = check(ctx, G, d, c)
    nan, inf = float("nan"), float("inf")
    G6 = np.ascontiguousarray(np.concatenate([G, G], axis=2))  # 6 channels: an image the library knows, not one the smoothing takes
    G4 = np.ascontiguousarray(np.concatenate([G, G[..., :1]], axis=2))  # no image at all: refused by the image check, as today

    def expect(status, word=SMOOTH | 3, guide=G, dd=d, cc=c, no_out=False, **kw):
        out = np.full((H, W), np.float32(-3.5))
        mask = kw.get("mask")
        assert raw_smooth(ctx, guide, dd, cc, None if no_out else out, word, **kw) == status, (hex(word), kw)
        assert (out == np.float32(-3.5)).all() and (mask is None or (mask == 9).all())  # a refused call writes nothing
        assert bits(ctx.smoothDisparity(G, d, c), good)  # and the context serves the next call

    # 1. null pointers and the guide as an image
    expect(bad, dd=None)
    expect(bad, cc=None)
    expect(bad, no_out=True)
    expect(bad, gimg=AswImage(G.ctypes.data, 0, W, 3, 0, G.strides[0]))
    expect(bad, gimg=AswImage(G.ctypes.data, H, W, 3, 0, W * 3 - 1))       # a short step
    # ... in front of the word, sigma_c and the channels
    expect(bad, word=SMOOTH | 9, sigma_c=nan, guide=G6, dd=None)
    # 2. the frame-size rule: more than 4 * 65535 rows (checked before anything is read: the image is not that large)
    # (6 channels: the rule is checked in front of the channels)
    rows = 4 * 65535 + 1
    column = np.zeros((rows, 1, 6), np.uint8)
    long = np.zeros((rows, 1), np.float32)
    out = np.full((rows, 1), np.float32(-3.5))
    assert raw_smooth(ctx, column, long, long, out, SMOOTH | 3) == bad and (out == np.float32(-3.5)).all()
    assert raw_smooth(ctx, column[:-1], long, long, out, SMOOTH | 3) == layout and (out == np.float32(-3.5)).all()
    # 3. the word: T outside 1..8, a stray bit; in front of sigma_c / lambda, the mask and the channels
    for word in (SMOOTH, SMOOTH | 9, SMOOTH | 16, SMOOTH | 0x100 | 3, SMOOTH | (1 << 29) | 3, SMOOTH | 0x3FFFFFFF):
        expect(bad, word=word)
    expect(bad, word=SMOOTH | 9, guide=G6)
    # 4. sigma_c / lambda: finite and > 0; in front of the mask and the channels
    for v in (0.0, -1.0, nan, inf, -inf):
        expect(bad, sigma_c=v)
        expect(bad, lam=v)
    expect(bad, sigma_c=nan, guide=G6)
    # 5. a mask is asked for: in front of the channels
    expect(bad, mask=np.full((H, W), 9, np.uint8))
    expect(bad, mask=np.full((H, W), 9, np.uint8), guide=G6)
    # 6. the channels
    expect(layout, guide=G6)
    expect(layout, guide=G4)
    expect(layout, guide=G4, word=SMOOTH | 9, sigma_c=nan)  # the image check comes first
    # the wrapper: iterations outside 1..8 travel as the invalid word
    for T in (0, 9, -2):
        with pytest.raises(AswError) as e:
            ctx.smoothDisparity(G, d, c, iterations=T)
        assert e.value.status == bad
    # no domain requirement on the map, and min_disparity / num_values / max_diff are not looked at
    out = np.zeros((H, W), np.float32)
    gi = asw._image(G)[0]
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = _lib.lib().asw_refine_disparity(ctx._h, C.byref(gi), p(d), p(c), -(1 << 25), -5, nan, SMOOTH | 3, 8.0, 900.0, p(out), None, None, None)
    assert rc == asw.OK and bits(out, good)


def test_statuses_of_the_matched_forms(ctx, ctx2):
    H, W, D = 12, 40, 12
    L, R = sr.textured_pair(H, W, 3, 4, 110)
    bad, unsupported, layout = asw.ERR_BAD_ARGUMENT, asw.ERR_UNSUPPORTED_METHOD, asw.ERR_UNSUPPORTED_LAYOUT
    good = ctx.stereoMatchingSmoothed(L, R, A.ADAPTIVE_WEIGHT, 5, 0, D)
    lib = _lib.lib()

    def call(left, right, out, alg, win, minD, numD, word, sigma_c=8.0, lam=900.0):
        li, ri, di = asw._image(left)[0], asw._image(right)[0], asw._image(out, 5)[0]
        return lib.asw_stereo_match_refined(ctx._h, C.byref(li), C.byref(ri), C.byref(di), int(alg), win, minD, numD, 0.0, word, sigma_c,
                                            lam, None, None)

    def expect(status, alg=A.ADAPTIVE_WEIGHT, win=5, minD=0, numD=D, word=SMOOTH | 3, left=L, right=R, two_channel=True, **kw):
        out = np.full(left.shape[:2], np.float32(-3.5))
        assert call(left, right, out, alg, win, minD, numD, word, **kw) == status, (int(alg), hex(word), kw)
        assert (out == np.float32(-3.5)).all()
        if two_channel:  # what a 2-channel asw_stereo_match returns for the same match
            with pytest.raises(AswError) as e:
                ctx2.stereoMatching(left, right, LEFT, alg, win, minD, numD, return_confidence=True)
            assert e.value.status == status
        assert bits(ctx.stereoMatchingSmoothed(L, R, A.ADAPTIVE_WEIGHT, 5, 0, D), good)

    # the methods that cannot give a confidence
    for alg, numD in ((A.SGBM, 16), (A.BM, 16), (A.NCC, D), (13, D), (255, D)):
        expect(unsupported, alg=alg, numD=numD)
    # the argument checks of a plain match, with its statuses
    expect(bad, numD=0)
    expect(bad, minD=-1)
    expect(bad, alg=asw.cross_algorithm(20, 0))
    expect(bad, win=65)
    expect(bad, alg=A.ADAPTIVE_WEIGHT_CROSS, win=37)
    expect(bad, alg=A.ADAPTIVE_WEIGHT_BLO1, minD=2)
    expect(layout, left=np.ascontiguousarray(L[..., :2]), right=np.ascontiguousarray(R[..., :2]))
    # the smoothing's own
    for word in (SMOOTH, SMOOTH | 9, SMOOTH | 0x100 | 3):
        expect(bad, word=word, two_channel=False)
    for v in (0.0, -2.0, float("nan"), float("inf")):
        expect(bad, sigma_c=v, two_channel=False)
        expect(bad, lam=v, two_channel=False)
    for T in (0, 9):
        with pytest.raises(AswError) as e:
            ctx.stereoMatchingSmoothed(L, R, A.ADAPTIVE_WEIGHT, 5, 0, D, iterations=T)
        assert e.value.status == bad
    # an even window keeps its status (and raises: the smoothed call is no reference function)
    with pytest.raises(AswError) as e:
        ctx.stereoMatchingSmoothed(L, R, A.ADAPTIVE_WEIGHT, 4, 0, D)
    assert e.value.status == asw.ERR_EVEN_WINDOW


def test_windows_without_the_flag_do_what_they_did(ctx, ctx2):
    """win_size 15 is the refinement, 37 (no window: above 35), 0 and a negative value are refused, through the same entries"""
    H, W, D = 14, 50, 10
    L, R = sr.textured_pair(H, W, 3, 3, 15)
    dl = ctx2.stereoMatching(L, R, 0, A.ADAPTIVE_WEIGHT_CROSS, 5, 0, D)
    dr = ctx2.stereoMatching(L, R, 1, A.ADAPTIVE_WEIGHT_CROSS, 5, 0, D)
    import refine_ref as rr

    want = rr.refine_vec(L, dl, dr, 0, D, 1.0, 15, 60.0, 9.0)
    ctx.smoothDisparity(L, dl, np.ones_like(dl))  # the smoothing has used the shared staging buffers just before
    got, nrej, nunf, mask = ctx.refineDisparity(L, dl, dr, 0, D, winSize=15, return_mask=True)
    assert bits(got, want["out"]) and np.array_equal(mask, want["mask"])
    assert (nrej, nunf) == (want["n_rejected"], want["n_unfillable"]) and nrej > 0
    m, nrej2, nunf2 = ctx.stereoMatchingRefined(L, R, A.ADAPTIVE_WEIGHT_CROSS, 5, 0, D, refineWin=15)
    assert bits(m, got) and (nrej2, nunf2) == (nrej, nunf)
    for win in (37, 0, -1, -(1 << 30), 16):
        with pytest.raises(AswError) as e:
            ctx.refineDisparity(L, dl, dr, 0, D, winSize=win)
        assert e.value.status == asw.ERR_BAD_ARGUMENT
        with pytest.raises(AswError) as e:
            ctx.stereoMatchingRefined(L, R, A.ADAPTIVE_WEIGHT_CROSS, 5, 0, D, refineWin=win)
        assert e.value.status == asw.ERR_BAD_ARGUMENT
    # a map outside the refinement's domain is still refused there, and accepted by the smoothing
    with pytest.raises(AswError) as e:
        ctx.refineDisparity(L, dl + np.float32(0.5), dr, 0, D, winSize=15)
    assert e.value.status == asw.ERR_BAD_ARGUMENT
    check(ctx, L, dl + np.float32(0.5), np.ones_like(dl))
