"""The integer kernels (k_sgbm.hip with filterSpeckles, k_bm.hip, k_refine.hip, k_subpixel.hip) on the inputs the textured pairs of
the neighbouring files never produce: costs that tie, frames of one or two rows or one valid column, padded rows, the edges of
filterSpeckles, and a seeded sweep over random shapes and parameters (tests/matcher_cases.py).  Every comparison is np.array_equal
against tests/sgbm_ref.py / tests/stereobm_ref.py / tests/refine_ref.py / tests/subpixel_ref.py.

The two matchers break ties in opposite directions (StereoSGBM: the smallest disparity, the lowest x in the left-right rule;
StereoBM: the largest disparity, the first x), and tests/test_matcher_cases_cpu.py pins the restatements' side of that by answers
derived from OpenCV's loops.  A tie case that degenerates to "everything invalid" would prove nothing, so the cases of that file's
table first assert, on the restatement alone, that at least half the pixels tie and at least half are not the invalid value."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matcher_cases as mc  # noqa: E402
import sgbm_ref  # noqa: E402
import stereobm_ref  # noqa: E402

A = asw.StereoMatchingAlgorithms
LEFT = asw.DISPARITY_LEFT
H, W, BLOCK = 20, 150, 5

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


# kind -> pair of H x W (x cn)
def _tie_pair(kind, cn):
    return mc.tie_pair(kind, H, W, cn)


TIE_KINDS = mc.TIE_KINDS


def _sgbm_check(ctx, L, R, minD, D, w, P1, P2, m12, cap, U, sw=0, sr=0):
    want = sgbm_ref.sgbm(L, R, minD, D, w, P1, P2, m12, cap, U, sw, sr)
    got, vol = ctx.sgbm(L, R, minD, D, w, P1, P2, m12, cap, U, sw, sr, return_cost_volume=True)
    tag = (L.shape, minD, D, w, P1, P2, m12, cap, U, sw, sr)
    assert np.array_equal(vol, np.moveaxis(want["S"], 2, 0).astype(np.float32)), tag
    assert got.dtype == np.int16 and np.array_equal(got, want["disp"]), tag
    return want


def _bm_check(ctx, L, R, minD, D, w, cap=31, tex=10, U=15, sw=0, sr=0, M=-1):
    want = stereobm_ref.stereo_bm(L, R, minD, D, w, cap, tex, U, sw, sr, M)
    got, vol = ctx.stereoBM(L, R, minD, D, w, asw.PREFILTER_XSOBEL, 9, cap, tex, U, sw, sr, M, return_cost_volume=True)
    tag = (L.shape, minD, D, w, cap, tex, U, sw, sr, M)
    assert np.array_equal(vol, want["vol"], equal_nan=True), tag
    assert got.dtype == np.int16 and np.array_equal(got, want["disp"]), tag
    return want


# ---------------------------------------------------------------- ties
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("D", [32, 80])  # D = 80: two candidates per lane, a tie can sit in two registers of one lane
@pytest.mark.parametrize("kind", TIE_KINDS)
def test_sgbm_tied_costs(ctx, kind, D, cn):
    L, R = _tie_pair(kind, cn)
    for cap, minD, U, m12 in itertools.product((1, 10, 63), (0, 5), (0, 10), (-1, 0, 1)):
        want = _sgbm_check(ctx, L, R, minD, D, BLOCK, 200, 800, m12, cap, U)
        # the rows of the table in tests/test_matcher_cases_cpu.py: floors on the restatement alone
        if (D, cn, cap, U, m12) != (32, 1, 10, 0, -1):
            continue
        ties = mc.tie_share(want["S"][:, minD + D:], 2)
        alive = float((want["disp"] != 16 * (minD - 1)).mean())
        if (kind, minD) == ("periodic4", 0):
            print("SGBM periodic(4, 3): tie share %.3f, not-invalid share %.3f" % (ties, alive))
            assert ties >= 0.5 and alive >= 0.5
        if (kind, minD) == ("constant", 5):  # the tie share only; at minD = 0 this pair does not tie under SGBM
            print("SGBM constant minD 5: tie share %.3f" % ties)
            assert ties >= 0.5
            assert (want["disp"][:, minD + D:] == 16 * minD).all()  # the smallest disparity


@pytest.mark.parametrize("D", [32, 80])
@pytest.mark.parametrize("kind", TIE_KINDS)
def test_stereo_bm_tied_costs(ctx, kind, D):
    L, R = _tie_pair(kind, 1)
    for cap, tex, U, m12, minD in itertools.product((1, 31), (0, 10), (0, 15), (-1, 0, 1), (0, 5)):
        want = _bm_check(ctx, L, R, minD, D, BLOCK, cap, tex, U, 0, 0, m12)
        # the rows of the table in tests/test_matcher_cases_cpu.py: floors on the restatement alone
        if (D, cap, tex, U, minD) != (32, 31, 0, 0, 0):
            continue
        ties = mc.tie_share(want["vol"], 0)
        if kind in ("periodic4", "periodic8") and m12 == 1:
            alive = float((want["disp"] != 16 * (minD - 1)).mean())
            print("BM %s: tie share %.3f, not-invalid share %.3f" % (kind, ties, alive))
            assert ties >= 0.5 and alive >= 0.5
        if kind == "constant" and m12 == -1:  # the tie share only
            print("BM constant: tie share %.3f" % ties)
            assert ties >= 0.5
            y0, y1, x0, x1 = stereobm_ref.valid_roi(H, W, minD, D, BLOCK)
            assert (want["disp"][y0:y1, x0:x1] == 16 * (minD + D - 1)).all()  # the largest disparity


@pytest.mark.parametrize("kind", ["constant", "periodic4", "periodic8"])
def test_selector_entries_on_tied_costs(ctx, kind):
    for cn in (1, 3):
        L, R = _tie_pair(kind, cn)
        for win, minD, D in ((5, 0, 32), (9, 5, 32), (5, 0, 80)):
            want = sgbm_ref.get_disparity_sgbm(L, R, win, minD, D)
            got = ctx.stereoMatching(L, R, LEFT, A.SGBM, win, minD, D)
            assert got.dtype == np.float32 and np.array_equal(got, want), (cn, win, minD, D)
            assert np.array_equal(ctx.getDisparity_SGBM(L, R, win, minD, D), want), (cn, win, minD, D)
    L, R = _tie_pair(kind, 1)
    for win, minD, D in ((5, 0, 32), (9, 5, 32), (5, 0, 80)):
        want = stereobm_ref.get_disparity_bm(L, R, win, minD, D)
        got = ctx.getDisparity_BM(L, R, win, minD, D)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (win, minD, D)


# ---------------------------------------------------------------- tiny and ragged frames
_noise = mc.noise


@pytest.mark.parametrize("Hn,Wn,minD,D,w", mc.SGBM_TINY_FRAMES)
def test_sgbm_tiny_and_ragged_frames(ctx, Hn, Wn, minD, D, w):
    L, R = _noise(Hn, Wn, Hn * 1000 + Wn)
    assert Wn - minD - D >= 1
    for P1, P2, m12, cap, U in mc.sgbm_tiny_settings(w):
        want = _sgbm_check(ctx, L, R, minD, D, w, P1, P2, m12, cap, U)
        assert want["S"][:, minD + D:].any()
    L3 = np.stack([L, R, L], axis=2)
    R3 = np.stack([R, L, R[::-1]], axis=2)
    _sgbm_check(ctx, np.ascontiguousarray(L3), np.ascontiguousarray(R3), minD, D, w, 0, 0, 0, 0, -1)


@pytest.mark.parametrize("Hn,Wn,minD,D,w", [
    (5, 40, 0, 16, 5), (6, 40, 0, 16, 5),       # one and two valid rows, odd and even H
    (9, 24, 0, 16, 9), (9, 25, 0, 16, 9),       # valid_roi one and two pixels wide
    (12, 100, 3, 48, 11),
])
def test_stereo_bm_tiny_and_ragged_frames(ctx, Hn, Wn, minD, D, w):
    L, R = _noise(Hn, Wn, Hn * 1000 + Wn)
    y0, y1, x0, x1 = stereobm_ref.valid_roi(Hn, Wn, minD, D, w)
    if (Hn, Wn) in ((5, 40), (9, 24)):
        assert (y1 - y0 == 1) if Hn == 5 else (x1 - x0 == 1)
    for tex, U, m12 in ((0, 0, -1), (10, 15, 1), (0, 0, 0)):
        want = _bm_check(ctx, L, R, minD, D, w, 31, tex, U, 0, 0, m12)
    assert (_bm_check(ctx, L, R, minD, D, w, 31, 0, 0, 0, 0, -1)["disp"][y0:y1, x0:x1] != 16 * (minD - 1)).all()
    assert want["disp"].shape == (Hn, Wn)


# ---------------------------------------------------------------- padded rows for SGBM and filterSpeckles
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("Wn", [97, 129])
def test_sgbm_padded_views(ctx, Wn, cn):
    Hn = 31
    Lw, Rw = mc.textured(Hn, Wn + 37, cn, seed=Wn, D=32)
    L, R = Lw[:, 5:5 + Wn], Rw[:, 5:5 + Wn]            # padded rows: step = (Wn + 37) * cn
    assert L.strides[0] == (Wn + 37) * cn and not L.flags["C_CONTIGUOUS"]
    args = (1, 32, 7, 8 * cn * 49, 32 * cn * 49, 1, 10, 10, 20, 2)
    want = _sgbm_check(ctx, L, R, *args)
    assert (want["disp"] != 0).any()
    # a padded int16 output: rows of Wn + 3 shorts, the padding untouched
    out = np.full((Hn, Wn + 3), 12345, np.int16)
    li, _ = asw._image(L)
    ri, _ = asw._image(R)
    assert li.step == (Wn + 37) * cn
    oi = _lib.AswImage(out.ctypes.data, Hn, Wn, 1, 3, (Wn + 3) * 2)
    rc = _lib.lib().asw_sgbm(ctx._h, C.byref(li), C.byref(ri), C.byref(oi), *args, asw.MODE_SGBM_3WAY, None, 0)
    assert rc == 0
    assert np.array_equal(out[:, :Wn], want["disp"]) and (out[:, Wn:] == 12345).all()
    # the selector's entry on the same views
    got = ctx.stereoMatching(L, R, LEFT, A.SGBM, 7, 1, 32)
    assert np.array_equal(got, sgbm_ref.get_disparity_sgbm(L, R, 7, 1, 32))
    assert np.array_equal(got, ctx.stereoMatching(np.ascontiguousarray(L), np.ascontiguousarray(R), LEFT, A.SGBM, 7, 1, 32))


def _speckles_in_place(ctx, view, new_val, size, diff):
    """asw_filter_speckles on `view` itself (the Python binding works on a copy)"""
    img = _lib.AswImage(view.ctypes.data, view.shape[0], view.shape[1], 1, 3, view.strides[0])
    return _lib.lib().asw_filter_speckles(ctx._h, C.byref(img), new_val, size, diff)


@pytest.mark.parametrize("Hn,Wn,pad", [(40, 97, 3), (1, 130, 1), (33, 1, 7)])
def test_filter_speckles_padded_view_in_place(ctx, Hn, Wn, pad):
    m = mc.build_case("speckles", (Hn, Wn, 11, -16, 20, 16))["map"]
    wide = np.full((Hn, Wn + pad), 12345, np.int16)
    wide[:, :Wn] = m
    assert _speckles_in_place(ctx, wide[:, :Wn], -16, 20, 16) == 0
    want = sgbm_ref.filter_speckles(m, -16, 20, 16)
    assert np.array_equal(wide[:, :Wn], want) and (wide[:, Wn:] == 12345).all()
    if Hn * Wn > 1000:
        assert not np.array_equal(want, m) and (want != -16).any()


# ---------------------------------------------------------------- filterSpeckles edges
def _spk(ctx, m, new_val, size, diff):
    m = np.ascontiguousarray(m, np.int16)
    want = sgbm_ref.filter_speckles(m, new_val, size, diff)
    assert np.array_equal(ctx.filterSpeckles(m, new_val, size, diff), want), (m.shape, new_val, size, diff)
    return want


def test_filter_speckles_one_pixel_and_one_line(ctx):
    one = np.array([[40]], np.int16)
    assert _spk(ctx, one, -16, 0, 16)[0, 0] == 40      # maxSpeckleSize 0: kept
    assert _spk(ctx, one, -16, 1, 16)[0, 0] == -16     # a component of 1 pixel: removed
    assert _spk(ctx, np.array([[-16]], np.int16), -16, 1, 16)[0, 0] == -16
    for shape in ((1, 300), (300, 1)):
        m = mc.build_case("speckles", shape + (3, -16, 0, 0))["map"]
        for size, diff in ((0, 16), (3, 16), (20, 48), (300, 1000), (2, 0)):
            _spk(ctx, m, -16, size, diff)
        assert not np.array_equal(_spk(ctx, m, -16, 20, 48), m)
        assert np.array_equal(_spk(ctx, m, -16, 0, 48), m)


def test_filter_speckles_contents(ctx):
    full = np.full((9, 70), -16, np.int16)
    assert np.array_equal(_spk(ctx, full, -16, 100, 16), full)                 # all newVal: nothing to label
    m = mc.build_case("speckles", (23, 131, 5, -16, 0, 0))["map"]
    assert (m != -1000).all()
    for size in (0, 1, 20, 400):
        _spk(ctx, m, -1000, size, 16)                                         # no newVal in the map at all
    assert (_spk(ctx, m, -1000, 23 * 131, 1 << 20) == -1000).all()            # one component: the whole map
    ext = np.array([[32767, -32768, 32767], [-32768, 0, -32768]], np.int16)    # a difference taken in 16 bits would wrap
    # maxDiff 65534: |32767 - -32768| = 65535 keeps the corners apart, 0 joins its three neighbours into a component of 4
    assert np.array_equal(_spk(ctx, ext, -16, 3, 65534), [[-16, -32768, -16], [-32768, 0, -32768]])
    assert (_spk(ctx, ext, -16, 6, 65535) == -16).all()                       # one component of 6
    assert np.array_equal(_spk(ctx, ext, -16, 5, 65535), ext)


def test_filter_speckles_size_and_difference_thresholds(ctx):
    m = np.full((12, 40), -16, np.int16)
    m[2:4, 3:8] = 100          # 10 pixels
    m[7:8, 3:14] = 100         # 11 pixels
    want = _spk(ctx, m, -16, 10, 0)       # maxDiff 0: equal values still join
    assert (want[2:4, 3:8] == -16).all() and (want[7, 3:14] == 100).all()
    m[2, 3:8] = 101                        # maxDiff 0 now splits the 10 into two fives
    assert (_spk(ctx, m, -16, 5, 0)[2:4, 3:8] == -16).all()
    assert np.array_equal(_spk(ctx, m, -16, 4, 0), m)
    assert (_spk(ctx, m, -16, 10, 1)[7, 3:14] == 100).all()


@pytest.mark.parametrize("Wn", [63, 64, 65, 255, 256, 257])
def test_filter_speckles_runs_across_wavefront_boundaries(ctx, Wn):
    # horizontal runs that start and end on either side of the 64-pixel boundaries k_spk_flatten counts by
    m = np.full((6, Wn), -16, np.int16)
    m[0, :] = 10                                   # the whole row: Wn pixels
    m[2, max(Wn - 70, 0):Wn - 1] = 20              # ends one short of the row's end
    m[4, 1:min(66, Wn)] = 30                       # crosses the first boundary
    m[5, 60:min(130, Wn)] = 40                     # next to it, |40 - 30| > maxDiff: a component of its own
    sizes = sorted({Wn, int((m[2] == 20).sum()), int((m[4] == 30).sum()), int((m[5] == 40).sum())})
    for n in sizes:
        for size in (n - 1, n):
            _spk(ctx, m, -16, size, 5)
    assert (_spk(ctx, m, -16, Wn, 5) == -16).all() and (_spk(ctx, m, -16, Wn - 1, 5)[0] == 10).all()


# ---------------------------------------------------------------- the seeded sweep
@pytest.mark.parametrize("seed", mc.SWEEP_SEEDS)
@pytest.mark.parametrize("family", mc.FAMILIES)
def test_seeded_sweep(ctx, family, seed):
    for case in mc.cases(family, seed):
        got, want = mc.gpu_result(ctx, case)
        for k in want:
            floating = np.issubdtype(np.asarray(want[k]).dtype, np.floating)
            assert np.array_equal(got[k], want[k], equal_nan=floating), \
                "%s differs: matcher_cases.build_case(%r, %r)" % (k, family, case["tag"])
