"""Block matching on the GPU (asw_stereo_bm, asw_get_disparity_bm, the C++ shim's getDisparity_BM) against the integer
restatement of tests/stereobm_ref.py.  Every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib
from aswstereomatch_amd.synth import make_pair, shifted_pair

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvlite  # noqa: E402
import stereobm_ref as ref  # noqa: E402
from shim_build import build_demo  # noqa: E402

A = asw.StereoMatchingAlgorithms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


def _pair(H, W, D, seed, cn=1):
    L, R, _ = make_pair(H, W, max(2, min(D, W // 3) // 2), seed=seed, block=16)
    if cn == 1:
        return np.ascontiguousarray(L[:, :, 1]), np.ascontiguousarray(R[:, :, 1])
    return L, R


def _check(ctx, L, R, minD, D, w, cap=31, tex=10, U=15, sw=0, sr=0, M=-1):
    want = ref.stereo_bm(L, R, minD, D, w, cap, tex, U, sw, sr, M)
    got, vol = ctx.stereoBM(L, R, minD, D, w, asw.PREFILTER_XSOBEL, 9, cap, tex, U, sw, sr, M, return_cost_volume=True)
    assert got.dtype == np.int16 and np.array_equal(got, want["disp"])
    assert np.array_equal(vol, want["vol"], equal_nan=True)
    assert np.array_equal(ctx.stereoBM(L, R, minD, D, w, asw.PREFILTER_XSOBEL, 9, cap, tex, U, sw, sr, M), got)  # no volume
    return want


# H, W, minD, D, w, preFilterCap, textureThreshold, uniquenessRatio, disp12MaxDiff, speckleWindowSize, speckleRange
CASES = [
    (40, 120, 0, 16, 5, 31, 10, 15, -1, 0, 0),
    (37, 131, 3, 32, 9, 1, 0, 0, 0, 0, 0),              # cap 1, odd H, no rules, disp12MaxDiff 0
    (50, 150, 17, 48, 15, 63, 10, 100, 1, 0, 0),        # minD 17, cap 63, uniqueness 100
    (45, 200, 5, 64, 21, 31, 500, 15, 200, 50, 16),     # a large texture threshold, speckles
    (64, 300, 0, 80, 7, 20, 10, 15, 1, 20, 2),          # D = 80: two chunks per lane, lanes past D masked
    (70, 160, 2, 16, 51, 31, 10, 15, 1, 100, 32),       # w = 51
    (30, 90, 0, 16, 5, 31, 10 ** 6, 15, 1, 0, 0),       # texture beyond every window: all FILTERED
    (41, 260, 1, 160, 11, 31, 10, 15, 1, 100, 32),      # D = 160: three chunks
    (23, 700, 0, 512, 5, 31, 10, 15, 1, 0, 0),          # D = 512: eight chunks
    (25, 1100, 0, 1024, 5, 31, 10, 0, 0, 10, 4),        # D = 1024: sixteen chunks
]


@pytest.mark.parametrize("H,W,minD,D,w,cap,tex,U,M,sw,sr", CASES)
def test_stereo_bm_matches_restatement(ctx, H, W, minD, D, w, cap, tex, U, M, sw, sr):
    L, R = _pair(H, W, D, seed=H * 13 + W)
    want = _check(ctx, L, R, minD, D, w, cap, tex, U, sw, sr, M)
    if tex == 10 ** 6:
        assert (want["disp"] == 16 * (minD - 1)).all()
    if sw == 0 and U == 0:
        assert (want["disp"] != 16 * (minD - 1)).any()


def test_stereo_bm_widest_window(ctx):
    L, R = _pair(262, 300, 16, seed=255)
    _check(ctx, L, R, 0, 16, 255, 31, 10, 15, 10, 4, 1)


def test_stereo_bm_shifted_pair(ctx):
    d0 = 13
    L3, R3 = shifted_pair(60, 200, d0)
    L, R = L3[:, :, 1].copy(), R3[:, :, 1].copy()
    want = _check(ctx, L, R, 0, 32, 9, M=1)
    y0, y1, x0, x1 = ref.valid_roi(60, 200, 0, 32, 9)
    assert ((want["disp"][y0:y1, x0:x1] + 8) >> 4 == d0).mean() > 0.98


@pytest.mark.parametrize("W", [97, 129, 1021])
def test_stereo_bm_awkward_widths_and_padded_views(ctx, W):
    H = 53
    Lw, Rw = _pair(H, W + 37, 32, seed=W)
    L, R = Lw[:, 5:5 + W], Rw[:, 5:5 + W]          # padded rows: step = W + 37
    assert L.strides[0] == W + 37
    want = _check(ctx, L, R, 1, 32, 7, 31, 10, 15, 20, 2, 1)
    # a padded int16 output: rows of W + 3 shorts, the padding untouched
    out = np.full((H, W + 3), 12345, np.int16)
    li, _ = asw._image(L)
    ri, _ = asw._image(R)
    oi = _lib.AswImage(out.ctypes.data, H, W, 1, 3, (W + 3) * 2)
    rc = _lib.lib().asw_stereo_bm(ctx._h, C.byref(li), C.byref(ri), C.byref(oi), 1, 32, 7, 1, 9, 31, 10, 15, 20, 2, 1, None, 0)
    assert rc == 0
    assert np.array_equal(out[:, :W], want["disp"]) and (out[:, W:] == 12345).all()


@pytest.mark.parametrize("H,W,minD,D,w", [(30, 38, 0, 32, 9), (20, 20, 3, 16, 5), (12, 64, 60, 16, 5)])
def test_stereo_bm_empty_valid_region(ctx, H, W, minD, D, w):
    L, R = _pair(H, W, D, seed=3)
    assert ref.valid_roi(H, W, minD, D, w) is None
    got, vol = ctx.stereoBM(L, R, minD, D, w, speckleWindowSize=100, speckleRange=32, disp12MaxDiff=1, return_cost_volume=True)
    assert (got == 16 * (minD - 1)).all() and np.isnan(vol).all()


def test_stereo_bm_shape_changes_on_one_context(ctx):
    shapes = [(120, 400, 2, 64, 15), (31, 90, 0, 16, 5), (200, 640, 0, 128, 9), (31, 90, 0, 16, 5), (45, 210, 5, 32, 7)]
    for i, (H, W, minD, D, w) in enumerate(shapes):
        L, R = _pair(H, W, D, seed=70 + i)
        _check(ctx, L, R, minD, D, w, 31, 10, 15, 100, 32, 1)


def _status(ctx, L, R, disp=None, vol=None, vol_floats=0, **kw):
    args = dict(minD=0, numD=16, w=5, ptype=1, psize=9, cap=31, tex=10, U=15, sw=0, sr=0, M=-1)
    args.update(kw)
    li, _ = asw._image(L)
    ri, _ = asw._image(R)
    if disp is None:
        disp = np.zeros(L.shape[:2], np.int16)
    depth = {np.dtype(np.int16): 3, np.dtype(np.float32): 5, np.dtype(np.uint8): 0}[disp.dtype]
    di = _lib.AswImage(disp.ctypes.data, disp.shape[0], disp.shape[1], 1, depth, disp.strides[0])
    pv = None if vol is None else vol.ctypes.data_as(C.c_void_p)
    return _lib.lib().asw_stereo_bm(ctx._h, C.byref(li), C.byref(ri), C.byref(di), args["minD"], args["numD"], args["w"],
                                    args["ptype"], args["psize"], args["cap"], args["tex"], args["U"], args["sw"], args["sr"],
                                    args["M"], pv, vol_floats)


def test_stereo_bm_error_statuses(ctx):
    L, R = _pair(40, 100, 16, seed=5)
    assert _status(ctx, L, R) == asw.OK
    for kw, st in [(dict(ptype=0), asw.ERR_UNSUPPORTED_METHOD), (dict(ptype=2), asw.ERR_BAD_ARGUMENT),
                   (dict(psize=4), asw.ERR_BAD_ARGUMENT), (dict(psize=8), asw.ERR_BAD_ARGUMENT),
                   (dict(psize=257), asw.ERR_BAD_ARGUMENT), (dict(cap=0), asw.ERR_BAD_ARGUMENT),
                   (dict(cap=64), asw.ERR_BAD_ARGUMENT), (dict(w=3), asw.ERR_BAD_ARGUMENT), (dict(w=6), asw.ERR_BAD_ARGUMENT),
                   (dict(w=41), asw.ERR_BAD_ARGUMENT), (dict(numD=0), asw.ERR_BAD_ARGUMENT),
                   (dict(numD=24), asw.ERR_BAD_ARGUMENT), (dict(numD=1040), asw.ERR_BAD_ARGUMENT),
                   (dict(minD=-1), asw.ERR_BAD_ARGUMENT), (dict(minD=2000, numD=64), asw.ERR_BAD_ARGUMENT),
                   (dict(tex=-1), asw.ERR_BAD_ARGUMENT), (dict(U=-1), asw.ERR_BAD_ARGUMENT)]:
        assert _status(ctx, L, R, **kw) == st, kw
    assert _status(ctx, L, R, w=39) == asw.OK                               # blockSize up to min(H, W) = 40 is allowed
    L3, R3 = _pair(40, 100, 16, seed=5, cn=3)
    assert _status(ctx, L3, R3) == asw.ERR_UNSUPPORTED_LAYOUT                # StereoBM takes 8UC1 only
    assert _status(ctx, L, R, disp=np.zeros((40, 100), np.float32)) == asw.ERR_UNSUPPORTED_LAYOUT
    assert _status(ctx, L, R, disp=np.zeros((40, 99), np.int16)) == asw.ERR_BAD_ARGUMENT
    assert _status(ctx, L, R[:, :99].copy()) == asw.ERR_SIZE_MISMATCH
    vol = np.full(16 * 40 * 100, 7.0, np.float32)
    assert _status(ctx, L, R, vol=vol, vol_floats=vol.size - 1) == asw.ERR_BAD_ARGUMENT
    assert (vol == 7.0).all()                                                # refused before anything is written
    with pytest.raises(asw.AswError) as e:
        ctx.stereoBM(L, R, 0, 16, 5, preFilterType=asw.PREFILTER_NORMALIZED_RESPONSE)
    assert e.value.status == asw.ERR_UNSUPPORTED_METHOD


def test_get_disparity_bm_error_statuses(ctx):
    L, R = _pair(40, 100, 16, seed=6)
    for win, minD, numD, st in [(15, 0, 24, asw.ERR_UNSUPPORTED_METHOD), (14, 0, 64, asw.ERR_UNSUPPORTED_METHOD),
                                (0, 0, 64, asw.ERR_UNSUPPORTED_METHOD), (3, 0, 16, asw.ERR_UNSUPPORTED_METHOD),
                                (41, 0, 16, asw.ERR_UNSUPPORTED_METHOD), (257, 0, 16, asw.ERR_UNSUPPORTED_METHOD),
                                (15, 0, 0, asw.ERR_UNSUPPORTED_METHOD), (15, -1, 16, asw.ERR_BAD_ARGUMENT)]:
        with pytest.raises(asw.AswError) as e:
            ctx.getDisparity_BM(L, R, win, minD, numD)
        assert e.value.status == st, (win, minD, numD)
    with pytest.raises(asw.AswError) as e:
        ctx.getDisparity_BM(np.zeros((0, 0), np.uint8), np.zeros((0, 0), np.uint8), 15, 0, 16)
    assert e.value.status == asw.ERR_UNSUPPORTED_METHOD
    # the selector's BM value is left as it was
    with pytest.raises(asw.AswError) as e:
        ctx.stereoMatching(L, R, asw.DISPARITY_LEFT, A.BM, 15, 0, 64)
    assert e.value.status == asw.ERR_UNSUPPORTED_METHOD


@pytest.mark.parametrize("H,W,D", [(360, 640, 64), (1080, 1920, 128)])
def test_get_disparity_bm_driver_shapes(ctx, H, W, D):
    L3, R3 = _pair(H, W, D, seed=H, cn=3)
    try:
        for bits in (14, 15):
            ctx.set_gray_bits(bits)
            gl, gr = cvlite.cvtColor_BGR2GRAY(L3, bits), cvlite.cvtColor_BGR2GRAY(R3, bits)
            want = ref.get_disparity_bm(gl, gr, 15, 0, D)
            got = ctx.getDisparity_BM(L3, R3, 15, 0, D)
            assert got.dtype == np.uint8 and np.array_equal(got, want), bits
            assert np.array_equal(ctx.getDisparity_BM(gl, gr, 15, 0, D), want), bits   # 1-channel input
            assert (want > 0).mean() > 0.3
    finally:
        ctx.set_gray_bits(14)


def test_get_disparity_bm_defaults_and_module_binding(ctx):
    L, R = _pair(80, 200, 32, seed=8)
    assert np.array_equal(ctx.getDisparity_BM(L, R, -1, 2, 32), ref.get_disparity_bm(L, R, -1, 2, 32))  # win <= 0 -> 9
    assert np.array_equal(asw.getDisparity_BM(L, R, 7, 0, 32), ref.get_disparity_bm(L, R, 7, 0, 32))


@pytest.mark.parametrize("cv", [False, True])
def test_shim_get_disparity_bm(ctx, tmp_path, cv):
    exe = build_demo("bm_demo.cpp", tmp_path / "bm_demo", cv)
    for cn in (3, 1):
        L, R = _pair(48, 160, 32, seed=90 + cn, cn=cn)
        L.tofile(tmp_path / "l.raw")
        R.tofile(tmp_path / "r.raw")
        out = tmp_path / "d.raw"
        r = subprocess.run([exe, "48", "160", str(cn), str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), "9", "0", "32", str(out)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.strip() == "ok 48 160 selector_throws=1", (r.stdout, r.stderr)
        got = np.fromfile(out, np.uint8).reshape(48, 160)
        gl, gr = (L, R) if cn == 1 else (cvlite.cvtColor_BGR2GRAY(L), cvlite.cvtColor_BGR2GRAY(R))
        assert np.array_equal(got, ref.get_disparity_bm(gl, gr, 9, 0, 32))
    for win, numD in (("8", "32"), ("9", "24")):
        r = subprocess.run([exe, "48", "160", "1", str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), win, "0", numD, str(out)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("error"), r.stdout
