"""Semi-global matching over a chosen set of path directions on the GPU (asw_sgbm_paths, the C++ shim's getDisparity_SGBM_paths)
against the integer restatement of tests/sgbm_paths_ref.py.  Every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib
from aswstereomatch_amd.synth import make_pair

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgbm_paths_ref as pref  # noqa: E402
import sgbm_ref as ref  # noqa: E402
from shim_build import build_demo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


def _pair(H, W, D, cn, seed):
    L, R, _ = make_pair(H, W, max(2, D // 2), seed=seed, block=16)
    if cn == 1:
        return np.ascontiguousarray(L[:, :, 1]), np.ascontiguousarray(R[:, :, 1])
    return L, R


def _check(ctx, L, R, minD, D, w, P1, P2, m12, cap, U, sw, sr, paths):
    want = pref.sgbm_paths(L, R, minD, D, w, P1, P2, m12, cap, U, sw, sr, paths)
    got, vol = ctx.sgbm_paths(L, R, minD, D, w, P1, P2, m12, cap, U, sw, sr, paths=paths, return_cost_volume=True)
    assert np.array_equal(vol, np.moveaxis(want["S"], 2, 0).astype(np.float32))
    assert np.array_equal(got, want["disp"])
    return want


def _selector(cn, w):
    return 8 * cn * w * w, 32 * cn * w * w


# uniqueness 10, disp12MaxDiff 1, speckles 20 / 2 wherever there are more than 8 valid columns
FULL = (1, 10, 10, 20, 2)
# H, W, D, w, minD, cn, (P1, P2), (disp12MaxDiff, preFilterCap, uniquenessRatio, speckleWindowSize, speckleRange)
SHAPES = [
    (24, 40, 16, 1, 0, 3, _selector(3, 1), FULL),        # Wv = H: a full-length main diagonal
    (9, 131, 32, 5, 3, 3, _selector(3, 5), FULL),        # Wv >> H
    (90, 40, 16, 3, 0, 1, (10, 40), FULL),               # H >> Wv: lines bounded by the width
    (1, 60, 16, 3, 0, 1, _selector(1, 3), FULL),         # one row: every column and diagonal has length 1
    (30, 17, 16, 3, 0, 3, (7, 50), (0, 10, 0, 0, 0)),    # Wv = 1
    (33, 100, 80, 9, 0, 1, (600, 100), FULL),            # two candidates per lane, the second register partial; P2 <= P1
    (12, 300, 256, 3, 0, 3, _selector(3, 3), FULL),      # four candidates per lane
    (30, 40, 32, 5, 8, 3, (100, 400), FULL),             # W <= minD + D: the map all INVALID, the volume all zeros
]
MASKS = [0x07 | b for b in pref.NEW_BITS] + [pref.PATHS_HH4, pref.PATHS_SGBM, pref.PATHS_HH]
WIDEST = (4, 1100, 1024, 3, 0, 1, (20, 200), FULL)        # sixteen candidates per lane, every direction at once
CASES = [s + (m,) for s in SHAPES for m in MASKS] + [WIDEST + (pref.PATHS_HH,)]


@pytest.mark.parametrize("H,W,D,w,minD,cn,P,rest,paths", CASES)
def test_sgbm_paths_matches_restatement(ctx, H, W, D, w, minD, cn, P, rest, paths):
    L, R = _pair(H, W, min(D, 64), cn, seed=H * 7 + W)
    want = _check(ctx, L, R, minD, D, w, P[0], P[1], *rest, paths)
    if W <= minD + D:
        assert (want["disp"] == 16 * (minD - 1)).all() and not want["S"].any()


def test_sgbm_paths_many_concurrent_lines(ctx):
    # 120 + 196 - 1 = 315 lines per diagonal launch
    L, R = _pair(120, 260, 64, 3, seed=77)
    _check(ctx, L, R, 0, 64, 5, *_selector(3, 5), 1, 10, 10, 20, 2, pref.PATHS_HH)


@pytest.mark.parametrize("H,W,D,w,minD,cn,P,rest", [SHAPES[1], SHAPES[5]])
def test_three_way_mask_equals_sgbm(ctx, H, W, D, w, minD, cn, P, rest):
    L, R = _pair(H, W, D, cn, seed=H + W)
    a, va = ctx.sgbm(L, R, minD, D, w, P[0], P[1], *rest, return_cost_volume=True)
    b, vb = ctx.sgbm_paths(L, R, minD, D, w, P[0], P[1], *rest, paths=asw.SGBM_PATHS_3WAY, return_cost_volume=True)
    assert np.array_equal(a, b) and np.array_equal(va, vb)
    assert ctx.timing()["aggregate_launches"] == 2
    ctx.sgbm_paths(L, R, minD, D, w, P[0], P[1], *rest, paths=asw.SGBM_PATHS_HH)
    t = ctx.timing()
    assert t["aggregate_launches"] == 5 and 0 < t["aggregate_ms"] <= t["total_ms"]


def test_sgbm_paths_argument_errors(ctx):
    L, R = _pair(20, 64, 16, 3, seed=3)
    for kw, status in [(dict(paths=0x100), asw.ERR_BAD_ARGUMENT), (dict(paths=0x107), asw.ERR_BAD_ARGUMENT),
                       (dict(paths=-1), asw.ERR_BAD_ARGUMENT),
                       (dict(paths=0x30), asw.ERR_UNSUPPORTED_METHOD), (dict(paths=0x06), asw.ERR_UNSUPPORTED_METHOD),
                       (dict(paths=0), asw.ERR_UNSUPPORTED_METHOD),
                       # the cases of asw_sgbm (test_gpu_sgbm.py::test_sgbm_argument_errors) that do not involve mode
                       (dict(numDisparities=24), asw.ERR_BAD_ARGUMENT), (dict(numDisparities=0), asw.ERR_BAD_ARGUMENT),
                       (dict(minDisparity=-1), asw.ERR_BAD_ARGUMENT),
                       (dict(preFilterCap=1 << 24, blockSize=31), asw.ERR_BAD_ARGUMENT)]:   # n (C_max + P2) >= 2^31
        args = dict(minDisparity=0, numDisparities=16, blockSize=5)
        args.update(kw)
        with pytest.raises(asw.AswError) as e:
            ctx.sgbm_paths(L, R, args.pop("minDisparity"), args.pop("numDisparities"), args.pop("blockSize"), **args)
        assert e.value.status == status, kw
    with pytest.raises(asw.AswError) as e:
        ctx.sgbm_paths(L, R, 0, 16, 35, 8, 1 << 23, 0, 63, 10, 0, 0, return_cost_volume=True)
    assert e.value.status == asw.ERR_BAD_ARGUMENT
    ctx.sgbm_paths(L, R, 0, 16, 35, 8, 1 << 23, 0, 63, 10, 0, 0)
    # the bounds count the paths: C_max = 3 * (2 * 63 + 63) * 35^2 = 694575, P2 = 2^21: 8 (C_max + P2) = 22.3e6 >= 2^24 > 3 (C_max + P2)
    assert 8 * (ref.cost_bound(3, 35, 63) + (1 << 21)) >= 1 << 24 > 3 * (ref.cost_bound(3, 35, 63) + (1 << 21))
    with pytest.raises(asw.AswError) as e:
        ctx.sgbm_paths(L, R, 0, 16, 35, 8, 1 << 21, 0, 63, 10, 0, 0, paths=0xFF, return_cost_volume=True)
    assert e.value.status == asw.ERR_BAD_ARGUMENT
    ctx.sgbm_paths(L, R, 0, 16, 35, 8, 1 << 21, 0, 63, 10, 0, 0, paths=0xFF)
    ctx.sgbm_paths(L, R, 0, 16, 35, 8, 1 << 21, 0, 63, 10, 0, 0, paths=0x07, return_cost_volume=True)
    # 2^31: P2 = 2^28 passes with three paths (asw_sgbm's bound) and not with eight
    ctx.sgbm_paths(L, R, 0, 16, 5, 8, 1 << 28, 0, 10, 10, 0, 0, paths=0x07)
    with pytest.raises(asw.AswError) as e:
        ctx.sgbm_paths(L, R, 0, 16, 5, 8, 1 << 28, 0, 10, 10, 0, 0, paths=0xFF)
    assert e.value.status == asw.ERR_BAD_ARGUMENT


def test_sgbm_paths_output_layout(ctx):
    L, R = _pair(20, 64, 16, 3, seed=4)
    li, _ = asw._image(L)
    ri, _ = asw._image(R)
    out = np.zeros((20, 64), np.float32)
    oi = _lib.AswImage(out.ctypes.data, 20, 64, 1, 5, 64 * 4)
    # asw_sgbm_paths is an inline function of the header: asw_sgbm with ASW_SGBM_MODE_PATHS | paths as its mode
    hdr = open(os.path.join(ROOT, "include", "asw_mi355x.h")).read()
    assert "ASW_SGBM_MODE_PATHS = 0x%X" % asw._SGBM_MODE_PATHS in hdr
    rc = _lib.lib().asw_sgbm(ctx._h, C.byref(li), C.byref(ri), C.byref(oi), 0, 16, 5, 0, 0, 0, 0, 0, 0, 0,
                             asw._SGBM_MODE_PATHS | 0xFF, None, 0)
    assert rc == asw.ERR_UNSUPPORTED_LAYOUT
    # a mode that neither StereoSGBM nor a path mask forms stays unserved
    oi16 = np.zeros((20, 64), np.int16)
    oj, _ = asw._image(oi16, 3)
    for mode, status in ((-1, asw.ERR_UNSUPPORTED_METHOD), (3, asw.ERR_UNSUPPORTED_METHOD), (0x100, asw.ERR_UNSUPPORTED_METHOD),
                         (asw._SGBM_MODE_PATHS | 0x100, asw.ERR_BAD_ARGUMENT), (asw._SGBM_MODE_PATHS | 0x30, asw.ERR_UNSUPPORTED_METHOD),
                         (asw._SGBM_MODE_PATHS | 0x07, asw.OK)):
        rc = _lib.lib().asw_sgbm(ctx._h, C.byref(li), C.byref(ri), C.byref(oj), 0, 16, 5, 0, 0, 0, 0, 0, 0, 0, mode, None, 0)
        assert rc == status, hex(mode)


# ---------------------------------------------------------------- the C++ shim
@pytest.mark.parametrize("cv", [False, True])
def test_shim_get_disparity_sgbm_paths(ctx, tmp_path, cv):
    exe = build_demo("sgbm_paths_demo.cpp", tmp_path / "sgbm_paths_demo", cv)
    L, R = _pair(40, 96, 32, 3, seed=53)
    L.tofile(tmp_path / "l.raw")
    R.tofile(tmp_path / "r.raw")
    out = tmp_path / "d.raw"
    for paths in (pref.PATHS_HH, pref.PATHS_SGBM):
        r = subprocess.run([exe, "40", "96", "3", str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), "5", "0", "32", hex(paths), str(out)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.strip() == "ok 40 96 three_way_same=1", (r.stdout, r.stderr)
        got = np.fromfile(out, np.uint8).reshape(40, 96)
        assert np.array_equal(got, pref.get_disparity_sgbm_paths(L, R, 5, 0, 32, paths))
    for win, numD, paths in (("4", "32", "0xff"), ("5", "24", "0xff"), ("5", "32", "0x30"), ("5", "32", "0x100")):
        r = subprocess.run([exe, "40", "96", "3", str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), win, "0", numD, paths, str(out)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("error"), r.stdout
