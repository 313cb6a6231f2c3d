"""Semi-global block matching on the GPU (asw_sgbm, asw_filter_speckles, the selector's SGBM entry, the C++ shim) against the
integer restatement of tests/sgbm_ref.py.  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd.synth import make_pair, shifted_pair

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgbm_ref as ref  # noqa: E402
from shim_build import build_demo  # noqa: E402

A = asw.StereoMatchingAlgorithms
LEFT, RIGHT = asw.DISPARITY_LEFT, asw.DISPARITY_RIGHT

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


def _check(ctx, L, R, minD, D, w, P1, P2, m12, cap, U, sw, sr):
    want = ref.sgbm(L, R, minD, D, w, P1, P2, m12, cap, U, sw, sr)
    got, vol = ctx.sgbm(L, R, minD, D, w, P1, P2, m12, cap, U, sw, sr, return_cost_volume=True)
    assert np.array_equal(vol, np.moveaxis(want["S"], 2, 0).astype(np.float32))
    assert np.array_equal(got, want["disp"])
    return want


# H, W, D, w, minD, cn, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio, speckleWindowSize, speckleRange
CASES = [
    (24, 40, 16, 1, 0, 3, 8, 32, 1, 10, 10, 0, 0),
    (37, 131, 32, 5, 3, 3, 8 * 3 * 25, 32 * 3 * 25, 200, 10, 10, 0, 0),
    (64, 200, 64, 15, 0, 3, 8 * 3 * 225, 32 * 3 * 225, 200, 10, 10, 175, 32),
    (120, 260, 16, 3, 0, 1, 8 * 9, 32 * 9, 1, 10, 10, 20, 2),
    (100, 180, 48, 35, 0, 3, 8 * 3 * 1225, 32 * 3 * 1225, 200, 10, 10, 0, 0),
    (30, 40, 32, 5, 8, 3, 100, 400, 1, 10, 10, 10, 1),        # W <= maxD: every pixel INVALID
    (30, 70, 16, 3, 0, 3, 0, 0, 0, 0, -1, 0, 0),               # every parameter at its default (step 0)
    (40, 96, 32, 5, 0, 1, 600, 100, 3, 31, 0, 0, 0),           # P2 <= P1, cap 31, no uniqueness rule
    (40, 96, 32, 5, 2, 3, 50, 800, 2, 62, 25, 30, 4),          # cap 62, strict uniqueness, speckles
    (20, 64, 16, 7, 0, 3, 20, 200, 1, 15, 5, 4, 1),            # 64-bit uniqueness products
    (33, 100, 80, 9, 0, 1, 100, 1000, 5, 20, 10, 50, 3),       # D = 80: two candidates per lane
]


@pytest.mark.parametrize("H,W,D,w,minD,cn,P1,P2,m12,cap,U,sw,sr", CASES)
def test_sgbm_matches_restatement(ctx, H, W, D, w, minD, cn, P1, P2, m12, cap, U, sw, sr):
    L, R = _pair(H, W, D, cn, seed=H * 7 + W)
    want = _check(ctx, L, R, minD, D, w, P1, P2, m12, cap, U, sw, sr)
    if W <= minD + D:
        assert (want["disp"] == 16 * (minD - 1)).all()


def test_sgbm_large_candidate_count(ctx):
    # D = 256: four candidates per lane
    L, R = _pair(20, 300, 256, 3, seed=11)
    _check(ctx, L, R, 0, 256, 3, 72, 288, 1, 10, 10, 0, 0)


@pytest.mark.parametrize("H,W,D,cn", [(8, 600, 512, 1), (4, 1100, 1024, 1)])
def test_sgbm_widest_candidate_forms(ctx, H, W, D, cn):
    # D = 512 / 1024: eight / sixteen candidates per lane, the largest register arrays and LDS rows (4 D ints) of the path kernels
    L, R = _pair(H, W, 64, cn, seed=D)
    _check(ctx, L, R, 0, D, 3, 72, 288, 1, 10, 10, 20, 2)


def test_sgbm_output_layout(ctx):
    # a map that is not CV_16SC1 is refused with the status asw_filter_speckles gives it
    from aswstereomatch_amd import _lib
    import ctypes as C

    L, R = _pair(20, 64, 16, 3, seed=4)
    li, _ = asw._image(L)
    ri, _ = asw._image(R)
    out = np.zeros((20, 64), np.float32)
    oi = _lib.AswImage(out.ctypes.data, 20, 64, 1, 5, 64 * 4)
    rc = _lib.lib().asw_sgbm(ctx._h, C.byref(li), C.byref(ri), C.byref(oi), 0, 16, 5, 0, 0, 0, 0, 0, 0, 0, 2, None, 0)
    assert rc == asw.ERR_UNSUPPORTED_LAYOUT


def test_sgbm_shifted_pair(ctx):
    d0 = 9
    L, R = shifted_pair(48, 160, d0)
    disp = ctx.sgbm(L, R, 0, 32, 5, 600, 2400, 1, 10, 10, 0, 0)
    assert (disp[4:-4, 40:-8] == 16 * d0).mean() > 0.99


def test_sgbm_argument_errors(ctx):
    L, R = _pair(20, 64, 16, 3, seed=3)
    for kw, status in [(dict(numDisparities=24), asw.ERR_BAD_ARGUMENT), (dict(numDisparities=0), asw.ERR_BAD_ARGUMENT),
                       (dict(mode=0), asw.ERR_UNSUPPORTED_METHOD), (dict(mode=1), asw.ERR_UNSUPPORTED_METHOD),
                       (dict(minDisparity=-1), asw.ERR_BAD_ARGUMENT),
                       (dict(preFilterCap=1 << 24, blockSize=31), asw.ERR_BAD_ARGUMENT)]:   # 3 (C_max + P2) >= 2^31
        args = dict(minDisparity=0, numDisparities=16, blockSize=5)
        args.update(kw)
        with pytest.raises(asw.AswError) as e:
            ctx.sgbm(L, R, args.pop("minDisparity"), args.pop("numDisparities"), args.pop("blockSize"), **args)
        assert e.value.status == status, kw
    # the f32 volume must be exact: w 35, cap 63, P2 = 2^23 -> S can pass 2^24
    with pytest.raises(asw.AswError) as e:
        ctx.sgbm(L, R, 0, 16, 35, 8, 1 << 23, 0, 63, 10, 0, 0, return_cost_volume=True)
    assert e.value.status == asw.ERR_BAD_ARGUMENT
    ctx.sgbm(L, R, 0, 16, 35, 8, 1 << 23, 0, 63, 10, 0, 0)  # ... while the map alone is fine


# ---------------------------------------------------------------- filterSpeckles
def _piecewise(H, W, seed, holes=0.1, block=6, levels=5, step=16):
    rng = np.random.default_rng(seed)
    by, bx = (H + block - 1) // block, (W + block - 1) // block
    base = rng.integers(0, levels, size=(by, bx)) * step * 3
    m = np.repeat(np.repeat(base, block, 0), block, 1)[:H, :W]
    m = m + rng.integers(-step, step + 1, size=(H, W)) * (rng.random((H, W)) < 0.3)
    m[rng.random((H, W)) < holes] = -16
    return m.astype(np.int16)


@pytest.mark.parametrize("H,W,seed,size,diff", [(50, 70, 1, 20, 16), (97, 131, 2, 60, 32), (64, 256, 3, 1, 0), (5, 300, 4, 400, 48)])
def test_filter_speckles_random(ctx, H, W, seed, size, diff):
    m = _piecewise(H, W, seed)
    assert np.array_equal(ctx.filterSpeckles(m, -16, size, diff), ref.filter_speckles(m, -16, size, diff))


def _spiral(H, W):
    """one 1-pixel-wide path that winds from the border to the centre, separated from itself by walls of newVal"""
    m = np.full((H, W), -16, np.int16)
    top, left, bottom, right = 0, 0, H - 1, W - 1
    v = 0
    while top <= bottom and left <= right:
        m[top, left:right + 1] = v
        m[top:bottom + 1, right] = v
        if bottom > top:
            m[bottom, left:right + 1] = v
        if right > left:
            m[top + 2:bottom + 1, left] = v
            if top + 2 <= bottom - 2 and left + 2 <= right - 2:
                m[top + 2, left + 1] = v  # the step into the next, inner turn
        top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
        v += 1  # a step of 1 along the path, within maxDiff
    return m


def test_filter_speckles_spiral_spans_the_frame(ctx):
    m = _spiral(257, 311)
    n = int((m != -16).sum())
    want = ref.filter_speckles(m, -16, n - 1, 1)
    assert np.array_equal(ctx.filterSpeckles(m, -16, n - 1, 1), want)
    assert np.array_equal(ctx.filterSpeckles(m, -16, n, 1), np.full_like(m, -16))
    kept = ctx.filterSpeckles(m, -16, n - 1, 1)
    assert np.array_equal(kept, m)  # one component of n pixels: kept at size n - 1


def test_filter_speckles_full_frame(ctx):
    m = _piecewise(1080, 1920, 9, holes=0.05, block=24)
    assert np.array_equal(ctx.filterSpeckles(m, -16, 175, 32), ref.filter_speckles(m, -16, 175, 32))


def test_filter_speckles_layout(ctx):
    with pytest.raises(TypeError):
        ctx.filterSpeckles(np.zeros((4, 4), np.uint8), 0, 4, 1)
    from aswstereomatch_amd import _lib
    import ctypes as C

    a = np.zeros((4, 4), np.uint8)
    img = _lib.AswImage(a.ctypes.data, 4, 4, 1, 0, 4)
    assert _lib.lib().asw_filter_speckles(ctx._h, C.byref(img), 0, 4, 1) == asw.ERR_UNSUPPORTED_LAYOUT


# ---------------------------------------------------------------- the selector
def test_selector_sgbm_matches_restatement(ctx):
    L, R = _pair(96, 220, 64, 3, seed=21)
    want = ref.get_disparity_sgbm(L, R, 15, 0, 64)
    got = ctx.stereoMatching(L, R, LEFT, A.SGBM, 15, 0, 64)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(ctx.stereoMatching(L, R, RIGHT, A.SGBM, 15, 0, 64), got)   # disparityType is ignored
    u8 = ctx.getDisparity_SGBM(L, R, 15, 0, 64)
    assert u8.dtype == np.uint8 and np.array_equal(u8, want)
    for win, numD in ((14, 64), (15, 24), (7, 8), (0, 64)):                            # CV_Error in the reference
        with pytest.raises(asw.AswError) as e:
            ctx.stereoMatching(L, R, LEFT, A.SGBM, win, 0, numD)
        assert e.value.status == asw.ERR_UNSUPPORTED_METHOD
    with pytest.raises(asw.AswError) as e:                                              # no selector volume for SGBM
        ctx.stereoMatching(L, R, LEFT, A.SGBM, 15, 0, 64, return_cost_volume=True)
    assert e.value.status == asw.ERR_BAD_ARGUMENT
    with pytest.raises(asw.AswError) as e:                                              # BM is still not served
        ctx.stereoMatching(L, R, LEFT, A.BM, 15, 0, 64)
    assert e.value.status == asw.ERR_UNSUPPORTED_METHOD


def test_selector_sgbm_gray_and_small_window(ctx):
    L, R = _pair(70, 150, 32, 1, seed=22)
    for win, minD in ((5, 0), (-1, 2), (1, 0)):
        got = ctx.stereoMatching(L, R, LEFT, A.SGBM, win, minD, 32)
        assert np.array_equal(got, ref.get_disparity_sgbm(L, R, win, minD, 32)), (win, minD)


def test_selector_sgbm_resident_and_batch(ctx):
    frames = [_pair(48, 140, 32, 3, seed=30 + i) for i in range(4)]
    singles = [ctx.stereoMatching(L, R, LEFT, A.SGBM, 7, 0, 32) for L, R in frames]
    for i, (L, R) in enumerate(frames):
        ctx.upload_pair(5, L, R)
        ctx.match_resident(5, LEFT, A.SGBM, 7, 0, 32, keep_volume=True)
        assert np.array_equal(ctx.download_disparity(5, L.shape[:2]), singles[i])
        with pytest.raises(asw.AswError) as e:  # keep_volume keeps nothing for SGBM
            ctx.download_volume(5, (32,) + L.shape[:2])
        assert e.value.status == asw.ERR_NO_FRAME
    outs = asw.stereoMatchingBatch([f[0] for f in frames], [f[1] for f in frames], LEFT, A.SGBM, 7, 0, 32, device_ids=[0])
    for o, s in zip(outs, singles):
        assert np.array_equal(o, s)


# ---------------------------------------------------------------- whole frames
def test_selector_sgbm_full_hd(ctx):
    L, R = _pair(1080, 1920, 128, 3, seed=40)
    got = ctx.stereoMatching(L, R, LEFT, A.SGBM, 15, 0, 128)
    assert np.array_equal(got, ref.get_disparity_sgbm(L, R, 15, 0, 128))


def test_sgbm_kitti_shape_with_volume(ctx):
    L, R = _pair(375, 1242, 64, 3, seed=41)
    _check(ctx, L, R, 0, 64, 5, 8 * 3 * 25, 32 * 3 * 25, 1, 15, 10, 100, 2)


# ---------------------------------------------------------------- the C++ shim
@pytest.mark.parametrize("cv", [False, True])
def test_shim_get_disparity_sgbm(ctx, tmp_path, cv):
    exe = build_demo("sgbm_demo.cpp", tmp_path / "sgbm_demo", cv)
    for cn in (3, 1):
        L, R = _pair(40, 120, 32, cn, seed=50 + cn)
        L.tofile(tmp_path / "l.raw")
        R.tofile(tmp_path / "r.raw")
        out = tmp_path / "d.raw"
        r = subprocess.run([exe, "40", "120", str(cn), str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), "9", "0", "32", str(out)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.strip() == "ok 40 120 same=1", (r.stdout, r.stderr)
        got = np.fromfile(out, np.uint8).reshape(40, 120)
        assert np.array_equal(got, ctx.getDisparity_SGBM(L, R, 9, 0, 32))
        assert np.array_equal(got, ref.get_disparity_sgbm(L, R, 9, 0, 32))
    r = subprocess.run([exe, "40", "120", "1", str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), "8", "0", "32", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("error"), r.stdout
