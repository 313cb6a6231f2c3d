"""The confidence channel on the GPU (a 2-channel `disp` image; k_confidence.hip).

A 2-channel call is held to three things: channel 0 and the returned volume are those of the same call with a 1-channel image on a
SECOND context (bit for bit; NaN slots in the same places), and channel 1 is tests/confidence_ref.py applied to the volume the
2-channel call itself returned (equal f32 bit patterns: the rule has one rounding, and +0 is not -0).

The kernel's constants (k_confidence.hip): a workgroup has 256 lanes; a lane owns 4 consecutive pixels and loads 16 bytes per plane
where rows * cols is a multiple of 4 (1024 pixels per workgroup), one pixel otherwise (256 per workgroup); planes are loaded 4 at a
time (CONF_UNROLL), the rest one by one."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib
from aswstereomatch_amd._lib import AswError, AswImage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asw_cases as ac  # noqa: E402
import confidence_ref as cr  # noqa: E402
import matcher_cases as mc  # noqa: E402
import scanline_ref as sr  # noqa: E402
from test_gpu_scanline import METHODS  # noqa: E402  (the method rows: selector value, RIGHT served, window, minD, scanline code)

A = asw.StereoMatchingAlgorithms
LEFT, RIGHT = asw.DISPARITY_LEFT, asw.DISPARITY_RIGHT
P, E = asw.SUBPIXEL_PARABOLA, asw.SUBPIXEL_EQUIANGULAR
same, bits = sr.same, cr.same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx2():
    """the context the 1-channel results come from: it shares no call history with the context under test"""
    c = asw.Context(0)
    yield c
    c.close()


def _planes(alg, D):
    return _lib.lib().asw_volume_planes(int(alg), D)


def check(ctx, ctx2, L, R, dt, alg, win, minD, numD):
    """dt may carry flags.  -> (map, volume, confidence) of the 2-channel call"""
    d0, v0 = ctx2.stereoMatching(L, R, dt, alg, win, minD, numD, return_cost_volume=True)
    d, v, c = ctx.stereoMatching(L, R, dt, alg, win, minD, numD, return_cost_volume=True, return_confidence=True)
    assert v.shape == (_planes(alg, numD),) + L.shape[:2]
    assert bits(d, d0), np.argwhere(d != d0)[:5]
    assert same(v, v0)
    want = cr.confidence_vec(v)
    assert bits(c, want), (np.argwhere(c != want)[:5], c[c != want][:5], want[c != want][:5])
    d2, c2 = ctx.stereoMatching(L, R, dt, alg, win, minD, numD, return_confidence=True)  # no kept volume: the same pair
    assert bits(d2, d) and bits(c2, c)
    return d, v, c


# ---- every method row of the scanline suite, both directions where it serves both ----
@pytest.mark.parametrize("method", list(METHODS))
def test_methods(ctx, ctx2, method):
    alg, right, win, minD, code = METHODS[method]
    H, W, numD = 21, 66, 13
    L, R = sr.textured_pair(H, W, 3, minD + 4, 11)
    for dt in (LEFT, RIGHT) if right else (LEFT,):
        d, v, c = check(ctx, ctx2, L, R, dt, alg, win, minD, numD)
        print("%s dt %d: confidence mean %.3f, zero share %.3f" % (method, dt, float(c.mean()), float((c == 0).mean())))
        # the bilateral grid at the selector's rates leaves next to no finite cost on a frame this small: all zero there
        assert (c > 0).any() or method == "bilgrid"


@pytest.mark.parametrize("method", ["blo1", "cross", "twopass", "permeability", "bilgrid"])
def test_gray_pairs(ctx, ctx2, method):
    alg, right, win, minD, code = METHODS[method]
    L, R = sr.textured_pair(13, 37, 1, minD + 2, 12)
    check(ctx, ctx2, L, R, LEFT, alg, win, minD, 9)


# ---- frames: from 1 x 1 up; rows * cols of every residue mod 4 (16-byte and scalar loads); a frame that ends inside a workgroup
# and one that fills it, for both forms' pixels per workgroup (1024 and 256: the scalar form runs only where rows * cols is no
# multiple of 4, so its frames end one pixel short of and one pixel past a workgroup) ----
SHAPES = [(1, 1), (1, 2), (1, 3), (2, 2), (1, 5), (2, 3), (1, 7), (3, 4), (3, 5), (7, 9), (5, 51), (1, 255), (16, 16), (1, 257),
          (3, 86), (12, 85), (32, 32), (4, 257), (11, 93), (33, 31), (2, 1024), (29, 71)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes(ctx, ctx2, H, W):
    L, R = sr.textured_pair(H, W, 3, 5, H * 1000 + W)
    check(ctx, ctx2, L, R, LEFT, A.ADAPTIVE_WEIGHT_CROSS, 5, 3, 7)
    check(ctx, ctx2, L, R, RIGHT, asw.twopass_algorithm(), 3, 1, 8)


def test_shapes_cover_both_load_forms():
    planes = [h * w for h, w in SHAPES]
    assert {p % 4 for p in planes} == {0, 1, 2, 3}
    assert 1024 in planes and 2048 in planes and any(p % 4 == 0 and 1024 < p < 2048 for p in planes)  # 16-byte form
    assert 255 in planes and 257 in planes and any(p % 4 and p > 1024 for p in planes)                 # scalar form


# ---- plane counts: 1 .. 5 and 7 .. 9 (both sides of the unroll width and of twice it), 63 .. 65; the winner at both ends ----
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65])
def test_plane_counts(ctx, ctx2, n):
    for H, W in ((6, 41), (6, 42)):  # scalar and 16-byte loads
        for shift in (2, 2 + n - 1):  # the pair's shift names the winner: the first and the last plane
            R, L = sr.textured_pair(H, W, 3, shift, n)  # swapped: L(x) = R(x - shift), the left view's disparity is +shift
            d, v, c = check(ctx, ctx2, L, R, LEFT, A.ADAPTIVE_WEIGHT_CROSS, 5, 2, n)  # n planes
            k1 = np.where(np.isfinite(v), v, np.inf).argmin(axis=0)
            if n <= 9:  # the shift stays well inside the frame's 41 columns
                assert (k1 == shift - 2).mean() > 0.5
            if n <= 2:
                assert (c == 0).all()  # nobody beside the winner's neighbours
            if n > 1:
                check(ctx, ctx2, L, R, RIGHT, asw.twopass_algorithm(), 5, 2, n - 1)  # an inclusive range: numD + 1 planes


# ---- call forms ----
def test_per_method_entry_points(ctx, ctx2):
    H, W, D = 15, 66, 10
    L, R = sr.textured_pair(H, W, 3, 4, 80)
    calls = [
        (A.ADAPTIVE_WEIGHT, 5, lambda c, dt, **k: c.computeAdaptiveWeight(L, R, 30, 20, dt, 5, 0, D, **k)),
        (A.ADAPTIVE_WEIGHT_8DIRECT, 5, lambda c, dt, **k: c.computeAdaptiveWeight_direct8(L, R, dt, 5, 0, D, **k)),
        (A.ADAPTIVE_WEIGHT_GEODESIC, 5, lambda c, dt, **k: c.computeAdaptiveWeight_geodesic(L, R, dt, 5, 0, D, **k)),
        (A.ADAPTIVE_WEIGHT_GUIDED_FILTER, 5, lambda c, dt, **k: c.computeAdaptiveWeight_GuidedF(L, R, dt, 1e-6, 5, 0, D, **k)),
        (A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2, 5, lambda c, dt, **k: c.computeAdaptiveWeight_GuidedF_2(L, R, dt, 1e-6, 5, 0, D, **k)),
        (A.ADAPTIVE_WEIGHT_GUIDED_FILTER_3, 5, lambda c, dt, **k: c.computeAdaptiveWeight_GuidedF_3(L, R, dt, 1e-6, 5, 0, D, **k)),
        (A.ADAPTIVE_WEIGHT_BLO1, 5, lambda c, dt, **k: c.computeAdaptiveWeight_BLO1(L, R, dt, 0.015, 5, 0, D, **k)),
        (A.ADAPTIVE_WEIGHT_BILATERAL_GRID, 1, lambda c, dt, **k: c.computeAdaptiveWeight_bilateralGrid(L, R, dt, 10, 10, 0, D, **k)),
        (A.ADAPTIVE_WEIGHT_MEDIAN, 3, lambda c, dt, **k: c.computeAdaptiveWeight_WeightedMedian(L, R, dt, 3, 10, 10, 0, D, **k)),
        (A.ADAPTIVE_WEIGHT_CROSS, 5, lambda c, dt, **k: c.computeAdaptiveWeight_cross(L, R, dt, 20, 20, 5, 0, D, **k)),
        (asw.adcensus_algorithm(), 5, lambda c, dt, **k: c.computeAdaptiveWeight_adcensus(L, R, dt, 20, 10, 30, 5, 0, D, **k)),
        (asw.twopass_algorithm(), 5, lambda c, dt, **k: c.computeAdaptiveWeight_twopass(L, R, 30, 20, dt, 5, 0, D, **k)),
        (asw.permeability_algorithm(), 0, lambda c, dt, **k: c.computeAdaptiveWeight_permeability(L, R, dt, 8, 20, 0, D, **k)),
    ]
    for alg, win, call in calls:
        d0, v0 = call(ctx2, LEFT, return_cost_volume=True)
        d, v, c = call(ctx, LEFT, return_cost_volume=True, return_confidence=True)
        assert bits(d, d0) and same(v, v0) and bits(c, cr.confidence_vec(v)), int(alg)
        d2, c2 = call(ctx, LEFT, return_confidence=True)
        assert bits(d2, d) and bits(c2, c), int(alg)
        assert bits(call(ctx, LEFT), d)  # and the 1-channel call afterwards is the plain one


def raw_match(ctx, L, R, out, dt, alg, win, minD, numD, channels=None, step=None, fn="asw_stereo_match"):
    """asw_stereo_match (or asw_ncc_disparity / asw_stereo_match_refined) with `out` as the disparity image, as it lies in memory"""
    li, la = asw._image(L)
    ri, ra = asw._image(R)
    di = AswImage(out.ctypes.data, L.shape[0], L.shape[1], out.shape[2] if channels is None else channels, 5,
                  out.strides[0] if step is None else step)
    lib = _lib.lib()
    if fn == "asw_ncc_disparity":
        return lib.asw_ncc_disparity(ctx._h, C.byref(li), C.byref(ri), C.byref(di), int(dt), win, minD, numD)
    if fn == "asw_stereo_match_refined":
        return lib.asw_stereo_match_refined(ctx._h, C.byref(li), C.byref(ri), C.byref(di), int(alg), win, minD, numD, 1.0, 5, 60.0, 9.0,
                                            None, None)
    return lib.asw_stereo_match(ctx._h, C.byref(li), C.byref(ri), C.byref(di), int(dt), int(alg), win, minD, numD, None, 0)


@pytest.mark.parametrize("W,pad", [(64, 5), (37, 3), (33, 1)])
def test_padded_output_rows(ctx, ctx2, W, pad):
    """step > cols * 8: the padding floats keep what they held; padded input rows as well"""
    H = 10
    Lw, Rw = sr.textured_pair(H, W + 7, 3, 4, 130)
    L, R = Lw[:, :W], Rw[:, :W]
    d, v, c = check(ctx, ctx2, L, R, LEFT, A.ADAPTIVE_WEIGHT, 5, 2, 14)
    wide = np.full((H, W + pad, 2), np.float32(-7.5))
    assert raw_match(ctx, L, R, wide, LEFT, A.ADAPTIVE_WEIGHT, 5, 2, 14, step=wide.strides[0]) == asw.OK
    assert bits(wide[:, :W, 0], d) and bits(wide[:, :W, 1], c)
    assert (wide[:, W:] == np.float32(-7.5)).all()


def test_two_channel_image_layout(ctx, ctx2):
    """the image is interleaved: pixel (y, x) is the pair at byte y * step + 8 x"""
    L, R = sr.textured_pair(9, 30, 3, 3, 4)
    d, v, c = check(ctx, ctx2, L, R, LEFT, A.ADAPTIVE_WEIGHT_CROSS, 5, 0, 9)
    out = np.zeros((9, 30, 2), np.float32)
    assert raw_match(ctx, L, R, out, LEFT, A.ADAPTIVE_WEIGHT_CROSS, 5, 0, 9) == asw.OK
    flat = out.reshape(-1)
    assert bits(flat[0::2].reshape(9, 30), d) and bits(flat[1::2].reshape(9, 30), c)


# ---- flags: channel 0 is the flagged map, the confidence is that of the flagged volume ----
@pytest.mark.parametrize("method", ["classic", "cross", "guided2"])
def test_flags(ctx, ctx2, method):
    alg, right, win, minD, code = METHODS[method]
    L, R = sr.textured_pair(20, 70, 3, minD + 5, 70)
    d_plain, v_plain, c_plain = check(ctx, ctx2, L, R, LEFT, alg, win, minD, 12)
    for sub in (P, E):  # the volume a sub-pixel call returns is the unflagged one: so is its confidence
        d, v, c = check(ctx, ctx2, L, R, int(LEFT) | sub, alg, win, minD, 12)
        assert same(v, v_plain) and bits(c, c_plain) and not bits(d, d_plain)
    steps = {"cross_scale": asw.cross_scale(3, 19), "scanline": asw.scanline(*code)}
    for name, flag in steps.items():
        d, v, c = check(ctx, ctx2, L, R, int(LEFT) | flag, alg, win, minD, 12)
        assert not same(v, v_plain) and not bits(c, c_plain), name  # the step's volume, and its confidence
        for sub in (P, E):
            ds, vs, c_sub = check(ctx, ctx2, L, R, int(LEFT) | flag | sub, alg, win, minD, 12)
            assert same(vs, v) and bits(c_sub, c) and not bits(ds, d), name


# ---- non-finite volumes ----
def test_geodesic_on_flat_regions(ctx, ctx2):
    Lf, Rf = mc.constant(6, 20, 3)
    d, v, c = check(ctx, ctx2, Lf, Rf, LEFT, A.ADAPTIVE_WEIGHT_GEODESIC, 5, 0, 8)
    assert np.isnan(v).all() and (c == 0).all() and not np.signbit(c).any()
    L, R = sr.textured_pair(12, 40, 3, 3, 5)
    L, R = L.copy(), R.copy()
    L[:, :20] = 77
    R[:, :20] = 77
    for dt in (LEFT, RIGHT):
        d, v, c = check(ctx, ctx2, L, R, dt, A.ADAPTIVE_WEIGHT_GEODESIC, 5, 0, 8)
        dead = np.isnan(v).all(axis=0)
        assert 0.2 <= dead.mean() <= 0.8  # the share test_gpu_scanline.py holds this pair to
        assert (c[dead] == 0).all() and (c[~dead] > 0).any()


def test_bilateral_grid_volume_of_infinities(ctx, ctx2):
    """a 40 x 96 frame at the selector's rates: most of the grid's cells are never touched, the volume is +inf there"""
    from aswstereomatch_amd.synth import make_pair

    L, R, _ = make_pair(40, 96, 12, seed=5)
    d, v, c = check(ctx, ctx2, L, R, LEFT, A.ADAPTIVE_WEIGHT_BILATERAL_GRID, 1, 0, 15)  # 16 candidates
    share = float(np.isposinf(v).mean())
    print("bilateral grid: +inf share %.3f, pixels with a positive confidence %.3f" % (share, float((c > 0).mean())))
    assert share > 0.5 and not np.isnan(c).any() and (c >= 0).all() and (c <= 1).all()


# ---- tie-dense pairs: a non-adjacent tie at the minimum is exactly 0 ----
@pytest.mark.parametrize("row", ac.ONE_KERNEL_ROWS[:3])
@pytest.mark.parametrize("method", ["classic", "geodesic"])
def test_tie_dense_pairs(ctx, ctx2, method, row):
    H, W, p, shift, win, minD, numD = row
    L, R = ac.make_input(("periodic", p, shift), H, W, 0)
    alg = {"classic": A.ADAPTIVE_WEIGHT, "geodesic": A.ADAPTIVE_WEIGHT_GEODESIC}[method]
    for dt in (LEFT, RIGHT):
        d, v, c = check(ctx, ctx2, L, R, dt, alg, win, minD, numD)
        lo = np.where(np.isfinite(v), v, np.inf)
        k1 = lo.argmin(axis=0)
        k = np.arange(v.shape[0])[:, None, None]
        tied = ((lo == lo.min(axis=0)) & np.isfinite(v) & (np.abs(k - k1) >= 2)).any(axis=0)  # a non-adjacent tie at the minimum
        print("%s dt %d row %s: pixels with a non-adjacent tie %.3f" % (method, dt, row, float(tied.mean())))
        assert tied.mean() >= ac.TIE_FLOOR  # the floor the tie table holds these rows to (candidates p apart tie; p >= 5)
        assert (c[tied] == 0).all() and not np.signbit(c).any()


# ---- resident slots: the confidence comes with the download, from the kept volume ----
@pytest.mark.parametrize("method", ["classic", "guided", "cross", "permeability"])
def test_resident(ctx, ctx2, method):
    alg, right, win, minD, code = METHODS[method]
    H, W, D = 12, 68, 11
    L, R = sr.textured_pair(H, W, 3, minD + 3, 90)
    n = _planes(alg, D)
    d, v, c = check(ctx, ctx2, L, R, LEFT, alg, win, minD, D)
    ctx.upload_pair(25, L, R)
    ctx.match_resident(25, LEFT, alg, win, minD, D, keep_volume=True)
    launches = ctx.timing()["aggregate_launches"]
    plain = ctx.download_disparity(25, (H, W))
    assert bits(plain, d)  # the 1-channel download is what it was
    d1, c1 = ctx.download_disparity(25, (H, W), confidence=True)
    assert bits(d1, d) and bits(c1, c)
    assert same(ctx.download_volume(25, (n, H, W)), v)
    d2, c2 = ctx.download_disparity(25, (H, W), confidence=True)  # a second download: the same bits
    assert bits(d2, d) and bits(c2, c) and bits(ctx.download_disparity(25, (H, W)), d)
    assert ctx.timing()["aggregate_launches"] == launches
    # flags on the resident match: the kept volume is the one the call returns
    flag = asw.scanline(*code)
    ds, vs, c_s = check(ctx, ctx2, L, R, int(LEFT) | flag | P, alg, win, minD, D)
    ctx.match_resident(25, LEFT, alg, win, minD, D, keep_volume=True, subpixel=P, scanline=flag)
    d3, c3 = ctx.download_disparity(25, (H, W), confidence=True)
    assert bits(d3, ds) and bits(c3, c_s)
    # no kept volume: ERR_NO_FRAME, as asw_download_volume
    ctx.match_resident(25, LEFT, alg, win, minD, D, keep_volume=False)
    for fetch in (lambda: ctx.download_disparity(25, (H, W), confidence=True), lambda: ctx.download_volume(25, (n, H, W))):
        with pytest.raises(AswError) as e:
            fetch()
        assert e.value.status == asw.ERR_NO_FRAME
    assert bits(ctx.download_disparity(25, (H, W)), d)
    ctx.match_resident(25, LEFT, alg, win, minD, D, keep_volume=True)
    ctx.match_refined_resident(25, alg, win, minD, D)
    with pytest.raises(AswError) as e:
        ctx.download_disparity(25, (H, W), confidence=True)
    assert e.value.status == asw.ERR_NO_FRAME
    assert ctx.download_disparity(25, (H, W)).shape == (H, W)
    with pytest.raises(AswError) as e:  # an empty slot
        ctx.download_disparity(26, (H, W), confidence=True)
    assert e.value.status == asw.ERR_NO_FRAME


def test_resident_download_image_checks(ctx):
    H, W, D = 9, 34, 8
    L, R = sr.textured_pair(H, W, 3, 3, 91)
    ctx.upload_pair(27, L, R)
    ctx.match_resident(27, LEFT, A.ADAPTIVE_WEIGHT_CROSS, 5, 0, D, keep_volume=True)
    lib = _lib.lib()
    buf = np.full((H, W, 3), np.float32(4.25))
    for channels, step in ((3, W * 12), (2, W * 8 - 4), (2, W * 4), (0, W * 8)):
        di = AswImage(buf.ctypes.data, H, W, channels, 5, step)
        assert lib.asw_download_disparity(ctx._h, 27, C.byref(di)) == asw.ERR_BAD_ARGUMENT
    assert (buf == np.float32(4.25)).all()
    d, c = ctx.download_disparity(27, (H, W), confidence=True)
    assert bits(d, ctx.download_disparity(27, (H, W)))


# ---- statuses ----
def test_statuses(ctx, ctx2):
    H, W, D = 12, 40, 12
    L, R = sr.textured_pair(H, W, 3, 4, 110)
    bad, unsupported, layout = asw.ERR_BAD_ARGUMENT, asw.ERR_UNSUPPORTED_METHOD, asw.ERR_UNSUPPORTED_LAYOUT
    plain = ctx.stereoMatching(L, R, LEFT, A.ADAPTIVE_WEIGHT, 5, 0, D, return_cost_volume=True, return_confidence=True)

    def expect(status, dt, alg, win=5, minD=0, numD=D, left=L, right=R, same_as_one_channel=True):
        out = np.full(left.shape[:2] + (2,), np.float32(-3.5))
        assert raw_match(ctx, left, right, out, dt, alg, win, minD, numD) == status, (hex(int(dt)), int(alg))
        assert (out == np.float32(-3.5)).all()  # a refused call writes nothing
        if same_as_one_channel:
            one = np.full(left.shape[:2] + (1,), np.float32(-3.5))
            assert raw_match(ctx, left, right, one, dt, alg, win, minD, numD) == status
        again = ctx.stereoMatching(L, R, LEFT, A.ADAPTIVE_WEIGHT, 5, 0, D, return_cost_volume=True, return_confidence=True)
        assert all(same(a, b) for a, b in zip(again, plain))  # and the context serves the next call

    # the methods without a selector volume, or with a candidate range of their own
    for alg, numD in ((A.SGBM, 16), (A.BM, 16), (13, D), (255, D), (A.NCC, D)):
        expect(unsupported, LEFT, alg, numD=numD, same_as_one_channel=alg not in (A.SGBM, A.NCC))
    expect(unsupported, RIGHT, A.NCC, same_as_one_channel=False)
    expect(unsupported, LEFT, A.NCC, win=4, same_as_one_channel=False)  # before the runner's own checks, as a sub-pixel flag on NCC
    out = np.full((H, W, 2), np.float32(-3.5))
    assert raw_match(ctx, L, R, out, LEFT, A.NCC, 5, 0, D, fn="asw_ncc_disparity") == unsupported and (out == np.float32(-3.5)).all()
    # what a 1-channel call refuses, with its status: the image checks, the range, the two words, the runner's own checks
    expect(asw.ERR_SIZE_MISMATCH, LEFT, A.ADAPTIVE_WEIGHT, right=R[:, :30])
    expect(layout, LEFT, A.ADAPTIVE_WEIGHT, left=np.ascontiguousarray(L[..., :2]), right=np.ascontiguousarray(R[..., :2]))
    expect(bad, LEFT, A.ADAPTIVE_WEIGHT, numD=0)
    expect(bad, LEFT, A.ADAPTIVE_WEIGHT, minD=-1)
    expect(bad, LEFT, A.NCC, numD=0)                      # the range before the method's row
    expect(bad, P | E, A.ADAPTIVE_WEIGHT)
    expect(bad, P | E, A.NCC)                             # the word before the method's row
    expect(bad, 0x400, A.ADAPTIVE_WEIGHT)
    expect(bad, asw.SCANLINE, A.ADAPTIVE_WEIGHT)
    expect(bad, asw.scanline() | asw.cross_scale(), A.ADAPTIVE_WEIGHT)
    expect(bad, LEFT, asw.cross_algorithm(20, 0))
    expect(unsupported, LEFT, (1 << 30) | 2)              # asw_alg_cross()'s flag on a method without packed parameters
    expect(asw.ERR_EVEN_WINDOW, LEFT, A.ADAPTIVE_WEIGHT, win=4)
    expect(bad, LEFT, A.ADAPTIVE_WEIGHT, win=65)
    expect(bad, LEFT, A.ADAPTIVE_WEIGHT_CROSS, win=37)
    expect(bad, LEFT, A.ADAPTIVE_WEIGHT_BLO1, minD=2)
    for alg in (A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2, A.ADAPTIVE_WEIGHT_MEDIAN, A.ADAPTIVE_WEIGHT_8DIRECT, A.ADAPTIVE_WEIGHT_BILATERAL_GRID):
        expect(layout, RIGHT, alg)
    expect(bad, asw.scanline(), A.ADAPTIVE_WEIGHT, numD=1025)
    # the image itself: 3 channels, 0 channels, a short step, another depth, another size
    buf = np.full((H, W, 3), np.float32(-3.5))
    for channels, step in ((3, W * 12), (0, W * 8), (2, W * 8 - 4), (2, W * 4)):
        assert raw_match(ctx, L, R, buf, LEFT, A.ADAPTIVE_WEIGHT, 5, 0, D, channels=channels, step=step) == bad
    assert raw_match(ctx, L[:-1], R[:-1], buf, LEFT, A.ADAPTIVE_WEIGHT, 5, 0, D, channels=2, step=W * 8) == asw.OK  # rows as stated
    buf[:] = np.float32(-3.5)
    li, ri = asw._image(L)[0], asw._image(R)[0]
    for depth in (0, 3):
        di = AswImage(buf.ctypes.data, H, W, 2, depth, W * 8)
        assert _lib.lib().asw_stereo_match(ctx._h, C.byref(li), C.byref(ri), C.byref(di), 0, 2, 5, 0, D, None, 0) == bad
    di = AswImage(buf.ctypes.data, H + 1, W, 2, 5, W * 8)
    assert _lib.lib().asw_stereo_match(ctx._h, C.byref(li), C.byref(ri), C.byref(di), 0, 2, 5, 0, D, None, 0) == bad
    # a volume buffer that is too short, and SGBM with a volume buffer: as with 1 channel
    vol = np.zeros(5, np.float32)
    di = AswImage(buf.ctypes.data, H, W, 2, 5, W * 8)
    for alg in (A.ADAPTIVE_WEIGHT, A.SGBM):
        assert _lib.lib().asw_stereo_match(ctx._h, C.byref(li), C.byref(ri), C.byref(di), 0, int(alg), 5, 0, 16,
                                           vol.ctypes.data_as(C.c_void_p), vol.size) == bad
    # the calls that do not take the request refuse the image with the status they gave before
    assert raw_match(ctx, L, R, buf, LEFT, A.ADAPTIVE_WEIGHT, 5, 0, D, channels=2, step=W * 8, fn="asw_stereo_match_refined") == bad
    LI, RI, DI = (AswImage * 1)(li), (AswImage * 1)(ri), (AswImage * 1)(di)
    devs = (C.c_int * 1)(0)
    assert _lib.lib().asw_stereo_match_batch(1, LI, RI, DI, 0, 2, 5, 0, D, 1, devs) == bad
    assert _lib.lib().asw_sgbm(ctx._h, C.byref(li), C.byref(ri), C.byref(di), 0, 16, 5, 0, 0, 0, 0, 0, 0, 0, 2, None, 0) == layout
    assert _lib.lib().asw_stereo_bm(ctx._h, C.byref(li), C.byref(ri), C.byref(di), 0, 16, 5, 1, 9, 31, 10, 15, 0, 0, -1, None, 0) == layout
    assert (buf == np.float32(-3.5)).all()
    # the Python keyword: silent statuses give a tuple of None, the others raise
    assert ctx.stereoMatching(L, R, LEFT, A.ADAPTIVE_WEIGHT, 4, 0, D, return_confidence=True) == (None, None)
    assert ctx.stereoMatching(L, R, LEFT, A.ADAPTIVE_WEIGHT, 4, 0, D, return_cost_volume=True, return_confidence=True) == (None, None, None)
    assert asw.last_status() == asw.ERR_EVEN_WINDOW
    with pytest.raises(AswError) as e:
        ctx.stereoMatching(L, R, LEFT, A.SGBM, 5, 0, 16, return_confidence=True)
    assert e.value.status == unsupported
    again = ctx.stereoMatching(L, R, LEFT, A.ADAPTIVE_WEIGHT, 5, 0, D, return_cost_volume=True, return_confidence=True)
    assert all(same(a, b) for a, b in zip(again, plain))
    check(ctx, ctx2, L, R, LEFT, A.ADAPTIVE_WEIGHT, 5, 0, D)


def test_timing_counts_the_kernel_outside_the_aggregation(ctx):
    L, R = sr.textured_pair(20, 64, 3, 4, 7)
    ctx.stereoMatching(L, R, LEFT, A.ADAPTIVE_WEIGHT_CROSS, 5, 0, 12)
    launches = ctx.timing()["aggregate_launches"]
    ctx.stereoMatching(L, R, LEFT, A.ADAPTIVE_WEIGHT_CROSS, 5, 0, 12, return_confidence=True)
    t = ctx.timing()
    assert t["aggregate_launches"] == launches
    assert t["total_ms"] > 0 and t["total_ms"] >= t["aggregate_ms"] >= 0
    assert abs(t["cost_ms"] - (t["total_ms"] - t["aggregate_ms"])) < 1e-3


# ---- seeded sweep ----
def test_seeded_sweep():
    rng = np.random.default_rng(20269)
    a = b = None
    positive = 0
    try:
        for i in range(60):
            if i % 15 == 0:  # fresh contexts: no tables or scratch of earlier cases
                for c in (a, b):
                    if c is not None:
                        c.close()
                a, b = asw.Context(0), asw.Context(0)
            case = cr.random_case(rng)
            tag = "case %d: %s" % (i, case["tag"])
            dt = case["dt"] | case["subpixel"] | case["step"]
            args = (case["L"], case["R"], dt, case["alg"], case["win"], case["minD"], case["numD"])
            d0, v0 = b.stereoMatching(*args, return_cost_volume=True)
            d, v, c = a.stereoMatching(*args, return_cost_volume=True, return_confidence=True)
            assert bits(d, d0) and same(v, v0), tag
            assert bits(c, cr.confidence_vec(v)), tag
            d2, c2 = a.stereoMatching(*args, return_confidence=True)
            assert bits(d2, d) and bits(c2, c), tag
            positive += int((c > 0).any())
    finally:
        for c in (a, b):
            if c is not None:
                c.close()
    print("cases with a positive confidence somewhere: %d of 60" % positive)
    # a case has none when its volume has fewer than three planes (numD 1 or 2: one draw in 12 or so), one pixel column, or is the
    # bilateral grid's on a small frame (one method in 13): half of the cases is a floor far below the expectation
    assert positive >= 30
