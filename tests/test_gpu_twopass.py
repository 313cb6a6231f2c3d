"""Two-pass (separable) adaptive-support-weight aggregation on the GPU (asw_alg_twopass over selector entry 2, k_twopass.hip,
DESIGN.md section 4.16) against the restatement of tests/twopass_ref.py.  The arithmetic is fixed completely, so every comparison
is np.array_equal, on the volume and on the map.  The gray pair handed to the restatement is ctx.bgr2gray of the inputs (pinned to
the oracle by the existing tests), so the conversion is not stated a second time.

That the tie-dense pairs really tie, and the window limit the statuses test uses, are asserted on the restatement alone in
tests/test_twopass_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib
from aswstereomatch_amd._lib import AswError
from aswstereomatch_amd.synth import make_pair, shifted_pair

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_ref as rr  # noqa: E402
import subpixel_ref as sp  # noqa: E402
import twopass_ref as tp  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import asw_oracle as O  # noqa: E402

A = asw.StereoMatchingAlgorithms
LEFT, RIGHT = asw.DISPARITY_LEFT, asw.DISPARITY_RIGHT
MODES = (asw.SUBPIXEL_PARABOLA, asw.SUBPIXEL_EQUIANGULAR)
TOP = tp.max_window()

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


def _gray(ctx, img):
    return ctx.bgr2gray(img) if img.ndim == 3 else img


def _want(ctx, L, R, gammas, dt, win, minD, numD):
    """-> E f64, the volume, the map of the restatement"""
    return tp.twopass(_gray(ctx, L), _gray(ctx, R), gammas[0], gammas[1], win, minD, numD, int(dt))


def _check(ctx, L, R, gammas, dt, win, minD, numD):
    E, vol, disp = _want(ctx, L, R, gammas, dt, win, minD, numD)
    got, gv = ctx.computeAdaptiveWeight_twopass(L, R, gammas[0], gammas[1], dt, win, minD, numD, return_cost_volume=True)
    assert gv.shape == vol.shape and np.array_equal(gv, vol), np.argwhere(gv != vol)[:5]
    assert np.array_equal(got, disp), np.argwhere(got != disp)[:5]
    # without a kept volume: the same map, and the first strict minimum of the f64 E (not of the rounded volume)
    assert np.array_equal(ctx.computeAdaptiveWeight_twopass(L, R, gammas[0], gammas[1], dt, win, minD, numD), disp)
    best, bd = np.full(E.shape[1:], np.inf), np.zeros(E.shape[1:], np.float32)
    for k in range(E.shape[0]):
        lower = E[k] < best
        best, bd = np.where(lower, E[k], best), np.where(lower, np.float32(minD + k), bd)
    assert np.array_equal(disp, bd)
    return E, vol, disp


# H, W, channels, win, minD, numD, direction, gammas.  The kernel's tile is 64 columns x 4 rows (tp.ROW_TILE), its chunks are 8
# candidates wide with remainders 4 / 2 / 1: planes 2, 3, 5, 9, 17, 18, 33, 34 meet every chunk width and remainder
CASES = [
    (1, 1, 3, 3, 0, 1, LEFT, (30, 20)),
    (1, 1, 1, 35, 3, 4, RIGHT, (1, 1)),          # min_d + num_d > cols
    (1, 40, 3, 7, 0, 4, LEFT, (7, 36)),
    (1, 40, 1, 15, 3, 16, RIGHT, (30, 20)),
    (40, 1, 3, 7, 0, 1, LEFT, (255, 255)),
    (40, 1, 1, 35, 0, 4, RIGHT, (30, 20)),       # min_d + num_d > cols
    (3, 5, 3, 15, 3, 4, LEFT, (30, 20)),         # a window larger than the frame, candidates past the image
    (3, 5, 1, 1, 0, 16, RIGHT, (30, 20)),
    (3, 63, 3, 3, 0, 2, LEFT, (30, 20)),         # one column short of a tile, a whole tile, one column more; one row short ...
    (4, 64, 3, 7, 3, 17, RIGHT, (7, 36)),
    (5, 65, 1, 15, 0, 8, LEFT, (1, 1)),
    (7, 65, 3, 35, 0, 4, RIGHT, (255, 255)),
    (8, 64, 1, 3, 0, 33, LEFT, (30, 20)),
    (9, 130, 3, 1, 0, 4, LEFT, (30, 20)),        # win 1: E = |gL - gR|
    (9, 130, 1, 1, 3, 17, RIGHT, (1, 1)),
    (37, 130, 1, 15, 3, 17, LEFT, (30, 20)),
    (37, 130, 3, 35, 0, 17, RIGHT, (7, 36)),
    (33, 130, 3, 35, 0, 1, RIGHT, (30, 20)),
    (12, 150, 1, 7, 0, 32, LEFT, (255, 255)),
    (12, 150, 3, 15, 2, 33, RIGHT, (1, 1)),
    (65, 150, 3, 3, 0, 16, RIGHT, (255, 255)),
    (65, 301, 3, 15, 3, 2, LEFT, (30, 20)),
    (20, 301, 3, 15, 0, 17, LEFT, (7, 36)),      # five tiles a row
    (20, 301, 1, 7, 3, 8, RIGHT, (7, 36)),
    (20, 301, 3, 35, 0, 33, LEFT, (30, 20)),
    (20, 301, 1, 35, 290, 16, RIGHT, (1, 1)),    # min_d + num_d > cols on a wide frame
    (20, 301, 1, 15, 290, 17, LEFT, (30, 20)),
    (9, 130, 3, 25, 0, 8, LEFT, (30, 20)),       # 25 | 27: the dynamic-LDS opt-in above 64 KB
    (9, 130, 1, 27, 3, 8, RIGHT, (30, 20)),
    (6, 90, 3, TOP, 0, 4, LEFT, (30, 20)),       # the last served window
    (9, 130, 1, TOP, 3, 8, RIGHT, (255, 255)),
]


@pytest.mark.parametrize("H,W,cn,win,minD,numD,dt,gammas", CASES)
def test_matches_restatement(ctx, H, W, cn, win, minD, numD, dt, gammas):
    L, R = tp.textured_pair(H, W, cn, 3, H * 1000 + W)
    _check(ctx, L, R, gammas, dt, win, minD, numD)


@pytest.mark.parametrize("H,W,cn,win,minD,numD,dt", [(9, 70, 3, 7, 0, 4, LEFT), (34, 129, 1, 15, 3, 17, RIGHT), (5, 64, 3, 35, 0, 4, LEFT)])
def test_padded_row_views(ctx, H, W, cn, win, minD, numD, dt):
    Lp, Rp = tp.textured_pair(H, W + 5, cn, 3, 77)
    L, R = Lp[:, :W], Rp[:, :W]  # views whose rows carry padding
    assert L.strides[0] > W * cn and not L.flags.c_contiguous
    E, vol, disp = _check(ctx, L, R, (30, 20), dt, win, minD, numD)
    assert np.array_equal(ctx.computeAdaptiveWeight_twopass(np.ascontiguousarray(L), np.ascontiguousarray(R), 30, 20, dt, win, minD, numD), disp)


@pytest.mark.parametrize("name", ["periodic", "constant"])
@pytest.mark.parametrize("dt", [LEFT, RIGHT])
def test_tie_dense_pairs(ctx, name, dt):
    L, R, win, minD, numD = tp.tie_cases()[name]
    E, vol, disp = _check(ctx, L, R, (30, 20), dt, win, minD, numD)
    if name == "constant":
        assert (disp == minD).all()


# ---------------------------------------------------------------- forms and paths
def test_selector_forms_and_paths(ctx):
    H, W, numD, win = 37, 130, 17, 15
    L, R = tp.textured_pair(H, W, 3, 4, 41)
    enc = asw.twopass_algorithm(30, 20)
    n = numD + 1
    for dt in (LEFT, RIGHT):
        E, vol, disp = _want(ctx, L, R, (30, 20), dt, win, 0, numD)
        d, v = ctx.stereoMatching(L, R, dt, enc, win, 0, numD, return_cost_volume=True)
        assert v.shape == (n, H, W) and np.array_equal(d, disp) and np.array_equal(v, vol)
        assert np.array_equal(ctx.stereoMatching(L, R, dt, enc, win, 0, numD), disp)
        t = ctx.timing()
        assert t["aggregate_launches"] == 1 and t["total_ms"] >= t["aggregate_ms"] > 0 and t["cost_ms"] > 0
        d, v = ctx.computeAdaptiveWeight_twopass(L, R, 30, 20, dt, win, 0, numD, return_cost_volume=True)
        assert np.array_equal(d, disp) and np.array_equal(v, vol)
        # the resident path, with and without the volume
        ctx.upload_pair(31, L, R)
        ctx.match_resident(31, dt, enc, win, 0, numD, keep_volume=True)
        assert np.array_equal(ctx.download_disparity(31, (H, W)), disp)
        assert np.array_equal(ctx.download_volume(31, (n, H, W)), vol)
        ctx.match_resident(31, dt, enc, win, 0, numD, keep_volume=False)
        assert np.array_equal(ctx.download_disparity(31, (H, W)), disp)
        with pytest.raises(AswError) as e:
            ctx.download_volume(31, (n, H, W))
        assert e.value.status == asw.ERR_NO_FRAME
        # a fresh context
        fresh = asw.Context(0)
        try:
            d, v = fresh.stereoMatching(L, R, dt, enc, win, 0, numD, return_cost_volume=True)
            assert np.array_equal(d, disp) and np.array_equal(v, vol)
        finally:
            fresh.close()
    # other gammas travel in the encoded value, and the table cache follows them back and forth
    E, vol, disp = _want(ctx, L, R, (7, 36), LEFT, win, 0, numD)
    for gammas, want in (((7, 36), vol), ((30, 20), _want(ctx, L, R, (30, 20), LEFT, win, 0, numD)[1]), ((7, 36), vol)):
        d, v = ctx.stereoMatching(L, R, LEFT, asw.twopass_algorithm(*gammas), win, 0, numD, return_cost_volume=True)
        assert np.array_equal(v, want)
    assert not np.array_equal(vol, _want(ctx, L, R, (30, 20), LEFT, win, 0, numD)[1])
    # the module-level binding and its defaults (gammas 30 / 20, win 15, min 0, 64 + 1 candidates)
    assert np.array_equal(asw.computeAdaptiveWeight_twopass(L, R), ctx.stereoMatching(L, R, LEFT, enc, 15, 0, 64))


def test_entry_2_is_unchanged_and_the_flag_is_not_a_no_op(ctx):
    H, W, numD, win = 20, 90, 8, 7
    L, R = tp.textured_pair(H, W, 3, 4, 43)
    for dt in (LEFT, RIGHT):
        rc, odisp, ovol = O.asw_classic(L, R, 30.0, 20.0, int(dt), win, 0, numD, want_vol=True)
        assert rc == 0
        two = ctx.stereoMatching(L, R, dt, asw.twopass_algorithm(30, 20), win, 0, numD, return_cost_volume=True)  # the table cache is warm
        d, v = ctx.stereoMatching(L, R, dt, A.ADAPTIVE_WEIGHT, win, 0, numD, return_cost_volume=True)
        assert np.array_equal(d, odisp) and np.array_equal(v, ovol)
        assert v.shape == two[1].shape and not np.array_equal(v, two[1])
        assert np.array_equal(two[1], _want(ctx, L, R, (30, 20), dt, win, 0, numD)[1])


def test_batch_equals_single_calls(ctx):
    H, W, numD, win = 24, 150, 12, 15
    pairs = [tp.textured_pair(H, W, 3, 3, 200 + i) for i in range(5)]
    for alg in (asw.twopass_algorithm(30, 20), asw.twopass_algorithm(3, 9)):
        for dt in (LEFT, RIGHT):
            outs = asw.stereoMatchingBatch([p[0] for p in pairs], [p[1] for p in pairs], dt, alg, win, 0, numD, device_ids=[0, 0])
            for (L, R), o in zip(pairs, outs):
                assert np.array_equal(o, ctx.stereoMatching(L, R, dt, alg, win, 0, numD))
    L, R = pairs[0]
    assert np.array_equal(outs[0], _want(ctx, L, R, (3, 9), RIGHT, win, 0, numD)[2])


@pytest.mark.parametrize("dt", [LEFT, RIGHT])
def test_subpixel_flags(ctx, dt):
    H, W, numD, win = 30, 130, 12, 7
    L, R = tp.textured_pair(H, W, 3, 5, 45)
    for gammas, minD in (((30, 20), 0), ((12, 40), 3)):
        alg = asw.twopass_algorithm(*gammas)
        E, vol, disp = _want(ctx, L, R, gammas, dt, win, minD, numD)
        for mode in MODES:
            want, ok = sp.subpixel_vec(disp, vol, minD, mode)
            print("dt %d mode %#x: refined share %.3f" % (int(dt), mode, ok.mean()))
            assert (want != disp).mean() >= 0.1  # on the restatement: the flag has something to move
            d1, v1 = ctx.stereoMatching(L, R, dt, alg, win, minD, numD, return_cost_volume=True, subpixel=mode)
            assert np.array_equal(v1, vol) and np.array_equal(d1, want), np.argwhere(d1 != want)[:5]
            assert np.array_equal(ctx.stereoMatching(L, R, int(dt) | mode, alg, win, minD, numD), want)  # no kept volume
            ctx.upload_pair(32, L, R)
            ctx.match_resident(32, dt, alg, win, minD, numD, keep_volume=False, subpixel=mode)
            assert np.array_equal(ctx.download_disparity(32, (H, W)), want)


def test_refined_calls(ctx):
    H, W, numD, win = 60, 160, 16, 7
    L, R, _ = make_pair(H, W, numD, seed=5, block=16)
    for gammas, minD, rwin, gc in (((30, 20), 0, 15, 150.0), ((10, 30), 2, 7, 150.0)):
        alg = asw.twopass_algorithm(*gammas)
        dl = _want(ctx, L, R, gammas, LEFT, win, minD, numD)[2]
        dr = _want(ctx, L, R, gammas, RIGHT, win, minD, numD)[2]
        want = rr.refine_vec(L, dl, dr, minD, numD + 1, 1.0, rwin, gc, 9.0)
        rejected, moved = rr.vacuity_shares(want)
        print("rejected share %.3f, median != fill on %.3f of the filled pixels" % (rejected, moved))
        assert rejected >= 0.05 and moved >= 0.02  # the conditions of tests/test_gpu_refine.py, on the restatements alone
        got, nrej, nunf = ctx.stereoMatchingRefined(L, R, alg, win, minD, numD, 1.0, rwin, gc, 9.0)
        assert np.array_equal(got, want["out"]) and (nrej, nunf) == (want["n_rejected"], want["n_unfillable"])
        ctx.upload_pair(33, L, R)
        assert ctx.match_refined_resident(33, alg, win, minD, numD, 1.0, rwin, gc, 9.0) == (nrej, nunf)
        assert np.array_equal(ctx.download_disparity(33, (H, W)), want["out"])
        t = ctx.timing()
        assert t["aggregate_launches"] == 2 and t["total_ms"] >= t["aggregate_ms"] > 0


# ---------------------------------------------------------------- identities and statuses
def test_shifted_pair_recovers_its_shift(ctx):
    L, R = shifted_pair(40, 64, 5)
    d = ctx.stereoMatching(L, R, LEFT, asw.twopass_algorithm(30, 20), 15, 0, 10)
    assert (d[8:-8, 16:-8] == 5).all()
    assert np.array_equal(d, _want(ctx, L, R, (30, 20), LEFT, 15, 0, 10)[2])


def test_statuses(ctx):
    H, W, numD = 20, 70, 12
    L, R = tp.textured_pair(H, W, 3, 3, 8)
    ok = asw.twopass_algorithm(30, 20)
    ctx.upload_pair(34, L, R)

    def expect(status, alg, win=15, minD=0, numD=numD):
        ctx.match_resident(34, LEFT, ok, 15, 0, 12, keep_volume=True)  # a previous result
        with pytest.raises(AswError) as e:
            ctx.match_resident(34, LEFT, alg, win, minD, numD, keep_volume=True)
        assert e.value.status == status, (hex(int(alg)), win, e.value.status)
        with pytest.raises(AswError) as e:  # a failed match drops the slot's results
            ctx.download_disparity(34, (H, W))
        assert e.value.status == asw.ERR_NO_FRAME
        for dt in (LEFT, RIGHT):
            if status == asw.ERR_EVEN_WINDOW:  # the reference's silent return
                assert ctx.stereoMatching(L, R, dt, alg, win, minD, numD) is None and asw.last_status() == status
                assert asw.stereoMatchingBatch([L], [R], dt, alg, win, minD, numD, device_ids=[0]) is None
            else:
                with pytest.raises(AswError) as e:
                    ctx.stereoMatching(L, R, dt, alg, win, minD, numD)
                assert e.value.status == status
                with pytest.raises(AswError) as e:
                    asw.stereoMatchingBatch([L], [R], dt, alg, win, minD, numD, device_ids=[0])
                assert e.value.status == status
        with pytest.raises(AswError) as e:
            ctx.stereoMatchingRefined(L, R, alg, win, minD, numD)
        assert e.value.status == status
        with pytest.raises(AswError) as e:
            ctx.match_refined_resident(34, alg, win, minD, numD)
        assert e.value.status == status

    expect(asw.ERR_EVEN_WINDOW, ok, win=14)
    expect(asw.ERR_EVEN_WINDOW, ok, win=TOP + 1)   # the even-window check comes first
    expect(asw.ERR_BAD_ARGUMENT, ok, win=TOP + 2)  # the launcher's first refused window
    expect(asw.ERR_BAD_ARGUMENT, ok, numD=0)
    expect(asw.ERR_BAD_ARGUMENT, ok, minD=-1)
    for bad in (asw.twopass_algorithm(0, 20), asw.twopass_algorithm(30, 0), asw.twopass_algorithm(256, 20), asw.twopass_algorithm(30, -1),
                ok | 0x01000000, ok | 0x08000000, ok - (1 << 32) + (1 << 31)):
        expect(asw.ERR_BAD_ARGUMENT, bad)
    for other in ((ok & ~0xFF) | 3, (ok & ~0xFF) | 12, (ok & ~0xFF) | 13, ok & ~0xFF):
        expect(asw.ERR_UNSUPPORTED_METHOD, other)
    expect(asw.ERR_UNSUPPORTED_METHOD, 13)
    assert ctx.computeAdaptiveWeight_twopass(L, R, 30, 20, LEFT, 14, 0, numD) is None and asw.last_status() == asw.ERR_EVEN_WINDOW
    with pytest.raises(AswError) as e:
        ctx.computeAdaptiveWeight_twopass(L, R, 30, 256, LEFT, 15, 0, numD)
    assert e.value.status == asw.ERR_BAD_ARGUMENT
    two = np.zeros((H, W, 2), np.uint8)
    with pytest.raises(AswError) as e:
        ctx.stereoMatching(two, two, LEFT, ok, 15, 0, numD)
    assert e.value.status == asw.ERR_UNSUPPORTED_LAYOUT
    # plain entry 2 still refuses a 1-channel pair; the two-pass value serves it
    g = np.ascontiguousarray(L[:, :, 1])
    with pytest.raises(AswError) as e:
        ctx.stereoMatching(g, g, LEFT, A.ADAPTIVE_WEIGHT, 15, 0, numD)
    assert e.value.status == asw.ERR_UNSUPPORTED_LAYOUT
    # a short volume buffer (numD + 1 planes are needed) is refused before anything is computed
    li, la = asw._image(L)
    ri, ra = asw._image(R)
    disp = np.full((H, W), -7, np.float32)
    di, _ = asw._image(disp, 5)
    vol = np.zeros((numD + 1) * H * W - 1, np.float32)
    rc = _lib.lib().asw_stereo_match(ctx._h, C.byref(li), C.byref(ri), C.byref(di), 0, ok, 15, 0, numD, vol.ctypes.data_as(C.c_void_p), vol.size)
    assert rc == asw.ERR_BAD_ARGUMENT and (disp == -7).all()
    # and the slot works again afterwards, in the right view too
    ctx.match_resident(34, RIGHT, ok, 15, 0, numD)
    assert np.array_equal(ctx.download_disparity(34, (H, W)), _want(ctx, L, R, (30, 20), RIGHT, 15, 0, numD)[2])


# ---------------------------------------------------------------- seeded sweep
def test_seeded_sweep():
    rng = np.random.default_rng(20261)
    c = None
    try:
        for i in range(300):
            if i % 50 == 0:  # a fresh context every 50 cases
                if c is not None:
                    c.close()
                c = asw.Context(0)
            case = tp.random_case(rng, i)
            (v, d, d2), (vol, disp) = tp.gpu_result(c, case)
            assert np.array_equal(v, vol) and np.array_equal(d, disp) and np.array_equal(d2, disp), (i, case["tag"])
    finally:
        if c is not None:
            c.close()
