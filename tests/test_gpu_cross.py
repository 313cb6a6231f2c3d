"""Cross-based support-region aggregation on the GPU (selector entry 12, k_cross.hip) against the
restatement of tests/cross_ref.py.  Every sum is an integer and the one division is correctly rounded: every comparison is
np.array_equal, on the volume and on the map.  The raw cost handed to the restatement is ctx.computeAD's u8 volume for the same
direction (pinned to the oracle by the existing tests), so its border rule is not stated a second time.

What the region_pair cases exercise (arms of length 0, between and L, tied minima) is asserted on the restatement alone in
tests/test_cross_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib
from aswstereomatch_amd._lib import AswError
from aswstereomatch_amd.synth import shifted_pair

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cross_ref as cr  # noqa: E402
import refine_ref as rr  # noqa: E402
import subpixel_ref as sp  # noqa: E402

A = asw.StereoMatchingAlgorithms
LEFT, RIGHT = asw.DISPARITY_LEFT, asw.DISPARITY_RIGHT
CROSS = A.ADAPTIVE_WEIGHT_CROSS
MODES = (asw.SUBPIXEL_PARABOLA, asw.SUBPIXEL_EQUIANGULAR)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


def _pair(H, W, cn, D, seed=None, pad=0):
    L, R, _ = cr.region_pair(H, W + pad, max(2, D), H * 1000 + W if seed is None else seed, (5, 7), 0.12, block=8)
    if cn == 1:
        L, R = np.ascontiguousarray(L[:, :, 1]), np.ascontiguousarray(R[:, :, 1])
    return L[:, :W], R[:, :W]  # pad > 0: views whose rows carry padding


def _want(ctx, L, R, dt, tau, trunc, win, minD, D):
    e = np.stack(ctx.computeAD(L, R, dt, minD, D))
    return cr.aggregate(e, cr.arms(R if int(dt) else L, tau, win // 2), trunc, minD)


def _check(ctx, L, R, dt, tau, trunc, win, minD, D):
    S, N, E, disp = _want(ctx, L, R, dt, tau, trunc, win, minD, D)
    got, vol = ctx.computeAdaptiveWeight_cross(L, R, dt, tau, trunc, win, minD, D, return_cost_volume=True)
    assert vol.shape == E.shape and np.array_equal(vol, E), np.argwhere(vol != E)[:5]
    assert np.array_equal(got, disp), np.argwhere(got != disp)[:5]
    # without a kept volume the running minimum inside the kernel is the argmin of the kept volume
    assert np.array_equal(ctx.computeAdaptiveWeight_cross(L, R, dt, tau, trunc, win, minD, D), disp)
    assert np.array_equal(disp, (np.argmin(vol, axis=0) + minD).astype(np.float32))
    return E, disp


# H, W, channels, win, minD, D, direction, tau, trunc
CASES = [
    (1, 1, 3, 3, 0, 1, LEFT, 20, 20),
    (1, 1, 3, 35, 3, 5, RIGHT, 20, 20),       # min_d + num_d > cols
    (1, 40, 3, 7, 0, 5, LEFT, 20, 20),
    (1, 40, 1, 15, 3, 17, RIGHT, 20, 255),
    (40, 1, 3, 7, 0, 1, LEFT, 20, 20),
    (40, 1, 3, 35, 0, 5, RIGHT, 0, 1),        # min_d + num_d > cols
    (3, 5, 3, 15, 3, 5, LEFT, 20, 20),        # a window larger than the frame, candidates past the image
    (3, 5, 3, 1, 0, 17, RIGHT, 255, 20),
    (7, 63, 3, 3, 0, 5, LEFT, 20, 20),        # one column short of a tile, a whole tile, one column more
    (7, 64, 3, 7, 3, 17, RIGHT, 20, 20),
    (7, 65, 3, 15, 0, 17, LEFT, 20, 1),
    (7, 65, 1, 35, 0, 5, RIGHT, 255, 255),
    (37, 130, 3, 1, 0, 5, LEFT, 20, 20),      # win 1: every region is its pixel
    (37, 130, 1, 15, 3, 17, LEFT, 0, 20),
    (33, 130, 3, 35, 0, 1, RIGHT, 255, 20),   # a band and one row; one candidate
    (65, 150, 3, 35, 3, 5, LEFT, 20, 255),
    (65, 150, 3, 3, 0, 17, RIGHT, 0, 1),
    (20, 301, 3, 15, 0, 17, LEFT, 20, 20),    # five tiles a row
    (20, 301, 3, 7, 3, 5, RIGHT, 0, 20),
    (20, 301, 3, 35, 0, 17, LEFT, 255, 20),
    (20, 301, 1, 35, 290, 17, RIGHT, 20, 20), # min_d + num_d > cols on a wide frame
]


@pytest.mark.parametrize("H,W,cn,win,minD,D,dt,tau,trunc", CASES)
def test_matches_restatement(ctx, H, W, cn, win, minD, D, dt, tau, trunc):
    L, R = _pair(H, W, cn, D)
    _check(ctx, L, R, dt, tau, trunc, win, minD, D)


@pytest.mark.parametrize("H,W,D,cell,seed,amp,win", cr.REGION_CASES)
@pytest.mark.parametrize("dt", [LEFT, RIGHT])
def test_region_cases(ctx, H, W, D, cell, seed, amp, win, dt):
    L, R, _ = cr.region_pair(H, W, D, seed, cell, amp)
    _check(ctx, L, R, dt, 20, 20, win, 0, D)


@pytest.mark.parametrize("H,W,cn,win,minD,D,dt", [(9, 70, 3, 7, 0, 5, LEFT), (34, 129, 1, 15, 3, 17, RIGHT), (5, 64, 3, 35, 0, 5, LEFT)])
def test_padded_row_views(ctx, H, W, cn, win, minD, D, dt):
    L, R = _pair(H, W, cn, D, pad=5)
    assert L.strides[0] > W * cn and not L.flags.c_contiguous
    E, disp = _check(ctx, L, R, dt, 20, 20, win, minD, D)
    assert np.array_equal(ctx.computeAdaptiveWeight_cross(np.ascontiguousarray(L), np.ascontiguousarray(R), dt, 20, 20, win, minD, D), disp)


# ---------------------------------------------------------------- forms and paths
def test_selector_forms_and_paths(ctx):
    H, W, D, cell, seed, amp, win = cr.REGION_CASES[1]
    L, R, _ = cr.region_pair(H, W, D, seed, cell, amp)
    enc = asw.cross_algorithm(20, 20)
    for dt in (LEFT, RIGHT):
        S, N, E, disp = _want(ctx, L, R, dt, 20, 20, win, 0, D)
        for alg in (CROSS, 12, enc):
            d, v = ctx.stereoMatching(L, R, dt, alg, win, 0, D, return_cost_volume=True)
            assert np.array_equal(d, disp) and np.array_equal(v, E)
            assert np.array_equal(ctx.stereoMatching(L, R, dt, alg, win, 0, D), disp)
        t = ctx.timing()
        assert t["aggregate_launches"] == 3 and t["total_ms"] >= t["aggregate_ms"] > 0 and t["cost_ms"] > 0
        # the resident path, with and without the volume
        ctx.upload_pair(21, L, R)
        for alg in (CROSS, enc):
            ctx.match_resident(21, dt, alg, win, 0, D, keep_volume=True)
            assert np.array_equal(ctx.download_disparity(21, (H, W)), disp)
            assert np.array_equal(ctx.download_volume(21, (D, H, W)), E)
            ctx.match_resident(21, dt, alg, win, 0, D, keep_volume=False)
            assert np.array_equal(ctx.download_disparity(21, (H, W)), disp)
            with pytest.raises(AswError) as e:
                ctx.download_volume(21, (D, H, W))
            assert e.value.status == asw.ERR_NO_FRAME
        # a fresh context
        fresh = asw.Context(0)
        try:
            d, v = fresh.stereoMatching(L, R, dt, CROSS, win, 0, D, return_cost_volume=True)
            assert np.array_equal(d, disp) and np.array_equal(v, E)
        finally:
            fresh.close()
    # other parameters travel in the encoded value: against the restatement and against the per-method call
    S, N, E, disp = _want(ctx, L, R, LEFT, 7, 33, win, 0, D)
    d, v = ctx.stereoMatching(L, R, LEFT, asw.cross_algorithm(7, 33), win, 0, D, return_cost_volume=True)
    assert np.array_equal(d, disp) and np.array_equal(v, E)
    assert not np.array_equal(v, _want(ctx, L, R, LEFT, 20, 20, win, 0, D)[2])
    # the module-level binding and its defaults (tau 20, trunc 20, win 15, min 0, 64 candidates)
    assert np.array_equal(asw.computeAdaptiveWeight_cross(L, R), ctx.stereoMatching(L, R, LEFT, CROSS, 15, 0, 64))


def test_batch_equals_single_calls(ctx):
    H, W, D, win = 40, 150, 12, 15
    pairs = [cr.region_pair(H, W, D, 200 + i, (9, 13), 0.12)[:2] for i in range(5)]
    for alg in (CROSS, asw.cross_algorithm(20, 20), asw.cross_algorithm(3, 9)):
        for dt in (LEFT, RIGHT):
            outs = asw.stereoMatchingBatch([p[0] for p in pairs], [p[1] for p in pairs], dt, alg, win, 0, D, device_ids=[0, 0])
            for (L, R), o in zip(pairs, outs):
                assert np.array_equal(o, ctx.stereoMatching(L, R, dt, alg, win, 0, D))
    L, R = pairs[0]
    assert np.array_equal(outs[0], _want(ctx, L, R, RIGHT, 3, 9, win, 0, D)[3])


@pytest.mark.parametrize("dt", [LEFT, RIGHT])
def test_subpixel_flags(ctx, dt):
    H, W, D, cell, seed, amp, win = cr.REGION_CASES[1]
    L, R, _ = cr.region_pair(H, W, D, seed, cell, amp)
    for alg, tau, trunc, minD in ((CROSS, 20, 20, 0), (asw.cross_algorithm(12, 40), 12, 40, 3)):
        S, N, E, disp = _want(ctx, L, R, dt, tau, trunc, win, minD, D)
        for mode in MODES:
            want, ok = sp.subpixel_vec(disp, E, minD, mode)
            print("dt %d mode %#x: refined share %.3f" % (int(dt), mode, ok.mean()))
            assert (want != disp).mean() >= 0.1  # on the restatement: the flag has something to move
            d1, v1 = ctx.stereoMatching(L, R, dt, alg, win, minD, D, return_cost_volume=True, subpixel=mode)
            assert np.array_equal(v1, E) and np.array_equal(d1, want), np.argwhere(d1 != want)[:5]
            assert np.array_equal(ctx.stereoMatching(L, R, int(dt) | mode, alg, win, minD, D), want)  # no kept volume
            ctx.upload_pair(22, L, R)
            ctx.match_resident(22, dt, alg, win, minD, D, keep_volume=False, subpixel=mode)
            assert np.array_equal(ctx.download_disparity(22, (H, W)), want)


def test_refined_calls(ctx):
    H, W, D, cell, seed, amp, win = cr.REGION_CASES[1]
    L, R, _ = cr.region_pair(H, W, D, seed, cell, amp)
    for alg, tau, trunc, minD, rwin, gc in ((CROSS, 20, 20, 0, 15, 150.0), (asw.cross_algorithm(10, 30), 10, 30, 3, 7, 60.0)):
        dl = _want(ctx, L, R, LEFT, tau, trunc, win, minD, D)[3]
        dr = _want(ctx, L, R, RIGHT, tau, trunc, win, minD, D)[3]
        want = rr.refine_vec(L, dl, dr, minD, D, 1.0, rwin, gc, 9.0)
        rejected, moved = rr.vacuity_shares(want)
        print("rejected share %.3f, median != fill on %.3f of the filled pixels" % (rejected, moved))
        assert rejected >= 0.05 and moved >= 0.02  # the conditions of tests/test_gpu_refine.py, on the restatements alone
        got, nrej, nunf = ctx.stereoMatchingRefined(L, R, alg, win, minD, D, 1.0, rwin, gc, 9.0)
        assert np.array_equal(got, want["out"]) and (nrej, nunf) == (want["n_rejected"], want["n_unfillable"])
        ctx.upload_pair(23, L, R)
        assert ctx.match_refined_resident(23, alg, win, minD, D, 1.0, rwin, gc, 9.0) == (nrej, nunf)
        assert np.array_equal(ctx.download_disparity(23, (H, W)), want["out"])
        t = ctx.timing()
        assert t["aggregate_launches"] == 6 and t["total_ms"] >= t["aggregate_ms"] > 0


# ---------------------------------------------------------------- identities and statuses
def test_shifted_pair_recovers_its_shift(ctx):
    L, R = shifted_pair(40, 64, 5)
    d = ctx.stereoMatching(L, R, LEFT, CROSS, 15, 0, 10)
    assert (d[8:-8, 16:-8] == 5).all()
    assert np.array_equal(d, _want(ctx, L, R, LEFT, 20, 20, 15, 0, 10)[3])


def test_statuses(ctx):
    H, W, D = 20, 70, 12
    L, R, _ = cr.region_pair(H, W, D, 8, (9, 13), 0.16)
    ok = asw.cross_algorithm(20, 20)
    ctx.upload_pair(24, L, R)

    def expect(status, alg, win=15, minD=0, numD=D):
        ctx.match_resident(24, LEFT, CROSS, 15, 0, D, keep_volume=True)  # a previous result
        with pytest.raises(AswError) as e:
            ctx.match_resident(24, LEFT, alg, win, minD, numD, keep_volume=True)
        assert e.value.status == status, (hex(int(alg)), win, e.value.status)
        with pytest.raises(AswError) as e:  # a failed match drops the slot's results
            ctx.download_disparity(24, (H, W))
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
            ctx.match_refined_resident(24, alg, win, minD, numD)
        assert e.value.status == status

    for alg in (CROSS, ok):
        expect(asw.ERR_EVEN_WINDOW, alg, win=14)
        expect(asw.ERR_BAD_ARGUMENT, alg, win=37)
        expect(asw.ERR_BAD_ARGUMENT, alg, numD=0)
        expect(asw.ERR_BAD_ARGUMENT, alg, minD=-1)
    for bad in (asw.cross_algorithm(256, 1), asw.cross_algorithm(5, 0), asw.cross_algorithm(-1, 7), 0x40000000 | 12, ok | 0x02000000,
                ok | 0x20000000):
        expect(asw.ERR_BAD_ARGUMENT, bad)
    for other in ((ok & ~0xFF) | 11, (ok & ~0xFF) | 2, ok & ~0xFF, (ok & ~0xFF) | 13):
        expect(asw.ERR_UNSUPPORTED_METHOD, other)
    expect(asw.ERR_UNSUPPORTED_METHOD, 13)
    assert ctx.computeAdaptiveWeight_cross(L, R, LEFT, 20, 20, 14, 0, D) is None and asw.last_status() == asw.ERR_EVEN_WINDOW
    with pytest.raises(AswError) as e:
        ctx.computeAdaptiveWeight_cross(L, R, LEFT, 20, 256, 15, 0, D)
    assert e.value.status == asw.ERR_BAD_ARGUMENT
    two = np.zeros((H, W, 2), np.uint8)
    with pytest.raises(AswError) as e:
        ctx.stereoMatching(two, two, LEFT, CROSS, 15, 0, D)
    assert e.value.status == asw.ERR_UNSUPPORTED_LAYOUT
    # a short volume buffer is refused before anything is computed, for the encoded value too
    li, la = asw._image(L)
    ri, ra = asw._image(R)
    disp = np.full((H, W), -7, np.float32)
    di, _ = asw._image(disp, 5)
    vol = np.zeros(D * H * W - 1, np.float32)
    rc = _lib.lib().asw_stereo_match(ctx._h, C.byref(li), C.byref(ri), C.byref(di), 0, ok, 15, 0, D, vol.ctypes.data_as(C.c_void_p), vol.size)
    assert rc == asw.ERR_BAD_ARGUMENT and (disp == -7).all()
    # and the slot works again afterwards, in the right view too
    ctx.match_resident(24, RIGHT, ok, 15, 0, D)
    assert np.array_equal(ctx.download_disparity(24, (H, W)), _want(ctx, L, R, RIGHT, 20, 20, 15, 0, D)[3])


# ---------------------------------------------------------------- one mid-size frame
def test_mid_size_frame_in_both_forms(ctx):
    """270 x 480, 64 candidates, win 15: the whole volume and map against the integral form; the literal form takes a quarter of a
    minute on this frame, so it is evaluated on every ninth row and the last (the two forms are compared pixel for pixel on whole
    frames in tests/test_cross_cpu.py).  Plain 12 and the encoded value, resident, without and with the volume."""
    H, W, D, win = 270, 480, 64, 15
    L, R, _ = cr.region_pair(H, W, D, 5, (25, 40), 0.12)
    e = np.stack(ctx.computeAD(L, R, LEFT, 0, D))
    a = cr.arms(L, 20, win // 2)
    S, N, E, disp = cr.aggregate(e, a, 20)
    rows = sorted(set(range(0, H, 9)) | {H - 1})
    S2, N2, E2, disp2 = cr.aggregate_loop(e, a, 20, rows=rows)
    assert np.array_equal(E[:, rows], E2[:, rows]) and np.array_equal(disp[rows], disp2[rows])
    ctx.upload_pair(25, L, R)
    ctx.match_resident(25, LEFT, CROSS, win, 0, D, keep_volume=False)
    assert np.array_equal(ctx.download_disparity(25, (H, W)), disp)
    ctx.match_resident(25, LEFT, asw.cross_algorithm(20, 20), win, 0, D, keep_volume=True)
    got, vol = ctx.download_disparity(25, (H, W)), ctx.download_volume(25, (D, H, W))
    assert np.array_equal(vol, E) and np.array_equal(got, disp)
    assert np.array_equal(vol[:, rows], E2[:, rows]) and np.array_equal(got[rows], disp2[rows])
