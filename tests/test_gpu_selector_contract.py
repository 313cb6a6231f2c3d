"""What every selector method with an encoded `algorithm` value and a per-method wrapper owes its callers, written once and run over the
descriptors of tests/selector_methods.py (cross-based regions, AD-Census, two-pass ASW): the forms of a call and the paths it can take,
the batch, the sub-pixel flags, the refined calls, the shifted-pair identity, the status matrix and a seeded sweep.  The
restatements fix every number, so every comparison is np.array_equal, on the volume and on the map.  What belongs to one method's
kernels (tile boundaries, padded rows at them, tie-dense inputs, a mid-size frame) stays in tests/test_gpu_<method>.py."""
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
import refine_ref as rr  # noqa: E402
import subpixel_ref as sp  # noqa: E402
from selector_methods import METHODS  # noqa: E402

LEFT, RIGHT = asw.DISPARITY_LEFT, asw.DISPARITY_RIGHT
MODES = (asw.SUBPIXEL_PARABOLA, asw.SUBPIXEL_EQUIANGULAR)

pytestmark = [pytest.mark.gpu, pytest.mark.parametrize("m", METHODS, ids=lambda m: m.name)]


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


def _raises(status, call, *args, **kw):
    with pytest.raises(AswError) as e:
        call(*args, **kw)
    assert e.value.status == status, (args, e.value.status)


# ---------------------------------------------------------------- forms and paths
def test_selector_forms_and_paths(ctx, m):
    L, R, win, D = m.forms_input()
    H, W = L.shape[:2]
    n = m.planes(D)
    enc = m.encode(*m.default)
    assert enc == m.encode() and enc in m.equivalents
    for dt in (LEFT, RIGHT):
        E, disp = m.want(ctx, L, R, dt, m.default, win, 0, D)
        for alg in m.equivalents:
            d, v = ctx.stereoMatching(L, R, dt, alg, win, 0, D, return_cost_volume=True)
            assert v.shape == (n, H, W) and np.array_equal(d, disp) and np.array_equal(v, E)
            assert np.array_equal(ctx.stereoMatching(L, R, dt, alg, win, 0, D), disp)
            t = ctx.timing()
            assert t["aggregate_launches"] == m.launches_match and t["total_ms"] >= t["aggregate_ms"] > 0 and t["cost_ms"] > 0
        d, v = m.call(ctx, L, R, dt, m.default, win, 0, D, return_cost_volume=True)
        assert np.array_equal(d, disp) and np.array_equal(v, E)
        # the resident path, with and without the volume
        ctx.upload_pair(21, L, R)
        for alg in m.equivalents:
            ctx.match_resident(21, dt, alg, win, 0, D, keep_volume=True)
            assert np.array_equal(ctx.download_disparity(21, (H, W)), disp)
            assert np.array_equal(ctx.download_volume(21, (n, H, W)), E)
            ctx.match_resident(21, dt, alg, win, 0, D, keep_volume=False)
            assert np.array_equal(ctx.download_disparity(21, (H, W)), disp)
            _raises(asw.ERR_NO_FRAME, ctx.download_volume, 21, (n, H, W))
        # a fresh context
        fresh = asw.Context(0)
        try:
            for alg in m.equivalents:
                d, v = fresh.stereoMatching(L, R, dt, alg, win, 0, D, return_cost_volume=True)
                assert np.array_equal(d, disp) and np.array_equal(v, E)
        finally:
            fresh.close()
    # other parameters travel in the encoded value, and whatever a context caches by them follows them back and forth
    E0 = m.want(ctx, L, R, LEFT, m.default, win, 0, D)[0]
    E, disp = m.want(ctx, L, R, LEFT, m.forms_alt, win, 0, D)
    assert not np.array_equal(E, E0)
    for params, want in ((m.forms_alt, E), (m.default, E0), (m.forms_alt, E)):
        d, v = ctx.stereoMatching(L, R, LEFT, m.encode(*params), win, 0, D, return_cost_volume=True)
        assert np.array_equal(v, want) and (params == m.default or np.array_equal(d, disp))
    if m.other_plain is not None:  # a plain entry that shares the low byte is another method
        assert not np.array_equal(ctx.stereoMatching(L, R, LEFT, m.other_plain, win, 0, D, return_cost_volume=True)[1], E0)
    # the module-level binding and its defaults (the default parameters, win 15, min 0, 64 candidates)
    assert np.array_equal(m.binding(L, R), ctx.stereoMatching(L, R, LEFT, m.equivalents[0], 15, 0, 64))


def test_batch_equals_single_calls(ctx, m):
    pairs, win, D = m.batch_input()
    for alg, params in m.batch_algs:
        for dt in (LEFT, RIGHT):
            outs = asw.stereoMatchingBatch([p[0] for p in pairs], [p[1] for p in pairs], dt, alg, win, 0, D, device_ids=[0, 0])
            for (L, R), o in zip(pairs, outs):
                assert np.array_equal(o, ctx.stereoMatching(L, R, dt, alg, win, 0, D))
            assert np.array_equal(outs[0], m.want(ctx, pairs[0][0], pairs[0][1], dt, params, win, 0, D)[1])


@pytest.mark.parametrize("dt", [LEFT, RIGHT])
def test_subpixel_flags(ctx, m, dt):
    L, R, win, D = m.subpixel_input()
    H, W = L.shape[:2]
    for alg, params, minD in m.subpixel_rows:
        E, disp = m.want(ctx, L, R, dt, params, win, minD, D)
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


def test_refined_calls(ctx, m):
    L, R, win, D = m.refined_input()
    H, W = L.shape[:2]
    for alg, params, minD, rwin, gc in m.refined_rows:
        dl = m.want(ctx, L, R, LEFT, params, win, minD, D)[1]
        dr = m.want(ctx, L, R, RIGHT, params, win, minD, D)[1]
        want = rr.refine_vec(L, dl, dr, minD, m.planes(D), 1.0, rwin, gc, 9.0)
        rejected, moved = rr.vacuity_shares(want)
        print("rejected share %.3f, median != fill on %.3f of the filled pixels" % (rejected, moved))
        assert rejected >= 0.05 and moved >= 0.02  # the conditions of tests/test_gpu_refine.py, on the restatements alone
        got, nrej, nunf = ctx.stereoMatchingRefined(L, R, alg, win, minD, D, 1.0, rwin, gc, 9.0)
        assert np.array_equal(got, want["out"]) and (nrej, nunf) == (want["n_rejected"], want["n_unfillable"])
        assert nrej > 0
        ctx.upload_pair(23, L, R)
        assert ctx.match_refined_resident(23, alg, win, minD, D, 1.0, rwin, gc, 9.0) == (nrej, nunf)
        assert np.array_equal(ctx.download_disparity(23, (H, W)), want["out"])
        t = ctx.timing()
        assert t["aggregate_launches"] == m.launches_refined and t["total_ms"] >= t["aggregate_ms"] > 0


# ---------------------------------------------------------------- identities and statuses
def test_shifted_pair_recovers_its_shift(ctx, m):
    L, R = shifted_pair(40, 64, 5)
    d = ctx.stereoMatching(L, R, LEFT, m.equivalents[0], 15, 0, 10)
    assert (d[8:-8, 16:-8] == 5).all()
    assert np.array_equal(d, m.want(ctx, L, R, LEFT, m.default, 15, 0, 10)[1])


def test_statuses(ctx, m):
    H, W, D = 20, 70, 12
    L, R = m.status_input()
    ok = m.encode(*m.default)
    ctx.upload_pair(24, L, R)

    def expect(status, alg, win=15, minD=0, numD=D):
        ctx.match_resident(24, LEFT, ok, 15, 0, D, keep_volume=True)  # a previous result
        with pytest.raises(AswError) as e:
            ctx.match_resident(24, LEFT, alg, win, minD, numD, keep_volume=True)
        assert e.value.status == status, (hex(int(alg)), win, e.value.status)
        _raises(asw.ERR_NO_FRAME, ctx.download_disparity, 24, (H, W))  # a failed match drops the slot's results
        for dt in (LEFT, RIGHT):
            if status == asw.ERR_EVEN_WINDOW:  # the reference's silent return
                assert ctx.stereoMatching(L, R, dt, alg, win, minD, numD) is None and asw.last_status() == status
                assert asw.stereoMatchingBatch([L], [R], dt, alg, win, minD, numD, device_ids=[0]) is None
            else:
                _raises(status, ctx.stereoMatching, L, R, dt, alg, win, minD, numD)
                _raises(status, asw.stereoMatchingBatch, [L], [R], dt, alg, win, minD, numD, device_ids=[0])
        _raises(status, ctx.stereoMatchingRefined, L, R, alg, win, minD, numD)
        _raises(status, ctx.match_refined_resident, 24, alg, win, minD, numD)

    for alg in m.equivalents:
        expect(asw.ERR_EVEN_WINDOW, alg, win=14)
        if m.even_window_above_top is not None:  # the even-window check comes first
            expect(asw.ERR_EVEN_WINDOW, alg, win=m.even_window_above_top)
        expect(asw.ERR_BAD_ARGUMENT, alg, win=m.first_refused_window)
        expect(asw.ERR_BAD_ARGUMENT, alg, numD=0)
        expect(asw.ERR_BAD_ARGUMENT, alg, minD=-1)
    for bad in m.bad_algs:
        expect(asw.ERR_BAD_ARGUMENT, bad)
    for other in m.unsupported_algs:
        expect(asw.ERR_UNSUPPORTED_METHOD, other)
    expect(asw.ERR_UNSUPPORTED_METHOD, 13)
    assert m.call(ctx, L, R, LEFT, m.default, 14, 0, D) is None and asw.last_status() == asw.ERR_EVEN_WINDOW
    _raises(asw.ERR_BAD_ARGUMENT, m.call, ctx, L, R, LEFT, m.bad_wrapper_params, 15, 0, D)
    two = np.zeros((H, W, 2), np.uint8)
    _raises(asw.ERR_UNSUPPORTED_LAYOUT, ctx.stereoMatching, two, two, LEFT, m.equivalents[0], 15, 0, D)
    # a short volume buffer is refused before anything is computed, for the encoded value too
    li, la = asw._image(L)
    ri, ra = asw._image(R)
    disp = np.full((H, W), -7, np.float32)
    di, _ = asw._image(disp, 5)
    vol = np.zeros(m.planes(D) * H * W - 1, np.float32)
    rc = _lib.lib().asw_stereo_match(ctx._h, C.byref(li), C.byref(ri), C.byref(di), 0, ok, 15, 0, D, vol.ctypes.data_as(C.c_void_p), vol.size)
    assert rc == asw.ERR_BAD_ARGUMENT and (disp == -7).all()
    # and the slot works again afterwards, in the right view too
    ctx.match_resident(24, RIGHT, ok, 15, 0, D)
    assert np.array_equal(ctx.download_disparity(24, (H, W)), m.want(ctx, L, R, RIGHT, m.default, 15, 0, D)[1])


# ---------------------------------------------------------------- seeded sweep
def test_seeded_sweep(m):
    rng = np.random.default_rng(m.sweep_seed)
    c = None
    try:
        for i in range(m.sweep_count):
            if i % 50 == 0:  # a fresh context every 50 cases
                if c is not None:
                    c.close()
                c = asw.Context(0)
            case = m.random_case(rng, i)
            (v, d, d2), (vol, disp) = m.gpu_result(c, case)
            assert np.array_equal(v, vol) and np.array_equal(d, disp) and np.array_equal(d2, disp), (i, case["tag"])  # m.build_case(tag)
    finally:
        if c is not None:
            c.close()
