"""Recursive (permeability) aggregation on the GPU (asw_alg_permeability over selector entry 12, k_permeability.hip, DESIGN.md section
4.17) against the restatement of tests/permeability_ref.py.  The arithmetic is fixed completely, so every comparison is
np.array_equal, on the volume and on the map.  The AD volume handed to the restatement is ctx.computeAD of the inputs (pinned to the
oracle by the existing tests), so its border rule is not stated a second time.  That the tie cases really tie is asserted on the
restatement alone in tests/test_permeability_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib
from aswstereomatch_amd._lib import AswError
from aswstereomatch_amd.synth import make_pair

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adcensus_ref as ac  # noqa: E402
import cross_ref as cr  # noqa: E402
import permeability_ref as pm  # noqa: E402
import refine_ref as rr  # noqa: E402
import subpixel_ref as sp  # noqa: E402

A = asw.StereoMatchingAlgorithms
LEFT, RIGHT = asw.DISPARITY_LEFT, asw.DISPARITY_RIGHT
MODES = (asw.SUBPIXEL_PARABOLA, asw.SUBPIXEL_EQUIANGULAR)
PA = asw.permeability_algorithm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


def _raises(status, call, *args, **kw):
    with pytest.raises(AswError) as e:
        call(*args, **kw)
    assert e.value.status == status, (args, e.value.status)


def _want(ctx, L, R, dt, sigma, trunc, minD, D):
    """-> E f64, the volume, the map of the restatement"""
    e = np.stack(ctx.computeAD(L, R, dt, minD, D))
    return pm.aggregate(e, R if int(dt) else L, sigma, trunc, minD)[:3]


def _check(ctx, L, R, dt, sigma, trunc, minD, D, want=None):
    E, vol, disp = want or _want(ctx, L, R, dt, sigma, trunc, minD, D)
    got, gv = ctx.computeAdaptiveWeight_permeability(L, R, dt, sigma, trunc, minD, D, return_cost_volume=True)
    assert gv.shape == vol.shape and np.array_equal(gv, vol), np.argwhere(gv != vol)[:5]
    assert np.array_equal(got, disp), np.argwhere(got != disp)[:5]
    # without a kept volume: the same map, and the first strict minimum of the f64 E (not of the rounded volume)
    assert np.array_equal(ctx.computeAdaptiveWeight_permeability(L, R, dt, sigma, trunc, minD, D), disp)
    best, bd = np.full(E.shape[1:], np.inf), np.zeros(E.shape[1:], np.float32)
    for k in range(E.shape[0]):
        lower = E[k] < best
        best, bd = np.where(lower, E[k], best), np.where(lower, np.float32(minD + k), bd)
    assert np.array_equal(disp, bd)
    return E, vol, disp


# H, W, channels, minD, D, direction, sigma, trunc.  The kernels scan in segments of 16 positions (pm.SEGMENT, both passes), the
# horizontal pass stages 64 columns of costs (pm.COST_TILE; going back it re-stages at columns = 48 mod 64), the vertical workgroup
# holds 8 columns (pm.COLUMNS_PER_WORKGROUP), a wavefront 64 candidates: both sides of each, in widths, heights and plane counts
CASES = [
    (1, 1, 3, 0, 1, LEFT, 8, 20),
    (1, 1, 1, 3, 5, RIGHT, 1, 255),            # min_d + num_d > cols
    (1, 9, 3, 0, 3, LEFT, 255, 1),
    (1, 9, 1, 3, 2, RIGHT, 8, 20),
    (9, 1, 3, 0, 2, LEFT, 1, 20),
    (9, 1, 1, 0, 5, RIGHT, 8, 255),            # min_d + num_d > cols
    (2, 2, 3, 0, 3, LEFT, 8, 20),
    (2, 63, 1, 3, 2, RIGHT, 255, 20),
    (63, 2, 3, 0, 5, LEFT, 8, 1),
    (64, 7, 1, 0, 3, RIGHT, 1, 20),
    (65, 8, 3, 3, 2, LEFT, 8, 255),
    (7, 64, 1, 0, 5, LEFT, 8, 20),
    (8, 65, 3, 0, 3, RIGHT, 255, 255),
    (9, 9, 1, 0, 63, LEFT, 8, 20),             # min_d + num_d > cols; one candidate short of a wavefront
    (15, 15, 3, 0, 64, RIGHT, 8, 20),
    (16, 16, 1, 3, 65, LEFT, 1, 1),
    (17, 17, 3, 0, 130, RIGHT, 8, 20),         # three wavefronts of candidates
    (31, 47, 1, 0, 2, LEFT, 8, 20),
    (32, 48, 3, 3, 3, RIGHT, 1, 255),
    (33, 49, 1, 0, 5, LEFT, 255, 20),
    (129, 31, 3, 0, 1, RIGHT, 8, 20),
    (130, 33, 1, 0, 2, LEFT, 8, 1),
    (5, 127, 3, 0, 3, LEFT, 8, 20),
    (4, 128, 1, 3, 5, RIGHT, 8, 255),
    (3, 129, 3, 0, 2, LEFT, 1, 20),
    (6, 130, 1, 0, 3, RIGHT, 255, 20),
    (20, 301, 3, 290, 16, LEFT, 8, 20),        # min_d + num_d > cols on a wide frame
    (20, 301, 1, 290, 17, RIGHT, 8, 20),
    (37, 130, 3, 0, 17, LEFT, 8, 20),
    (37, 130, 1, 3, 17, RIGHT, 1, 60),
    (70, 150, 3, 0, 8, RIGHT, 8, 20),
]


@pytest.mark.parametrize("H,W,cn,minD,D,dt,sigma,trunc", CASES)
def test_matches_restatement(ctx, H, W, cn, minD, D, dt, sigma, trunc):
    L, R = pm.textured_pair(H, W, cn, 3, H * 1000 + W)
    _check(ctx, L, R, dt, sigma, trunc, minD, D)


@pytest.mark.parametrize("sigma", pm.SIGMAS)
@pytest.mark.parametrize("trunc", pm.TRUNCS)
def test_every_sigma_and_trunc(ctx, sigma, trunc):
    L, R = pm.textured_pair(34, 70, 3, 4, 17)
    for dt in (LEFT, RIGHT):
        _check(ctx, L, R, dt, sigma, trunc, 0, 9)


@pytest.mark.parametrize("H,W,cn,minD,D,dt", [(9, 70, 3, 0, 4, LEFT), (34, 129, 1, 3, 17, RIGHT), (17, 64, 3, 0, 4, LEFT)])
def test_padded_row_views(ctx, H, W, cn, minD, D, dt):
    Lp, Rp = pm.textured_pair(H, W + 5, cn, 3, 77)
    L, R = Lp[:, :W], Rp[:, :W]  # views whose rows carry padding
    assert L.strides[0] > W * cn and not L.flags.c_contiguous
    E, vol, disp = _check(ctx, L, R, dt, 8, 20, minD, D)
    assert np.array_equal(ctx.computeAdaptiveWeight_permeability(np.ascontiguousarray(L), np.ascontiguousarray(R), dt, 8, 20, minD, D), disp)


# ---------------------------------------------------------------- chunking
@pytest.mark.parametrize("H,W,cn,minD,D,dt", [(20, 70, 3, 0, 7, LEFT), (33, 40, 1, 3, 70, RIGHT)])
def test_chunk_size_does_not_change_a_bit(ctx, H, W, cn, minD, D, dt):
    L, R = pm.textured_pair(H, W, cn, 3, 5)
    want = _check(ctx, L, R, dt, 8, 20, minD, D)
    for chunk in (1, 3, D):
        c = asw.Context(0, env={"ASW_PERM_CHUNK": str(chunk)})
        try:
            _check(c, L, R, dt, 8, 20, minD, D, want)
            c.stereoMatching(L, R, dt, PA(8, 20), 15, minD, D)
            assert c.timing()["aggregate_launches"] == 4 + 2 * ((D + chunk - 1) // chunk)
        finally:
            c.close()


# ---------------------------------------------------------------- ties, cache, win_size
@pytest.mark.parametrize("cn", [1, 3])
def test_tie_cases(ctx, cn):
    for L, R in (pm.constant_pair(9, 70, cn), pm.row_constant_pair(11, 70, cn)):
        for dt in (LEFT, RIGHT):
            E, vol, disp = _check(ctx, L, R, dt, 8, 20, 3, 8)
            assert (disp == 3).all()
    L, R, D, sigma, trunc = pm.barrier_pair(cn)
    E, vol, disp = _check(ctx, L, R, LEFT, sigma, trunc, 0, D)
    assert (disp[:, 62:120] == 5).all()
    c = asw.Context(0, env={"ASW_PERM_CHUNK": "8"})  # the tied candidates 5, 13 and 21 in three different chunks
    try:
        _check(c, L, R, LEFT, sigma, trunc, 0, D, (E, vol, disp))
    finally:
        c.close()


def test_sigma_table_cache_follows_sigma_back_and_forth(ctx):
    L, R = pm.textured_pair(20, 70, 3, 3, 9)
    wants = {s: _want(ctx, L, R, LEFT, s, 20, 0, 6) for s in (8, 3)}
    assert not np.array_equal(wants[8][1], wants[3][1])
    for s in (8, 3, 8, 8, 3):
        d, v = ctx.stereoMatching(L, R, LEFT, PA(s, 20), 15, 0, 6, return_cost_volume=True)
        assert np.array_equal(v, wants[s][1]) and np.array_equal(d, wants[s][2])


def test_win_size_is_not_read(ctx):
    L, R = pm.textured_pair(20, 70, 3, 3, 10)
    E, vol, disp = _want(ctx, L, R, LEFT, 8, 20, 0, 6)
    for win in (-3, 0, 15, 16):
        d, v = ctx.stereoMatching(L, R, LEFT, PA(8, 20), win, 0, 6, return_cost_volume=True)
        assert np.array_equal(v, vol) and np.array_equal(d, disp)
        assert asw.last_status() == 0


# ---------------------------------------------------------------- call forms
def _forms_pair():
    return pm.textured_pair(37, 130, 3, 4, 41) + (17,)


def test_selector_forms_and_paths(ctx):
    L, R, D = _forms_pair()
    H, W = L.shape[:2]
    alg = PA(8, 20)
    assert alg == PA()
    for dt in (LEFT, RIGHT):
        E, vol, disp = _want(ctx, L, R, dt, 8, 20, 0, D)
        d, v = ctx.stereoMatching(L, R, dt, alg, 15, 0, D, return_cost_volume=True)
        assert v.shape == (D, H, W) and np.array_equal(d, disp) and np.array_equal(v, vol)
        assert np.array_equal(ctx.stereoMatching(L, R, dt, alg, 15, 0, D), disp)
        t = ctx.timing()
        assert t["aggregate_launches"] == 6 and t["total_ms"] >= t["aggregate_ms"] > 0 and t["cost_ms"] > 0  # one chunk: 4 + 2
        d, v = ctx.computeAdaptiveWeight_permeability(L, R, dt, 8, 20, 0, D, return_cost_volume=True)
        assert np.array_equal(d, disp) and np.array_equal(v, vol)
        ctx.upload_pair(21, L, R)  # the resident path, with and without the volume
        ctx.match_resident(21, dt, alg, 15, 0, D, keep_volume=True)
        assert np.array_equal(ctx.download_disparity(21, (H, W)), disp)
        assert np.array_equal(ctx.download_volume(21, (D, H, W)), vol)
        ctx.match_resident(21, dt, alg, 15, 0, D, keep_volume=False)
        assert np.array_equal(ctx.download_disparity(21, (H, W)), disp)
        _raises(asw.ERR_NO_FRAME, ctx.download_volume, 21, (D, H, W))
        fresh = asw.Context(0)
        try:
            d, v = fresh.stereoMatching(L, R, dt, alg, 15, 0, D, return_cost_volume=True)
            assert np.array_equal(d, disp) and np.array_equal(v, vol)
        finally:
            fresh.close()
    # other parameters travel in the encoded value
    E2, vol2, disp2 = _want(ctx, L, R, LEFT, 3, 60, 0, D)
    d, v = ctx.stereoMatching(L, R, LEFT, PA(3, 60), 15, 0, D, return_cost_volume=True)
    assert np.array_equal(v, vol2) and np.array_equal(d, disp2) and not np.array_equal(vol2, _want(ctx, L, R, LEFT, 8, 20, 0, D)[1])
    # the module-level binding and its defaults (sigma 8, trunc 20, min 0, 64 candidates)
    assert np.array_equal(asw.computeAdaptiveWeight_permeability(L, R), ctx.stereoMatching(L, R, LEFT, alg, 15, 0, 64))


def test_batch_equals_single_calls(ctx):
    pairs = [pm.textured_pair(24, 150, 3, 3, 200 + i) for i in range(5)]
    for alg, params in ((PA(8, 20), (8, 20)), (PA(3, 9), (3, 9))):
        for dt in (LEFT, RIGHT):
            outs = asw.stereoMatchingBatch([p[0] for p in pairs], [p[1] for p in pairs], dt, alg, 15, 0, 12, device_ids=[0, 0])
            for (L, R), o in zip(pairs, outs):
                assert np.array_equal(o, ctx.stereoMatching(L, R, dt, alg, 15, 0, 12))
            assert np.array_equal(outs[0], _want(ctx, pairs[0][0], pairs[0][1], dt, params[0], params[1], 0, 12)[2])


@pytest.mark.parametrize("dt", [LEFT, RIGHT])
def test_subpixel_flags(ctx, dt):
    L, R = pm.textured_pair(30, 130, 3, 5, 45)
    H, W = L.shape[:2]
    for sigma, trunc, minD in ((8, 20, 0), (12, 40, 3)):
        E, vol, disp = _want(ctx, L, R, dt, sigma, trunc, minD, 12)
        for mode in MODES:
            want, ok = sp.subpixel_vec(disp, vol, minD, mode)
            assert (want != disp).any() and (np.abs(want - disp) <= 0.5).all()  # on the restatement: something moves, by half a disparity at most
            d1, v1 = ctx.stereoMatching(L, R, dt, PA(sigma, trunc), 15, minD, 12, return_cost_volume=True, subpixel=mode)
            assert np.array_equal(v1, vol) and np.array_equal(d1, want), np.argwhere(d1 != want)[:5]
            assert (d1 != disp).any() and (np.abs(d1 - disp) <= 0.5).all()
            assert np.array_equal(ctx.stereoMatching(L, R, int(dt) | mode, PA(sigma, trunc), 15, minD, 12), want)  # no kept volume
            ctx.upload_pair(22, L, R)
            ctx.match_resident(22, dt, PA(sigma, trunc), 15, minD, 12, keep_volume=False, subpixel=mode)
            assert np.array_equal(ctx.download_disparity(22, (H, W)), want)


def test_refined_calls(ctx):
    L, R = make_pair(60, 160, 16, seed=5, block=16)[:2]  # a warped pair: occlusions
    H, W = L.shape[:2]
    for sigma, trunc, minD, rwin, gc in ((8, 20, 0, 15, 150.0), (10, 30, 2, 7, 150.0)):
        dl = _want(ctx, L, R, LEFT, sigma, trunc, minD, 16)[2]
        dr = _want(ctx, L, R, RIGHT, sigma, trunc, minD, 16)[2]
        want = rr.refine_vec(L, dl, dr, minD, 16, 1.0, rwin, gc, 9.0)
        got, nrej, nunf = ctx.stereoMatchingRefined(L, R, PA(sigma, trunc), 15, minD, 16, 1.0, rwin, gc, 9.0)
        assert np.array_equal(got, want["out"]) and (nrej, nunf) == (want["n_rejected"], want["n_unfillable"])
        assert nrej > 0
        ctx.upload_pair(23, L, R)
        assert ctx.match_refined_resident(23, PA(sigma, trunc), 15, minD, 16, 1.0, rwin, gc, 9.0) == (nrej, nunf)
        assert np.array_equal(ctx.download_disparity(23, (H, W)), want["out"])
        t = ctx.timing()
        assert t["aggregate_launches"] == 12 and t["total_ms"] >= t["aggregate_ms"] > 0


# ---------------------------------------------------------------- statuses
def test_statuses(ctx):
    H, W, D = 20, 70, 12
    L, R = pm.textured_pair(H, W, 3, 3, 8)
    ok = PA(8, 20)
    ctx.upload_pair(24, L, R)

    def expect(status, alg, win=15, minD=0, numD=D):
        ctx.match_resident(24, LEFT, ok, 15, 0, D, keep_volume=True)  # a previous result
        with pytest.raises(AswError) as e:
            ctx.match_resident(24, LEFT, alg, win, minD, numD, keep_volume=True)
        assert e.value.status == status, (hex(int(alg)), win, e.value.status)
        _raises(asw.ERR_NO_FRAME, ctx.download_disparity, 24, (H, W))  # a failed match drops the slot's results
        for dt in (LEFT, RIGHT):
            _raises(status, ctx.stereoMatching, L, R, dt, alg, win, minD, numD)
            _raises(status, asw.stereoMatchingBatch, [L], [R], dt, alg, win, minD, numD, device_ids=[0])
        _raises(status, ctx.stereoMatchingRefined, L, R, alg, win, minD, numD)
        _raises(status, ctx.match_refined_resident, 24, alg, win, minD, numD)

    for win in (14, 15):  # no window: an even one changes nothing
        expect(asw.ERR_BAD_ARGUMENT, ok, win=win, numD=0)
        expect(asw.ERR_BAD_ARGUMENT, ok, win=win, minD=-1)
    for bad in (PA(0, 20), PA(8, 0), PA(256, 20), PA(8, 256), PA(-1, 7), 0x08000000 | 12,       # a zero field
                ok | 0x01000000, ok | 0x02000000, ok | 0x04000000, ok - (1 << 32) + (1 << 31)):  # bits 24..26, bit 31
        expect(asw.ERR_BAD_ARGUMENT, bad)
    for other in ((ok & ~0xFF) | 11, (ok & ~0xFF) | 2, ok & ~0xFF, (ok & ~0xFF) | 13):          # another low byte
        expect(asw.ERR_UNSUPPORTED_METHOD, other)
    expect(asw.ERR_UNSUPPORTED_METHOD, 13)
    expect(asw.ERR_BAD_ARGUMENT, asw.cross_algorithm(20, 20) | 0x08000000)    # bit 27 under bit 30 / bit 28: refused as before
    expect(asw.ERR_BAD_ARGUMENT, asw.twopass_algorithm(30, 20) | 0x08000000)
    _raises(asw.ERR_BAD_ARGUMENT, ctx.computeAdaptiveWeight_permeability, L, R, LEFT, 0, 20, 0, D)
    _raises(asw.ERR_BAD_ARGUMENT, ctx.computeAdaptiveWeight_permeability, L, R, LEFT, 8, 256, 0, D)
    _raises(asw.ERR_BAD_ARGUMENT, ctx.stereoMatching, L, R, 2, ok, 15, 0, D)  # a bad direction
    two = np.zeros((H, W, 2), np.uint8)
    _raises(asw.ERR_UNSUPPORTED_LAYOUT, ctx.stereoMatching, two, two, LEFT, ok, 15, 0, D)
    # a short volume buffer is refused before anything is computed
    li, la = asw._image(L)
    ri, ra = asw._image(R)
    disp = np.full((H, W), -7, np.float32)
    di, _ = asw._image(disp, 5)
    vol = np.zeros(D * H * W - 1, np.float32)
    rc = _lib.lib().asw_stereo_match(ctx._h, C.byref(li), C.byref(ri), C.byref(di), 0, ok, 15, 0, D, vol.ctypes.data_as(C.c_void_p), vol.size)
    assert rc == asw.ERR_BAD_ARGUMENT and (disp == -7).all()
    # and the slot works again afterwards, in the right view too
    ctx.match_resident(24, RIGHT, ok, 15, 0, D)
    assert np.array_equal(ctx.download_disparity(24, (H, W)), _want(ctx, L, R, RIGHT, 8, 20, 0, D)[2])


def test_the_other_encodings_of_entry_12_are_unchanged(ctx):
    H, W, D, cell, seed, amp, win = cr.REGION_CASES[1]
    L, R = cr.region_pair(H, W, D, seed, cell, amp)[:2]
    perm = ctx.stereoMatching(L, R, LEFT, PA(20, 20), win, 0, D, return_cost_volume=True)[1]  # the table cache is warm
    for dt in (LEFT, RIGHT):
        e = np.stack(ctx.computeAD(L, R, dt, 0, D))
        E, disp = cr.aggregate(e, cr.arms(R if int(dt) else L, 20, win // 2), 20, 0)[2:]
        for alg in (A.ADAPTIVE_WEIGHT_CROSS, asw.cross_algorithm(20, 20)):
            d, v = ctx.stereoMatching(L, R, dt, alg, win, 0, D, return_cost_volume=True)
            assert np.array_equal(d, disp) and np.array_equal(v, E)
        E, disp = ac.match(L, R, int(dt), 20, 10, 30, win, 0, D)[2:]
        d, v = ctx.stereoMatching(L, R, dt, asw.adcensus_algorithm(20, 10, 30), win, 0, D, return_cost_volume=True)
        assert np.array_equal(d, disp) and np.array_equal(v, E)
        if dt == LEFT:
            assert v.shape == perm.shape and not np.array_equal(v, perm)
    _raises(asw.ERR_BAD_ARGUMENT, ctx.stereoMatching, L, R, LEFT, asw.cross_algorithm(20, 20), 37, 0, D)
    assert ctx.stereoMatching(L, R, LEFT, A.ADAPTIVE_WEIGHT_CROSS, 14, 0, D) is None and asw.last_status() == asw.ERR_EVEN_WINDOW


# ---------------------------------------------------------------- seeded sweep
def test_seeded_sweep():
    rng = np.random.default_rng(20264)
    c = None
    try:
        for i in range(200):
            if i % 50 == 0:  # a fresh context every 50 cases
                if c is not None:
                    c.close()
                c = asw.Context(0)
            case = pm.random_case(rng, i)
            (v, d, d2), (vol, disp) = pm.gpu_result(c, case)
            assert np.array_equal(v, vol) and np.array_equal(d, disp) and np.array_equal(d2, disp), (i, case["tag"])  # pm.build_case(tag)
    finally:
        if c is not None:
            c.close()
