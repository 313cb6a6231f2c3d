"""Semi-global matching over a census cost on the GPU (asw_sgbm_census) against the integer restatement of
tests/sgbm_census_ref.py.  Every comparison is exact.  tests/test_sgbm_census_cpu.py shows on the restatement alone that the shapes
used here exercise something."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matcher_cases as mc  # noqa: E402
import sgbm_census_ref as cref  # noqa: E402
import sgbm_paths_ref as pref  # noqa: E402

pytestmark = pytest.mark.gpu

BOTH = asw._SGBM_MODE_PATHS | asw._SGBM_MODE_CENSUS


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


def _check(ctx, L, R, minD, D, w, P1, P2, m12, U, sw, sr, paths, bits=14):
    want = cref.sgbm_census(L, R, minD, D, w, P1, P2, m12, U, sw, sr, paths, bits)
    got, vol = ctx.sgbm_census(L, R, minD, D, w, P1, P2, m12, U, sw, sr, paths=paths, return_cost_volume=True)
    assert np.array_equal(vol, np.moveaxis(want["S"], 2, 0).astype(np.float32))
    assert np.array_equal(got, want["disp"])
    assert np.array_equal(ctx.sgbm_census(L, R, minD, D, w, P1, P2, m12, U, sw, sr, paths=paths), want["disp"])
    return want


MASKS = [0x07 | b for b in pref.NEW_BITS] + [pref.PATHS_HH4, pref.PATHS_SGBM, pref.PATHS_HH]
# 0x07, 0xFF and one added direction on every shape; every mask on two shapes
CASES = [(i, m) for i in range(len(cref.SHAPES)) for m in (0x07, 0xFF, 0x07 | pref.NEW_BITS[i % 5])]
CASES += [(i, m) for i in (1, 9) for m in MASKS if (i, m) not in CASES]


@pytest.mark.parametrize("i,paths", CASES)
def test_sgbm_census_matches_restatement(ctx, i, paths):
    L, R, minD, D, w, P1, P2, rest = cref.shape_case(i)
    want = _check(ctx, L, R, minD, D, w, P1, P2, *rest, paths)
    if L.shape[1] <= minD + D:
        assert (want["disp"] == 16 * (minD - 1)).all() and not want["S"].any()


@pytest.mark.parametrize("i", [1, 2])
def test_padded_rows(ctx, i):
    """both images and the int16 map as views into longer rows"""
    L, R, minD, D, w, P1, P2, rest = cref.shape_case(i)
    want = cref.sgbm_census(L, R, minD, D, w, P1, P2, *rest, 0xFF)
    Lp, Rp = mc.padded_view(L, 5, 0), mc.padded_view(R, 3, 255)
    assert Lp.strides[0] > L.strides[0] and np.array_equal(Lp, L)
    got, vol = ctx.sgbm_census(Lp, Rp, minD, D, w, P1, P2, *rest, paths=0xFF, return_cost_volume=True)
    assert np.array_equal(got, want["disp"]) and np.array_equal(vol, np.moveaxis(want["S"], 2, 0).astype(np.float32))
    # the map: a raw call into a wider int16 buffer, whose padding must stay as it was
    H, W = L.shape[:2]
    wide = np.full((H, W + 7), 12345, np.int16)
    li, _ = asw._image(Lp)
    ri, _ = asw._image(Rp)
    di = _lib.AswImage(wide.ctypes.data, H, W, 1, 3, (W + 7) * 2)
    rc = _lib.lib().asw_sgbm(ctx._h, C.byref(li), C.byref(ri), C.byref(di), minD, D, w, P1, P2, rest[0], 0, rest[1], rest[2], rest[3],
                             BOTH | 0xFF, None, 0)
    assert rc == asw.OK
    assert np.array_equal(wide[:, :W], want["disp"]) and (wide[:, W:] == 12345).all()


def test_gray_bits(ctx):
    L, R = cref.gray_bits_pair()
    try:
        ctx.set_gray_bits(15)
        b = _check(ctx, L, R, 0, 16, 3, 72, 288, 1, 10, 20, 2, 0xFF, bits=15)
    finally:
        ctx.set_gray_bits(14)
    a = _check(ctx, L, R, 0, 16, 3, 72, 288, 1, 10, 20, 2, 0xFF, bits=14)
    assert not np.array_equal(a["S"], b["S"])


@pytest.mark.parametrize("i", [1, 5])
def test_settings(ctx, i):
    """P1 = P2 = 0 with the uniqueness rule's default (-1), and penalties with every later stage at work"""
    L, R, minD, D, w, _, _, _ = cref.shape_case(i)
    _check(ctx, L, R, minD, D, w, 0, 0, 0, -1, 0, 0, 0xFF)
    _check(ctx, L, R, minD, D, w, 8 * w * w, 32 * w * w, 1, 10, 20, 2, 0x37)


def test_width_limit(ctx):
    """both code rows of a frame row are staged in LDS: 10240 columns fill the 160 KB, one more is refused"""
    D = 16
    L, R = cref.shape_pair(2, 10241, D, 1, seed=5)
    Lw, Rw = np.ascontiguousarray(L[:, :10240]), np.ascontiguousarray(R[:, :10240])
    _check(ctx, Lw, Rw, 0, D, 3, 72, 288, 1, 10, 20, 2, 0x07)
    with pytest.raises(asw.AswError) as e:
        ctx.sgbm_census(L, R, 0, D, 3, 72, 288, 1, 10, 20, 2, paths=0x07)
    assert e.value.status == asw.ERR_BAD_ARGUMENT
    Ls, Rs, minD, Ds, w, P1, P2, rest = cref.shape_case(0)
    _check(ctx, Ls, Rs, minD, Ds, w, P1, P2, *rest, 0x07)


def _raw(ctx, L, R, mode, cap=0, P2=0, w=5, vol=None, vol_floats=0):
    li, _ = asw._image(L)
    ri, _ = asw._image(R)
    out = np.zeros(L.shape[:2], np.int16)
    oi, _ = asw._image(out, 3)
    pv = None if vol is None else vol.ctypes.data_as(C.c_void_p)
    rc = _lib.lib().asw_sgbm(ctx._h, C.byref(li), C.byref(ri), C.byref(oi), 0, 16, w, 8, P2, 1, cap, 10, 20, 2, mode, pv, vol_floats)
    return rc, out


def test_statuses(ctx):
    L, R, _, _, _, _, _, _ = cref.shape_case(0)
    H, W = L.shape[:2]
    for mode, status in ((BOTH | 0x100, asw.ERR_BAD_ARGUMENT), (BOTH | 0x30, asw.ERR_UNSUPPORTED_METHOD),
                         (BOTH | 0x20000, asw.ERR_BAD_ARGUMENT), (asw._SGBM_MODE_CENSUS, asw.ERR_UNSUPPORTED_METHOD),
                         (asw._SGBM_MODE_CENSUS | 0x07, asw.ERR_UNSUPPORTED_METHOD), (BOTH | 0x07, asw.OK), (BOTH | 0xFF, asw.OK)):
        assert _raw(ctx, L, R, mode)[0] == status, hex(mode)
    for kw, status in ((dict(paths=0x100), asw.ERR_BAD_ARGUMENT), (dict(paths=-1), asw.ERR_BAD_ARGUMENT),
                       (dict(paths=0x30), asw.ERR_UNSUPPORTED_METHOD), (dict(paths=0), asw.ERR_UNSUPPORTED_METHOD)):
        with pytest.raises(asw.AswError) as e:
            ctx.sgbm_census(L, R, 0, 16, 5, **kw)
        assert e.value.status == status, kw
    with pytest.raises(asw.AswError) as e:
        ctx.sgbm_census(L, R, 0, 24, 5)
    assert e.value.status == asw.ERR_BAD_ARGUMENT
    # n (62 k^2 + P2) >= 2^31 with k = 5: 62 * 25 = 1550
    for n, mask in ((3, 0x07), (8, 0xFF)):
        edge = -((-(1 << 31)) // n) - 1550  # the smallest P2 that is refused
        assert n * (1550 + edge) >= 1 << 31 > n * (1550 + edge - 1)
        assert _raw(ctx, L, R, BOTH | mask, P2=edge)[0] == asw.ERR_BAD_ARGUMENT
        assert _raw(ctx, L, R, BOTH | mask, P2=edge - 1)[0] == asw.OK
        # the Birchfield-Tomasi bound has C_max = 3 * (2 * 15 + 63) * 25 = 6975 > 1550: it refuses a P2 the census cost takes
        assert _raw(ctx, L, R, asw._SGBM_MODE_PATHS | mask, P2=edge - 1)[0] == asw.ERR_BAD_ARGUMENT
        # with the volume the same bound at 2^24
        edge24 = -((-(1 << 24)) // n) - 1550
        vol = np.zeros((16, H, W), np.float32)
        assert _raw(ctx, L, R, BOTH | mask, P2=edge24, vol=vol, vol_floats=vol.size)[0] == asw.ERR_BAD_ARGUMENT
        assert _raw(ctx, L, R, BOTH | mask, P2=edge24 - 1, vol=vol, vol_floats=vol.size)[0] == asw.OK
        assert _raw(ctx, L, R, BOTH | mask, P2=edge24)[0] == asw.OK
    vol = np.zeros((16, H, W), np.float32)
    assert _raw(ctx, L, R, BOTH | 0xFF, vol=vol, vol_floats=vol.size - 1)[0] == asw.ERR_BAD_ARGUMENT
    assert _raw(ctx, L, R, BOTH | 0xFF, vol=vol, vol_floats=vol.size)[0] == asw.OK


@pytest.mark.parametrize("kind,mask", cref.INVARIANCE)
def test_gain_and_offset_on_the_gpu(ctx, kind, mask):
    """without the restatement: another gain and offset in the right camera changes nothing under the census cost, and changes
    the result under the Birchfield-Tomasi cost"""
    L, R, R2 = cref.invariance_pair(kind)
    minD, D, w, P1, P2, m12, U, sw, sr = cref.INVARIANCE_ARGS
    a, va = ctx.sgbm_census(L, R, minD, D, w, P1, P2, m12, U, sw, sr, paths=mask, return_cost_volume=True)
    b, vb = ctx.sgbm_census(L, R2, minD, D, w, P1, P2, m12, U, sw, sr, paths=mask, return_cost_volume=True)
    assert np.array_equal(a, b) and np.array_equal(va, vb) and va.any()
    c, vc = ctx.sgbm_paths(L, R, minD, D, w, P1, P2, m12, 10, U, sw, sr, paths=mask, return_cost_volume=True)
    d, vd = ctx.sgbm_paths(L, R2, minD, D, w, P1, P2, m12, 10, U, sw, sr, paths=mask, return_cost_volume=True)
    assert not np.array_equal(vc, vd) and not np.array_equal(c, d)


def test_pre_filter_cap_is_ignored(ctx):
    L, R, _, _, _, _, _, _ = cref.shape_case(0)
    rc0, a = _raw(ctx, L, R, BOTH | 0xFF, cap=0)
    rc1, b = _raw(ctx, L, R, BOTH | 0xFF, cap=63)
    assert rc0 == rc1 == asw.OK and np.array_equal(a, b)
    assert np.array_equal(a, cref.sgbm_census(L, R, 0, 16, 5, 8, 0, 1, 10, 20, 2, 0xFF)["disp"])
    # the same slot does change asw_sgbm_paths' result
    assert not np.array_equal(_raw(ctx, L, R, asw._SGBM_MODE_PATHS | 0xFF, cap=0)[1],
                              _raw(ctx, L, R, asw._SGBM_MODE_PATHS | 0xFF, cap=63)[1])


def test_no_state_leaks_into_the_other_matchers(ctx):
    """the census codes live where the prefiltered planes live: sgbm and sgbm_paths after a census call return what they returned
    before it"""
    L, R, minD, D, w, P1, P2, rest = cref.shape_case(1)
    bt = (rest[0], 10) + rest[1:]
    a0 = ctx.sgbm(L, R, minD, D, w, P1, P2, *bt, return_cost_volume=True)
    b0 = ctx.sgbm_paths(L, R, minD, D, w, P1, P2, *bt, paths=0xFF, return_cost_volume=True)
    c0 = ctx.sgbm_census(L, R, minD, D, w, P1, P2, *rest, paths=0xFF, return_cost_volume=True)
    a1 = ctx.sgbm(L, R, minD, D, w, P1, P2, *bt, return_cost_volume=True)
    c1 = ctx.sgbm_census(L, R, minD, D, w, P1, P2, *rest, paths=0xFF, return_cost_volume=True)
    b1 = ctx.sgbm_paths(L, R, minD, D, w, P1, P2, *bt, paths=0xFF, return_cost_volume=True)
    for x, y in ((a0, a1), (b0, b1), (c0, c1)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
    assert not np.array_equal(b0[1], c0[1])


def test_timing(ctx):
    L, R, minD, D, w, P1, P2, rest = cref.shape_case(1)
    for mask, launches in ((0x07, 2), (0x0F, 3), (0x17, 3), (0x57, 3), (0x37, 4), (0xFF, 5)):
        ctx.sgbm_census(L, R, minD, D, w, P1, P2, *rest, paths=mask)
        t = ctx.timing()
        assert t["aggregate_launches"] == launches and 0 < t["aggregate_ms"] < t["total_ms"], hex(mask)
