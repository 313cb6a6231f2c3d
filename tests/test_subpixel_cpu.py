"""Sub-pixel rule without a GPU: the restatement of tests/subpixel_ref.py on hand cases, its non-vacuity
and its value on the CPU oracle's volumes, and the constants of the public surface."""
import os
import re
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd.synth import make_pair
from oracle import asw_oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subpixel_ref as sp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = np.float32(np.nan), np.float32(np.inf)
PAIRS = {"a": (96, 260, 24, 11, 32), "b": (60, 160, 16, 5, 16)}

# the selector's literals (M.cpp:58-82), LEFT view -> (rc, integer map, aggregated volume)
ORACLE = {
    "classic": lambda L, R, win, minD, D: asw_oracle.asw_classic(L, R, 30.0, 20.0, 0, win, minD, D, want_vol=True),
    "geodesic": lambda L, R, win, minD, D: asw_oracle.asw_geodesic(L, R, 0, win, minD, D, want_vol=True),
    "GuidedF": lambda L, R, win, minD, D: asw_oracle.asw_guided(L, R, 0, 1e-6, win, minD, D, want_vol=True),
    "GuidedF_2": lambda L, R, win, minD, D: asw_oracle.asw_guided2(L, R, 0, 1e-6, win, minD, D, want_vol=True),
    "GuidedF_3": lambda L, R, win, minD, D: asw_oracle.asw_guided3(L, R, 0, 1e-6, win, minD, D, want_vol=True),
    "median": lambda L, R, win, minD, D: asw_oracle.asw_wmedian(L, R, 0, win, 10.0, 10.0, minD, D, want_vol=True),
    "BLO1": lambda L, R, win, minD, D: asw_oracle.asw_blo1(L, R, 0, 0.015, win, minD, D, want_vol=True),
    "direct8": lambda L, R, win, minD, D: asw_oracle.asw_direct8(L, R, 0, win, minD, D, want_vol=True),
    "bilgrid": lambda L, R, win, minD, D: asw_oracle.asw_bilgrid(L, R, 0, 10.0, 10.0, minD, D, want_vol=True),
}
SHARE_METHODS = ["classic", "geodesic", "GuidedF", "GuidedF_2", "median", "BLO1", "direct8"]


def _column(costs, d, minD=0):
    """One pixel: volume [n][1][1] of `costs`, integer map [[d]]."""
    return np.full((1, 1), d, np.float32), np.asarray(costs, np.float32).reshape(-1, 1, 1), minD


# ---- 1. hand cases ----
@pytest.mark.parametrize("mode", sp.MODES)
def test_hand_cases(mode):
    def one(costs, d, minD=0):
        disp, vol, minD = _column(costs, d, minD)
        out, ok = sp.subpixel_vec(disp, vol, minD, mode)
        lo, ok2 = sp.subpixel_loop(disp, vol, minD, mode)
        assert out.tobytes() == lo.tobytes() and np.array_equal(ok, ok2)
        assert out.dtype == np.float32
        return float(out[0, 0]), bool(ok[0, 0])

    assert one([5, 2, 5], 1) == (1.0, True)                 # a symmetric triple: offset 0, but refined
    # sign convention, by hand: cm = c0 says the minimum lies half-way towards k - 1 -> off = (c0 - cp) / (2 (cp - c0)) = -0.5
    assert one([2, 2, 5], 1) == (0.5, True)
    assert one([5, 2, 2], 1) == (1.5, True)                 # cp = c0: +0.5
    # cm = 4, c0 = 1, cp = 2 by hand: parabola (4 - 2) / (2 * (3 + 1)) = 0.25; equiangular (4 - 2) / (2 * 3) = 1 / 3
    want = 0.25 if mode == sp.PARABOLA else 1.0 / 3.0
    assert one([4, 1, 2], 1) == (float(np.float32(1.0 + want)), True)
    assert one([2, 1, 4], 1) == (float(np.float32(1.0 - want)), True)
    # minD > 0: d = 7, k = 3 -> cm = 3, c0 = 1, cp = 2: parabola 1 / (2 * (2 + 1)) = 1 / 6, equiangular 1 / (2 * 2) = 0.25
    want = 1.0 / 6.0 if mode == sp.PARABOLA else 0.25
    assert one([9, 7, 3, 1, 2, 8], 7, minD=4) == (float(np.float32(7.0 + want)), True)
    # untouched: edge planes, non-finite neighbours, a plateau, a winner that is not a local minimum, a map value outside the volume
    assert one([1, 2, 3], 0) == (0.0, False)
    assert one([3, 2, 1], 2) == (2.0, False)
    assert one([1, 2], 0) == (0.0, False) and one([2, 1], 1) == (1.0, False) and one([1], 0) == (0.0, False)
    for bad in (NAN, INF, -INF):
        assert one([bad, 1, 2], 1) == (1.0, False)
        assert one([2, 1, bad], 1) == (1.0, False)
    assert one([2, NAN, 3], 1) == (1.0, False) and one([2, -INF, 3], 1) == (1.0, False)
    assert one([2, 2, 2], 1) == (1.0, False)                # den = 0
    assert one([1, 2, 3], 1) == (1.0, False)                # cm < c0
    assert one([3, 2, 1], 1) == (1.0, False)                # cp < c0
    assert one([5, 2, 5], 0, minD=3) == (0.0, False)        # the literal 0 of a pixel without a winner, minD > 0
    assert one([5, 2, 5], 9) == (9.0, False)
    out, ok = sp.subpixel_vec(np.full((1, 1), NAN), np.zeros((3, 1, 1), np.float32), 0, mode)
    assert np.isnan(out[0, 0]) and not ok[0, 0]


@pytest.mark.parametrize("mode", sp.MODES)
def test_loop_form_equals_vector_form(mode):
    rng = np.random.default_rng(3)
    n, H, W, minD = 9, 17, 23, 2
    vol = rng.integers(0, 6, (n, H, W)).astype(np.float32) / 4  # many ties and plateaus
    vol[rng.random(vol.shape) < 0.05] = NAN
    vol[rng.random(vol.shape) < 0.03] = INF
    disp = asw_oracle.wta(vol, minD)
    disp[0, :5] = [NAN, INF, -7.0, float(minD + n), 1e30]
    a, oka = sp.subpixel_vec(disp, vol, minD, mode)
    b, okb = sp.subpixel_loop(disp, vol, minD, mode)
    assert a.tobytes() == b.tobytes() and np.array_equal(oka, okb)
    assert 0.1 < oka.mean() < 0.9
    with np.errstate(invalid="ignore"):
        assert (np.abs(a - disp)[oka] <= 0.5).all() and a[~oka].tobytes() == disp[~oka].tobytes()


# ---- 2. non-vacuity on the oracle's volumes ----
# GuidedF_3 refines only about half of the pixels of pair b: a share is required of it on pair a alone
SHARE_CASES = [(p, m) for p in ("a", "b") for m in SHARE_METHODS + ["bilgrid"]] + [("a", "GuidedF_3")]


@pytest.mark.parametrize("pair,method", SHARE_CASES)
def test_refined_share_on_oracle_volumes(pair, method):
    H, W, D, seed, block = PAIRS[pair]
    L, R, _ = make_pair(H, W, D, seed=seed, block=block)
    rc, disp, vol = ORACLE[method](L, R, 15, 0, D)
    assert rc == 0
    for mode in sp.MODES:
        out, ok = sp.subpixel_vec(disp, vol, 0, mode)
        print("%s pair %s mode %#x: refined share %.3f" % (method, pair, mode, ok.mean()))
        if method == "bilgrid":  # its volume is almost all non-finite on these pairs: the guards leave the map alone
            assert out.tobytes() == disp.tobytes()
            continue
        assert ok.mean() >= 0.75
        assert (np.abs(out - disp) <= 0.5).all() and (out != disp).mean() >= 0.5


# ---- 3. value: the slanted plane ----
@pytest.mark.parametrize("method", ["classic", "geodesic", "GuidedF", "GuidedF_2", "BLO1", "median"])
def test_slanted_plane_value(method):
    L, R, gt = sp.slanted_plane_pair()
    rc, disp, vol = ORACLE[method](L, R, 15, 0, 16)
    assert rc == 0
    mae_int = sp.cropped_mae(disp, gt)
    for mode in sp.MODES:
        mae_sub = sp.cropped_mae(sp.subpixel_vec(disp, vol, 0, mode)[0], gt)
        print("%s mode %#x: MAE integer %.4f, sub-pixel %.4f, ratio %.3f" % (method, mode, mae_int, mae_sub, mae_sub / mae_int))
        if method == "median":
            assert mae_sub < mae_int
        else:
            assert mae_sub <= 0.6 * mae_int


# ---- 4. surface ----
def test_public_surface():
    hdr = open(os.path.join(ROOT, "include", "asw_mi355x.h")).read()
    assert re.search(r"ASW_DISPARITY_SUBPIXEL_PARABOLA\s*=\s*0x100\b", hdr)
    assert re.search(r"ASW_DISPARITY_SUBPIXEL_EQUIANGULAR\s*=\s*0x200\b", hdr)
    assert asw.SUBPIXEL_PARABOLA == 0x100 == sp.PARABOLA and asw.SUBPIXEL_EQUIANGULAR == 0x200 == sp.EQUIANGULAR
    assert "SUBPIXEL_PARABOLA" in asw.__all__ and "SUBPIXEL_EQUIANGULAR" in asw.__all__
    assert (asw.DISPARITY_RIGHT | asw.SUBPIXEL_EQUIANGULAR) == 0x201
    import inspect

    for fn in (asw.Context.stereoMatching, asw.Context.match_resident, asw.stereoMatchingBatch):
        assert inspect.signature(fn).parameters["subpixel"].default is None
