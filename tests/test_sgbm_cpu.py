"""CPU-side checks of the SGBM feature: the two restatements of tests/sgbm_ref.py agree, hand-worked answers of each step, and the
C-ABI exports (no GPU needed)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from aswstereomatch_amd import _lib, build
from aswstereomatch_amd.synth import make_pair, shifted_pair

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgbm_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(H, W, cn, seed):
    L, R, _ = make_pair(H, W, 8, seed=seed, block=8)
    if cn == 1:
        return np.ascontiguousarray(L[:, :, 0]), np.ascontiguousarray(R[:, :, 0])
    return L, R


# H, W, cn, minD, D, block, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio
@pytest.mark.parametrize("H,W,cn,minD,D,w,P1,P2,M,cap,U", [
    (5, 37, 3, 0, 16, 3, 72, 288, 1, 10, 10),     # odd W
    (2, 29, 1, 0, 16, 5, 200, 800, 1, 10, 10),    # H < block
    (6, 41, 1, 3, 16, 1, 8, 32, 0, 31, 5),        # minD > 0, block 1
    (4, 34, 3, 0, 16, 5, 0, 0, 2, 62, 0),         # default P1 / P2, no uniqueness rule
    (3, 50, 3, 1, 32, 3, 300, 100, 1, 10, 15),    # P2 <= P1
    (7, 19, 1, 0, 16, 3, 10, 40, 1, 10, 10),      # W <= maxD: all INVALID
])
def test_vectorised_equals_scalar(H, W, cn, minD, D, w, P1, P2, M, cap, U):
    L, R = _pair(H, W, cn, seed=H * W)
    got = ref.sgbm(L, R, minD, D, w, P1, P2, M, cap, U, 0, 0)
    S, disp = ref.sgbm_scalar(L, R, minD, D, w, P1, P2, M, cap, U)
    assert np.array_equal(got["S"], np.array(S, np.int64))
    assert np.array_equal(got["raw"], np.array(disp, np.int16))


def test_bt_interval_and_cost_on_a_row():
    a = np.array([10, 20, 14, 14, 30, 0], np.int64)
    lo, hi = ref.bt_minmax(a)
    assert lo.tolist() == [10, 15, 14, 14, 15, 0]
    assert hi.tolist() == [15, 20, 17, 22, 30, 15]
    # u = a[1] against v = a[2]: min(max(0, 20 - 17, 14 - 20), max(0, 14 - 20, 15 - 14)) = min(3, 1)
    assert ref.bt_cost(a[1], lo[1], hi[1], a[2], lo[2], hi[2]) == 1
    assert ref.bt_cost(a[2], lo[2], hi[2], a[3], lo[3], hi[3]) == 0  # equal values
    # u = 30 lies 15 above v's interval [0, 15]; v = 0 lies 15 below u's [15, 30]
    assert ref.bt_cost(a[4], lo[4], hi[4], a[5], lo[5], hi[5]) == 15


def test_prefilter_border_columns_hold_ftzero():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(6, 9, 3)).astype(np.uint8)
    p = ref.prefilter(img, 15)
    assert p.shape == (6, 6, 9)
    assert (p[:, :, 0] == 15).all() and (p[:, :, -1] == 15).all()  # Sobel and raw planes alike
    assert np.array_equal(p[3:, :, 1:-1], img[:, 1:-1].transpose(2, 0, 1))
    assert p[:3].min() >= 0 and p[:3].max() <= 30


def test_sobel_value_and_clip():
    img = np.zeros((3, 5), np.uint8)
    img[:, 3] = 4  # a step between columns 2 and 3
    p = ref.prefilter(img, 15)[0]
    # x = 2, every row: 2 * (4 - 0) + (4 - 0) + (4 - 0) = 16 -> clipped to 15, shifted to 30
    assert p[:, 2].tolist() == [30, 30, 30]
    img[:, 3] = 2
    assert ref.prefilter(img, 15)[0][:, 2].tolist() == [8 + 15] * 3
    assert ref.prefilter(img, 15)[0][:, 1].tolist() == [15] * 3


@pytest.mark.parametrize("cap,ftzero", [(10, 15), (31, 31), (62, 63), (0, 15), (16, 17)])
def test_ftzero(cap, ftzero):
    assert ref.effective_params(5, 8, 32, 1, cap, 10)[1] == ftzero


def test_effective_penalties_and_defaults():
    assert ref.effective_params(0, 0, 0, 0, 0, -1) == (5, 15, 2, 5, 1, 10)
    assert ref.effective_params(3, 600, 100, 1, 10, 10)[2:4] == (600, 601)  # P2 <= P1 -> P1 + 1
    assert ref.effective_params(3, 10, 11, 1, 10, 10)[2:4] == (10, 11)
    assert ref.effective_params(3, 10, 3, 7, 10, 0)[2:] == (10, 11, 7, 0)


def test_selector_bound_fits_int16_limit_documented():
    # win 15, cn 3 (the reference's call): C_max = 62775 fits u16; S = 3 (C_max + P2) passes int16 -- DESIGN.md section 4.8
    p = ref.selector_params(3, 15)
    cmax = ref.cost_bound(3, 15, 15)
    assert cmax == 62775 and 3 * (cmax + p["P2"]) > 32767
    assert 3 * (cmax + p["P2"]) < 2 ** 24


def test_speckles_island_size():
    m = np.zeros((7, 7), np.int16)
    m[2:5, 2:5] = 100  # a 9-pixel island, |100 - 0| > maxDiff
    removed = ref.filter_speckles(m, -16, 9, 16)
    assert (removed[2:5, 2:5] == -16).all() and (removed[m == 0] == -16).sum() == 0
    assert np.array_equal(ref.filter_speckles(m, -16, 8, 16), m)


def test_speckles_join_threshold():
    m = np.zeros((4, 4), np.int16)
    m[:, 2:] = 16
    # |delta| = maxDiff joins the halves into one component of 16 pixels; maxDiff - 1 leaves two of 8
    assert np.array_equal(ref.filter_speckles(m, -16, 15, 16), m)
    assert (ref.filter_speckles(m, -16, 8, 15) == -16).all()
    assert np.array_equal(ref.filter_speckles(m, -16, 7, 15), m)


def test_speckles_new_val_never_joins():
    m = np.zeros((3, 7), np.int16)
    m[:, 3] = -16  # a wall of newVal between two 9-pixel halves; -16 is within maxDiff of 0 but never joins
    out = ref.filter_speckles(m, -16, 9, 64)
    assert (out == -16).all()
    assert np.array_equal(ref.filter_speckles(m, -16, 8, 64), m)


def test_median_corners():
    a = np.arange(1, 10, dtype=np.int16).reshape(3, 3)
    med = ref.median3(a)
    assert med[0, 0] == 2 and med[2, 2] == 8 and med[1, 1] == 5 and med[0, 2] == 3 and med[2, 0] == 7


def test_u8_rounding_ties_and_saturation():
    v = np.array([-16, 0, 7, 8, 9, 24, 40, 56, 4072, 4088, 4096, 8000], np.int16)
    assert ref.disp16_to_u8(v).tolist() == [0, 0, 0, 0, 1, 2, 2, 4, 254, 255, 255, 255]


def _lr(entries, W=24, minD=0, D=16, M=1, subpix=None):
    """one row with the given (x, best, minS) winners; subpix: {x: scaled disparity} overrides"""
    x0 = minD + D
    valid = np.zeros(W - x0, bool)
    best = np.zeros(W - x0, np.int64)
    minS = np.zeros(W - x0, np.int64)
    disp = np.full(W, 16 * (minD - 1), np.int64)
    for x, b, s in entries:
        valid[x - x0], best[x - x0], minS[x - x0] = True, b, s
        disp[x] = 16 * (b + minD)
    for x, v in (subpix or {}).items():
        disp[x] = v
    return ref.lr_check_row(disp, valid, best, minS, x0, W, minD, M)


def test_lr_rule():
    INVALID = -16
    # x 20 -> x2 15 (disp2 5); x 21 -> x2 16 (disp2 5, minS 50 beats x 22's 70); x 22 (d 6) reads disp2[16] = 5
    e = [(20, 5, 100), (21, 5, 50), (22, 6, 70)]
    assert _lr(e, M=1)[22] == 96            # |5 - 6| <= 1
    assert _lr(e, M=0)[22] == INVALID       # lo = hi = 6: both columns disagree
    # subpixel 101: lo 6 reads disp2[16] = 5, hi 7 reads disp2[15] = 5; invalid only when BOTH disagree
    assert _lr(e, M=0, subpix={22: 101})[22] == INVALID
    assert _lr(e, M=1, subpix={22: 101})[22] == 101
    # a tie on minS: the smallest x wins the target column (x 20 with d 4 and x 21 with d 5 both map to 16)
    t = [(20, 4, 50), (21, 5, 50), (22, 6, 70)]
    assert _lr(t, M=1)[22] == INVALID       # disp2[16] = 4: |4 - 6| > 1
    t2 = [(20, 4, 60), (21, 5, 50), (22, 6, 70)]
    assert _lr(t2, M=1)[22] == 96           # disp2[16] = 5
    # a target column no pixel chose holds minD - 1 and never invalidates
    assert _lr([(22, 6, 70)], M=0)[22] == 96


def test_shifted_pair_gives_the_shift():
    d0 = 7
    L, R = shifted_pair(24, 80, d0)
    out = ref.sgbm(L, R, 0, 16, 5, 600, 2400, 1, 10, 10, 0, 0)
    assert (out["raw"][2:-2, 24:-4] == 16 * d0).all()


# ---------------------------------------------------------------- the C-ABI (fails before the SGBM entry points exist)
@pytest.fixture(scope="module")
def so():
    build.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_sgbm_abi(so):
    for name in ("asw_sgbm", "asw_filter_speckles"):
        assert name in _lib.ABI_SYMBOLS and hasattr(so, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {"asw_sgbm", "asw_filter_speckles"} <= {l.split()[2] for l in out.splitlines() if len(l.split()) == 3}
    hdr = open(os.path.join(ROOT, "include", "asw_mi355x.h")).read()
    assert re.search(r"\bASW_16S\s*=\s*3\b", hdr)
    assert re.search(r"^int asw_sgbm\(", hdr, flags=re.M) and re.search(r"^int asw_filter_speckles\(", hdr, flags=re.M)
    l = _lib.lib()
    assert l.asw_volume_planes(1, 64) == 0 and l.asw_volume_planes(0, 64) == 0
    # no context needed to refuse a null one
    img = _lib.AswImage(None, 1, 1, 1, 3, 2)
    assert l.asw_filter_speckles(None, ctypes.byref(img), 0, 1, 1) == 7
    assert l.asw_sgbm(None, None, None, None, 0, 16, 5, 0, 0, 0, 0, 0, 0, 0, 2, None, 0) == 7
