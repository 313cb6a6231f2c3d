"""CPU-side checks of semi-global matching over a census cost (asw_sgbm_census): the two statements of the
block cost in tests/sgbm_census_ref.py agree, the cost bound is what the host layer assumes and is reached, a gain and offset
between the cameras leaves the census result unchanged and changes the Birchfield-Tomasi result, the vacuity conditions that keep
the GPU parity tests of tests/test_gpu_sgbm_census.py from passing on inputs that exercise nothing, and the encoding (the header's
inline function, the Python mask travel).  No GPU needed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matcher_cases as mc  # noqa: E402
import sgbm_census_ref as cref  # noqa: E402
import sgbm_paths_ref as pref  # noqa: E402
from shim_build import C99, build_demo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "asw_mi355x.h")

# H, W, minD, D, block: the tiny frames of the SGBM files, and two where the window is wider and taller than the valid area
TINY = mc.SGBM_TINY_FRAMES + [(2, 40, 0, 16, 11), (1, 33, 0, 32, 9)]


# ---------------------------------------------------------------- the two statements agree
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("H,W,minD,D,w", TINY)
def test_literal_and_vectorised_block_costs_agree(H, W, minD, D, w, cn):
    L, R = mc.make_input("textured", H, W, cn, seed=H * 31 + W, D=D)
    C = cref.block_cost(L, R, minD, D, w)
    assert C.shape == (H, W - minD - D, D)
    assert C.tolist() == cref.block_cost_loop(L, R, minD, D, w)
    assert C.min() >= 0 and C.max() <= cref.cost_bound(w)


def test_gray_bits_reach_the_cost():
    L, R = cref.gray_bits_pair()
    assert not np.array_equal(cref.block_cost(L, R, 0, 16, 3, 14), cref.block_cost(L, R, 0, 16, 3, 15))
    a = cref.sgbm_census(L, R, 0, 16, 3, 72, 288, 1, 10, 20, 2, 0xFF, bits=14)
    b = cref.sgbm_census(L, R, 0, 16, 3, 72, 288, 1, 10, 20, 2, 0xFF, bits=15)
    assert not np.array_equal(a["S"], b["S"])


def test_cost_bound_is_reached():
    """62 per pixel is reached: a left pixel all of whose 62 neighbours are below it (code: all ones) against a flat right image
    (code 0) costs 62 at every candidate; with block 1 that is C_max.  A larger block sums k^2 pixels of at most 62 each."""
    H, W, D = 9, 40, 16
    L = np.full((H, W), 10, np.uint8)
    L[4, 30] = 200
    R = np.full((H, W), 50, np.uint8)
    C = cref.block_cost(L, R, 0, D, 1)
    assert C.max() == 62 == cref.cost_bound(1) and (C[4, 30 - D] == 62).all()
    assert C.tolist() == cref.block_cost_loop(L, R, 0, D, 1)
    for w in (3, 5, 11):
        k = 2 * (w // 2) + 1
        assert cref.cost_bound(w) == 62 * k * k and 62 <= cref.block_cost(L, R, 0, D, w).max() <= cref.cost_bound(w)


# ---------------------------------------------------------------- what the cost is wanted for
@pytest.mark.parametrize("kind,mask", cref.INVARIANCE)
def test_gain_and_offset_leave_the_census_result_unchanged(kind, mask):
    L, R, R2 = cref.invariance_pair(kind)
    assert R2.max() <= 254 and np.array_equal(R2.astype(int), 2 * R.astype(int) + 10)
    minD, D, w, P1, P2, m12, U, sw, sr = cref.INVARIANCE_ARGS
    a = cref.sgbm_census(L, R, minD, D, w, P1, P2, m12, U, sw, sr, mask)
    b = cref.sgbm_census(L, R2, minD, D, w, P1, P2, m12, U, sw, sr, mask)
    assert np.array_equal(a["S"], b["S"]) and np.array_equal(a["disp"], b["disp"])
    assert len(np.unique(a["disp"])) > 2
    # the Birchfield-Tomasi cost on the same inputs: S changes, and the map on more than a tenth of the pixels (a condition
    # that keeps this test from being vacuous, not a measurement)
    c = pref.sgbm_paths(L, R, minD, D, w, P1, P2, m12, 10, U, sw, sr, mask)
    d = pref.sgbm_paths(L, R2, minD, D, w, P1, P2, m12, 10, U, sw, sr, mask)
    moved = float((c["disp"] != d["disp"]).mean())
    print("%s mask %#x: BT map changed on %.3f of the pixels" % (kind, mask, moved))
    assert not np.array_equal(c["S"], d["S"]) and moved > 0.1


def test_census_map_differs_from_the_bt_map():
    for cn in (1, 3):
        L, R = mc.make_input("textured", 23, 90, cn, seed=11, D=32)
        a = cref.sgbm_census(L, R, 1, 32, 5, 200, 800, 1, 10, 20, 2, 0xFF)["disp"]
        b = pref.sgbm_paths(L, R, 1, 32, 5, 200, 800, 1, 10, 10, 20, 2, 0xFF)["disp"]
        assert float((a != b)[:, 33:].mean()) > 0.05


# ---------------------------------------------------------------- the GPU shapes exercise something
@pytest.mark.parametrize("i", range(len(cref.SHAPES)))
def test_gpu_shapes_are_not_vacuous(i):
    """per shape of tests/test_gpu_sgbm_census.py: more than one valid disparity in the expected map, a map that is not the
    Birchfield-Tomasi map, and an S that depends on the path mask"""
    L, R, minD, D, w, P1, P2, rest = cref.shape_case(i)
    a = cref.sgbm_census(L, R, minD, D, w, P1, P2, *rest, 0x07)
    b = cref.sgbm_census(L, R, minD, D, w, P1, P2, *rest, 0xFF)
    INVALID = 16 * (minD - 1)
    if L.shape[1] <= minD + D:
        assert (b["disp"] == INVALID).all() and not b["S"].any()
        return
    assert not np.array_equal(a["S"], b["S"])
    bt = pref.sgbm_paths(L, R, minD, D, w, P1, P2, rest[0], 10, *rest[1:], 0xFF)
    assert not np.array_equal(b["S"], bt["S"]) and not np.array_equal(b["disp"], bt["disp"])
    assert len(np.unique(b["disp"][b["disp"] != INVALID])) > 1


# ---------------------------------------------------------------- encoding
def test_header_and_inline_function(tmp_path):
    text = open(HEADER).read()
    assert "ASW_SGBM_MODE_CENSUS = 0x%X" % asw._SGBM_MODE_CENSUS in text and asw._SGBM_MODE_CENSUS == 0x10000
    assert re.search(r"^static inline int asw_sgbm_census\(", text, re.M)
    # the inline function from a C99 program that supplies its own asw_sgbm and prints what arrives there
    src = tmp_path / "enc.c"
    src.write_text('#include <stdio.h>\n#include "asw_mi355x.h"\n'
                   'int asw_sgbm(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp16, int min_disparity,\n'
                   '             int num_disparities, int block_size, int p1, int p2, int disp12_max_diff, int pre_filter_cap,\n'
                   '             int uniqueness_ratio, int speckle_window_size, int speckle_range, int mode, float* cost_volume_out,\n'
                   '             size_t cost_volume_floats)\n{\n'
                   '    (void)ctx; (void)left; (void)right; (void)disp16; (void)cost_volume_out;\n'
                   '    printf("%d %d %d %d %d %d %d %d %d %d %d %d\\n", min_disparity, num_disparities, block_size, p1, p2, disp12_max_diff,\n'
                   '           pre_filter_cap, uniqueness_ratio, speckle_window_size, speckle_range, mode, (int)cost_volume_floats);\n'
                   '    return 0;\n}\n'
                   'int main(void)\n{\n'
                   '    asw_sgbm_census(0, 0, 0, 0, 1, 32, 5, 8, 9, 10, 11, 12, 13, 0x37, 0, 14);\n'
                   '    asw_sgbm_census(0, 0, 0, 0, 1, 32, 5, 8, 9, 10, 11, 12, 13, 0x107, 0, 14);\n'
                   '    asw_sgbm_census(0, 0, 0, 0, 1, 32, 5, 8, 9, 10, 11, 12, 13, -1, 0, 14);\n'
                   '    asw_sgbm_census(0, 0, 0, 0, 1, 32, 5, 8, 9, 10, 11, 12, 13, 0x10007, 0, 14);\n'
                   '    asw_sgbm_paths(0, 0, 0, 0, 1, 32, 5, 8, 9, 10, 63, 11, 12, 13, 0x37, 0, 14);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "enc"
    build_demo(src, exe, link=False, **C99)
    rows = [[int(v) for v in line.split()]
            for line in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()]
    head = [1, 32, 5, 8, 9, 10]
    both = asw._SGBM_MODE_PATHS | asw._SGBM_MODE_CENSUS
    assert rows == [head + [0, 11, 12, 13, both | 0x37, 14], head + [0, 11, 12, 13, both | 0x100, 14],
                    head + [0, 11, 12, 13, both | 0x100, 14], head + [0, 11, 12, 13, both | 0x100, 14],
                    head + [63, 11, 12, 13, asw._SGBM_MODE_PATHS | 0x37, 14]]


def test_python_mask_travel():
    assert "sgbm_census" in asw.__all__ and callable(asw.sgbm_census) and callable(asw.Context.sgbm_census)
    c = object.__new__(asw.Context)  # no device: only what sgbm_census hands to _sgbm_call is looked at
    c._h = None
    seen = []
    c._sgbm_call = lambda *a: seen.append(a)
    both = asw._SGBM_MODE_PATHS | asw._SGBM_MODE_CENSUS
    for paths, mask in ((0x07, 0x07), (0xFF, 0xFF), (0x30, 0x30), (0x100, 0x100), (0x1FF, 0x100), (-1, 0x100), (0x10007, 0x100)):
        c.sgbm_census("L", "R", 1, 32, 5, 8, 9, 10, 11, 12, 13, paths=paths, return_cost_volume=True)
        assert seen[-1] == ("asw_sgbm_census", "L", "R", 1, 32, 5, 8, 9, 10, 0, 11, 12, 13, both | mask, True), hex(paths)
    c.sgbm_census("L", "R", 0, 16, 3)
    assert seen[-1][-2] == both | 0xFF and seen[-1][-1] is False


def test_exported_set_is_unchanged():
    assert len(_lib.ABI_SYMBOLS) == 46 and len(set(_lib.ABI_SYMBOLS)) == 46
    assert not any("census" in n and "sgbm" in n for n in _lib.ABI_SYMBOLS)
    shim = open(os.path.join(ROOT, "include", "aswMethods_mi355x.hpp")).read()
    assert "getDisparity_SGBM_census(" in shim
