"""CPU-side checks of the multi-path semi-global matcher's restatement (tests/sgbm_paths_ref.py): the
three-path mask reproduces tests/sgbm_ref.py, the vectorised and the scalar statement agree on every direction (on textured and on
tie-dense inputs), flipping the cost volume permutes the directions as it must, the whole pipeline commutes with turning the pair
upside down, and the tie-dense pairs of tests/matcher_cases.py still tie once the added directions are summed in (no GPU needed)."""
import os
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd.synth import make_pair

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matcher_cases as mc  # noqa: E402
import sgbm_paths_ref as pref  # noqa: E402
import sgbm_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASKS = [0x07] + [0x07 | b for b in pref.NEW_BITS] + [0xFF]


def _pair(H, W, cn, seed):
    L, R, _ = make_pair(H, W, 8, seed=seed, block=8)
    if cn == 1:
        return np.ascontiguousarray(L[:, :, 0]), np.ascontiguousarray(R[:, :, 0])
    return L, R


# three of the small cases of test_sgbm_cpu.py: H, W, cn, minD, D, block, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio
@pytest.mark.parametrize("H,W,cn,minD,D,w,P1,P2,M,cap,U", [
    (5, 37, 3, 0, 16, 3, 72, 288, 1, 10, 10),
    (6, 41, 1, 3, 16, 1, 8, 32, 0, 31, 5),
    (3, 50, 3, 1, 32, 3, 300, 100, 1, 10, 15),
])
def test_three_paths_equal_sgbm_ref(H, W, cn, minD, D, w, P1, P2, M, cap, U):
    L, R = _pair(H, W, cn, seed=H * W)
    want = ref.sgbm(L, R, minD, D, w, P1, P2, M, cap, U, 6, 1)
    got = pref.sgbm_paths(L, R, minD, D, w, P1, P2, M, cap, U, 6, 1, pref.PATHS_3WAY)
    for k in ("S", "raw", "med", "disp"):
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("paths", MASKS)
@pytest.mark.parametrize("H,W,cn,minD,D,w,P1,P2", [
    (6, 30, 3, 0, 16, 3, 72, 288),
    (13, 24, 1, 2, 16, 3, 10, 40),     # taller than the valid columns are wide (Wv = 6)
    (13, 24, 3, 2, 16, 1, 300, 100),   # P2 <= P1
    (1, 20, 1, 0, 16, 3, 8, 32),       # one row: every vertical and diagonal line has one pixel
])
def test_vectorised_equals_scalar(H, W, cn, minD, D, w, P1, P2, paths):
    L, R = _pair(H, W, cn, seed=H * W + cn)
    got = pref.sgbm_paths(L, R, minD, D, w, P1, P2, 1, 10, 10, 0, 0, paths)
    S, disp = pref.sgbm_paths_scalar(L, R, minD, D, w, P1, P2, 1, 10, 10, paths)
    assert np.array_equal(got["S"], np.array(S, np.int64))
    assert np.array_equal(got["raw"], np.array(disp, np.int16))


def test_named_masks_and_flips():
    assert (pref.PATHS_3WAY, pref.PATHS_HH4, pref.PATHS_SGBM, pref.PATHS_HH) == (0x07, 0x0F, 0x37, 0xFF)
    assert pref.PATHS_SGBM == pref.PATH_LR | pref.PATH_RL | pref.PATH_TB | pref.PATH_TLBR | pref.PATH_TRBL
    for m in range(256):
        assert pref.vflip(pref.vflip(m)) == m and pref.hflip(pref.hflip(m)) == m
        assert bin(pref.vflip(m)).count("1") == bin(m).count("1") == bin(pref.hflip(m)).count("1")
    assert pref.vflip(pref.PATH_TLBR) == pref.PATH_BLTR and pref.hflip(pref.PATH_TLBR) == pref.PATH_TRBL
    assert pref.vflip(pref.PATH_LR) == pref.PATH_LR and pref.hflip(pref.PATH_TB) == pref.PATH_TB


@pytest.mark.parametrize("shape", [(7, 5, 16), (5, 9, 16), (1, 6, 16), (6, 1, 16)])
def test_mirror_property(shape):
    # a diagonal walked from the wrong corner breaks this even where both statements share the mistake
    rng = np.random.default_rng(sum(shape))
    C = rng.integers(0, 200, size=shape).astype(np.int64)
    for m in [1 << i for i in range(8)] + [0x07, 0x37, 0x5A, 0xFF]:
        want = pref.aggregate_paths(C, 7, 30, m)
        assert np.array_equal(pref.aggregate_paths(C[::-1], 7, 30, pref.vflip(m))[::-1], want), hex(m)
        assert np.array_equal(pref.aggregate_paths(C[:, ::-1], 7, 30, pref.hflip(m))[:, ::-1], want), hex(m)
    # a single direction against a hand-walked line: the main diagonal of TLBR starts at (0, 0) with L = C
    L = pref.path(C, 7, 30, 1, 1)
    assert np.array_equal(L[0], C[0]) and np.array_equal(L[:, 0], C[:, 0])
    L = pref.path(C, 7, 30, -1, -1)
    assert np.array_equal(L[-1], C[-1]) and np.array_equal(L[:, -1], C[:, -1])


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("kind", mc.PATHS_FLIP_KINDS)
def test_whole_pipeline_commutes_with_a_vertical_flip(kind, cn):
    # Every stage is symmetric under y -> H-1-y (the prefilter's vertical taps 1 2 1, the block window, the 3x3 median, the
    # 4-connected speckle components; ties are broken along d and x only), and the directions permute by vflip.  For 0x0F this
    # ties PATH_BT to PATH_TB, which tests/test_sgbm_cpu.py pins through the three-path matcher.
    L, R = mc.paths_flip_pair(kind, cn)
    assert [0x07 | b for b in pref.NEW_BITS[1:]] == mc.PATHS_FLIP_MASKS[1:5]
    # with PATH_BT added to each mask as well: those are the masks whose flip the library serves (a superset of the three paths)
    for m in mc.PATHS_FLIP_MASKS + sorted({m | pref.PATH_BT for m in mc.PATHS_FLIP_MASKS} - set(mc.PATHS_FLIP_MASKS)):
        want = pref.sgbm_paths(L, R, *mc.paths_flip_args(cn), m)
        got = pref.sgbm_paths(L[::-1], R[::-1], *mc.paths_flip_args(cn), pref.vflip(m))
        assert np.array_equal(got["S"][::-1], want["S"]), hex(m)
        assert np.array_equal(got["disp"][::-1], want["disp"]), hex(m)
        invalid = float((want["disp"] == 0).mean())       # INVALID = 16 (minD - 1) = 0
        assert 0.2 < invalid < 0.8, (hex(m), invalid)     # neither all rejected nor nothing for steps 5-9 to do
        if pref.vflip(m) != m:                            # the unflipped mask on the flipped pair is another result
            assert not np.array_equal(pref.sgbm_paths(L[::-1], R[::-1], *mc.paths_flip_args(cn), m)["S"][::-1], want["S"]), hex(m)


TIE_H, TIE_W, TIE_D, TIE_BLOCK = 20, 150, 32, 5   # tests/test_matcher_cases_cpu.py


def paths_tie_shares(want, minD, D):
    """(tie share of S over the valid columns, share of the map that is not INVALID)"""
    return mc.tie_share(want["S"][:, minD + D:], 2), float((want["disp"] != 16 * (minD - 1)).mean())


@pytest.mark.parametrize("paths", [pref.PATHS_3WAY, pref.PATHS_HH4, pref.PATHS_SGBM, pref.PATHS_HH])
def test_tie_generators_tie_under_every_named_mask(paths):
    # the floors of test_matcher_cases_cpu.py::test_tie_generators_really_tie, with the added directions summed into S
    want = pref.sgbm_paths(*mc.periodic(TIE_H, TIE_W, 1, 4, 3), 0, TIE_D, TIE_BLOCK, 200, 800, -1, 10, 0, 0, 0, paths)
    ties, alive = paths_tie_shares(want, 0, TIE_D)
    print("paths 0x%02X periodic(4, 3): tie share %.3f, not-invalid share %.3f" % (paths, ties, alive))
    assert ties >= 0.5 and alive >= 0.5
    want = pref.sgbm_paths(*mc.constant(TIE_H, TIE_W, 1), 5, TIE_D, TIE_BLOCK, 200, 800, -1, 10, 0, 0, 0, paths)
    ties, _ = paths_tie_shares(want, 5, TIE_D)
    print("paths 0x%02X constant minD 5: tie share %.3f" % (paths, ties))
    assert ties >= 0.5
    assert (want["disp"][:, 5 + TIE_D:] == 16 * 5).all()   # the smallest disparity, whatever the directions


@pytest.mark.parametrize("paths", [pref.PATHS_HH4, pref.PATHS_SGBM, pref.PATHS_HH])
@pytest.mark.parametrize("kind,H,Wv,cn,minD", [
    ("constant", 4, 7, 1, 2), ("constant", 6, 3, 3, 5),      # at minD 0 a constant pair does not tie under SGBM
    ("periodic", 5, 10, 1, 0), ("periodic", 3, 9, 3, 1),
    ("quantised", 6, 10, 1, 0), ("quantised", 6, 8, 3, 3),
])
def test_scalar_equals_vectorised_on_tied_inputs(kind, H, Wv, cn, minD, paths):
    D = 16
    W = minD + D + Wv
    L, R = {"constant": lambda: mc.constant(H, W, cn), "periodic": lambda: mc.periodic(H, W, cn, 4, 3),
            "quantised": lambda: mc.quantised(H, W, cn, seed=H + Wv, D=D)}[kind]()
    got = pref.sgbm_paths(L, R, minD, D, 3, 20, 80, 1, 10, 10, 0, 0, paths)
    S, disp = pref.sgbm_paths_scalar(L, R, minD, D, 3, 20, 80, 1, 10, 10, paths)
    assert np.array_equal(got["S"], np.array(S, np.int64))
    assert np.array_equal(got["raw"], np.array(disp, np.int16))
    if kind != "quantised":   # plateaus, not exact ties everywhere
        assert mc.tie_share(got["S"][:, minD + D:], 2) >= 0.5


def test_named_masks_of_every_layer():
    assert (asw.SGBM_PATHS_3WAY, asw.SGBM_PATHS_HH4, asw.SGBM_PATHS_SGBM, asw.SGBM_PATHS_HH) == (0x07, 0x0F, 0x37, 0xFF)
    names = ("LR", "RL", "TB", "BT", "TLBR", "TRBL", "BRTL", "BLTR")
    assert [getattr(asw, "SGBM_PATH_" + n) for n in names] == [getattr(pref, "PATH_" + n) for n in names]
    hdr = open(os.path.join(ROOT, "include", "asw_mi355x.h")).read()
    for n in names:
        assert "ASW_SGBM_PATH_%s = 0x%02X," % (n, getattr(asw, "SGBM_PATH_" + n)) in hdr
