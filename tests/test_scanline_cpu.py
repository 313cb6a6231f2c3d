"""CPU-side checks of scanline optimisation: the flag's encoding against the header's inline function, the two
restatements of tests/scanline_ref.py against each other, the non-finite rules, the closed forms at both ends of the penalty range, and -- on
the oracle's classic, geodesic and GuidedF_2 volumes of one small pair -- that the encoded penalties the GPU tests use move every
entry and at least 1 % of the winners, which is what makes the comparisons of tests/test_gpu_scanline.py meaningful.  No GPU needed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib
from aswstereomatch_amd.synth import make_pair

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scanline_ref as sr  # noqa: E402
from shim_build import C99, build_demo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "asw_mi355x.h")
GRID = [(a, u, r) for a in range(-1, 131) for u in range(-1, 10) for r in range(0, 11)]


# ---------------------------------------------------------------- encoding
def _c_values(tmp_path):
    """asw_disparity_scanline as the header's inline function computes it, from a C99 program, over GRID in GRID's order"""
    src = tmp_path / "enc.c"
    src.write_text('#include <stdio.h>\n#include "asw_mi355x.h"\nint main(void) {\n    int a, u, r;\n'
                   '    printf("%d\\n", ASW_DISPARITY_SCANLINE);\n'
                   '    for (a = -1; a <= 130; a++) for (u = -1; u <= 9; u++) for (r = 0; r <= 10; r++)\n'
                   '        printf("%d\\n", asw_disparity_scanline(a, u, r));\n    return 0;\n}\n')
    exe = tmp_path / "enc"
    build_demo(src, exe, link=False, **C99)
    return [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split()]


def test_encoding_and_surface(tmp_path):
    v = sr.encode(100, 7, 8)
    assert v & sr.FLAG and (v >> 1) & 0x7F == 100 and (v >> 25) & 7 == 7 and (v >> 28) & 7 == 7 and 0 < v < 1 << 31
    assert v & 0x00FFFF01 == 0  # bits 0, 8..23 stay free for RIGHT, the sub-pixel flags and the cross-scale fields
    assert sr.encode(*sr.DEFAULT) == sr.FLAG | (8 << 1) | (5 << 25) | (3 << 28) == asw.scanline()
    for a, u, r in ((0, 5, 4), (128, 5, 4), (8, -1, 4), (8, 8, 4), (8, 5, 0), (8, 5, 9)):
        assert sr.encode(a, u, r) == sr.FLAG  # the a field 0: what the library refuses
    want = [sr.FLAG] + [sr.encode(*g) for g in GRID]
    assert _c_values(tmp_path) == want
    assert [asw.scanline(*g) for g in GRID] == want[1:]
    assert len({sr.encode(a, u, r) for a in range(1, 128) for u in range(8) for r in range(1, 9)}) == 127 * 8 * 8
    assert asw.SCANLINE == sr.FLAG == 0x01000000
    for name in ("scanline", "SCANLINE", "scanline_penalties"):
        assert name in asw.__all__
    text = open(HEADER).read()
    assert re.search(r"ASW_DISPARITY_SCANLINE\s*=\s*0x01000000\b", text)
    assert re.search(r"^static inline int asw_disparity_scanline\(int p1_code, int unit_code, int p2_ratio\)", text, re.M)
    shim = open(os.path.join(ROOT, "include", "aswMethods_mi355x.hpp")).read()
    assert "stereoMatchingScanline(" in shim


def test_penalties():
    assert sr.penalties(*sr.DEFAULT) == (np.float32(8), np.float32(32)) == asw.scanline_penalties(asw.scanline())
    assert sr.penalties(1, 0, 1) == (np.float32(1 / 1024), np.float32(1 / 1024))
    assert sr.penalties(127, 7, 8) == (np.float32(127 * 16), np.float32(8 * 127 * 16))
    for a in (1, 3, 127):
        for u in range(8):
            for r in (1, 5, 8):
                p = asw.scanline_penalties(asw.scanline(a, u, r))
                assert p == sr.penalties(a, u, r) and all(isinstance(v, np.float32) for v in p)


def test_both_keywords_are_refused_before_the_library():
    with pytest.raises(asw.AswError) as e:
        asw.stereoMatchingBatch([], [], 0, 2, cross_scale=asw.cross_scale(), scanline=asw.scanline())
    assert e.value.status == asw.ERR_BAD_ARGUMENT and asw.last_status() == asw.ERR_BAD_ARGUMENT


def test_abi_is_unchanged():
    assert len(_lib.ABI_SYMBOLS) == 46 and not any("scanline" in n for n in _lib.ABI_SYMBOLS)


# ---------------------------------------------------------------- the two restatements
@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (7, 1), (3, 5)])
@pytest.mark.parametrize("n", [1, 2, 3, 9])
def test_restatements_agree(H, W, n):
    rng = np.random.default_rng(H * 1000 + W * 10 + n)
    V = (rng.random((n, H, W)) * 50).astype(np.float32)
    for code in ((8, 5, 4), (1, 0, 1), (127, 7, 8), (3, 4, 2)):
        P1, P2 = sr.penalties(*code)
        a, b = sr.optimise(V, P1, P2), sr.optimise_literal(V, P1, P2)
        assert a.dtype == np.float32 and a.shape == V.shape and np.array_equal(a, b)
    if H * W == 1:  # no predecessor anywhere: four starts
        assert np.array_equal(a, ((V + V) + V) + V)


def test_one_step_by_hand():
    """two pixels in a row, three candidates, P1 = 1, P2 = 4: every statement written out"""
    V = np.array([[[5, 1]], [[2, 1]], [[9, 1]]], np.float32)  # [k][0][x]
    f = np.float32
    # LR at x = 1 from q = x 0 (5, 2, 9; minq 2): m = min(5, 3, -, 6) = 3; min(2, 6, 10, 6) = 2; min(9, 3, -, 6) = 3
    lr1 = [f(1) + (f(3) - f(2)), f(1) + (f(2) - f(2)), f(1) + (f(3) - f(2))]
    # RL at x = 0 from q = x 1 (1, 1, 1; minq 1): m = min(1, 2, 5) = 1 everywhere
    rl0 = [f(5), f(2), f(9)]
    out = sr.optimise(V, 1, 4)
    for k in range(3):
        assert out[k, 0, 1] == ((lr1[k] + V[k, 0, 1]) + V[k, 0, 1]) + V[k, 0, 1]  # RL starts at x = 1; TB and BT start everywhere (H = 1)
        assert out[k, 0, 0] == ((V[k, 0, 0] + rl0[k]) + V[k, 0, 0]) + V[k, 0, 0]
    assert sr.wta(out, 3).tolist() == [[4.0, 4.0]]


# ---------------------------------------------------------------- non-finite costs
def test_non_finite_rules():
    rng = np.random.default_rng(3)
    V = (rng.random((5, 6, 7)) * 50).astype(np.float32)
    V[2, :, 5] = -np.inf     # a column of one plane
    V[:, 2, 3] = np.nan      # a pixel without a finite candidate
    V[:, 4, :] = np.nan      # a row of them
    V[1, 0, 0] = np.inf
    V[3, 1, 1] = np.nan      # one entry of a pixel that keeps finite ones
    P1, P2 = sr.penalties(*sr.DEFAULT)
    out = sr.optimise(V, P1, P2)
    assert np.array_equal(out, sr.optimise_literal(V, P1, P2), equal_nan=True)
    bad = ~np.isfinite(V)
    assert np.array_equal(out[bad], V[bad], equal_nan=True)  # non-finite entries stay where and what they were
    assert np.isfinite(out[~bad]).all()                       # and no new one appears
    # the paths restart behind a pixel without a finite candidate: row 5 below the NaN row is the volume of rows 5.. on their own for
    # the TB path, so the whole frame equals two frames optimised apart in the vertical direction -- checked through the literal loop
    # above; here, the direct consequence for a frame that is ONE row under a NaN row:
    two = np.stack([V[:, 4, :], V[:, 5, :]], axis=1)
    alone = V[:, 5:6, :]
    assert np.array_equal(sr.optimise(two, P1, P2)[:, 1], sr.optimise(alone, P1, P2)[:, 0], equal_nan=True)
    # -inf wins the map as in k_wta, NaN and +inf never do, a pixel without a winner is 0
    d = sr.wta(out, 2)
    assert (d[:, 5][np.arange(6) != 4] == 4.0).all() and (d[4] == 0.0).all() and d[2, 3] == 0.0


def test_all_nan_volume_is_returned_unchanged():
    V = np.full((4, 3, 5), np.nan, np.float32)
    for fn in (sr.optimise, sr.optimise_literal):
        out = fn(V, 8, 32)
        assert out.dtype == np.float32 and np.isnan(out).all()
    assert (sr.wta(sr.optimise(V, 8, 32), 3) == 0).all()
    V = np.full((2, 2, 2), np.inf, np.float32)
    assert np.array_equal(sr.optimise(V, 8, 32), V)


# ---------------------------------------------------------------- sanity identities at the ends of the penalty range
def _accumulate(V):
    """the rule without its three transitions: L(p,k) = c(p,k) + (L(q,k) - minq), four paths summed in the rule's order"""
    n, H, W = V.shape
    S = None
    for axis, back in ((2, False), (2, True), (1, False), (1, True)):
        cm = np.moveaxis(V, axis, 0)
        L = np.empty_like(cm)
        order = list(range(cm.shape[0]))[::-1] if back else list(range(cm.shape[0]))
        for i, t in enumerate(order):
            L[t] = cm[t] if i == 0 else cm[t] + (L[order[i - 1]] - L[order[i - 1]].min(axis=0)[None])
        L = np.moveaxis(L, 0, axis)
        S = L if S is None else S + L
    return S


def test_largest_penalties_leave_only_the_straight_transition():
    """The feature's proposal expected the map at the largest penalties to equal that of the summed path starts (4 c).  It does
    not: with P1 = P2 = 127 * 16 against costs in [0, 1], t1, t2 and t3 exceed t0 at every step (t0 - minq stays below the
    path length), so m = t0 and L(p,k) = c(p,k) + (L(q,k) - minq) -- each candidate accumulates its own costs along the path, the
    fronto-parallel limit, not the unregularised one.  That closed form is asserted instead, exactly (multiples of 1/64: every sum
    is exact), and that its map is NOT the starts' map."""
    rng = np.random.default_rng(11)
    V = (np.round(rng.random((9, 8, 12)) * 64) / 64).astype(np.float32)
    P1, P2 = sr.penalties(127, 7, 1)
    assert P1 == P2 == np.float32(2032)
    out = sr.optimise(V, P1, P2)
    assert np.array_equal(out, _accumulate(V))
    assert np.array_equal(out, sr.optimise_literal(V, P1, P2))
    assert (sr.wta(out, 0) != sr.wta(sr.starts_sum(V), 0)).mean() > 0.2


def test_smallest_penalties_relative_to_the_volume_give_the_map_of_the_starts():
    """P1 = P2 = 1 / 1024 against costs that are distinct multiples of 1024 in every pixel: 0 <= m - minq <= P2, so every L is its c
    plus at most 1 / 1024 and the sum of the four paths is 4 c plus at most 4 / 1024 -- far below the gaps between candidates: the map
    is that of the per-pixel sum of the four unregularised starts, while the volume is not that sum."""
    rng = np.random.default_rng(12)
    n, H, W = 9, 8, 12
    V = (rng.permuted(np.tile(np.arange(n)[:, None, None], (1, H, W)), axis=0) * 1024).astype(np.float32)
    P1, P2 = sr.penalties(1, 0, 1)
    out = sr.optimise(V, P1, P2)
    starts = sr.starts_sum(V)
    assert np.array_equal(starts, 4 * V) and not np.array_equal(out, starts)
    assert (np.abs(out.astype(np.float64) - starts) <= 4.0 / 1024).all()
    assert np.array_equal(sr.wta(out, 0), sr.wta(starts, 0))
    assert np.array_equal(sr.wta(out, 0), np.argmin(V, axis=0).astype(np.float32))


# ---------------------------------------------------------------- the GPU tests' penalties move the oracle's volumes
def test_encoded_penalties_move_the_oracles_volumes(oracle):
    L, R, _ = make_pair(24, 48, 12, seed=5)
    vols = {"classic": oracle.asw_classic(L, R, 30.0, 20.0, 0, 5, 0, 12, want_vol=True),
            "geodesic": oracle.asw_geodesic(L, R, 0, 5, 0, 12, want_vol=True),
            "guided2": oracle.asw_guided2(L, R, 0, 1e-6, 5, 0, 12, want_vol=True)}
    for name, (rc, d, v) in vols.items():
        assert rc == 0 and np.isfinite(v).all()
        P1, P2 = sr.penalties(*sr.CODES[name])
        out = sr.optimise(v, P1, P2)
        moved = float((sr.wta(out, 0) != sr.wta(v, 0)).mean())
        with np.errstate(invalid="ignore"):
            ties = ((out == out.min(axis=0)).sum(axis=0) >= 2).mean()
        print("%s: P1 %g P2 %g (sigma %.3g), winners moved %.4f, tied minima %.4f" % (name, P1, P2, v.std(), moved, ties))
        assert (out != v).all()  # every finite entry changes
        assert moved >= 0.01     # measured: classic 0.044, geodesic 0.050, guided2 0.032
        assert out.dtype == np.float32


def test_random_case_is_seeded_and_covers_its_ranges():
    a = [sr.random_case(np.random.default_rng(5)) for _ in range(2)]
    assert all(np.array_equal(a[0][k], a[1][k]) for k in a[0])
    rng = np.random.default_rng(1)
    cases = [sr.random_case(rng) for _ in range(300)]
    assert {c["method"] for c in cases} == set(sr.METHODS) and {c["u"] for c in cases} == set(range(8))
    assert {c["ratio"] for c in cases} == set(range(1, 9)) and {1, 8, 127} <= {c["a"] for c in cases}
    assert {c["dt"] for c in cases} == {0, 1} and {c["subpixel"] for c in cases} == {0, 0x100, 0x200}
    assert any(c["numD"] + c["extra"] > 64 for c in cases) and any(c["numD"] + c["extra"] == 64 for c in cases)
    assert any(c["L"].shape[0] == 1 for c in cases) and any(c["L"].shape[0] > 32 for c in cases)
    assert all(c["L"].shape[0] * c["L"].shape[1] <= 2600 for c in cases)
    assert all(sr.encode(c["a"], c["u"], c["ratio"]) != sr.FLAG for c in cases)
