"""CPU-side checks of cross-scale cost aggregation: the pieces of tests/cross_scale_ref.py against plain
loops and numpy's solver, the flag's encoding against the header's inline function, and -- on the oracle's classic volumes of one
small pair -- that every scale's term reaches the combined volume, which is what makes the comparisons of
tests/test_gpu_cross_scale.py meaningful.  No GPU needed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cross_scale_ref as cs  # noqa: E402
from shim_build import C99, build_demo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "asw_mi355x.h")
ARGS = [(S, q) for S in range(-1, 9) for q in (-1, 0, 1, 2, 19, 63, 64, 65, 127, 128, 254, 255, 256, 257, 511, 1000)]


# ---------------------------------------------------------------- encoding
def _c_values(tmp_path):
    """asw_disparity_cross_scale as the header's inline function computes it, from a C99 program, over ARGS and then every (S, q) with
    S in 0..7 and q in 0..300"""
    src = tmp_path / "enc.c"
    pairs = ", ".join("{%d, %d}" % a for a in ARGS)
    src.write_text('#include <stdio.h>\n#include "asw_mi355x.h"\nstatic const int args[][2] = {%s};\nint main(void) {\n'
                   '    int i, S, q;\n    printf("%%d\\n", ASW_DISPARITY_CROSS_SCALE);\n'
                   '    for (i = 0; i < %d; i++) printf("%%d\\n", asw_disparity_cross_scale(args[i][0], args[i][1]));\n'
                   '    for (S = 0; S < 8; S++) for (q = 0; q <= 300; q++) printf("%%d\\n", asw_disparity_cross_scale(S, q));\n'
                   '    return 0;\n}\n' % (pairs, len(ARGS)))
    exe = tmp_path / "enc"
    build_demo(src, exe, link=False, **C99)
    return [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split()]


def test_encoding_and_surface(tmp_path):
    v = cs.encode(4, 200)
    assert v & 0x1000 and (v >> 13) & 7 == 4 and (v >> 16) & 0xFF == 200 and v >> 24 == 0 and v & 0xFFF == 0
    assert cs.encode(3, 19) == 0x1000 | (3 << 13) | (19 << 16) == asw.cross_scale()
    for S, q in ((1, 19), (6, 19), (3, 0), (3, 256), (0, 0), (-1, -1)):
        assert (cs.encode(S, q) >> 13) & 7 == 0 and cs.encode(S, q) & 0x1000
    want = [0x1000] + [cs.encode(S, q) for S, q in ARGS] + [cs.encode(S, q) for S in range(8) for q in range(301)]
    assert _c_values(tmp_path) == want
    assert [asw.cross_scale(S, q) for S, q in ARGS] == [cs.encode(S, q) for S, q in ARGS]
    assert asw.CROSS_SCALE == cs.FLAG == 0x1000
    for name in ("cross_scale", "CROSS_SCALE"):
        assert name in asw.__all__
    text = open(HEADER).read()
    assert re.search(r"ASW_DISPARITY_CROSS_SCALE\s*=\s*0x1000\b", text)
    assert re.search(r"^static inline int asw_disparity_cross_scale\(int scales, int lambda_q\)", text, re.M)
    shim = open(os.path.join(ROOT, "include", "aswMethods_mi355x.hpp")).read()
    assert "stereoMatchingCrossScale(" in shim


def test_abi_is_unchanged():
    assert len(_lib.ABI_SYMBOLS) == 46 and not any("cross_scale" in n or "pyramid" in n for n in _lib.ABI_SYMBOLS)


# ---------------------------------------------------------------- weights
@pytest.mark.parametrize("S", [2, 3, 4, 5])
def test_weights(S):
    for q in (1, 2, 19, 63, 64, 65, 128, 255):
        w64, w = cs.weights64(S, q), cs.weights(S, q)
        assert w.dtype == np.float32 and w.shape == (S,)
        assert (w > 0).all() and (np.diff(w) < 0).all()
        ulp = float(np.spacing(np.float32(1.0)))
        assert abs(float(w.astype(np.float64).sum()) - 1.0) <= S * ulp
        e0 = np.zeros(S)
        e0[0] = 1.0
        assert np.abs(w64 - np.linalg.solve(cs.matrix(S, q), e0)).max() <= 1e-12
        assert np.array_equal(w, w64.astype(np.float32))


def test_weights_move_with_lambda():
    assert cs.weights(3, 19)[0] < cs.weights(3, 1)[0] < 1.0 and cs.weights(3, 255)[0] < cs.weights(3, 19)[0]
    assert not np.array_equal(cs.weights(3, 19), cs.weights(3, 20))


# ---------------------------------------------------------------- pyramid
def _down2_loop(img):
    H, W = img.shape[:2]
    out = np.zeros(((H + 1) // 2, (W + 1) // 2) + img.shape[2:], np.uint8)
    for Y in range(out.shape[0]):
        for X in range(out.shape[1]):
            s = 0
            for j in (0, 1):
                for i in (0, 1):
                    s = s + img[min(2 * Y + j, H - 1), min(2 * X + i, W - 1)].astype(np.int64)
            out[Y, X] = (s + 2) >> 2
    return out


@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (2, 1), (3, 3), (5, 8)])
@pytest.mark.parametrize("cn", [1, 3])
def test_down2(H, W, cn):
    rng = np.random.default_rng(H * 100 + W * 10 + cn)
    img = rng.integers(0, 256, (H, W) if cn == 1 else (H, W, 3)).astype(np.uint8)
    got = cs.down2(img)
    assert got.dtype == np.uint8 and got.shape[:2] == ((H + 1) // 2, (W + 1) // 2) and got.shape[2:] == img.shape[2:]
    assert np.array_equal(got, _down2_loop(img))
    top = np.full_like(img, 255)
    assert (cs.down2(top) == 255).all()  # no wrap in the 8-bit sum


def test_down2_rounds_half_up():
    assert cs.down2(np.array([[0, 1], [1, 0]], np.uint8))[0, 0] == 1 and cs.down2(np.array([[0, 1], [0, 0]], np.uint8))[0, 0] == 0
    assert cs.down2(np.array([[1, 2, 9]], np.uint8)).tolist() == [[2, 9]]


# ---------------------------------------------------------------- candidate ranges
def test_scale_ranges_against_brute_force():
    for minD in range(10):
        for n in range(1, 41):
            for S in range(2, 6):
                for extra in (0, 1):
                    if n - extra < 1:
                        continue
                    got = cs.scale_ranges(minD, n, extra, S)
                    sets = [sorted({d >> s for d in range(minD, minD + n)}) for s in range(S)]
                    if any(len(c) - extra < 1 for c in sets):
                        assert got is None
                        continue
                    for s, c in enumerate(sets):
                        assert c == list(range(c[0], c[0] + len(c)))  # contiguous
                        assert got[s] == (c[0], len(c), len(c) - extra)
                    assert got[0] == (minD, n, n - extra)


# ---------------------------------------------------------------- every scale reaches the combined volume
def test_every_scale_reaches_the_combined_volume(oracle):
    H, W, minD, numD, S, q = 20, 44, 3, 13, 4, 19
    L, R = cs.textured_pair(H, W, 3, 4, 7)
    ranges = cs.scale_ranges(minD, numD + 1, 1, S)
    vols = []
    for s, (Ls, Rs) in enumerate(zip(cs.pyramid(L, S), cs.pyramid(R, S))):
        rc, d, v = oracle.asw_classic(Ls, Rs, 30.0, 20.0, 0, 5, ranges[s][0], ranges[s][2], want_vol=True)
        assert rc == 0 and v.shape == (ranges[s][1],) + Ls.shape[:2]
        vols.append(v)
    w = cs.weights(S, q)
    out = cs.combine(vols, minD, w)
    assert out.dtype == np.float32 and out.shape == vols[0].shape and np.isfinite(out).all()
    assert (out != vols[0]).mean() >= 0.9
    for s in range(S):
        assert (cs.combine(vols, minD, w, drop=s) != out).mean() >= 0.9, s
    assert not np.array_equal(out, cs.combine(vols, minD, cs.weights(S, q + 1)))
    assert not np.array_equal(cs.wta(out, minD), cs.wta(vols[0], minD))  # and the map moves
    # the literal loop on a crop
    for k, y, x in ((0, 0, 0), (1, 5, 7), (6, 19, 43), (13, 10, 21)):
        acc = 0.0
        for s in range(S):
            acc += float(w[s]) * float(vols[s][((minD + k) >> s) - (minD >> s), y >> s, x >> s])
        assert out[k, y, x] == np.float32(acc)


def test_wta_rule():
    v = np.array([[[3, np.nan, np.inf, 2]], [[3, 1, np.inf, np.nan]], [[2, 1, np.inf, 2]]], np.float32)
    assert cs.wta(v, 4).tolist() == [[6.0, 5.0, 0.0, 4.0]]


def test_random_case_is_seeded_and_covers_its_ranges():
    a = [cs.random_case(np.random.default_rng(5)) for _ in range(2)]
    assert all(np.array_equal(a[0][k], a[1][k]) for k in a[0])
    rng = np.random.default_rng(1)
    cases = [cs.random_case(rng) for _ in range(200)]
    assert {c["method"] for c in cases} == set(cs.METHODS) and {c["S"] for c in cases} == {2, 3, 4, 5}
    assert {c["dt"] for c in cases} == {0, 1} and {c["subpixel"] for c in cases} == {0, 0x100, 0x200}
    assert {c["L"].shape[1] % 4 for c in cases} == {0, 1, 2, 3} and {1, 19, 64, 255} <= {c["q"] for c in cases}
    assert any(c["minD"] % 2 for c in cases) and any(c["L"].shape[0] == 1 for c in cases)
    assert all(c["L"].shape[0] * c["L"].shape[1] <= 2500 for c in cases)
    assert all(cs.scale_ranges(c["minD"], c["numD"] + c["extra"], c["extra"], c["S"]) is not None for c in cases)
