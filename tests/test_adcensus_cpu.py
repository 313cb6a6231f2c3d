"""CPU-side checks of AD-Census matching: the two independent restatements of tests/adcensus_ref.py agree,
the properties a census cost is wanted for (gain / offset invariance, left-right symmetry), the margin that makes bit-equal tables
a fair demand, the vacuity conditions that keep the GPU parity tests of tests/test_gpu_adcensus.py from passing on inputs that
exercise nothing, and the selector encoding (the header's inline functions, the Python names, asw_volume_planes).  No GPU needed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adcensus_ref as ac  # noqa: E402
import cross_ref as cr  # noqa: E402
from shim_build import C99, build_demo  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import asw_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "asw_mi355x.h")

# every (lambda_ad, lambda_census) of tests/test_gpu_adcensus.py, and the values adcensus_ref.random_case draws from
GPU_LAMBDAS = [(10, 30), (31, 255), (1, 1), (5, 12), (17, 45)]
FUZZ_LAMBDA_AD, FUZZ_LAMBDA_CENSUS = (1, 5, 10, 17, 31), (1, 12, 30, 45, 255)


def _pair(H, W, cn, seed, D):
    L, R, _ = cr.region_pair(H, W, max(2, D), seed, (4, 6), 0.15, block=8)
    if cn == 1:
        return np.ascontiguousarray(L[:, :, 1]), np.ascontiguousarray(R[:, :, 1])
    return L, R


# ---------------------------------------------------------------- the two forms agree
# H, W, channels, seed, direction, minD, D, lambda_ad, lambda_census
SMALL = [
    (1, 1, 3, 1, 0, 0, 2, 10, 30),
    (1, 9, 1, 2, 1, 0, 3, 10, 30),
    (3, 5, 3, 3, 0, 3, 5, 10, 30),      # narrower and lower than the half-window, candidates past the image
    (9, 1, 1, 4, 1, 0, 2, 1, 1),
    (8, 13, 3, 5, 0, 0, 5, 10, 30),
    (8, 13, 3, 5, 1, 2, 5, 31, 255),
    (7, 12, 1, 6, 0, 0, 4, 5, 12),
    (7, 12, 1, 6, 1, 10, 4, 17, 45),    # min_d + num_d > cols: repeated reflection
]


@pytest.mark.parametrize("H,W,cn,seed,dt,minD,D,la,lc", SMALL)
def test_literal_and_vectorised_forms_agree(H, W, cn, seed, dt, minD, D, la, lc):
    L, R = _pair(H, W, cn, seed, D)
    gl, gr = ac.gray_pair(L, R)
    for g in (gl, gr):
        code = ac.census(g)
        assert code.dtype == np.uint64 and code.tolist() == ac.census_loop(g)
        assert not (code >> np.uint64(63)).any() and not ((code >> np.uint64(31)) & np.uint64(1)).any()  # 62 bits, the centre clear
    ham, adv, e = ac.cost_loop(L, R, dt, la, lc, minD, D)
    assert np.array_equal(ham, ac.hamming(L, R, dt, minD, D)) and ham.max() <= 62
    assert np.array_equal(adv, ac.ad(L, R, dt, minD, D))
    rc, want = O.compute_ad(L, R, dt, minD, D)  # the AD term is computeAD's, borders included
    assert rc == 0 and np.array_equal(adv, want)
    got = ac.cost(L, R, dt, la, lc, minD, D)
    assert got.dtype == np.uint8 and np.array_equal(e, got)
    ta, tc = ac.tables(la, lc)
    assert ta[0] == 0 and tc[0] == 0 and ta.max() <= 127 and tc.max() <= 127 and (np.diff(ta) >= 0).all() and (np.diff(tc) >= 0).all()


def test_gray_bits_reach_the_codes():
    L, R = _pair(12, 40, 3, 7, 4)
    assert not np.array_equal(ac.gray_pair(L, R, 14)[0], ac.gray_pair(L, R, 15)[0])
    assert not np.array_equal(ac.hamming(L, R, 0, 0, 4, 14), ac.hamming(L, R, 0, 0, 4, 15))


def test_flat_pair_has_code_zero():
    g = np.full((6, 11), 93, np.uint8)
    assert not ac.census(g).any()
    assert not ac.hamming(g, g + 1, 0, 0, 3).any()


# ---------------------------------------------------------------- what a census cost is for
def test_census_is_invariant_to_gain_and_offset():
    """G -> 2 G + 10 on one image of a gray pair (intensities <= 115: nothing saturates) keeps every comparison, so the Hamming
    volume is unchanged, while the AD volume is not"""
    L, R = _pair(14, 40, 1, 9, 6)
    L, R = (L // 3 + 20).astype(np.uint8), (R // 3 + 20).astype(np.uint8)
    assert L.max() <= 115 and R.max() <= 115
    R2 = (2 * R.astype(np.int64) + 10).astype(np.uint8)
    assert R2.max() <= 240
    for dt in (0, 1):
        h = ac.hamming(L, R, dt, 0, 6)
        assert h.max() > 20 and np.array_equal(h, ac.hamming(L, R2, dt, 0, 6))
        assert not np.array_equal(ac.ad(L, R, dt, 0, 6), ac.ad(L, R2, dt, 0, 6))


@pytest.mark.parametrize("cn", [1, 3])
def test_left_and_right_costs_are_symmetric(cn):
    """where both columns lie inside the image, the LEFT cost at (y, x, d) is the RIGHT cost at (y, x - d, d)"""
    D, minD = 7, 2
    L, R = _pair(10, 33, cn, 12, D)
    left, right = ac.cost(L, R, 0, 10, 30, minD, D), ac.cost(L, R, 1, 10, 30, minD, D)
    for k in range(D):
        d = minD + k
        assert np.array_equal(left[k][:, d:], right[k][:, :L.shape[1] - d])


# ---------------------------------------------------------------- tables
def test_table_margins():
    """host libm and numpy may differ in the last ulp of exp: no table entry of a lambda the GPU tests use lies that close to a
    rounding boundary"""
    pairs = GPU_LAMBDAS + [(a, c) for a in FUZZ_LAMBDA_AD for c in FUZZ_LAMBDA_CENSUS]
    for la, lc in pairs:
        ma, mc = ac.table_margin(la, 256), ac.table_margin(lc, 63)
        print("lambda_ad %d: %.2e, lambda_census %d: %.2e" % (la, ma, lc, mc))
        assert ma >= 1e-6 and mc >= 1e-6, (la, lc, ma, mc)


# ---------------------------------------------------------------- vacuity conditions of the GPU cases, on the restatement alone
@pytest.mark.parametrize("H,W,D,cell,seed,amp,win", cr.REGION_CASES)
@pytest.mark.parametrize("dt", [0, 1])
def test_region_cases_exercise_both_terms(H, W, D, cell, seed, amp, win, dt):
    L, R, _ = cr.region_pair(H, W, D, seed, cell, amp)
    ham = ac.hamming(L, R, dt, 0, D)
    e = ac.cost(L, R, dt, 10, 30, 0, D)
    disp = ac.match(L, R, dt, 20, 10, 30, win, 0, D, e=e)[3]
    ta, _ = ac.tables(10, 30)
    ad_only = ac.match(L, R, dt, 20, 10, 30, win, 0, D, e=ta[ac.ad(L, R, dt, 0, D)].astype(np.uint8))[3]
    moved = float((disp != ad_only).mean())
    print("hamming %d..%d, cost max %d, winner != AD-only winner on %.3f" % (ham.min(), ham.max(), e.max(), moved))
    assert ham.min() == 0 and ham.max() == 62
    assert e.max() > 127
    assert moved >= 0.05


# ---------------------------------------------------------------- encoding
def _c_values(tmp_path):
    """asw_alg_adcensus as the header's inline function computes it, from a C99 program"""
    src = tmp_path / "alg.c"
    src.write_text('#include <stdio.h>\n#include "asw_mi355x.h"\nint main(void) {\n'
                   '    printf("%d %d %d %d %d %d %d %d %d\\n", asw_alg_adcensus(20, 10, 30), asw_alg_adcensus(0, 1, 1),\n'
                   '           asw_alg_adcensus(255, 31, 255), asw_alg_adcensus(256, 10, 30), asw_alg_adcensus(20, 32, 30),\n'
                   '           asw_alg_adcensus(20, 0, 30), asw_alg_adcensus(20, 10, 0), asw_alg_adcensus(-1, 10, 256),\n'
                   '           ASW_ALG_ADCENSUS_PARAMS);\n    return 0;\n}\n')
    exe = tmp_path / "alg"
    build_demo(src, exe, **C99)
    return [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split()]


def test_encoding_and_surface(tmp_path):
    v = asw.adcensus_algorithm(37, 21, 201)
    assert v & 0xFF == 12 and (v >> 8) & 0xFF == 37 and (v >> 16) & 0xFF == 201 and (v >> 24) & 0x1F == 21
    assert v & 0x20000000 and not v & 0x40000000 and 0 < v < 1 << 31
    assert asw.adcensus_algorithm() == 0x20000000 | (10 << 24) | (30 << 16) | (20 << 8) | 12
    for bad in (asw.adcensus_algorithm(256, 10, 30), asw.adcensus_algorithm(-1, 10, 30), asw.adcensus_algorithm(20, 32, 30),
                asw.adcensus_algorithm(20, 0, 30), asw.adcensus_algorithm(20, 10, 0), asw.adcensus_algorithm(20, 10, 256)):
        assert bad & 0x20000000 and (bad >> 24) & 0x1F == 0 and bad & 0xFF == 12
    for name in ("adcensus_algorithm", "computeCensus", "computeADCensus", "computeAdaptiveWeight_adcensus"):
        assert name in asw.__all__ and callable(getattr(asw, name))
    for name in ("computeCensus", "computeADCensus", "computeAdaptiveWeight_adcensus"):
        assert callable(getattr(asw.Context, name))
    text = open(HEADER).read()
    assert re.search(r"ASW_ALG_ADCENSUS_PARAMS\s*=\s*0x20000000\b", text)
    assert re.search(r"^static inline int asw_alg_adcensus\(int tau, int lambda_ad, int lambda_census\)", text, re.M)
    assert re.search(r"^static inline int asw_aggregate_adcensus\(", text, re.M)
    # the two cost builders are inline too, over asw_cost_tad: the library's exported set does not grow
    assert re.search(r"ASW_COST_CENSUS_PARAMS\s*=\s*0x40000000\b", text)
    assert re.search(r"^static inline int asw_cost_census\(", text, re.M) and re.search(r"^static inline int asw_cost_adcensus\(", text, re.M)
    assert not any(n.startswith("asw_alg_") or n in ("asw_aggregate_adcensus", "asw_cost_census", "asw_cost_adcensus")
                   for n in _lib.ABI_SYMBOLS)
    want = [asw.adcensus_algorithm(20, 10, 30), asw.adcensus_algorithm(0, 1, 1), asw.adcensus_algorithm(255, 31, 255),
            asw.adcensus_algorithm(256, 10, 30), asw.adcensus_algorithm(20, 32, 30), asw.adcensus_algorithm(20, 0, 30),
            asw.adcensus_algorithm(20, 10, 0), asw.adcensus_algorithm(-1, 10, 256), 0x20000000]
    assert _c_values(tmp_path) == want
    shim = open(os.path.join(ROOT, "include", "aswMethods_mi355x.hpp")).read()
    assert "computeAdaptiveWeight_adcensus(" in shim


def test_volume_planes_of_the_encoded_values():
    planes = _lib.lib().asw_volume_planes
    ok = asw.adcensus_algorithm(20, 10, 30)
    assert planes(ok, 64) == 64 and planes(asw.adcensus_algorithm(0, 1, 1), 17) == 17 and planes(asw.adcensus_algorithm(255, 31, 255), 5) == 5
    for bad in (asw.adcensus_algorithm(256, 10, 30), asw.adcensus_algorithm(20, 32, 30), asw.adcensus_algorithm(20, 0, 30),
                asw.adcensus_algorithm(20, 10, 0), ok & ~(0x1F << 24), ok & ~(0xFF << 16),   # lambda fields 0
                (ok & ~0xFF) | 11, (ok & ~0xFF) | 13, (ok & ~0xFF) | 2, ok & ~0xFF,            # another low byte
                ok - (1 << 32) + (1 << 31),                                                      # bit 31
                ok | 0x40000000):                                                                # bit 30: decoded as asw_alg_cross, bits 24-29 set
        assert planes(bad, 64) == 0, hex(bad)
    # what existed is what it was
    assert [planes(a, 64) for a in range(12)] == [0, 0, 65, 65, 65, 65, 64, 64, 64, 64, 64, 64]
    assert planes(12, 64) == 64 and planes(13, 64) == 0 and planes(asw.cross_algorithm(20, 20), 64) == 64
