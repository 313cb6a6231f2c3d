"""CPU-side checks of cross-based support-region aggregation (selector entry 12): the two independent
restatements of tests/cross_ref.py agree, hand-made cases with known answers, the ABI surface (asw_volume_planes, the header's
constants and inline functions, the Python names), and the vacuity conditions that keep the GPU parity tests of
tests/test_gpu_cross.py from passing on inputs that exercise nothing (no GPU needed)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib
from aswstereomatch_amd.synth import shifted_pair

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cross_ref as cr  # noqa: E402
from shim_build import C99, build_demo  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import asw_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "asw_mi355x.h")


def _ad(L, R, dt, minD, D):
    rc, e = O.compute_ad(L, R, dt, minD, D)
    assert rc == 0
    return e


def _box(e, L):
    """clipped box sums of e [D][H][W] and the box sizes, by plain loops"""
    D, H, W = e.shape
    S = np.zeros((D, H, W), np.int64)
    N = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            y0, y1, x0, x1 = max(0, y - L), min(H, y + L + 1), max(0, x - L), min(W, x + L + 1)
            S[:, y, x] = e[:, y0:y1, x0:x1].sum(axis=(1, 2))
            N[y, x] = (y1 - y0) * (x1 - x0)
    return S, N


# ---------------------------------------------------------------- the two forms agree
# H, W, channels, seed, cell, amp, tau, trunc, win, direction, minD, D
SMALL = [
    (1, 1, 3, 1, (3, 3), 0.1, 20, 20, 3, 0, 0, 1),
    (1, 23, 3, 2, (3, 5), 0.1, 20, 20, 7, 0, 0, 5),
    (19, 1, 3, 3, (4, 3), 0.1, 20, 20, 7, 1, 0, 4),
    (3, 5, 3, 4, (2, 2), 0.2, 20, 20, 15, 0, 3, 5),      # a window larger than the frame, candidates past the image
    (12, 21, 3, 5, (5, 7), 0.12, 20, 20, 7, 0, 0, 6),
    (12, 21, 3, 5, (5, 7), 0.12, 20, 20, 7, 1, 3, 6),
    (11, 26, 1, 6, (5, 7), 0.12, 20, 5, 15, 0, 0, 5),    # 1-channel
    (11, 26, 1, 6, (5, 7), 0.12, 0, 255, 5, 1, 0, 5),
    (14, 30, 3, 7, (6, 9), 0.1, 255, 1, 35, 0, 0, 4),
    (9, 17, 3, 8, (4, 6), 0.3, 8, 20, 1, 0, 0, 17),      # win 1: every region is its pixel; min_d + num_d = cols
]


def _small_pair(H, W, cn, seed, cell, amp, D):
    L, R, _ = cr.region_pair(H, W, max(2, D), seed, cell, amp, block=8)
    if cn == 1:
        return np.ascontiguousarray(L[:, :, 1]), np.ascontiguousarray(R[:, :, 1])
    return L, R


@pytest.mark.parametrize("H,W,cn,seed,cell,amp,tau,trunc,win,dt,minD,D", SMALL)
def test_literal_and_integral_forms_agree(H, W, cn, seed, cell, amp, tau, trunc, win, dt, minD, D):
    L, R = _small_pair(H, W, cn, seed, cell, amp, D)
    view = R if dt else L
    a = cr.arms(view, tau, win // 2)
    assert np.array_equal(a, cr.arms_loop(view, tau, win // 2))
    assert a.min() >= 0 and a.max() <= win // 2
    e = _ad(L, R, dt, minD, D)
    one, two = cr.aggregate(e, a, trunc, minD), cr.aggregate_loop(e, a, trunc, minD)
    for x, y in zip(one, two):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    S, N, E, disp = one
    assert E.dtype == np.float32 and disp.dtype == np.float32 and E.shape == (D, H, W)
    assert N.min() >= 1 and N.max() <= win * win and S.max() <= trunc * win * win
    assert disp.min() >= minD and disp.max() <= minD + D - 1
    # the f32 division equals the f64 division rounded to f32 (operands below 2^24)
    assert np.array_equal(E, (S.astype(np.float64) / N.astype(np.float64)[None]).astype(np.float32))


def test_rows_subset_of_the_literal_form():
    L, R = _small_pair(12, 21, 3, 5, (5, 7), 0.12, 6)
    a, e = cr.arms(L, 20, 3), _ad(L, R, 0, 0, 6)
    full, part = cr.aggregate_loop(e, a, 20), cr.aggregate_loop(e, a, 20, rows=[0, 5, 11])
    for x, y in zip(full, part):
        assert np.array_equal(x[..., [0, 5, 11], :], y[..., [0, 5, 11], :])


# ---------------------------------------------------------------- hand-made cases
def test_constant_image_gives_clipped_boxes():
    H, W, D, Lc = 9, 14, 4, 3
    img = np.full((H, W, 3), 77, np.uint8)
    a = cr.arms(img, 0, Lc)
    ys, xs = np.mgrid[0:H, 0:W]
    assert np.array_equal(a[0], np.minimum(Lc, xs)) and np.array_equal(a[1], np.minimum(Lc, W - 1 - xs))
    assert np.array_equal(a[2], np.minimum(Lc, ys)) and np.array_equal(a[3], np.minimum(Lc, H - 1 - ys))
    e = np.random.default_rng(1).integers(0, 256, size=(D, H, W)).astype(np.uint8)
    S, N, E, disp = cr.aggregate(e, a, 40)
    assert np.array_equal(N, (a[0] + a[1] + 1) * (a[2] + a[3] + 1))
    bs, bn = _box(np.minimum(e.astype(np.int64), 40), Lc)
    assert np.array_equal(S, bs) and np.array_equal(N, bn)
    assert np.array_equal(E, bs.astype(np.float32) / bn.astype(np.float32)[None])


def test_vertical_step_edge_stops_the_horizontal_arms():
    H, W, Lc, c0 = 6, 20, 7, 11
    img = np.full((H, W), 50, np.uint8)
    img[:, c0:] = 200
    for form in (cr.arms, cr.arms_loop):
        a = form(img, 20, Lc)
        xs = np.broadcast_to(np.arange(W), (H, W))
        left_of = xs < c0
        assert np.array_equal(a[1][left_of], np.minimum(Lc, c0 - 1 - xs)[left_of])      # right arms end at the edge
        assert np.array_equal(a[0][~left_of], np.minimum(Lc, xs - c0)[~left_of])        # left arms too
        assert np.array_equal(a[0][left_of], np.minimum(Lc, xs)[left_of])
        assert np.array_equal(a[1][~left_of], np.minimum(Lc, W - 1 - xs)[~left_of])
        ys = np.broadcast_to(np.arange(H)[:, None], (H, W))
        assert np.array_equal(a[2], np.minimum(Lc, ys)) and np.array_equal(a[3], np.minimum(Lc, H - 1 - ys))
    # the anchor rule: a ramp of +15 per pixel passes a previous-pixel test everywhere, the anchor test only for one step
    ramp = (np.arange(12) * 15).astype(np.uint8)[None, :].repeat(3, axis=0)
    a = cr.arms(ramp, 20, 5)
    assert a[1][:, :-1].max() == 1 and a[0][:, 1:].max() == 1


def test_tau_255_is_a_box_filter():
    L, R = _small_pair(10, 18, 3, 11, (4, 5), 0.3, 5)
    e = _ad(L, R, 0, 0, 5)
    for form in (cr.aggregate, cr.aggregate_loop):
        S, N, E, disp = form(e, cr.arms(L, 255, 2), 30)
        bs, bn = _box(np.minimum(e.astype(np.int64), 30), 2)
        assert np.array_equal(S, bs) and np.array_equal(N, bn)


def test_tau_0_without_equal_neighbours_is_the_truncated_cost():
    H, W, D = 8, 15, 6
    ys, xs = np.mgrid[0:H, 0:W]
    L = np.stack([(3 * xs + 7 * ys) % 256, (5 * xs + 11 * ys + 9) % 256, (xs * 13 + ys) % 256], axis=2).astype(np.uint8)
    assert (L[:, 1:, 0] != L[:, :-1, 0]).all() and (L[1:, :, 0] != L[:-1, :, 0]).all()
    R = np.roll(L, -2, axis=1)
    a = cr.arms(L, 0, 7)
    assert a.max() == 0
    e = _ad(L, R, 0, 0, D)
    S, N, E, disp = cr.aggregate(e, a, 20)
    assert (N == 1).all() and np.array_equal(E, np.minimum(e, 20).astype(np.float32))


def test_shifted_pair_recovers_its_shift():
    L, R = shifted_pair(40, 64, 5)
    S, N, E, disp = cr.aggregate(_ad(L, R, 0, 0, 10), cr.arms(L, 20, 7), 20)
    assert (disp[8:-8, 16:-8] == 5).all()


# ---------------------------------------------------------------- vacuity conditions of the GPU cases, on the restatement alone
@pytest.mark.parametrize("H,W,D,cell,seed,amp,win", cr.REGION_CASES)
@pytest.mark.parametrize("dt", [0, 1])
def test_region_cases_exercise_every_arm_length_and_ties(H, W, D, cell, seed, amp, win, dt):
    L, R, _ = cr.region_pair(H, W, D, seed, cell, amp)
    a = cr.arms(R if dt else L, 20, win // 2)
    zero, between, full = cr.arm_shares(a, win // 2)
    S, N, E, disp = cr.aggregate(_ad(L, R, dt, 0, D), a, 20)
    ties = cr.tie_share(E)
    print("arms 0 / between / L: %.3f %.3f %.3f, ties %.3f" % (zero, between, full, ties))
    assert zero >= 0.03 and between >= 0.03 and full >= 0.03
    assert ties >= 0.01


# ---------------------------------------------------------------- ABI and Python surface
def _c_values(tmp_path):
    """asw_alg_cross as the header's inline function computes it, from a C99 program"""
    src = tmp_path / "alg.c"
    src.write_text('#include <stdio.h>\n#include "asw_mi355x.h"\nint main(void) {\n'
                   '    printf("%d %d %d %d %d %d %d %d\\n", asw_alg_cross(20, 20), asw_alg_cross(0, 255), asw_alg_cross(255, 1),\n'
                   '           asw_alg_cross(256, 1), asw_alg_cross(5, 0), asw_alg_cross(-1, 7), ASW_ALG_ADAPTIVE_WEIGHT_CROSS,\n'
                   '           ASW_ALG_CROSS_PARAMS);\n    return 0;\n}\n')
    exe = tmp_path / "alg"
    build_demo(src, exe, **C99)
    return [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split()]


def test_volume_planes_of_the_cross_entry():
    planes = _lib.lib().asw_volume_planes
    assert planes(12, 64) == 64
    assert planes(asw.cross_algorithm(20, 20), 64) == 64 and planes(asw.cross_algorithm(0, 255), 17) == 17
    assert planes(asw.cross_algorithm(255, 1), 5) == 5
    for bad in (asw.cross_algorithm(256, 1), asw.cross_algorithm(5, 0), asw.cross_algorithm(-1, 7), 0x40000000 | 12,  # trunc 0
                0x40141400 | 11, 0x40141400 | 2, 0x40000000, 0x42141400 | 12, 0x60141400 | 12, 0x40141400 | 12 | 0x01000000,
                (0x40141400 | 12) - (1 << 32) + (1 << 31)):  # bit 31
        assert planes(bad, 64) == 0, hex(bad)
    assert planes(99, 64) == 0 and planes(11, 64) == 64 and planes(2, 64) == 65 and planes(13, 64) == 0


def test_header_and_python_surface(tmp_path):
    assert asw.StereoMatchingAlgorithms.ADAPTIVE_WEIGHT_CROSS == 12
    for name in ("cross_algorithm", "computeAdaptiveWeight_cross"):
        assert name in asw.__all__ and callable(getattr(asw, name))
    assert callable(asw.Context.computeAdaptiveWeight_cross)
    text = open(HEADER).read()
    assert re.search(r"ASW_ALG_ADAPTIVE_WEIGHT_CROSS\s*=\s*12\b", text)
    assert re.search(r"ASW_ALG_CROSS_PARAMS\s*=\s*0x40000000\b", text)
    # inline functions keep `static inline` on the declaration line: not symbols, not seen by the ABI pattern
    assert re.search(r"^static inline int asw_alg_cross\(int tau, int trunc\)", text, re.M)
    assert re.search(r"^static inline int asw_aggregate_cross\(", text, re.M)
    assert not any(n.startswith("asw_alg_cross") or n == "asw_aggregate_cross" for n in _lib.ABI_SYMBOLS)
    c = _c_values(tmp_path)
    want = [asw.cross_algorithm(20, 20), asw.cross_algorithm(0, 255), asw.cross_algorithm(255, 1), asw.cross_algorithm(256, 1),
            asw.cross_algorithm(5, 0), asw.cross_algorithm(-1, 7), 12, 0x40000000]
    assert c == want
    v = asw.cross_algorithm(37, 201)
    assert v & 0xFF == 12 and (v >> 8) & 0xFF == 37 and (v >> 16) & 0xFF == 201 and v >> 24 == 0x40
    assert asw.cross_algorithm() == 0x40141400 | 12
    assert asw.cross_algorithm(256, 1) & 0x01000000 and asw.cross_algorithm(5, 0) & 0x01000000
    shim = open(os.path.join(ROOT, "include", "aswMethods_mi355x.hpp")).read()
    assert re.search(r"ADAPTIVE_WEIGHT_CROSS\s*=\s*12\b", shim) and "computeAdaptiveWeight_cross(" in shim
