"""CPU-side checks of the two-pass (separable) adaptive-support-weight aggregation: the two forms of
tests/twopass_ref.py agree bit for bit, the identities of the definition, the conditions that keep the tie-dense GPU cases of
tests/test_gpu_twopass.py from passing on inputs that tie nowhere, and the selector encoding (the header's inline function, the
Python name, asw_volume_planes, the unchanged values).  No GPU needed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import twopass_ref as tp  # noqa: E402
from shim_build import C99, build_demo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "asw_mi355x.h")


# ---------------------------------------------------------------- the two forms agree
# H, W, seed, win, minD, numD, gammas
SMALL = [
    (6, 11, 1, 3, 0, 4, (30, 20)),
    (6, 11, 2, 5, 0, 4, (1, 1)),        # table entries that are zero or denormal
    (6, 11, 3, 7, 2, 3, (255, 255)),
    (6, 11, 4, 7, 0, 12, (7, 36)),      # candidates past the image
    (1, 1, 5, 3, 0, 2, (30, 20)),
    (1, 9, 6, 5, 1, 3, (1, 1)),
    (9, 1, 7, 5, 0, 2, (30, 20)),
    (3, 5, 8, 15, 3, 4, (30, 20)),      # a window larger than the frame
]


@pytest.mark.parametrize("H,W,seed,win,minD,numD,gammas", SMALL)
@pytest.mark.parametrize("dt", [tp.LEFT, tp.RIGHT])
def test_literal_and_vectorised_forms_agree(H, W, seed, win, minD, numD, gammas, dt):
    L, R = tp.textured_pair(H, W, 1, 2, seed)
    E, vol, disp = tp.twopass(L, R, gammas[0], gammas[1], win, minD, numD, dt)
    E2, vol2, disp2 = tp.twopass_loop(L, R, gammas[0], gammas[1], win, minD, numD, dt)
    assert E.shape == (numD + 1, H, W) and E.dtype == np.float64 and vol.dtype == np.float32 and disp.dtype == np.float32
    assert np.array_equal(E, E2) and np.array_equal(vol, vol2) and np.array_equal(disp, disp2)
    assert np.isfinite(E).all() and (E >= 0).all() and (E <= 255).all()


def test_table():
    T = tp.table(30, 20, 15)
    assert T.shape == (8, 256) and T.dtype == np.float32 and T[0, 0] == 1.0
    assert (np.diff(T, axis=1) < 0).all() and (np.diff(T, axis=0) < 0).all()
    T1 = tp.table(1, 1, 35)
    tiny = np.finfo(np.float32).tiny
    assert (T1 == 0).any() and ((T1 > 0) & (T1 < tiny)).any()  # zero and denormal entries: gammas (1, 1) meet both


def test_win_1_is_the_absolute_difference():
    L, R = tp.textured_pair(7, 23, 1, 3, 11)
    for dt in (tp.LEFT, tp.RIGHT):
        E, vol, disp = tp.twopass(L, R, 30, 20, 1, 2, 6, dt)
        a, b = (R[:, ::-1], L[:, ::-1]) if dt else (L, R)
        X = np.arange(23)
        want = np.stack([np.abs(a.astype(np.int32) - b[:, np.maximum(0, X - d)].astype(np.int32)) for d in range(2, 9)])
        if dt:
            want = want[:, :, ::-1]
        assert np.array_equal(E, want.astype(np.float64)) and np.array_equal(vol, want.astype(np.float32))


@pytest.mark.parametrize("win,gammas", [(5, (30, 20)), (15, (7, 36))])
def test_right_is_the_mirrored_left(win, gammas):
    L, R = tp.textured_pair(9, 31, 1, 4, 21)
    Er, vr, dr = tp.twopass(L, R, gammas[0], gammas[1], win, 1, 6, tp.RIGHT)
    El, vl, dl = tp.twopass(np.ascontiguousarray(R[:, ::-1]), np.ascontiguousarray(L[:, ::-1]), gammas[0], gammas[1], win, 1, 6, tp.LEFT)
    assert np.array_equal(Er, El[:, :, ::-1]) and np.array_equal(vr, vl[:, :, ::-1])
    # the map is the first strict minimum of the mirrored-back volume
    assert np.array_equal(dr, (np.argmin(Er, axis=0) + 1).astype(np.float32))
    assert not np.array_equal(Er, tp.twopass(L, R, gammas[0], gammas[1], win, 1, 6, tp.LEFT)[0])


def test_the_gammas_and_the_window_reach_the_volume():
    L, R = tp.textured_pair(12, 40, 1, 3, 31)
    base = tp.twopass(L, R, 30, 20, 7, 0, 5)[0]
    assert not np.array_equal(base, tp.twopass(L, R, 31, 20, 7, 0, 5)[0])
    assert not np.array_equal(base, tp.twopass(L, R, 30, 21, 7, 0, 5)[0])
    assert not np.array_equal(base, tp.twopass(L, R, 30, 20, 9, 0, 5)[0])


def test_window_numbers_of_the_restated_layout():
    """the numbers tests/test_gpu_twopass.py takes from twopass_ref.kernel_lds, the Python copy of the kernel's layout: 95 is the
    last window whose layout fits 160 KB, 25 | 27 straddle the 64 KB opt-in, the sums take 50 KB at win 35.  This pins the copy, not
    the kernel: what ties the copy to Layout::total of k_twopass.hip is the GPU statuses test (window 95 served, 97 refused)."""
    assert tp.max_window() == 95 and tp.kernel_lds(95) == 162976 and tp.kernel_lds(97) > 160 * 1024
    assert tp.kernel_lds(25) <= 64 * 1024 < tp.kernel_lds(27)
    assert 4 * 8 * (64 + 34) * 16 == 50176
    text = open(os.path.join(ROOT, "aswstereomatch_amd", "csrc", "k_twopass.hip")).read()
    assert "int twopass_max_window()" in text and "#if" not in text


# ---------------------------------------------------------------- tie-dense inputs really tie
def test_tie_dense_inputs_tie():
    cases = tp.tie_cases()
    L, R, win, minD, numD = cases["periodic"]
    assert L.shape == (20, 150) and numD + 1 == 18 and win == 15
    for dt in (tp.LEFT, tp.RIGHT):
        E, vol, disp = tp.twopass(L, R, 30, 20, win, minD, numD, dt)
        share = tp.tie_share(E)
        print("periodic, direction %d: tied share %.3f" % (dt, share))
        assert share >= 0.5
        assert (disp == 5).mean() >= 0.5  # period 8, shift 3: candidates 5 and 13 tie, the first one wins
    L, R, win, minD, numD = cases["constant"]
    for dt in (tp.LEFT, tp.RIGHT):
        E, vol, disp = tp.twopass(L, R, 30, 20, win, minD, numD, dt)
        assert tp.tie_share(E) == 1.0 and not E.any() and (disp == minD).all()


def test_random_case_is_seeded_and_covers_its_ranges():
    a = [tp.random_case(np.random.default_rng(5)) for _ in range(2)]
    assert all(np.array_equal(a[0][k], a[1][k]) for k in a[0])
    rng = np.random.default_rng(6)
    cases = [tp.random_case(rng) for _ in range(200)]
    assert {c["dt"] for c in cases} == {0, 1} and {c["L"].ndim for c in cases} == {2, 3}
    assert {1, 15, 35} <= {c["win"] for c in cases} and any(c["minD"] + c["numD"] > c["L"].shape[1] for c in cases)
    assert all(1 <= c["gamma_c"] <= 255 and 1 <= c["gamma_g"] <= 255 and c["win"] % 2 == 1 for c in cases)


# ---------------------------------------------------------------- encoding
def _c_values(tmp_path):
    """asw_alg_twopass as the header's inline function computes it, from a C99 program"""
    src = tmp_path / "alg.c"
    src.write_text('#include <stdio.h>\n#include "asw_mi355x.h"\nint main(void) {\n'
                   '    printf("%d %d %d %d %d %d %d %d %d\\n", asw_alg_twopass(30, 20), asw_alg_twopass(1, 1),\n'
                   '           asw_alg_twopass(255, 255), asw_alg_twopass(7, 36), asw_alg_twopass(0, 20), asw_alg_twopass(30, 0),\n'
                   '           asw_alg_twopass(256, 20), asw_alg_twopass(-1, 256), ASW_ALG_TWOPASS_PARAMS);\n    return 0;\n}\n')
    exe = tmp_path / "alg"
    build_demo(src, exe, **C99)
    return [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split()]


def test_encoding_and_surface(tmp_path):
    v = asw.twopass_algorithm(37, 201)
    assert v & 0xFF == 2 and (v >> 8) & 0xFF == 37 and (v >> 16) & 0xFF == 201 and v >> 24 == 0x10
    assert asw.twopass_algorithm() == 0x10000000 | (20 << 16) | (30 << 8) | 2
    for bad, c, g in ((asw.twopass_algorithm(0, 20), 0, 20), (asw.twopass_algorithm(256, 20), 0, 20), (asw.twopass_algorithm(30, 0), 30, 0),
                      (asw.twopass_algorithm(30, 256), 30, 0), (asw.twopass_algorithm(-1, -1), 0, 0)):
        assert bad == 0x10000000 | (g << 16) | (c << 8) | 2
    for name in ("twopass_algorithm", "computeAdaptiveWeight_twopass"):
        assert name in asw.__all__ and callable(getattr(asw, name))
    assert callable(asw.Context.computeAdaptiveWeight_twopass)
    text = open(HEADER).read()
    assert re.search(r"ASW_ALG_TWOPASS_PARAMS\s*=\s*0x10000000\b", text)
    assert re.search(r"^static inline int asw_alg_twopass\(int gamma_c, int gamma_g\)", text, re.M)
    assert re.search(r"^static inline int asw_aggregate_twopass\(", text, re.M)
    want = [asw.twopass_algorithm(30, 20), asw.twopass_algorithm(1, 1), asw.twopass_algorithm(255, 255), asw.twopass_algorithm(7, 36),
            asw.twopass_algorithm(0, 20), asw.twopass_algorithm(30, 0), asw.twopass_algorithm(256, 20), asw.twopass_algorithm(-1, 256),
            0x10000000]
    assert _c_values(tmp_path) == want
    shim = open(os.path.join(ROOT, "include", "aswMethods_mi355x.hpp")).read()
    assert "computeAdaptiveWeight_twopass(" in shim


def test_abi_is_unchanged():
    assert len(_lib.ABI_SYMBOLS) == 46 and not any("twopass" in n for n in _lib.ABI_SYMBOLS)


def test_volume_planes():
    planes = _lib.lib().asw_volume_planes
    ok = asw.twopass_algorithm(30, 20)
    assert planes(ok, 64) == 65 and planes(asw.twopass_algorithm(1, 1), 17) == 18 and planes(asw.twopass_algorithm(255, 255), 5) == 6
    for bad in (asw.twopass_algorithm(0, 20), asw.twopass_algorithm(30, 0), asw.twopass_algorithm(256, 20), asw.twopass_algorithm(30, 256),
                ok & ~(0xFF << 8), ok & ~(0xFF << 16),                       # a zero field
                ok | 0x01000000, ok | 0x02000000, ok | 0x04000000, ok | 0x08000000,  # bits 24..27
                ok - (1 << 32) + (1 << 31),                                   # bit 31
                (ok & ~0xFF) | 3, (ok & ~0xFF) | 12, (ok & ~0xFF) | 13, ok & ~0xFF):  # another low byte
        assert planes(bad, 64) == 0, hex(bad)


def test_unchanged_values():
    planes = _lib.lib().asw_volume_planes
    assert [planes(a, 64) for a in range(14)] == [0, 0, 65, 65, 65, 65, 64, 64, 64, 64, 64, 64, 64, 0]
    assert planes(asw.cross_algorithm(20, 20), 64) == 64 and planes(asw.cross_algorithm(255, 1), 9) == 9
    assert planes(asw.cross_algorithm(20, 0), 64) == 0 and planes(asw.cross_algorithm(20, 20) | 0x10000000, 64) == 0  # bit 28 under bit 30
    ad = asw.adcensus_algorithm(20, 10, 30)
    assert planes(ad, 64) == 64 and planes(asw.adcensus_algorithm(0, 31, 255), 7) == 7  # lambda_ad 16..31 sets bit 28: still adcensus
    assert asw.adcensus_algorithm(0, 31, 255) & 0x10000000 and planes(asw.adcensus_algorithm(20, 17, 45), 64) == 64
    assert planes(asw.adcensus_algorithm(20, 0, 30), 64) == 0 and planes((ad & ~0xFF) | 2, 64) == 0
    assert asw.cross_algorithm(20, 20) == 0x40000000 | (20 << 16) | (20 << 8) | 12
    assert ad == 0x20000000 | (10 << 24) | (30 << 16) | (20 << 8) | 12
