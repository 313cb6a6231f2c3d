"""CPU-side checks of the recursive (permeability) aggregation: the two forms of tests/permeability_ref.py
agree bit for bit, the identities of the definition, the conditions that keep the tie cases of tests/test_gpu_permeability.py from
passing on inputs that tie nowhere, and the selector encoding (the header's inline function, the Python name, asw_volume_planes, the
unchanged values of the other three encodings).  The AD volume is the oracle's.  No GPU needed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import permeability_ref as pm  # noqa: E402
from shim_build import C99, build_demo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import asw_oracle as O  # noqa: E402

HEADER = os.path.join(ROOT, "include", "asw_mi355x.h")
PA = asw.permeability_algorithm


def _ad(L, R, dt, minD, D):
    rc, e = O.compute_ad(L, R, dt, minD, D)
    assert rc == 0
    return e


def _both(fn, L, R, dt, sigma, trunc, minD, D):
    return fn(_ad(L, R, dt, minD, D), R if dt else L, sigma, trunc, minD)


# ---------------------------------------------------------------- the two forms agree
# H, W, channels, seed, minD, D, sigma, trunc
SMALL = [
    (6, 11, 1, 1, 0, 4, 8, 20),
    (6, 11, 3, 2, 0, 4, 1, 20),      # sigma 1: table entries that are exactly zero (barriers)
    (6, 11, 1, 3, 2, 3, 255, 20),
    (6, 11, 3, 4, 0, 12, 8, 1),      # trunc 1; candidates past the image
    (6, 11, 1, 5, 0, 4, 8, 255),
    (1, 1, 3, 6, 0, 2, 8, 20),
    (1, 9, 1, 7, 1, 3, 1, 255),
    (9, 1, 3, 8, 0, 2, 255, 1),
    (17, 19, 1, 9, 3, 4, 8, 20),
]


@pytest.mark.parametrize("H,W,cn,seed,minD,D,sigma,trunc", SMALL)
@pytest.mark.parametrize("dt", [pm.LEFT, pm.RIGHT])
def test_literal_and_vectorised_forms_agree(H, W, cn, seed, minD, D, sigma, trunc, dt):
    L, R = pm.textured_pair(H, W, cn, 2, seed)
    E, vol, disp, N = _both(pm.aggregate, L, R, dt, sigma, trunc, minD, D)
    E2, vol2, disp2, N2 = _both(pm.aggregate_loop, L, R, dt, sigma, trunc, minD, D)
    assert E.shape == (D, H, W) and E.dtype == np.float64 and vol.dtype == np.float32 and disp.dtype == np.float32
    assert np.array_equal(E, E2) and np.array_equal(vol, vol2) and np.array_equal(disp, disp2) and np.array_equal(N, N2)
    assert (N >= 1).all() and np.isfinite(N).all()
    # a weighted mean of costs in 0..trunc, up to the rounding of S and N: a few hundred operations of 2^-53 each
    assert np.isfinite(E).all() and (E >= 0).all() and (E <= trunc * (1 + 1e-12)).all()


def test_table():
    P = pm.table(8)
    assert P.shape == (256,) and P.dtype == np.float64 and P[0] == 1.0 and (np.diff(P) < 0).all()
    assert all(float(np.float32(v)) == v for v in P)  # every entry is an f32 value
    P1 = pm.table(1)
    assert P1[103] > 0 and (P1[104:] == 0).all()  # k > 103.28 sigma: exactly zero
    assert (pm.table(255) > 0.36).all()


def test_one_pixel_and_single_lines():
    for H, W in ((1, 1), (1, 9), (9, 1)):
        L, R = pm.textured_pair(H, W, 1, 1, 40 + H + W)
        e = _ad(L, R, 0, 0, 3)
        E, vol, disp, N = pm.aggregate(e, L, 8, 20, 0)
        if H == 1 and W == 1:
            assert N[0, 0] == 1.0 and np.array_equal(E[:, 0, 0], np.minimum(e[:, 0, 0], 20).astype(np.float64))


def test_permeability_1_is_the_mean_of_the_frame():
    """permeability 1 everywhere: S is the sum of e over the frame, N the pixel count"""
    L = np.full((5, 7), 9, np.uint8)
    e = np.random.default_rng(1).integers(0, 30, (3, 5, 7)).astype(np.uint8)
    E, vol, disp, N = pm.aggregate(e, L, 8, 20, 0)
    assert (N == 35).all()
    assert np.array_equal(E, np.broadcast_to(np.minimum(e, 20).sum(axis=(1, 2))[:, None, None] / 35.0, E.shape))


@pytest.mark.parametrize("cn,sigma,trunc", [(1, 8, 20), (3, 1, 255), (3, 255, 1)])
def test_right_is_the_mirrored_left(cn, sigma, trunc):
    L, R = pm.textured_pair(9, 31, cn, 4, 21)
    Er, vr, dr, Nr = _both(pm.aggregate, L, R, pm.RIGHT, sigma, trunc, 1, 6)
    Lm, Rm = np.ascontiguousarray(R[:, ::-1]), np.ascontiguousarray(L[:, ::-1])
    El, vl, dl, Nl = _both(pm.aggregate, Lm, Rm, pm.LEFT, sigma, trunc, 1, 6)
    assert np.array_equal(Er, El[:, :, ::-1]) and np.array_equal(vr, vl[:, :, ::-1]) and np.array_equal(Nr, Nl[:, ::-1])
    assert np.array_equal(dr, (np.argmin(Er, axis=0) + 1).astype(np.float32))
    assert not np.array_equal(Er, _both(pm.aggregate, L, R, pm.LEFT, sigma, trunc, 1, 6)[0])


def test_the_parameters_reach_the_volume():
    L, R = pm.textured_pair(12, 40, 1, 3, 31)
    base = _both(pm.aggregate, L, R, 0, 8, 20, 0, 5)[0]
    assert not np.array_equal(base, _both(pm.aggregate, L, R, 0, 9, 20, 0, 5)[0])
    assert not np.array_equal(base, _both(pm.aggregate, L, R, 0, 8, 21, 0, 5)[0])


# ---------------------------------------------------------------- the tie cases really tie
@pytest.mark.parametrize("cn", [1, 3])
def test_constant_and_row_constant_pairs_tie_everywhere(cn):
    for L, R in (pm.constant_pair(9, 70, cn), pm.row_constant_pair(11, 70, cn)):
        for dt in (pm.LEFT, pm.RIGHT):
            E, vol, disp, N = _both(pm.aggregate, L, R, dt, 8, 20, 3, 8)
            assert pm.tie_share(E) == 1.0 and (E == E[0]).all() and (disp == 3).all()


@pytest.mark.parametrize("cn", [1, 3])
def test_barrier_pair_ties(cn):
    L, R, D, sigma, trunc = pm.barrier_pair(cn)
    assert L.shape[:2] == (12, 160) and (D, sigma, trunc) == (24, 1, 60)
    E, vol, disp, N = _both(pm.aggregate, L, R, pm.LEFT, sigma, trunc, 0, D)
    share, block = pm.tie_share(E), pm.tie_share(E[:, :, 62:120])
    print("barrier pair, %d channel(s): tied share %.3f over the frame, %.3f in the block" % (cn, share, block))
    assert share >= 0.5
    blk = E[:, :, 62:120]
    assert (blk[5] == blk[13]).all() and (blk[5] == blk[21]).all() and (blk[5] == blk.min(axis=0)).all()
    assert (disp[:, 62:120] == 5).all()


def test_random_case_is_seeded_and_covers_its_ranges():
    a = [pm.random_case(np.random.default_rng(5)) for _ in range(2)]
    assert all(np.array_equal(a[0][k], a[1][k]) for k in a[0])
    rng = np.random.default_rng(6)
    cases = [pm.random_case(rng) for _ in range(200)]
    assert {c["dt"] for c in cases} == {0, 1} and {c["L"].ndim for c in cases} == {2, 3}
    assert {1, 8, 255} <= {c["sigma"] for c in cases} and {1, 20, 255} <= {c["trunc"] for c in cases}
    assert any(c["minD"] + c["D"] > c["L"].shape[1] for c in cases) and any(not c["L"].flags.c_contiguous for c in cases)
    assert all(1 <= c["sigma"] <= 255 and 1 <= c["trunc"] <= 255 for c in cases)
    assert pm.build_case(cases[3]["tag"])["L"].tobytes() == cases[3]["L"].tobytes()


# ---------------------------------------------------------------- encoding
def _c_values(tmp_path):
    """asw_alg_permeability as the header's inline function computes it, from a C99 program"""
    src = tmp_path / "alg.c"
    src.write_text('#include <stdio.h>\n#include "asw_mi355x.h"\nint main(void) {\n'
                   '    printf("%d %d %d %d %d %d %d %d %d\\n", asw_alg_permeability(8, 20), asw_alg_permeability(1, 1),\n'
                   '           asw_alg_permeability(255, 255), asw_alg_permeability(7, 36), asw_alg_permeability(0, 20),\n'
                   '           asw_alg_permeability(8, 0), asw_alg_permeability(256, 20), asw_alg_permeability(-1, 256),\n'
                   '           ASW_ALG_PERMEABILITY_PARAMS);\n    return 0;\n}\n')
    exe = tmp_path / "alg"
    build_demo(src, exe, **C99)
    return [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split()]


def test_encoding_and_surface(tmp_path):
    v = PA(37, 201)
    assert v & 0xFF == 12 and (v >> 8) & 0xFF == 37 and (v >> 16) & 0xFF == 201 and v >> 24 == 0x08
    assert PA() == 0x08000000 | (20 << 16) | (8 << 8) | 12
    for bad, s, t in ((PA(0, 20), 0, 20), (PA(256, 20), 0, 20), (PA(8, 0), 8, 0), (PA(8, 256), 8, 0), (PA(-1, -1), 0, 0)):
        assert bad == 0x08000000 | (t << 16) | (s << 8) | 12
    for name in ("permeability_algorithm", "computeAdaptiveWeight_permeability"):
        assert name in asw.__all__ and callable(getattr(asw, name))
    assert callable(asw.Context.computeAdaptiveWeight_permeability)
    text = open(HEADER).read()
    assert re.search(r"ASW_ALG_PERMEABILITY_PARAMS\s*=\s*0x08000000\b", text)
    assert re.search(r"^static inline int asw_alg_permeability\(int sigma, int trunc\)", text, re.M)
    assert re.search(r"^static inline int asw_aggregate_permeability\(", text, re.M)
    want = [PA(8, 20), PA(1, 1), PA(255, 255), PA(7, 36), PA(0, 20), PA(8, 0), PA(256, 20), PA(-1, 256), 0x08000000]
    assert _c_values(tmp_path) == want
    shim = open(os.path.join(ROOT, "include", "aswMethods_mi355x.hpp")).read()
    assert "computeAdaptiveWeight_permeability(" in shim


def test_abi_is_unchanged():
    assert len(_lib.ABI_SYMBOLS) == 46 and not any("permeab" in n for n in _lib.ABI_SYMBOLS)


def test_volume_planes():
    planes = _lib.lib().asw_volume_planes
    ok = PA(8, 20)
    assert planes(ok, 64) == 64 and planes(PA(1, 1), 17) == 17 and planes(PA(255, 255), 5) == 5
    for bad in (PA(0, 20), PA(8, 0), PA(256, 20), PA(8, 256),
                ok & ~(0xFF << 8), ok & ~(0xFF << 16), 0x08000000 | 12,        # a zero field
                ok | 0x01000000, ok | 0x02000000, ok | 0x04000000,             # bits 24..26
                ok - (1 << 32) + (1 << 31),                                    # bit 31
                (ok & ~0xFF) | 2, (ok & ~0xFF) | 11, (ok & ~0xFF) | 13, ok & ~0xFF):  # another low byte
        assert planes(bad, 64) == 0, hex(bad)


def test_unchanged_values():
    """bit 27 is read only with bits 28, 29 and 30 clear: it is lambda_ad's under bit 29 and a refused bit under bits 28 and 30"""
    planes = _lib.lib().asw_volume_planes
    assert [planes(a, 64) for a in range(14)] == [0, 0, 65, 65, 65, 65, 64, 64, 64, 64, 64, 64, 64, 0]
    x, ad, tp = asw.cross_algorithm(20, 20), asw.adcensus_algorithm(20, 10, 30), asw.twopass_algorithm(30, 20)
    assert x == 0x40000000 | (20 << 16) | (20 << 8) | 12 and planes(x, 64) == 64 and planes(x | 0x08000000, 64) == 0
    assert ad == 0x20000000 | (10 << 24) | (30 << 16) | (20 << 8) | 12 and ad & 0x08000000 and planes(ad, 64) == 64
    assert planes(asw.adcensus_algorithm(20, 2, 30), 64) == 64 and planes(asw.adcensus_algorithm(20, 8, 30), 7) == 7  # bit 27 clear / lambda_ad == bit 27
    assert tp == 0x10000000 | (20 << 16) | (30 << 8) | 2 and planes(tp, 64) == 65 and planes(tp | 0x08000000, 64) == 0
    assert planes(PA(8, 20) | 0x10000000, 64) == 0 and planes(PA(8, 20) | 0x40000000, 64) == 0  # read as two-pass (low byte 12) / cross (bit 27 refused)
