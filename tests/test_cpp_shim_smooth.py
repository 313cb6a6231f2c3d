"""smoothDisparity and stereoMatchingSmoothed of the C++ surface (include/aswMethods_mi355x.hpp): tests/cpp/smooth_demo.cpp builds with
plain g++ on both Mat branches of the header, and -- on the GPU -- both give the map of the ctypes path, which is the restatement's,
and throw where the library refuses."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scanline_ref as sr  # noqa: E402
import smooth_ref as sm  # noqa: E402
from shim_build import build_demo  # noqa: E402

pytestmark = pytest.mark.parametrize("cv", [False, True])


def test_smooth_demo_compiles(tmp_path, cv):
    assert os.path.exists(build_demo("smooth_demo.cpp", tmp_path / "smooth_demo", cv))


@pytest.mark.gpu
def test_shim_matches_ctypes_path(tmp_path, cv):
    import aswstereomatch_amd as asw

    exe = build_demo("smooth_demo.cpp", tmp_path / "smooth_demo", cv)
    H, W, D = 23, 70, 13
    L, R = sr.textured_pair(H, W, 3, 4, 5)
    L.tofile(tmp_path / "l.raw")
    R.tofile(tmp_path / "r.raw")

    def run(alg, win, minD, sigma_c, lam, T):
        argv = [exe, H, W, 3, tmp_path / "l.raw", tmp_path / "r.raw", int(alg), win, minD, D, repr(float(sigma_c)), repr(float(lam)), T,
                tmp_path / "one.raw", tmp_path / "two.raw"]
        return subprocess.run([str(x) for x in argv], capture_output=True, text=True, timeout=120)

    ctx = asw.Context(0)
    try:
        # classic, and two methods without a DISPARITY_RIGHT branch
        for alg, win, minD, sigma_c, lam, T in ((2, 5, 0, 8.0, 900.0, 3), (3, 5, 0, 12.5, 40.0, 1), (8, 5, 0, 30.0, 2.0, 8)):
            d, c = ctx.stereoMatching(L, R, 0, alg, win, minD, D, return_confidence=True)
            want = ctx.smoothDisparity(L, d, c, sigma_c, lam, T)
            assert sm.same_bits(want, sm.smooth_vec(L, d, c, sigma_c, lam, T)) and not sm.same_bits(want, d)
            r = run(alg, win, minD, sigma_c, lam, T)
            assert r.returncode == 0 and r.stdout.strip() == "ok %d %d" % (H, W), (r.stdout, r.stderr)
            assert sm.same_bits(np.fromfile(tmp_path / "one.raw", np.float32).reshape(H, W), want)
            assert sm.same_bits(np.fromfile(tmp_path / "two.raw", np.float32).reshape(H, W), want)
        # the throwing rows: SGBM and NCC (no confidence), iterations and parameters out of range
        for alg, sigma_c, lam, T in ((1, 8.0, 900.0, 3), (11, 8.0, 900.0, 3), (2, 8.0, 900.0, 0), (2, 8.0, 900.0, 9), (2, 0.0, 900.0, 3),
                                     (2, 8.0, -1.0, 3)):
            r = run(alg, 5, 0, sigma_c, lam, T)
            assert r.returncode == 0 and r.stdout.startswith("error"), (r.stdout, r.stderr)
        r = run(2, 4, 0, 8.0, 900.0, 3)  # an even window: the silent return, an empty Mat
        assert r.returncode == 0 and r.stdout.strip() == "empty", (r.stdout, r.stderr)
    finally:
        ctx.close()
