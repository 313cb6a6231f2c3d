"""computeAdaptiveWeight_twopass of the C++ surface (include/aswMethods_mi355x.hpp): tests/cpp/twopass_demo.cpp builds with plain
g++ on both Mat branches of the header, and -- on the GPU -- gives the ctypes path's map."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _build(exe, cv):
    from aswstereomatch_amd import build

    if not os.path.exists(build.LIB):
        build.build()
    cmd = ["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "twopass_demo.cpp"),
           "-L" + os.path.join(ROOT, "aswstereomatch_amd"), "-lasw_mi355x", "-Wl,-rpath," + os.path.join(ROOT, "aswstereomatch_amd"),
           "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    if cv:  # the cv::Mat branch against the compile-only stand-in for the OpenCV declarations the header names
        cmd[3:3] = ["-Wextra", "-DASW_WITH_OPENCV", "-I" + os.path.join(ROOT, "tests", "cpp", "cv_stub")]
    subprocess.check_call(cmd)
    return exe


@pytest.mark.parametrize("cv", [False, True])
def test_twopass_demo_compiles(tmp_path, cv):
    assert os.path.exists(_build(str(tmp_path / "twopass_demo"), cv))


@pytest.mark.gpu
@pytest.mark.parametrize("cv", [False, True])
def test_shim_twopass_matches_ctypes_path(tmp_path, cv):
    import aswstereomatch_amd as asw
    import twopass_ref as tp

    exe = _build(str(tmp_path / "twopass_demo"), cv)
    H, W, D = 37, 130, 17
    L, R = tp.textured_pair(H, W, 3, 5, 3)
    L.tofile(tmp_path / "l.raw")
    R.tofile(tmp_path / "r.raw")
    out = tmp_path / "d.raw"

    def run(right, gamma_c, gamma_g, win, minD):
        return subprocess.run([exe, str(H), str(W), "3", str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), str(right), str(gamma_c),
                               str(gamma_g), str(win), str(minD), str(D), str(out)], capture_output=True, text=True, timeout=120)

    ctx = asw.Context(0)
    try:
        for right, gamma_c, gamma_g, win, minD in ((0, 30, 20, 15, 0), (1, 7, 36, 7, 3), (0, 255, 1, 35, 0)):
            r = run(right, gamma_c, gamma_g, win, minD)
            assert r.returncode == 0 and r.stdout.strip() == "ok %d %d selector_same=1" % (H, W), (r.stdout, r.stderr)
            want = ctx.computeAdaptiveWeight_twopass(L, R, gamma_c, gamma_g, right, win, minD, D)
            assert np.array_equal(np.fromfile(out, np.float32).reshape(H, W), want)
            E, vol, disp = tp.twopass(ctx.bgr2gray(L), ctx.bgr2gray(R), gamma_c, gamma_g, win, minD, D, right)
            assert np.array_equal(want, disp)
        r = run(0, 30, 20, 14, 0)  # even window: an empty Mat, like the neighbours
        assert r.returncode == 0 and r.stdout.strip() == "empty", (r.stdout, r.stderr)
        for gamma_c, gamma_g, win in ((0, 20, 15), (30, 256, 15), (30, 20, 97)):
            r = run(0, gamma_c, gamma_g, win, 0)
            assert r.returncode == 0 and r.stdout.startswith("error"), (r.stdout, r.stderr)
    finally:
        ctx.close()
