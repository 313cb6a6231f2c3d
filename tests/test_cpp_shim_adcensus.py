"""computeAdaptiveWeight_adcensus of the C++ surface (include/aswMethods_mi355x.hpp): tests/cpp/adcensus_demo.cpp builds with plain g++
on both Mat branches of the header, and -- on the GPU -- gives the ctypes path's map."""
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
    cmd = ["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "adcensus_demo.cpp"),
           "-L" + os.path.join(ROOT, "aswstereomatch_amd"), "-lasw_mi355x", "-Wl,-rpath," + os.path.join(ROOT, "aswstereomatch_amd"),
           "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    if cv:  # the cv::Mat branch against the compile-only stand-in for the OpenCV declarations the header names
        cmd[3:3] = ["-Wextra", "-DASW_WITH_OPENCV", "-I" + os.path.join(ROOT, "tests", "cpp", "cv_stub")]
    subprocess.check_call(cmd)
    return exe


@pytest.mark.parametrize("cv", [False, True])
def test_adcensus_demo_compiles(tmp_path, cv):
    assert os.path.exists(_build(str(tmp_path / "adcensus_demo"), cv))


@pytest.mark.gpu
@pytest.mark.parametrize("cv", [False, True])
def test_shim_adcensus_matches_ctypes_path(tmp_path, cv):
    import aswstereomatch_amd as asw
    import cross_ref as cr

    exe = _build(str(tmp_path / "adcensus_demo"), cv)
    H, W, D = 37, 130, 17
    L, R, _ = cr.region_pair(H, W, D, 3, (9, 13), 0.12)
    L.tofile(tmp_path / "l.raw")
    R.tofile(tmp_path / "r.raw")
    out = tmp_path / "d.raw"

    def run(right, tau, la, lc, win, minD):
        return subprocess.run([exe, str(H), str(W), "3", str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), str(right), str(tau),
                               str(la), str(lc), str(win), str(minD), str(D), str(out)], capture_output=True, text=True, timeout=120)

    ctx = asw.Context(0)
    try:
        for right, tau, la, lc, win, minD in ((0, 20, 10, 30, 15, 0), (1, 20, 10, 30, 7, 3), (0, 5, 17, 45, 15, 0)):
            r = run(right, tau, la, lc, win, minD)
            same = 1 if (tau, la, lc) == (20, 10, 30) else 0
            assert r.returncode == 0 and r.stdout.strip() == "ok %d %d selector_same=%d" % (H, W, same), (r.stdout, r.stderr)
            want = ctx.computeAdaptiveWeight_adcensus(L, R, right, tau, la, lc, win, minD, D)
            assert np.array_equal(np.fromfile(out, np.float32).reshape(H, W), want)
        r = run(0, 20, 10, 30, 14, 0)  # even window: an empty Mat, like the neighbours
        assert r.returncode == 0 and r.stdout.strip() == "empty", (r.stdout, r.stderr)
        for tau, la, lc, win in ((20, 0, 30, 15), (300, 10, 30, 15), (20, 32, 30, 15), (20, 10, 30, 37)):
            r = run(0, tau, la, lc, win, 0)
            assert r.returncode == 0 and r.stdout.startswith("error"), (r.stdout, r.stderr)
    finally:
        ctx.close()
