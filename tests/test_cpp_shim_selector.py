"""The per-method wrappers of the C++ surface (include/aswMethods_mi355x.hpp) whose parameters travel in the selector's algorithm value:
tests/cpp/selector_demo.cpp builds with plain g++ on both Mat branches of the header, and -- on the GPU -- gives, for every method of
tests/selector_methods.py, the map of the ctypes path and of the restatement."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from selector_methods import METHODS  # noqa: E402
from shim_build import build_demo  # noqa: E402

pytestmark = [pytest.mark.parametrize("m", METHODS, ids=lambda m: m.name), pytest.mark.parametrize("cv", [False, True])]


def test_selector_demo_compiles(tmp_path, m, cv):
    # one program serves every method; it is compiled for each so that every method keeps its compile-only test on a CPU box
    assert os.path.exists(build_demo("selector_demo.cpp", tmp_path / "selector_demo", cv))


@pytest.mark.gpu
def test_shim_matches_ctypes_path(tmp_path, m, cv):
    import aswstereomatch_amd as asw

    exe = build_demo("selector_demo.cpp", tmp_path / "selector_demo", cv)
    H, W, D = 37, 130, 17
    L, R = m.shim_input()
    L.tofile(tmp_path / "l.raw")
    R.tofile(tmp_path / "r.raw")
    out = tmp_path / "d.raw"

    def run(right, params, win, minD):
        argv = [exe, m.name, H, W, 3, tmp_path / "l.raw", tmp_path / "r.raw", right, *params, win, minD, D, out]
        return subprocess.run([str(a) for a in argv], capture_output=True, text=True, timeout=120)

    ctx = asw.Context(0)
    try:
        for right, params, win, minD, same in m.shim_good:
            r = run(right, params, win, minD)
            assert r.returncode == 0 and r.stdout.strip() == "ok %d %d selector_same=%d" % (H, W, same), (r.stdout, r.stderr)
            want = m.call(ctx, L, R, right, params, win, minD, D)
            assert np.array_equal(np.fromfile(out, np.float32).reshape(H, W), want)
            assert np.array_equal(want, m.want(ctx, L, R, right, params, win, minD, D)[1])  # and the restatement's
        r = run(0, m.default, 14, 0)  # even window: an empty Mat, like the neighbours
        assert r.returncode == 0 and r.stdout.strip() == "empty", (r.stdout, r.stderr)
        for params, win in m.shim_throwing:
            r = run(0, params, win, 0)
            assert r.returncode == 0 and r.stdout.startswith("error"), (r.stdout, r.stderr)
    finally:
        ctx.close()
