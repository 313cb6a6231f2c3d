"""computeAdaptiveWeight_permeability of the C++ surface (include/aswMethods_mi355x.hpp): tests/cpp/permeability_demo.cpp builds with
plain g++ on both Mat branches of the header, and -- on the GPU -- gives the map of the ctypes path and of the restatement, and throws
where its siblings throw."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import permeability_ref as pm  # noqa: E402
from shim_build import build_demo  # noqa: E402

pytestmark = pytest.mark.parametrize("cv", [False, True])


def test_permeability_demo_compiles(tmp_path, cv):
    assert os.path.exists(build_demo("permeability_demo.cpp", tmp_path / "permeability_demo", cv))


@pytest.mark.gpu
def test_shim_matches_ctypes_path(tmp_path, cv):
    import aswstereomatch_amd as asw

    exe = build_demo("permeability_demo.cpp", tmp_path / "permeability_demo", cv)
    H, W, D = 37, 130, 17
    L, R = pm.textured_pair(H, W, 3, 5, 3)
    L.tofile(tmp_path / "l.raw")
    R.tofile(tmp_path / "r.raw")
    out = tmp_path / "d.raw"

    def run(channels, right, sigma, trunc, minD):
        argv = [exe, H, W, channels, tmp_path / "l.raw", tmp_path / "r.raw", right, sigma, trunc, minD, D, out]
        return subprocess.run([str(a) for a in argv], capture_output=True, text=True, timeout=120)

    ctx = asw.Context(0)
    try:
        for right, sigma, trunc, minD in ((0, 8, 20, 0), (1, 8, 20, 3), (0, 1, 255, 0)):
            r = run(3, right, sigma, trunc, minD)
            assert r.returncode == 0 and r.stdout.strip() == "ok %d %d selector_same=1" % (H, W), (r.stdout, r.stderr)
            want = ctx.computeAdaptiveWeight_permeability(L, R, right, sigma, trunc, minD, D)
            assert np.array_equal(np.fromfile(out, np.float32).reshape(H, W), want)
            e = np.stack(ctx.computeAD(L, R, right, minD, D))
            assert np.array_equal(want, pm.aggregate(e, R if right else L, sigma, trunc, minD)[2])  # and the restatement's
        for channels, sigma, trunc in ((3, 0, 20), (3, 8, 256), (2, 8, 20)):  # the throwing rows; 2 channels: the first 2 H W bytes of the files
            r = run(channels, 0, sigma, trunc, 0)
            assert r.returncode == 0 and r.stdout.startswith("error"), (r.stdout, r.stderr)
    finally:
        ctx.close()
