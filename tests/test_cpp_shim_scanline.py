"""stereoMatchingScanline of the C++ surface (include/aswMethods_mi355x.hpp): tests/cpp/scanline_demo.cpp builds with plain g++ on both
Mat branches of the header, and -- on the GPU -- gives the map of the ctypes path and of the restatement, and throws where the
library refuses."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scanline_ref as sr  # noqa: E402
import subpixel_ref as sp  # noqa: E402
from shim_build import build_demo  # noqa: E402

pytestmark = pytest.mark.parametrize("cv", [False, True])


def test_scanline_demo_compiles(tmp_path, cv):
    assert os.path.exists(build_demo("scanline_demo.cpp", tmp_path / "scanline_demo", cv))


@pytest.mark.gpu
def test_shim_matches_ctypes_path(tmp_path, cv):
    import aswstereomatch_amd as asw

    exe = build_demo("scanline_demo.cpp", tmp_path / "scanline_demo", cv)
    H, W, D = 23, 70, 13
    L, R = sr.textured_pair(H, W, 3, 4, 5)
    L.tofile(tmp_path / "l.raw")
    R.tofile(tmp_path / "r.raw")

    def run(dt, alg, minD, a, u, ratio, sub):
        argv = [exe, H, W, 3, tmp_path / "l.raw", tmp_path / "r.raw", int(dt), int(alg), 5, minD, D, a, u, ratio, sub,
                tmp_path / "shim.raw", tmp_path / "c.raw"]
        return subprocess.run([str(x) for x in argv], capture_output=True, text=True, timeout=120)

    ctx, ctx2 = asw.Context(0), asw.Context(0)
    try:
        for dt, alg, minD, code, sub in ((0, 2, 0, (4, 5, 4), 0), (1, 12, 3, (1, 5, 1), 0), (0, asw.twopass_algorithm(), 1, (64, 3, 8), 0x100)):
            plain = ctx2.stereoMatching(L, R, dt, alg, 5, minD, D, return_cost_volume=True)[1]
            vol = sr.optimise(plain, *sr.penalties(*code))
            want = sr.wta(vol, minD)
            assert not np.array_equal(vol, plain)
            if sub:
                want = sp.subpixel_vec(want, vol, minD, sub)[0]
            r = run(dt, alg, minD, *code, sub)
            assert r.returncode == 0 and r.stdout.strip() == "ok %d %d" % (H, W), (r.stdout, r.stderr)
            assert np.array_equal(ctx.stereoMatching(L, R, dt, alg, 5, minD, D, subpixel=sub, scanline=asw.scanline(*code)), want)
            for name in ("shim.raw", "c.raw"):
                assert np.array_equal(np.fromfile(tmp_path / name, np.float32).reshape(H, W), want)
        # the throwing rows: a code out of range (three ways), NCC, GuidedF_2 in the right view, SGBM
        for dt, alg, code in ((0, 2, (0, 5, 4)), (0, 2, (8, 8, 4)), (0, 2, (8, 5, 9)), (0, 11, (8, 5, 4)), (1, 8, (8, 5, 4)), (0, 1, (8, 5, 4))):
            r = run(dt, alg, 0, *code, 0)
            assert r.returncode == 0 and r.stdout.startswith("error"), (r.stdout, r.stderr)
    finally:
        ctx.close()
        ctx2.close()
