"""stereoMatchingConfidence of the C++ surface (include/aswMethods_mi355x.hpp): tests/cpp/confidence_demo.cpp builds with plain g++ on
both Mat branches of the header, and -- on the GPU -- gives the two maps of asw_stereo_match with a 2-channel image (padded rows),
of the ctypes path and of the restatement, and throws where the library refuses."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import confidence_ref as cr  # noqa: E402
import scanline_ref as sr  # noqa: E402
from shim_build import build_demo  # noqa: E402

pytestmark = pytest.mark.parametrize("cv", [False, True])


def test_confidence_demo_compiles(tmp_path, cv):
    assert os.path.exists(build_demo("confidence_demo.cpp", tmp_path / "confidence_demo", cv))


@pytest.mark.gpu
def test_shim_matches_ctypes_path(tmp_path, cv):
    import aswstereomatch_amd as asw

    exe = build_demo("confidence_demo.cpp", tmp_path / "confidence_demo", cv)
    H, W, D = 23, 70, 13
    L, R = sr.textured_pair(H, W, 3, 4, 5)
    L.tofile(tmp_path / "l.raw")
    R.tofile(tmp_path / "r.raw")

    def run(dt, alg, win, minD):
        argv = [exe, H, W, 3, tmp_path / "l.raw", tmp_path / "r.raw", int(dt), int(alg), win, minD, D, tmp_path / "d.raw",
                tmp_path / "c.raw", tmp_path / "both.raw"]
        return subprocess.run([str(x) for x in argv], capture_output=True, text=True, timeout=120)

    ctx = asw.Context(0)
    try:
        rows = ((0, 2, 0), (1 | 0x100, asw.twopass_algorithm(), 1), (asw.scanline(4, 5, 4) | 0x200, 8, 0), (1 | asw.cross_scale(3, 19), 7, 2))
        for dt, alg, minD in rows:
            d, v, c = ctx.stereoMatching(L, R, dt, alg, 5, minD, D, return_cost_volume=True, return_confidence=True)
            assert cr.same_bits(c, cr.confidence_vec(v)) and (c > 0).any()
            r = run(dt, alg, 5, minD)
            assert r.returncode == 0 and r.stdout.strip() == "ok %d %d" % (H, W), (r.stdout, r.stderr)
            assert cr.same_bits(np.fromfile(tmp_path / "d.raw", np.float32).reshape(H, W), d)
            assert cr.same_bits(np.fromfile(tmp_path / "c.raw", np.float32).reshape(H, W), c)
            both = np.fromfile(tmp_path / "both.raw", np.float32).reshape(H, 2 * W + 3)
            assert cr.same_bits(both[:, 0:2 * W:2], d) and cr.same_bits(both[:, 1:2 * W:2], c)
            assert (both[:, 2 * W:] == np.float32(-7.5)).all()  # the padding of the C-ABI call's rows
        # the throwing rows: SGBM, NCC, both sub-pixel flags
        for dt, alg in ((0, 1), (0, 11), (0x300, 2)):
            r = run(dt, alg, 5, 0)
            assert r.returncode == 0 and r.stdout.startswith("error"), (r.stdout, r.stderr)
        r = run(0, 2, 4, 0)  # an even window: the silent return, two empty Mats
        assert r.returncode == 0 and r.stdout.strip() == "empty", (r.stdout, r.stderr)
    finally:
        ctx.close()
