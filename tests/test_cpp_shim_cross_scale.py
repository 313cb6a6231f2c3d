"""stereoMatchingCrossScale of the C++ surface (include/aswMethods_mi355x.hpp): tests/cpp/cross_scale_demo.cpp builds with plain g++ on
both Mat branches of the header, and -- on the GPU -- gives the map of the ctypes path and of the restatement, and throws where the
library refuses."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cross_scale_ref as cs  # noqa: E402
import subpixel_ref as sp  # noqa: E402
from shim_build import build_demo  # noqa: E402

pytestmark = pytest.mark.parametrize("cv", [False, True])


def test_cross_scale_demo_compiles(tmp_path, cv):
    assert os.path.exists(build_demo("cross_scale_demo.cpp", tmp_path / "cross_scale_demo", cv))


@pytest.mark.gpu
def test_shim_matches_ctypes_path(tmp_path, cv):
    import aswstereomatch_amd as asw
    from aswstereomatch_amd import _lib

    exe = build_demo("cross_scale_demo.cpp", tmp_path / "cross_scale_demo", cv)
    H, W, D = 23, 70, 13
    L, R = cs.textured_pair(H, W, 3, 4, 5)
    L.tofile(tmp_path / "l.raw")
    R.tofile(tmp_path / "r.raw")

    def run(dt, alg, minD, S, q, sub):
        argv = [exe, H, W, 3, tmp_path / "l.raw", tmp_path / "r.raw", int(dt), int(alg), 5, minD, D, S, q, sub, tmp_path / "shim.raw",
                tmp_path / "c.raw"]
        return subprocess.run([str(a) for a in argv], capture_output=True, text=True, timeout=120)

    ctx, ctx2 = asw.Context(0), asw.Context(0)
    try:
        for dt, alg, minD, S, q, sub in ((0, 2, 0, 3, 19, 0), (1, 12, 3, 4, 64, 0), (0, asw.twopass_algorithm(), 1, 2, 255, 0x100)):
            n = _lib.lib().asw_volume_planes(int(alg), D)
            ranges = cs.scale_ranges(minD, n, n - D, S)
            vols = [ctx2.stereoMatching(Ls, Rs, dt, alg, 5, ranges[s][0], ranges[s][2], return_cost_volume=True)[1]
                    for s, (Ls, Rs) in enumerate(zip(cs.pyramid(L, S), cs.pyramid(R, S)))]
            vol = cs.combine(vols, minD, cs.weights(S, q))
            want = cs.wta(vol, minD)
            assert not np.array_equal(vol, vols[0])
            if sub:
                want = sp.subpixel_vec(want, vol, minD, sub)[0]
            r = run(dt, alg, minD, S, q, sub)
            assert r.returncode == 0 and r.stdout.strip() == "ok %d %d" % (H, W), (r.stdout, r.stderr)
            assert np.array_equal(ctx.stereoMatching(L, R, dt, alg, 5, minD, D, subpixel=sub, cross_scale=asw.cross_scale(S, q)), want)
            for name in ("shim.raw", "c.raw"):
                assert np.array_equal(np.fromfile(tmp_path / name, np.float32).reshape(H, W), want)
        for dt, alg, S, q in ((0, 2, 6, 19), (0, 2, 3, 0), (0, 11, 3, 19), (1, 8, 3, 19), (0, 1, 3, 19)):  # the throwing rows
            r = run(dt, alg, 0, S, q, 0)
            assert r.returncode == 0 and r.stdout.startswith("error"), (r.stdout, r.stderr)
    finally:
        ctx.close()
        ctx2.close()
