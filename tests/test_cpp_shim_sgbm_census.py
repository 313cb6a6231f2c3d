"""getDisparity_SGBM_census of the C++ surface (include/aswMethods_mi355x.hpp): tests/cpp/sgbm_census_demo.cpp builds with plain g++
on both Mat branches of the header, and -- on the GPU -- gives the u8 map of the restatement (tests/sgbm_census_ref.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from shim_build import build_demo  # noqa: E402


@pytest.mark.parametrize("cv", [False, True])
def test_sgbm_census_demo_compiles(tmp_path, cv):
    assert os.path.exists(build_demo("sgbm_census_demo.cpp", tmp_path / "sgbm_census_demo", cv))


@pytest.mark.gpu
@pytest.mark.parametrize("cv", [False, True])
def test_shim_get_disparity_sgbm_census(tmp_path, cv):
    import sgbm_census_ref as cref
    import sgbm_paths_ref as pref

    exe = build_demo("sgbm_census_demo.cpp", tmp_path / "sgbm_census_demo", cv)
    out = tmp_path / "d.raw"
    for cn in (3, 1):
        L, R = cref.shape_pair(40, 96, 32, cn, seed=53)
        L.tofile(tmp_path / "l.raw")
        R.tofile(tmp_path / "r.raw")

        def run(win, numD, paths):
            return subprocess.run([exe, "40", "96", str(cn), str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), str(win), "0", str(numD),
                                   hex(paths), str(out)], capture_output=True, text=True, timeout=120)

        for paths in (pref.PATHS_HH, pref.PATHS_SGBM):
            r = run(5, 32, paths)
            assert r.returncode == 0 and r.stdout.strip() == "ok 40 96 bt_same=0", (r.stdout, r.stderr)
            want = cref.get_disparity_sgbm_census(L, R, 5, 0, 32, paths)
            assert len(np.unique(want)) > 2
            assert np.array_equal(np.fromfile(out, np.uint8).reshape(40, 96), want)
    for win, numD, paths in ((4, 32, 0xff), (5, 24, 0xff), (5, 32, 0x30), (5, 32, 0x100)):
        r = run(win, numD, paths)
        assert r.returncode == 0 and r.stdout.startswith("error"), (r.stdout, r.stderr)
