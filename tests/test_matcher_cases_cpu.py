"""CPU-side checks of tests/matcher_cases.py and of the tie rules of the two restatements (no GPU needed).

tests/sgbm_ref.py and tests/stereobm_ref.py break ties in opposite directions (DESIGN.md sections 4.8 and 4.9): StereoSGBM keeps
the first minimum over d = 0..D-1, the smallest disparity; StereoBM keeps the first minimum over k = 0..D-1 with disparity
minD + D-1-k, the largest.  The answers asserted here follow from OpenCV's loops, not from the GPU, so that an equal GPU result in
tests/test_gpu_matcher_degenerate.py means something; and the tie-dense inputs of that file are shown to tie, on the restatements
alone, before any kernel is compared on them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matcher_cases as mc  # noqa: E402
import sgbm_ref  # noqa: E402
import stereobm_ref  # noqa: E402
import subpixel_ref  # noqa: E402

H, W, D, BLOCK = 20, 150, 32, 5


@pytest.mark.parametrize("minD,value", [(0, 496), (5, 576)])
def test_bm_constant_pair_takes_the_largest_disparity(minD, value):
    # every SAD is 0: the first minimum is k = 0, disparity minD + D - 1; p = n, so the sub-pixel term is 0
    L, R = mc.constant(H, W, 1)
    want = stereobm_ref.stereo_bm(L, R, minD, D, BLOCK, 31, 0, 0, 0, 0, -1)
    y0, y1, x0, x1 = stereobm_ref.valid_roi(H, W, minD, D, BLOCK)
    assert value == 16 * (minD + D - 1)
    assert (want["disp"][y0:y1, x0:x1] == value).all()
    scalar, _ = stereobm_ref.stereo_bm_scalar(L[:8, :60], R[:8, :60], minD, D, BLOCK, 31, 0, 0, -1)  # OpenCV's loop form
    assert (scalar[2:6, minD + D + 1:58] == value).all()


@pytest.mark.parametrize("minD,value", [(0, 0), (5, 80)])
def test_sgbm_constant_pair_takes_the_smallest_disparity(minD, value):
    L, R = mc.constant(H, W, 1)
    want = sgbm_ref.sgbm(L, R, minD, D, BLOCK, 200, 800, -1, 10, 0, 0, 0)
    assert value == 16 * minD
    assert (want["disp"][:, minD + D:] == value).all()
    _, scalar = sgbm_ref.sgbm_scalar(L[:3, :minD + D + 6], R[:3, :minD + D + 6], minD, D, BLOCK, 200, 800, -1, 10, 0)
    assert (np.array(scalar)[:, minD + D:] == value).all()


def _sgbm_shares(L, R, minD, cap=10):
    want = sgbm_ref.sgbm(L, R, minD, D, BLOCK, 200, 800, -1, cap, 0, 0, 0)
    return mc.tie_share(want["S"][:, minD + D:], 2), float((want["disp"] != 16 * (minD - 1)).mean())


def _bm_shares(L, R, minD=0):
    want = stereobm_ref.stereo_bm(L, R, minD, D, BLOCK, 31, 0, 0, 0, 0, 1)
    return mc.tie_share(want["vol"], 0), float((want["disp"] != 16 * (minD - 1)).mean())


def test_tie_generators_really_tie():
    ties, alive = _sgbm_shares(*mc.periodic(H, W, 1, 4, 3), 0)
    print("SGBM periodic(4, 3): tie share %.3f, not-invalid share %.3f" % (ties, alive))
    assert ties >= 0.5 and alive >= 0.5
    for p in (4, 8):
        ties, alive = _bm_shares(*mc.periodic(H, W, 1, p, 3))
        print("BM periodic(%d, 3): tie share %.3f, not-invalid share %.3f" % (p, ties, alive))
        assert ties >= 0.5 and alive >= 0.5
    assert _bm_shares(*mc.constant(H, W, 1))[0] == 1.0
    assert _sgbm_shares(*mc.constant(H, W, 1), 5)[0] == 1.0


def test_tie_share_counts_shared_minima_over_finite_pixels():
    v = np.array([[[1, 1, 2], [1, 2, 3]], [[np.nan, 0, 0], [5, 4, 4]]], np.float32)  # [y][x][d]: tie, none, not finite, tie
    assert mc.tie_share(v, 2) == pytest.approx(2 / 3)
    assert mc.tie_share(np.moveaxis(v, 2, 0), 0) == pytest.approx(2 / 3)
    assert mc.tie_share(np.full((2, 2, 3), np.nan), 2) == 0.0


def test_generators_have_the_stated_structure():
    L, R = mc.periodic(7, 50, 3, 8, 3)
    assert L.shape == (7, 50, 3) and np.array_equal(L[:, 8:48], L[:, :40]) and np.array_equal(R, np.roll(L, -3, axis=1))
    L, R = mc.row_constant(9, 31, 1, seed=2)
    assert (L == L[:, :1]).all() and np.array_equal(L, R) and len(np.unique(L)) > 1
    L, R = mc.quantised(12, 40, 3, seed=1)
    assert set(np.unique(L)) <= {0, 64, 128, 192}
    Lf, _ = mc.flat_rects(20, 60, 1, seed=3)
    assert not np.array_equal(Lf, mc.textured(20, 60, 1, seed=3)[0])
    v = mc.padded_view(L, 5, 255)
    assert v.strides[0] == 45 * 3 and np.array_equal(v, L) and mc.padded_view(L, 0, 0) is L


def _same_case(a, b):
    return a["tag"] == b["tag"] and all(np.array_equal(a[k], b[k], equal_nan=True) if isinstance(a[k], np.ndarray) else a[k] == b[k]
                                        for k in a)


@pytest.mark.parametrize("family", mc.FAMILIES)
def test_random_case_is_deterministic_and_rebuilds_from_its_tag(family):
    seed = mc.SWEEP_SEEDS[0]
    first, second = mc.cases(family, seed, 8), mc.cases(family, seed, 8)
    assert len({c["tag"] for c in first}) > 1
    for a, b in zip(first, second):
        assert _same_case(a, b) and _same_case(a, mc.build_case(family, a["tag"]))
    assert mc.cases(family, mc.SWEEP_SEEDS[1], 8)[0]["tag"] != first[0]["tag"]


@pytest.mark.parametrize("seed", mc.SWEEP_SEEDS)
@pytest.mark.parametrize("family", ["sgbm", "bm", "speckles", "refine", "sgbm_paths"])
def test_restatements_accept_every_sweep_case(family, seed):
    padded = 0
    for case in mc.cases(family, seed):
        want = mc.reference(case)
        if family in ("sgbm", "bm", "sgbm_paths"):
            Hc, Wc = case["L"].shape[:2]
            padded += case["L"].strides[0] > Wc * (case["L"].shape[2] if case["L"].ndim == 3 else 1)
            assert want["disp"].shape == (Hc, Wc) and want["disp"].dtype == np.int16, case["tag"]
            assert want["vol"].shape == (case["args"][1], Hc, Wc), case["tag"]
        elif family == "speckles":
            assert want["map"].shape == case["map"].shape and want["map"].dtype == np.int16, case["tag"]
        else:
            assert want["out"].shape == case["dl"].shape and want["counts"][0] >= want["counts"][1], case["tag"]
    if family in ("sgbm", "bm", "sgbm_paths"):
        print("%s seed %d: %d padded cases" % (family, seed, padded))


@pytest.mark.parametrize("seed", mc.SWEEP_SEEDS)
def test_sgbm_paths_sweep_gives_the_line_kernel_work(seed):
    # the added directions run over the valid columns [minD + D, W) only: a family that drew W as the sgbm family does would leave
    # about a third of its cases without any
    cases = mc.cases("sgbm_paths", seed)
    assert len(cases) == 30
    empty = diagonal = 0
    for case in cases:
        kind, Hc, Wc, cn, minD, Dc, w, P1, P2, m12, cap, U = case["tag"][:12]
        paths = case["tag"][-1]
        assert case["paths"] == paths and paths & 0x07 == 0x07 and 0 <= paths <= 0xFF and Hc <= 40, case["tag"]
        assert case["L"].shape[:2] == (Hc, Wc) and case["args"][:3] == (minD, Dc, w), case["tag"]
        empty += Wc <= minD + Dc
        diagonal += Hc >= 2 and Wc - minD - Dc >= 2      # a diagonal longer than one pixel exists
        # the f32 volume is exact, so no case has to drop its comparison (n (C_max + P2) < 2^24)
        w_, ftzero, _, P2e, _, _ = sgbm_ref.effective_params(w, P1, P2, m12, cap, U)
        assert bin(paths).count("1") * (sgbm_ref.cost_bound(cn, w_, ftzero) + P2e) < 1 << 24, case["tag"]
    print("sgbm_paths seed %d: %d cases without a valid column, %d with a diagonal of two pixels or more, %d masks"
          % (seed, empty, diagonal, len({c["tag"][-1] for c in cases})))
    assert empty <= 3 and diagonal >= 20


@pytest.mark.parametrize("seed", mc.SWEEP_SEEDS)
def test_subpixel_restatement_accepts_every_sweep_shape(seed):
    # the sub-pixel cases are checked on the library's own map and volume; here the restatement sees a random map and volume of
    # every case's shape, numDisparity + 1 planes (the inclusive range of most methods)
    for case in mc.cases("subpixel", seed):
        rng = np.random.default_rng(case["tag"][-1])
        n = case["numD"] + 1
        Hc, Wc = case["L"].shape[:2]
        vol = rng.integers(0, 50, (n, Hc, Wc)).astype(np.float32)
        disp = (case["minD"] + vol.argmin(axis=0)).astype(np.float32)
        out, ok = subpixel_ref.subpixel_vec(disp, vol, case["minD"], case["mode"])
        assert out.shape == disp.shape and (np.abs(out - disp) <= 0.5).all(), case["tag"]
