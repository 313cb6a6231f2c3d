"""The left-right refinement rule without a GPU: known answers of the restatement in
tests/refine_ref.py, agreement of its two forms, its cross-check against the oracle's lr_check, and the three new names in the
C-ABI.  Every comparison is exact: the rule is stated in integers."""
import os
import re
import sys

import numpy as np
import pytest

from aswstereomatch_amd import _lib
from aswstereomatch_amd.synth import make_pair

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = np.float32(np.nan)


def _both(G, dl, dr, minD, n, max_diff, win, gc, gs):
    a = ref.refine_loop(G, dl, dr, minD, n, max_diff, win, gc, gs)
    b = ref.refine_vec(G, dl, dr, minD, n, max_diff, win, gc, gs)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    return a


# ---- hand-made known answers ----
def test_fill_takes_the_lower_neighbour():
    # valid, rejected x 3, valid with values 7 and 3 -> the run fills with 3 (the validity mask is given, not derived)
    dl = np.array([[7, 5, 5, 5, 3]], np.float32)
    valid = np.array([[True, False, False, False, True]])
    F, mask = ref.fill_loop(dl, valid, 0)
    assert F.tolist() == [[7, 3, 3, 3, 3]] and mask.tolist() == [[0, 1, 1, 1, 0]]
    F2, mask2 = ref.fill_vec(dl, valid, 0)
    assert np.array_equal(F, F2) and np.array_equal(mask, mask2)
    # the other order of the two values: still the lower one
    dl = np.array([[3, 9, 9, 7]], np.float32)
    F, _ = ref.fill_loop(dl, np.array([[True, False, False, True]]), 0)
    assert F.tolist() == [[3, 3, 3, 7]]


def test_edge_runs_take_the_one_existing_neighbour():
    dl = np.array([[9, 9, 4, 8, 8]], np.float32)
    valid = np.array([[False, False, True, False, False]])
    for fill in (ref.fill_loop, ref.fill_vec):
        F, mask = fill(dl, valid, 2)
        assert F.tolist() == [[2, 2, 2, 2, 2]] and mask.tolist() == [[1, 1, 0, 1, 1]]


def test_row_without_valid_pixel_is_unfillable_and_casts_no_vote():
    # row 0: one valid pixel (x = 4), four filled from it; rows 1 and 2: no valid pixel.  Flat guide, gamma_s 1e9: every tap of the
    # 5x5 window weighs 2^20.  A filled pixel of row 0 sees at most 5 taps of its own row and 10 of the dead rows.
    H, W, minD = 3, 5, 4
    dl = np.full((H, W), 4, np.float32)  # disparity 4 points outside a 5-column image except at x = 4
    dl[1:] = 6
    dr = np.full((H, W), NAN)
    dr[0, 0] = 4
    G = np.zeros((H, W), np.uint8)
    res = _both(G, dl, dr, minD, 3, 0.0, 5, 50.0, 1e9)
    assert res["mask"].tolist() == [[1, 1, 1, 1, 0], [2] * 5, [2] * 5]
    assert res["n_unfillable"] == 10 and res["n_rejected"] == 14
    assert (res["out"][1:] == minD - 1).all() and (res["out"][0] == 4).all()
    # known answer of the other rule: had the dead rows voted -- with the value they are given in the output, minD - 1, or with
    # their own dl, 6 -- their 10 taps would have outweighed row 0's 5 and every filled pixel of row 0 would have moved
    tc, ts = ref.tables(5, 50.0, 1e9, 1)
    assert (ts == 256).all() and tc[0] == 4096
    F, mask = ref.fill_vec(dl, ref.cross_check_vec(dl, dr, 0.0), minD)
    assert (F[1:] == -1).all() and (F[0] == 0).all()
    for dead_value, moved_to in ((0, 0), (3, 3)):  # offsets shifted by one: row 0 holds 1, the dead rows 0 (below it) or 3 (above it)
        voting = np.where(F < 0, dead_value, F + 1)
        for med in (ref.median_loop(G, voting, mask, 5, 50.0, 1e9), ref.median_vec(G, voting, mask, 4, 5, 50.0, 1e9)):
            assert (med[0, :4] == moved_to).all() and med[0, 4] == 1


def test_weighted_median_differs_from_unweighted():
    # 3x3 window around the filled centre (fill value 1): five taps vote 1 (the unweighted median), four vote 6; the guide makes
    # the four look like the centre and the five unlike it -> the weighted median is 6.  Only the centre is recomputed.
    F = np.array([[1, 1, 1], [6, 1, 1], [6, 6, 6]], np.int64)
    mask = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], np.uint8)
    G = np.array([[200, 200, 200], [10, 10, 200], [10, 10, 10]], np.uint8)
    assert sorted(F.ravel().tolist())[4] == 1
    want = F.copy()
    want[1, 1] = 6
    assert np.array_equal(ref.median_loop(G, F, mask, 3, 20.0, 100.0), want)
    assert np.array_equal(ref.median_vec(G, F, mask, 7, 3, 20.0, 100.0), want)
    # with a flat guide the same window gives the unweighted answer
    flat = np.zeros((3, 3), np.uint8)
    assert np.array_equal(ref.median_loop(flat, F, mask, 3, 20.0, 100.0), F)
    assert np.array_equal(ref.median_vec(flat, F, mask, 7, 3, 20.0, 100.0), F)


def test_tie_takes_the_smaller_value():
    # 1x3 row, win 3: the rejected centre fills with min(2, 5) = 2; flat guide, gamma_s huge -> the side taps weigh Tc[0] * Ts[0][1]
    # each and the centre 2^20: C(2) = centre + left, T = C(2) + right, so 2 C >= T at v = 2.  The tie proper: two taps only.
    G = np.zeros((1, 2), np.uint8)
    tc, ts = ref.tables(3, 10.0, 1e9, 1)
    assert ts[0, 1] == 256 and tc[0] == 4096
    F = np.array([[5, 2]], np.int64)
    mask = np.array([[1, 0]], np.uint8)  # pixel 0 filled (value 5), pixel 1 valid (value 2): equal weights 2^20 each
    for med in (lambda: ref.median_loop(G, F, mask, 3, 10.0, 1e9), lambda: ref.median_vec(G, F, mask, 8, 3, 10.0, 1e9)):
        assert med().tolist() == [[2, 2]]  # 2 * C(2) = T exactly -> the smaller value


def test_win_1_is_the_fill():
    rng = np.random.default_rng(3)
    H, W = 9, 70
    G = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    dl = rng.integers(0, 5, (H, W)).astype(np.float32)
    dr = rng.integers(0, 5, (H, W)).astype(np.float32)
    res = _both(G, dl, dr, 0, 5, 0.0, 1, 30.0, 3.0)
    assert np.array_equal(res["out"], res["fill"]) and (res["mask"] == 1).any()


def test_small_colour_gamma_makes_the_median_the_identity():
    # a small colour gamma on a high-contrast guide: every off-centre weight rounds to 0 and the median moves no pixel
    tc, _ = ref.tables(3, 1.0, 3.0, 3)
    assert tc[0] == 4096 and (tc[10:] == 0).all()
    rng = np.random.default_rng(4)
    dl = rng.integers(0, 6, (20, 40)).astype(np.float32)
    dr = rng.integers(0, 6, (20, 40)).astype(np.float32)
    G = (np.arange(800).reshape(20, 40) % 2 * 255).astype(np.uint8)  # checkerboard rows: neighbours differ by 255
    G[1::2] = 255 - G[1::2]
    res = ref.refine_vec(G, dl, dr, 0, 6, 0.0, 3, 1.0, 0.2)  # gamma_s 0.2: diagonal (equal colour) taps weigh 0 as well
    assert np.array_equal(res["out"], res["fill"]) and (res["mask"] == 1).sum() > 100


def test_domain_violations_raise():
    G = np.zeros((2, 3), np.uint8)
    good = np.array([[1, 2, 3], [1, 1, 1]], np.float32)
    for bad in (1.5, NAN, np.float32(np.inf), 4.0, 0.0):
        dl = good.copy()
        dl[1, 1] = bad
        for f in (ref.refine_loop, ref.refine_vec):
            with pytest.raises(ref.DomainError):
                f(G, dl, good, 1, 3, 1.0, 3, 30.0, 3.0)


# ---- the two forms agree ----
def _random_case(rng, H, W, C, n, minD, p_reject, dead_rows=()):
    G = rng.integers(0, 256, (H, W) if C == 1 else (H, W, 3)).astype(np.uint8)
    if rng.random() < 0.5:  # piece-wise flat guide so that off-centre colour weights are not all negligible
        G = (G // 64 * 64).astype(np.uint8)
    span = min(n, 40)
    dl = (minD + rng.integers(0, span, (H, W)) * ((n - 1) // max(1, span - 1) if span > 1 else 1)).astype(np.float32)
    dl = np.minimum(dl, minD + n - 1).astype(np.float32)
    dr = np.zeros((H, W), np.float32)
    for y in range(H):
        for x in range(W):
            xr = x - int(dl[y, x])
            if 0 <= xr < W:
                dr[y, xr] = dl[y, x]
    kill = rng.random((H, W)) < p_reject
    dr[kill] = np.where(rng.random(kill.sum()) < 0.5, NAN, -5.0)
    for y in dead_rows:
        dr[y] = NAN
    return G, dl, dr


@pytest.mark.parametrize("H,W,C,win,n,minD", [
    (5, 1, 1, 3, 2, 0), (7, 63, 3, 15, 2, 0), (9, 64, 1, 35, 9, 3), (11, 65, 3, 3, 1025, 0), (13, 131, 3, 1, 17, 5),
    (37, 41, 1, 15, 1025, 2), (3, 200, 3, 35, 30, 0), (40, 7, 1, 35, 4, 1),
])
def test_forms_agree_on_random_maps(H, W, C, win, n, minD):
    rng = np.random.default_rng(H * 1000 + W)
    G, dl, dr = _random_case(rng, H, W, C, n, minD, 0.3, dead_rows=(H // 2,) if H > 4 else ())
    res = _both(G, dl, dr, minD, n, 1.0, win, 80.0, 6.0)
    assert res["n_rejected"] > 0
    if H > 4:
        assert (res["mask"][H // 2] == 2).all() and res["n_unfillable"] >= W


# ---- step 1 equals the oracle's lr_check on the oracle's own classic maps ----
@pytest.mark.parametrize("shape", [(96, 260, 24, 11, 32), (60, 160, 16, 5, 16)])
def test_cross_check_equals_oracle_lr_check(oracle, shape):
    H, W, D, seed, block = shape
    L, R, _ = make_pair(H, W, D, seed=seed, block=block)
    rc0, dl, _ = oracle.asw_classic(L, R, 30, 20, 0, 15, 0, D)
    rc1, dr, _ = oracle.asw_classic(L, R, 30, 20, 1, 15, 0, D)
    assert rc0 == 0 and rc1 == 0
    want, bad = oracle.lr_check(dl, dr, 1.0, -1.0)
    for cc in (ref.cross_check_loop, ref.cross_check_vec):
        valid = cc(dl, dr, 1.0)
        assert np.array_equal(valid, want != -1.0) and int((~valid).sum()) == bad
    # the shares the GPU parity cases rely on (ISSUE table): rejected >= 5 %, the median moves >= 2 % of the filled pixels
    for win, gc, gs in ((15, 60.0, 9.0), (15, 150.0, 9.0), (7, 150.0, 3.0), (35, 150.0, 20.0)):
        res = ref.refine_vec(L, dl, dr, 0, D + 1, 1.0, win, gc, gs)
        rejected, moved = ref.vacuity_shares(res)
        assert rejected >= 0.05 and moved >= 0.02, (win, gc, gs, rejected, moved)
        assert res["n_unfillable"] == 0


# ---- ABI ----
def test_refine_names_are_in_the_abi():
    names = ["asw_refine_disparity", "asw_match_refined_resident", "asw_stereo_match_refined"]
    hdr = open(os.path.join(ROOT, "include", "asw_mi355x.h")).read()
    declared = set(re.findall(r"^\s*(?:int|void|const char\*)\s+(asw_[a-z0-9_]+)\s*\(", hdr, flags=re.M))
    for name in names:
        assert name in _lib.ABI_SYMBOLS and name in declared, name
    assert len(_lib.ABI_SYMBOLS) == 46 and len(set(_lib.ABI_SYMBOLS)) == 46


def test_python_surface():
    import aswstereomatch_amd as asw

    for name in ("refineDisparity", "stereoMatchingRefined", "match_refined_resident"):
        assert callable(getattr(asw.Context, name))
    for name in ("refineDisparity", "stereoMatchingRefined"):
        assert callable(getattr(asw, name)) and name in asw.__all__
