"""The launch-geometry table of tests/geometry_cases.py and the references of tests/test_gpu_launch_geometry.py, on the CPU alone.

Table position: every listed frame takes the value its label claims under the restated formula, each "last" / "first" pair of frames
sits on both sides of its threshold, and the lists cover every value a decision can take (or NOT_REACHED says why not).  The
constants of the formulas are read from the source text and must equal the restated ones: a changed launcher fails here.
Non-vacuity, on the references alone: every plane of every expected volume holds at least two values, every expected map more than
one disparity, and where the candidate range is split over grid.z the winners fall into at least two slices."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_cases as gc  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "aswstereomatch_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


def _int(text, pattern):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return int(m[0])


def _body(text, start, end="\n}\n"):
    i = text.index(start)
    return text[i:text.index(end, i)]


# ---------------------------------------------------------------- the constants, from the source text
def test_similarity_constants():
    t = _src("k_cost.hip")
    assert _int(t, r"constexpr int SIM_ROWS = (\d+);") == gc.SIM_ROWS
    assert _int(t, r"constexpr int SIM_DCH = (\d+);") == gc.SIM_DCH == max(gc.SIM_DCH_VALUES)
    assert _int(t, r"const long long sim_wg_target = (\d+);") == gc.SIM_WG_TARGET
    body = _body(t, "int launch_similarity(")
    assert "while (dch > %d && wg_xy * ((numD + dch - 1) / dch) < sim_wg_target) dch /= 2;" % gc.SIM_DCH_MIN in body
    assert "(long long)((W + %d) / %d) * ((H + SIM_ROWS - 1) / SIM_ROWS)" % (gc.SIM_COLS - 1, gc.SIM_COLS) in body
    assert "__launch_bounds__(%d) void k_similarity" % gc.SIM_COLS in t
    assert gc.SIM_DCH_VALUES == tuple(gc.SIM_DCH_MIN << i for i in range(7))


def test_split_constants():
    b, g = _src("k_bilateral.hip"), _src("k_geodesic.hip")
    assert _int(b, r"constexpr int TW = (\d+);") == gc.TILE_W and _int(b, r"constexpr int TH = (\d+);") == gc.TILE_H
    assert re.search(r"constexpr int TW = %d, TH = %d, GG" % (gc.TILE_W, gc.TILE_H), g)
    assert "tiles < %d) nz = std::min(chunks16, std::min(a.max_slices, (%d + tiles - 1) / tiles));" % (gc.BIL_TARGET, gc.BIL_TARGET) in b
    assert "tiles < %d) nz = std::min(chunks16, std::min(%d, (%d + tiles - 1) / tiles));" % (gc.GEO_TARGET, gc.MAX_SLICES, gc.GEO_TARGET) in g
    for t in (b, g):
        assert "chunks_per_z = (chunks16 + nz - 1) / nz;" in t and "nz = (chunks16 + chunks_per_z - 1) / chunks_per_z;" in t
        assert "p.cand_per_z = chunks_per_z * 16;" in t
    m = _src("asw_methods.hip")
    assert m.count("if (plane <= (size_t)1 << 20)") == 2 and gc.SPLIT_MAX_PLANE == 1 << 20
    assert "a.max_slices = %d;" % gc.MAX_SLICES in m and "slice_scratch(ctx, %d, plane, &partE, &partD)" % gc.MAX_SLICES in m
    assert "int bilateral_xq_candidates(int nwave) { return 16 * nwave; }" in _src("k_bilateral_xq.hip")
    assert "int geodesic_xq_pass_candidates(int nwave) { return 16 * nwave; }" in _src("k_geodesic_xq.hip")
    assert gc.XQ_MIN_CANDIDATES == 16 * 4 and "W >= %d" % gc.XQ_MIN_W in m


def test_bm_census_and_grid_constants():
    t = _body(_src("k_bm.hip"), "int launch_match(")
    assert "int TX = std::min(64, 4096 / (NPL * 64));" in t
    assert "while (TX > %d && (long long)((W - lofs + TX - 1) / TX) * ((Hv + %d) / %d) < %d) TX /= 2;" % (
        gc.BM_TX_MIN, gc.BM_STRIP_ROWS - 1, gc.BM_STRIP_ROWS, gc.BM_WAVES_TARGET) in t
    assert "std::max(1, %d / tiles)" % gc.BM_WAVES_TARGET in t and "strips_wanted, %d);" % gc.BM_ROWS_MIN in t
    t = _body(_src("k_sgbm.hip"), "int launch_hcost_census(")
    assert "const int want = spb * ((%d + H - 1) / H);" % gc.CENSUS_WG_TARGET in t
    assert "Wv / std::max(%d, 2 * (2 * h + 1))" % gc.CENSUS_SEG_MIN in t and "const int spb = 256 / std::min(D, 256);" in t
    t = _body(_src("k_prep.hip"), "int launch_disp_to_u8(")
    assert "(n + 256 * 8 - 1) / (256 * 8)" in t and "if (bx > 1024) bx = 1024;" in t
    t = _body(_src("k_cost.hip"), "int launch_slice_scales(")
    assert "(plane + 256 * 16 - 1) / (256 * 16)" in t and "if (bx > 64) bx = 64;" in t
    t = _body(_src("k_cost.hip"), "int launch_u8_scale(")
    assert "(nbytes + 256 * 64 - 1) / (256 * 64)" in t and "if (bx > 1024) bx = 1024;" in t
    assert (gc.DISP_U8_CAP, gc.SLICE_SCALES_CAP, gc.U8_SCALE_CAP) == (2097152, 262144, 16777216)
    t = _src("k_permeability.hip")
    assert _int(t, r"constexpr int SEG = (\d+);") == gc.PERM_SEG
    m = _src("asw_methods.hip")
    assert "const size_t budget = (size_t)2 << 30;" in m and "((size_t)2 << 30) / 6 / per_slice) / 8 * 8" in m and gc.BUDGET == 2 << 30


# ---------------------------------------------------------------- similarity
def test_similarity_table():
    assert sorted(gc.SIM_FIRST) == sorted(gc.SIM_DCH_VALUES)
    for H, W, minD, numD, dch in gc.sim_cases():
        g = gc.sim_launch(H, W, numD)
        assert g["dch"] == dch and numD > dch and numD % dch and g["nz"] >= 2 and 0 < g["last"] < dch, (H, W, numD, g)
        assert g["lds"] <= 64 * 1024 and H * W <= gc.MAX_PIXELS
        if dch > gc.SIM_DCH_MIN:  # the first frame of its value: one row less, one row block less, half the chunk
            assert H % gc.SIM_ROWS == 1 and gc.sim_launch(H - 1, W, numD)["dch"] == dch // 2, (H, W, numD)
    H, W, minD, numD, dch = gc.SIM_WIDE
    assert W > gc.SIM_COLS and W % gc.SIM_COLS and dch > gc.SIM_DCH_MIN and gc.sim_launch(H, W, numD)["gx"] == 2
    assert gc.sim_launch(*gc.SIM_FIRST[512][:2], 600) == {"dch": 512, "nz": 2, "last": 88, "gx": 1, "gy": 2048, "lds": 38912}  # the issue's example
    assert gc.sim_launch(8192, 16, 600)["dch"] == 512
    # what the parent's quick tests ran: 8 everywhere
    for H, W, numD in ((9, 16, 4), (37, 70, 24), (20, 33, 9), (6, 10, 25)):
        assert gc.sim_launch(H, W, numD)["dch"] == 8
    for (H, W, win, minD, numD, dch), least in ((gc.GUIDED2_CASE, 64), (gc.WMEDIAN_CASE, 64)):
        assert gc.sim_launch(H, W, numD)["dch"] == dch >= least and numD > dch and numD % dch


@pytest.mark.parametrize("case", gc.sim_cases(), ids=lambda c: "dch%d-%dx%d" % (c[4], c[0], c[1]))
def test_similarity_references_distinguish(oracle, case):
    H, W, minD, numD, dch = case
    for win in (None, gc.SIM_PAD_WIN):
        vol = gc.expected_similarity(oracle, case, win)
        h = 0 if win is None else win // 2
        assert vol.shape == (numD, H + 2 * h, W + 2 * h) and vol.dtype == np.float32
        assert all(gc.varies(p) for p in vol)
    vol = gc.expected_similarity(oracle, case)
    # the planes of different z slices differ: a slice written to another's planes would show
    assert dch % (2 * W) and not any(np.array_equal(vol[k], vol[k + dch]) for k in range(numD - dch))


def test_similarity_parameter_grid_distinguishes(oracle):
    """every thresC, thresG and regularity of the list changes the oracle's volume against its neighbour in the list, except where
    the list says two values must agree: thresC 9.999 truncates like 9.5 would (c is an integer), 254.6 and 300 clip nothing more"""
    L, R = gc.param_pair()
    H, W, minD, numD = gc.PARAM_FRAME
    vol = lambda r, c, g: gc._once(("param", r, c, g), lambda: oracle.compute_similarity(L, R, r, c, g, 0, minD, numD)[1])
    base = vol(0.4, 10.0, 50.0)
    assert all(len(gc.distinct(p)) >= 2 for p in base)
    assert not np.array_equal(vol(0.4, 0.0, 50.0), vol(0.4, 0.5, 50.0)) or not np.array_equal(vol(0.4, 0.5, 50.0), vol(0.4, 9.999, 50.0))
    assert not np.array_equal(vol(0.4, 9.999, 50.0), base)          # an integer colour sum of exactly 10 exists
    assert not np.array_equal(base, vol(0.4, 254.6, 50.0))
    assert not np.array_equal(vol(0.4, 10.0, 0.0), vol(0.4, 10.0, 49.5))
    assert not np.array_equal(vol(0.4, 10.0, 49.5), base) and not np.array_equal(base, vol(0.4, 10.0, 1e9))
    assert not np.array_equal(vol(0.0, 10.0, 50.0), base) and not np.array_equal(base, vol(1.0, 10.0, 50.0))


# ---------------------------------------------------------------- the grid.z split of classic and geodesic ASW
@pytest.mark.parametrize("kernel", sorted(gc.SPLIT_KERNELS))
def test_split_table(kernel):
    method, win, target = gc.SPLIT_KERNELS[kernel]
    cases = gc.SPLIT_CASES[kernel]
    for H, W, cwin, minD, numD, nz, per_z, what in cases:
        nD = numD + 1
        assert cwin == win and gc.split_launch(H, W, nD, target) == (nz, per_z), (kernel, what)
        assert not gc.takes_xq(W, win, nD) and H * W <= gc.SPLIT_MAX_PLANE and (nz - 1) * per_z < nD
    forms = {(nz, per_z) for *_, nz, per_z, _ in cases}
    assert {nz for nz, _ in forms} >= set(range(1, 9))
    assert {p for _, p in forms} >= {16, 32, 48}                          # 16, 32 and a larger slice, at every window
    assert (1, 32) in forms and any(gc.cdiv(H, gc.TILE_H) >= target for H, *_ in cases)  # one slice of 17 candidates: by the tile count
    if win == 5:                                                          # 32 a slice under 129 candidates: by the tile count
        assert any(nz == 2 and p == 32 and numD + 1 <= 128 for *_, numD, nz, p, _ in cases)
    for (ha, wa), (hb, wb), nD, fa, fb in gc.split_threshold_pairs(kernel):
        assert hb == ha + 1 and wa == wb and gc.split_launch(ha, wa, nD, target) == fa != fb == gc.split_launch(hb, wb, nD, target)
    assert win == 15 or gc.SPLIT_KERNELS[kernel][1] in (5, 35)


@pytest.mark.parametrize("kernel", sorted(gc.SPLIT_KERNELS))
def test_split_references_distinguish(oracle, kernel):
    for case in gc.SPLIT_CASES[kernel]:
        H, W, win, minD, numD, nz, per_z, what = case
        for dt in (0, 1):
            disp, vol = gc.expected_split(oracle, kernel, case, dt)
            assert vol.shape == (numD + 1, H, W) and all(gc.varies(p) for p in vol), (kernel, what, dt)
            assert len(np.unique(disp)) > 1
            slices = np.unique((disp.astype(np.int64) - minD) // per_z)
            assert slices.min() >= 0 and slices.max() < nz
            if nz > 1:
                assert len(slices) >= 2, (kernel, what, dt, slices)


# ---------------------------------------------------------------- StereoBM and the census cost of semi-global matching
def test_bm_table():
    assert sorted(gc.BM_FIRST) == [4, 8, 16, 32, 64]
    for TX, case in gc.BM_FIRST.items():
        H, W, minD, D, w = case
        g = gc.bm_launch(*case)
        assert g["TX"] == TX and H * W <= gc.MAX_PIXELS and W - (minD + D - 1) > 2 * (w // 2), (TX, g)
        if TX > gc.BM_TX_MIN:
            assert gc.bm_launch(H - 1, W, minD, D, w)["TX"] < TX       # the first frame of its value
            assert g["rows_per"] > gc.BM_ROWS_MIN and g["strips"] * g["tiles"] == gc.BM_WAVES_TARGET
        else:
            assert g["rows_per"] == gc.BM_ROWS_MIN
    assert gc.bm_launch(1080, 1920, 0, 64, 15)["TX"] == 16             # the one large frame of the suite before this file


@pytest.mark.parametrize("TX", sorted(gc.BM_FIRST))
def test_bm_references_distinguish(TX):
    case = gc.BM_FIRST[TX]
    want = gc.expected_bm(case)
    FILTERED = 16 * (case[2] - 1)
    found = np.unique(want["disp"][want["disp"] != FILTERED])
    assert len(found) > 1, found
    assert all(len(gc.distinct(p)) >= 2 for p in want["vol"])


def test_census_table():
    rows = {what: gc.census_launch(*case[:5]) for what, case in gc.CENSUS_BY_ROWS.items()}
    for what, case in gc.CENSUS_BY_ROWS.items():   # the rows decide, not the width
        assert rows[what]["want"] == rows[what]["nseg"] == case[5] < rows[what]["by_width"] and case[0] * case[1] <= gc.MAX_PIXELS, what
    one, under = gc.CENSUS_BY_ROWS["one segment by the rows"], gc.CENSUS_LAST_UNDER
    assert under[0] == one[0] - 1 and under[1:5] == one[1:5] and gc.census_launch(*under[:5])["nseg"] == under[5] == 2
    got = {what: gc.census_launch(*case[:5]) for what, case in gc.CENSUS_CASES.items()}
    for what, case in gc.CENSUS_CASES.items():
        assert got[what]["nseg"] == case[5], (what, got[what])
    assert {g["nseg"] for g in got.values()} >= {1, 2} and max(g["nseg"] for g in got.values()) > 8
    assert got["many segments"]["by_width"] == got["many segments"]["nseg"] < got["many segments"]["want"]
    # what the kernel is handed on the frames the GPU runs is what it is handed where the rows decide: candidates a thread, segments
    # a row and grid.y the same, the segment as long within a column
    for small, big in gc.CENSUS_SAME_LAUNCH.items():
        a, b = got[small], rows[big]
        assert (a["spb"], a["nseg"], a["gy"]) == (b["spb"], b["nseg"], b["gy"]) and 0 <= b["seglen"] - a["seglen"] <= 1, (small, a, b)
        assert gc.CENSUS_CASES[small][2:5] == gc.CENSUS_BY_ROWS[big][2:5]


@pytest.mark.parametrize("what", sorted(gc.CENSUS_CASES))
def test_census_references_distinguish(what):
    case = gc.CENSUS_CASES[what]
    H, W, minD, D, w, nseg = case
    want = gc.expected_census(case)
    valid = want["disp"][want["disp"] != 16 * (minD - 1)]
    assert len(np.unique(valid)) > 1
    S = want["S"][:, minD + D:]
    assert all(len(np.unique(S[:, :, d])) >= 2 for d in range(D))
    seglen = gc.census_launch(*case[:5])["seglen"]
    if nseg > 1:  # winners in more than one segment of the valid columns
        ys, xs = np.nonzero(want["disp"][:, minD + D:] != 16 * (minD - 1))
        assert len(np.unique(xs // seglen)) >= 2


# ---------------------------------------------------------------- the capped grids and the natural chunks
def test_capped_grids_and_chunks():
    H, W = gc.DISP_U8_FRAME
    assert gc.DISP_U8_CAP < H * W < gc.DISP_U8_CAP + 64 * W and gc.disp_u8_blocks(H * W) == 1024 == gc.disp_u8_blocks(gc.DISP_U8_CAP)
    assert (gc.DISP_U8_ROW - 2) * W >= gc.DISP_U8_CAP
    assert gc.disp_u8_blocks(gc.DISP_U8_CAP - 2048) == 1023
    for (H, W), mod4 in zip(gc.SLICE_SCALES_FRAMES, (True, False)):
        assert gc.SLICE_SCALES_CAP < H * W < gc.SLICE_SCALES_CAP + 2 * W and (H * W % 4 == 0) == mod4
        assert gc.slice_scales_blocks(H * W) == 64
    assert gc.slice_scales_blocks(360 * 640) == 57 and gc.u8_scale_blocks(1080 * 1920 * 3) == 380
    assert gc.u8_scale_blocks(gc.MAX_PIXELS * 3) < 1024        # not reached under 2^21 pixels
    assert gc.U8_SCALE_CAP // 3 + 1 > gc.MAX_PIXELS
    # the natural chunk sizes: more than one chunk from about 0.9 * 2^28 cost values (permeability) and 699 051 pixels at 35x35
    # (weighted median) on; at 15x15 only past 2^21 pixels
    assert gc.perm_chunk(1080, 1920, 128) == 64 and gc.perm_chunk(1024, 2048, 115) == 115 and gc.perm_chunk(1024, 2048, 116) == 64
    assert gc.perm_chunk(512, 1024, 476) == 476 and gc.perm_chunk(512, 1024, 477) == 448
    for H, W, n in ((375, 450, 64), (1080, 1920, 64), (32, 2048, 3000), (8, 8192, 3630)):
        assert gc.perm_chunk(H, W, n) == n and H * W * n < 0.9 * (1 << 28), (H, W, n)
    H, W, minD, n, sigma, trunc = gc.PERM_NATURAL
    chunk = gc.perm_chunk(H, W, n)
    assert chunk == 448 < n and H * W <= gc.MAX_PIXELS and gc.PERM_PLANES == (0, chunk - 1, chunk, n - 1)
    assert gc.wmedian_chunk(1080, 1920, 15, 64) == 16 and gc.wmedian_chunk(1024, 2048, 15, 64) == 16 and gc.wmedian_chunk(1024, 2048, 15, 16) == 16
    assert gc.wmedian_chunk(1673, 1672, 15, 9) == 8 and gc.wmedian_chunk(1448, 1448, 15, 9) == 9          # past 2^21 pixels only
    assert gc.wmedian_chunk(700, 1000, 35, 9) == 8 and gc.wmedian_chunk(836, 836, 35, 9) == 8 and gc.wmedian_chunk(500, 1000, 35, 9) == 9
    H, W, win, minD, n = gc.WMEDIAN_NATURAL
    assert gc.wmedian_chunk(H, W, win, n) == 8 < n and gc.wmedian_chunk(H - 8, W, win, n) == n and H * W <= gc.MAX_PIXELS
    assert gc.WMEDIAN_MARGIN == win // 2 + 1 < gc.WMEDIAN_BAND
    assert set(gc.NOT_REACHED) == {"launch_u8_scale past its cap", "the weighted median's natural list chunk at 15x15"}


def test_wmedian_band_references(oracle):
    """the oracle on a row band agrees with the oracle on the frame from WMEDIAN_MARGIN rows off the cut on (shown on a frame the
    oracle can afford whole), and in the bands of the natural-chunk frame the winners come from both list chunks"""
    H, W, win, minD, n = 90, 48, gc.WMEDIAN_NATURAL[2], 0, gc.WMEDIAN_NATURAL[4]
    L, R = gc.band_pair(H, W, n, 35, band=4)
    B, m = gc.WMEDIAN_BAND, gc.WMEDIAN_MARGIN
    rc, d, v = oracle.asw_wmedian(L, R, 0, win, 10, 10, minD, n, want_vol=True)
    rc, dt, vt = oracle.asw_wmedian(L[:B], R[:B], 0, win, 10, 10, minD, n, want_vol=True)
    rc, db, vb = oracle.asw_wmedian(L[H - B:], R[H - B:], 0, win, 10, 10, minD, n, want_vol=True)
    assert np.array_equal(vt[:, :B - m], v[:, :B - m]) and np.array_equal(dt[:B - m], d[:B - m])
    assert np.array_equal(vb[:, m:], v[:, H - B + m:]) and np.array_equal(db[m:], d[H - B + m:])
    assert not np.array_equal(vt[:, :B - m + 3], v[:, :B - m + 3])     # and not from three rows nearer: the margin is no wider than needed
    chunk = gc.wmedian_chunk(*gc.WMEDIAN_NATURAL[:3], n)
    for rows, dm, vol in gc.expected_wmedian_bands(oracle):
        assert rows.stop - rows.start == B - m and all(gc.varies(p) for p in vol)
        assert (dm - minD < chunk).any() and (dm - minD >= chunk).any()


@pytest.mark.parametrize("H,W", gc.SLICE_SCALES_FRAMES)
def test_slice_scales_reference_has_its_extreme_past_the_cap(oracle, H, W):
    L, R = gc.slice_scales_pair(H, W)
    win, minD, numD = gc.SLICE_SCALES_NCC
    rc, raw = oracle.cost_ncc(L, R, 0, win, minD, numD, raw=True)
    p = raw[0].ravel()
    assert rc == 0 and np.nanmax(p[gc.SLICE_SCALES_CAP:]) > np.nanmax(p[:gc.SLICE_SCALES_CAP])
    rc, norm = oracle.cost_ncc(L, R, 0, win, minD, numD)
    assert all(len(gc.distinct(q)) >= 2 for q in norm)


def test_disp_u8_reference_has_its_maximum_past_the_cap(oracle):
    d = gc.expected_disp_u8_map(oracle).ravel()
    win, minD, numD = gc.DISP_U8_MATCH
    assert gc.DISP_U8_TOP == minD + numD and d.max() == gc.DISP_U8_TOP and d.min() == minD
    assert d[:gc.DISP_U8_CAP].max() < gc.DISP_U8_TOP        # normalize's scale is wrong if the grid's last round is lost
    assert len(np.unique(d)) > 2
    for norm in (False, True):
        assert len(np.unique(oracle.disparity_to_u8(d.reshape(gc.DISP_U8_FRAME), norm))) > 2


def test_similarity_parameter_grid_two_restatements_agree(oracle):
    """the oracle and the literal second restatement over tests/cvlite.py (tests/similarity_ref.py, M.cpp:415-487 line by line) at every value
    of the grid: what the GPU is compared with there does not rest on one reading of the two double comparisons"""
    from similarity_ref import similarity_literal
    L, R = gc.param_pair()
    H, W, minD, numD = gc.PARAM_FRAME
    for r in gc.REGULARITY:
        for c in gc.THRES_C:
            for g in gc.THRES_G:
                rc, v = oracle.compute_similarity(L, R, r, c, g, 0, minD, numD)
                assert rc == 0 and np.array_equal(v, similarity_literal(L, R, r, c, g, minD, numD)), (r, c, g)
