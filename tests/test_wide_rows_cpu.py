"""The width table of tests/wide_cases.py and the references of tests/test_gpu_wide_rows.py, on the CPU alone.

Table position: every width sits on the side of 64 KB and of 160 KB of dynamic LDS that its label names, under the two budgets
restated from launch_cost_ad (k_basic.hip) and launch_cost_census (k_census.hip); each "last" / "first" pair differs by one; the
number of passes of the x4 loop is the one the label claims.  Non-vacuity: what the GPU file compares against has something to
distinguish past column 1024 -- at least two values in every plane of every expected cost volume, more than one disparity and a
region larger than its pixel in every expected matcher result.  Agreement at width: the loop form and the vectorised form of
tests/adcensus_ref.py, which the narrow tests of tests/test_adcensus_cpu.py compare, agree on a row that takes two passes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adcensus_ref as ac  # noqa: E402
import wide_cases as wc  # noqa: E402

FORMS = sorted(wc.FORMS)


# ---------------------------------------------------------------- the table
def test_budgets():
    """the two formulas at the workload's width and at the figures DESIGN.md section 4.13 gives"""
    assert wc.ad_lds(1920, 3) == 11520 and wc.ad_lds(1920, 1) == 3840
    assert wc.census_lds(1920, 3) == 22 * 1920 + 320 and wc.census_lds(1920, 1) == 18 * 1920 + 320 and wc.census_lds(1920, 0) == 16 * 1920
    assert wc.LDS_64K < wc.census_lds(3840, 3) == 84800 < wc.LDS_LIMIT  # a 3840-column AD-Census call lies between the two lines
    assert wc.PASS_PIXELS == 256 * 4 and (wc.LDS_64K, wc.LDS_LIMIT) == (65536, 163840)


def test_passes_widths():
    assert [w for w, _, _, _ in wc.PASSES] == [1023, 1024, 1025, 1028, 1920, 2049]
    for W, n, H, _ in wc.PASSES:
        assert wc.passes(W) == n == (W + 1023) // 1024 and 1 <= H <= 5
        for form in FORMS:
            assert wc.form_lds(form, W) < 48 * 1024, (form, W)  # well under 64 KB
    by_w = {w: (n, h) for w, n, h, _ in wc.PASSES}
    assert by_w[1025][0] == 2 and 1025 - 1024 == 1 and 1025 % 4        # byte stores, one pixel in the second pass
    assert by_w[1028][0] == 2 and 1028 - 1024 == 4 and 1028 % 4 == 0   # dword rows, one group in the second pass
    assert by_w[2049][0] == 3
    assert by_w[1025][1] == 5 and by_w[1028][1] == 5  # enough rows under a narrow overhang for the non-vacuity conditions


@pytest.mark.parametrize("form", FORMS)
def test_64k_line(form):
    last, first, next4 = wc.LINE_64K[form]
    assert wc.form_lds(form, last) <= wc.LDS_64K < wc.form_lds(form, first) and first == last + 1
    assert next4 > first and next4 % 4 == 0 and all(w % 4 for w in range(first + 1, next4))
    assert wc.LDS_64K < wc.form_lds(form, next4) <= wc.LDS_LIMIT
    assert wc.passes(last) >= 3
    if form == "hamming":
        assert wc.form_lds(form, last) == wc.LDS_64K


@pytest.mark.parametrize("form", FORMS)
def test_160k_line(form):
    last, first = wc.LINE_160K[form]
    assert wc.form_lds(form, last) <= wc.LDS_LIMIT < wc.form_lds(form, first) and first == last + 1
    assert wc.LINE_64K[form][2] < last


def test_case_lists_cover_the_table():
    low = {(k, W, cn, dt) for k, H, W, cn, dt, minD, D in wc.COST_CASES_LOW if minD == wc.MIN_D}
    assert low == {(k, W, cn, dt) for k in ("ad", "census") for W, _, _, _ in wc.PASSES for cn in (1, 3) for dt in (0, 1)}
    assert sorted(minD - W for k, H, W, cn, dt, minD, D in wc.COST_CASES_LOW if minD != wc.MIN_D) == [-5] * 4
    high = {(k, W, dt) for k, H, W, cn, dt, minD, D in wc.COST_CASES_HIGH}
    assert high == {(form, W, dt) for form in FORMS for W in wc.LINE_64K[form] for dt in (0, 1)}
    for k, H, W, cn, dt, minD, D in wc.COST_CASES_LOW + wc.COST_CASES_HIGH:
        assert 1 <= H <= 5 and (minD, D) in ((wc.MIN_D, wc.NUM_D), (W - 5, wc.NUM_D)) and (wc.MIN_D, wc.NUM_D) == (3, 17)
        if k in wc.FORMS:
            assert cn == wc.FORMS[k][2]
    assert {H for k, H, W, cn, dt, minD, D in wc.COST_CASES_LOW if k == "census"} >= {1, 5}
    # every launch of the "low" lists stays under 64 KB, every case of the "high" matcher lists is over it
    for k, H, W, cn, dt, minD, D in wc.COST_CASES_LOW:
        assert max(wc.ad_lds(W, cn), wc.census_lds(W, cn)) <= wc.LDS_64K
    for H, W, cn, win, minD, D, dt in wc.ADCENSUS_MATCH_LOW:
        assert wc.census_lds(W, cn) <= wc.LDS_64K
    for H, W, cn, win, minD, D, dt in wc.ADCENSUS_MATCH_HIGH:
        assert wc.LDS_64K < wc.census_lds(W, cn) <= wc.LDS_LIMIT
    for H, W, cn, win, minD, D, dt in wc.CROSS_MATCH_LOW:
        assert wc.ad_lds(W, cn) <= wc.LDS_64K
    for H, W, cn, win, minD, D, dt in wc.CROSS_MATCH_HIGH:
        assert wc.LDS_64K < wc.ad_lds(W, cn) <= wc.LDS_LIMIT
    assert [(f, a, r) for f, H, a, r, dt in wc.LIMIT_CASES] == [(f,) + wc.LINE_160K[f] for f in wc.AD_FORMS + wc.CENSUS_FORMS]
    assert all(H in (1, 2) for f, H, a, r, dt in wc.LIMIT_CASES) and wc.LIMIT_NUM_D == 2
    # winnerTakeAll: one pixel under the switch, the vector branch, the scalar branch
    (h0, w0, _), (h1, w1, _), (h2, w2, _) = wc.WTA_CASES
    assert h0 * w0 == wc.WTA_SWITCH - 1 and h1 * w1 == wc.WTA_SWITCH and h2 * w2 > wc.WTA_SWITCH and (h2 * w2) % 4 and wc.WTA_N == 3


# ---------------------------------------------------------------- non-vacuity, on the references alone
def _wide_columns_vary(name, vol):
    tail = vol[:, :, wc.PASS_PIXELS:]
    for k in range(tail.shape[0]):
        assert len(np.unique(tail[k])) >= 2, "%s plane %d holds one value past column %d" % (name, k, wc.PASS_PIXELS)


@pytest.mark.parametrize("case", wc.COST_CASES_LOW + wc.COST_CASES_HIGH, ids=lambda c: "-".join(map(str, c)))
def test_expected_costs_vary_past_column_1024(oracle, case):
    kernel, H, W, cn, dt, minD, D = case
    L, R = wc.cost_pair(H, W, cn, dt)
    assert L.shape[:2] == (H, W) and L.dtype == np.uint8 and (L.ndim == 3) == (cn == 3)
    want = wc.expected_costs(oracle, kernel, L, R, dt, minD, D)
    assert set(want) == ({"AD", "TAD", "SD"} if wc.is_ad_kernel(kernel) else {"Census"} if kernel == "hamming" else {"Census", "ADCensus"})
    for name, vol in want.items():
        assert vol.shape == (D, H, W) and vol.dtype == np.uint8
        if W > wc.PASS_PIXELS:  # 1023 and 1024 have no such column: they are the cases a value-only fault past it leaves alone
            _wide_columns_vary(name, vol)
    if "TAD" in want:
        assert set(np.unique(want["TAD"])) == {0, 255}
    if "Census" in want and W > wc.PASS_PIXELS:
        assert want["Census"][:, :, wc.PASS_PIXELS:].max() >= (55 if W >= 1920 else 40)  # Hamming distances up to about 60
    if "ADCensus" in want and W > wc.PASS_PIXELS:
        assert want["ADCensus"][:, :, wc.PASS_PIXELS:].max() > 127


@pytest.mark.parametrize("form,H,accepted,refused,dt", wc.LIMIT_CASES)
def test_expected_costs_at_the_limit_vary(oracle, form, H, accepted, refused, dt):
    L, R = wc.cost_pair(H, accepted, wc.FORMS[form][2], dt)
    for name, vol in wc.expected_costs(oracle, form, L, R, dt, wc.LIMIT_MIN_D, wc.LIMIT_NUM_D).items():
        _wide_columns_vary(name, vol)


def _matcher_varies(N, disp):
    assert len(np.unique(disp[:, wc.PASS_PIXELS:])) > 1 and N[:, wc.PASS_PIXELS:].max() > 1


@pytest.mark.parametrize("H,W,cn,win,minD,D,dt", wc.ADCENSUS_MATCH_LOW + wc.ADCENSUS_MATCH_HIGH)
def test_expected_adcensus_matches_vary(H, W, cn, win, minD, D, dt):
    L, R = wc.region_pair(H, W, cn, D)
    S, N, E, disp = wc.expected_adcensus(L, R, dt, win, minD, D)
    _matcher_varies(N, disp)


@pytest.mark.parametrize("H,W,cn,win,minD,D,dt", wc.CROSS_MATCH_LOW + wc.CROSS_MATCH_HIGH)
def test_expected_cross_matches_vary(oracle, H, W, cn, win, minD, D, dt):
    L, R = wc.region_pair(H, W, cn, D)
    S, N, E, disp = wc.expected_cross(oracle, L, R, dt, win, minD, D)
    _matcher_varies(N, disp)


def test_matcher_case_shapes():
    assert [c[:6] for c in wc.ADCENSUS_MATCH_LOW] == [(34, 1920, 3, 15, 0, 17)] * 2 and [c[6] for c in wc.ADCENSUS_MATCH_LOW] == [0, 1]
    assert [(c[:4], c[5]) for c in wc.ADCENSUS_MATCH_HIGH] == [((6, 2968, 3, 7), 5), ((5, 3628, 1, 3), 3)]
    assert [c[:6] for c in wc.CROSS_MATCH_LOW] == [(34, 1920, 3, 15, 0, 17)] * 2 and [c[6] for c in wc.CROSS_MATCH_LOW] == [0, 1]
    assert [(c[:4], c[5]) for c in wc.CROSS_MATCH_HIGH] == [((3, 10924, 3, 7), 3)]


def test_wta_volumes_hold_the_special_columns(oracle):
    for H, W, _ in wc.WTA_CASES:
        vol = wc.wta_volume(H, W, H)
        flat = vol.reshape(wc.WTA_N, -1)
        want = oracle.wta(vol, 3).reshape(-1)
        for base in (0, (H - 1) * W):
            assert np.isnan(flat[:, base]).all() and (flat[:, base + 1] == 0.5).all() and np.isposinf(flat[0, base + 2])
            assert np.isposinf(flat[:, base + 3]).all() and np.isneginf(flat[1:, base + 4]).all()
            # never-selected columns give 0 (not min_d), ties the lowest d, -inf wins once
            assert want[base] == 0 and want[base + 1] == 3 and want[base + 2] in (4, 5) and want[base + 3] == 0 and want[base + 4] == 4
        end = H * W
        assert np.isposinf(flat[0, end - 5]) and np.isnan(flat[:, end - 4]).all() and (flat[:, end - 3] == 0.5).all()
        assert np.isposinf(flat[:, end - 2]).all() and np.isneginf(flat[1:, end - 1]).all()
        assert list(want[end - 4:]) == [0, 3, 0, 4] and want[end - 5] in (4, 5)
        s = np.sort(vol[:, 2:H - 2:2], axis=0)  # the quantised rows
        assert 0.05 < (s[0] == s[1]).mean() < 0.5 and set(np.unique(want)) == {0, 3, 4, 5}


# ---------------------------------------------------------------- the two forms of the restatement, at width
@pytest.mark.parametrize("cn,dt,minD", [(3, 0, 3), (1, 1, 1025)])
def test_adcensus_loop_and_vectorised_forms_agree_on_a_wide_row(cn, dt, minD):
    H, W, D = 3, 1030, 3
    L, R = wc.cost_pair(H, W, cn, dt)
    ham, adv, e = ac.cost_loop(L, R, dt, wc.LAMBDA_AD, wc.LAMBDA_CENSUS, minD, D)
    assert np.array_equal(ham, ac.hamming(L, R, dt, minD, D))
    assert np.array_equal(adv, ac.ad(L, R, dt, minD, D))
    assert np.array_equal(e, ac.cost(L, R, dt, wc.LAMBDA_AD, wc.LAMBDA_CENSUS, minD, D))
    gA = ac.gray_pair(L, R)[0]
    assert np.array_equal(np.array(ac.census_loop(gA), dtype=np.uint64), ac.census(gA))
