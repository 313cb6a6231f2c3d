"""CPU-side checks of tests/asw_cases.py, on the oracle alone (no GPU needed): the non-vacuity test of tests/test_gpu_asw_ties.py
and tests/test_gpu_asw_sweep.py.

A tie-table row proves something about a reduction stage only if the oracle's volume really has bit-equal minima on it and the
winner is not simply the first candidate; an equal map means something only if the oracle's own map follows the stated winner rule;
and a printed tag is worth something only if it rebuilds the case.  Measured here (8 threads), tie share / share of pixels whose
winner is not minD, over the methods and directions that run a row: see the comments of the tables in tests/asw_cases.py, which this
file measures again and prints."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asw_cases as ac  # noqa: E402

TABLE_METHODS = [m for m in ac.METHODS if m != "bilgrid"]


def _shares(oracle, case):
    want = ac.reference(oracle, case)
    vol = want["vol"][:ac.wta_planes(case["method"], case["numD"])]
    return ac.tie_share(vol, 0), float((want["disp"] != case["minD"]).mean()), want


def _map_follows_the_rule(case, want):
    """the oracle's map against the arg-min of its own volume: first strict minimum in ascending d, NaN never selected, 0 where
    nothing is selected"""
    m, minD = case["method"], case["minD"]
    vol = want["vol"][:ac.wta_planes(m, case["numD"])]
    if m == "ncc" and case["dt"] == ac.RIGHT:
        return bool((want["disp"] == 0).all())          # the reference's RIGHT branch never writes (M.cpp:896)
    first = ac.first_strict_minimum(vol, minD) if vol.shape[0] else np.zeros(want["disp"].shape, np.float32)
    if m != "ncc":
        return np.array_equal(first, want["disp"])
    # NCC compares its costs in f64 and the volume holds them rounded to f32: rounding is monotone, so the map's cost is still a
    # minimum of the f32 plane stack, but two f64 costs that differ may round to one f32 value, and then the first minimum of
    # the volume may come before the map's
    sel = first != 0
    k = np.clip(want["disp"].astype(np.int64) - minD, 0, max(vol.shape[0] - 1, 0))[None]
    at = np.take_along_axis(vol, k, axis=0)[0] if vol.shape[0] else first
    floor = np.where(np.isnan(vol), np.inf, vol).min(axis=0) if vol.shape[0] else first
    return bool((first <= want["disp"]).all() and (at[sel] == floor[sel]).all())


@pytest.mark.parametrize("method", TABLE_METHODS)
def test_tie_table_rows_tie_and_move_the_winner(oracle, method):
    cases = ac.tie_cases(method)
    assert len(cases) == len(ac.tie_rows(method)) * len(ac.directions(method)) > 0
    for case in cases:
        kind, dt = case["kind"], case["dt"]
        ties, moved, want = _shares(oracle, case)
        print("%s %s dt %d: tie share %.3f, winner not minD %.3f" % (method, case["tag"][:6], dt, ties, moved))
        assert want["vol"].shape == (ac.planes(method, case["numD"]),) + case["L"].shape[:2], case["tag"]
        assert ties >= ac.TIE_FLOOR, (case["tag"], ties)
        if kind[2] > 0 and not (method == "ncc" and dt == ac.RIGHT):   # NCC's RIGHT map is never written: nothing to move
            assert moved >= ac.MOVED_FLOOR, (case["tag"], moved)
        assert _map_follows_the_rule(case, want), case["tag"]


@pytest.mark.parametrize("method", ["classic", "geodesic"])
def test_row_constant_pair_ties_everywhere(oracle, method):
    for dt in ac.directions(method):
        case = ac.row_constant_case(method, dt)
        ties, moved, want = _shares(oracle, case)
        print("%s row_constant dt %d: tie share %.3f, winner not minD %.3f" % (method, dt, ties, moved))
        assert ties >= 0.9 and _map_follows_the_rule(case, want)


def test_the_table_holds_the_rows_it_is_meant_to():
    assert len(ac.ONE_KERNEL_ROWS) == 4 and len(ac.XQ_ROWS) == 7
    assert {r[4] for r in ac.ONE_KERNEL_ROWS} == {3, 5, 7} and {r[4] for r in ac.XQ_ROWS} == {15}
    assert {r[4] for r in ac.WMEDIAN_TILE_ROWS} == {15, 17}
    assert ac.tie_rows("bilgrid") == []
    assert all(r[5] == 0 for r in ac.tie_rows("blo1")) and len(ac.tie_rows("blo1")) == 3
    assert len(ac.tie_rows("classic")) == len(ac.tie_rows("geodesic")) == 11 and len(ac.tie_rows("direct8")) == 4
    assert len(ac.tie_cases("classic")) == 22 and len(ac.tie_cases("direct8")) == 4 and len(ac.tie_cases("wmedian")) == 6
    assert ac.tie_rows("ncc")[1] != ac.ONE_KERNEL_ROWS[1] and len(ac.tie_rows("ncc")) == 4     # replaced, not dropped
    for m in ac.TOLERANCE:
        assert ac.tie_rows(m) == ac.GUIDED_ROWS
    L, R = ac.periodic_same(5, 40, 3, 8)
    assert np.array_equal(L, R) and np.array_equal(L[:, 8:40], L[:, :32]) and L.shape == (5, 40, 3)


def test_first_strict_minimum_is_the_winner_rule():
    nan, inf = np.nan, np.inf
    #                x = 0: tie      1: NaN first   2: all NaN   3: +inf only   4: -inf      5: later strict minimum
    vol = np.array([[[2, nan, nan, inf, 1, 3]], [[1, 5, nan, inf, -inf, 2]], [[1, 4, nan, nan, -inf, 1]]], np.float32)
    assert np.array_equal(ac.first_strict_minimum(vol, 0), [[1, 2, 0, 0, 1, 2]])
    assert np.array_equal(ac.first_strict_minimum(vol, 7), [[8, 9, 0, 0, 8, 9]])


def _same_case(a, b):
    return a["tag"] == b["tag"] and all(np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)


@pytest.mark.parametrize("method", ac.METHODS)
def test_random_case_is_deterministic_and_rebuilds_from_its_tag(method):
    first, second = ac.cases(method, ac.SWEEP_SEEDS[0]), ac.cases(method, ac.SWEEP_SEEDS[0])
    assert len(first) == ac.SWEEP_COUNT and len({c["tag"] for c in first}) == ac.SWEEP_COUNT
    for a, b in zip(first, second):
        assert _same_case(a, b) and _same_case(a, ac.build_case(method, a["tag"]))
        assert a["L"].shape == a["R"].shape == (a["tag"][1], a["tag"][2], 3) and a["L"].dtype == np.uint8
    assert ac.cases(method, ac.SWEEP_SEEDS[1])[0]["tag"] != first[0]["tag"]
    drawn = ac.random_case(np.random.default_rng(3), method)      # no index: everything is drawn
    assert _same_case(drawn, ac.build_case(method, drawn["tag"]))


def _sweep(method):
    return [c for seed in ac.SWEEP_SEEDS for c in ac.cases(method, seed)]


@pytest.mark.parametrize("method", ac.METHODS)
def test_sweep_draws_what_the_method_serves_and_all_of_it(method):
    cases = _sweep(method)
    met = {(c["kind"], c["dt"]) for c in cases}
    assert met == {(k, d) for k in ac.KINDS for d in ac.directions(method)}
    for c in cases:
        kind, H, W, win, minD, numD, dt, params, pad, seed = c["tag"]
        assert 1 <= H <= 40 and 1 <= numD <= 200 and minD >= 0 and len(params) == len(ac.TABLE_PARAMS[method]), c["tag"]
        xq = method in ("classic", "geodesic") and win == 15 and numD >= 63 and W >= 64
        assert 1 <= W <= (300 if xq else 160), c["tag"]
        assert win in ac.WINDOWS or (method == "guided2" and win - 1 in ac.WINDOWS), c["tag"]
        assert dt == ac.LEFT or ac.SERVES_RIGHT[method], c["tag"]
        assert method != "blo1" or minD == 0, c["tag"]
        assert method != "wmedian" or win <= 45, c["tag"]
        assert numD <= 47 or xq or (H <= 24 and W <= 96), c["tag"]
    if method in ("classic", "geodesic"):
        forced = [c for c in cases if c["win"] == 15 and c["numD"] >= 63 and c["L"].shape[1] >= 64]
        assert len(forced) >= 2 * (ac.SWEEP_COUNT // 8), len(forced)
        assert {c["dt"] for c in forced} == {ac.LEFT, ac.RIGHT}
    if method == "guided2":
        assert any(c["win"] % 2 == 0 for c in cases)


def test_sweep_includes_the_degenerate_sizes():
    cases = [c for m in ac.METHODS for c in _sweep(m)]
    assert len(cases) == len(ac.METHODS) * len(ac.SWEEP_SEEDS) * ac.SWEEP_COUNT
    count = lambda f: sum(1 for c in cases if f(c))
    found = {"win == 1": count(lambda c: c["win"] == 1), "H == 1": count(lambda c: c["L"].shape[0] == 1),
             "W == 1": count(lambda c: c["L"].shape[1] == 1), "numD > W": count(lambda c: c["numD"] > c["L"].shape[1]),
             "minD > 0": count(lambda c: c["minD"] > 0), "numD >= 48": count(lambda c: c["numD"] >= 48),
             "padded rows": count(lambda c: c["L"].strides[0] > c["L"].shape[1] * 3)}
    print(found)
    assert all(n >= 1 for n in found.values()), found


@pytest.mark.parametrize("method", ac.METHODS)
def test_oracle_accepts_the_sweep_and_its_maps_follow_the_rule(oracle, method):
    # one case of every kind (the first seven of the first seed): shapes, and the winner rule on volumes with NaN planes
    for case in ac.cases(method, ac.SWEEP_SEEDS[0])[:len(ac.KINDS)]:
        want = ac.reference(oracle, case)
        assert want["disp"].shape == case["L"].shape[:2] and want["disp"].dtype == np.float32, case["tag"]
        assert want["vol"].shape == (ac.planes(method, case["numD"]),) + case["L"].shape[:2], case["tag"]
        assert _map_follows_the_rule(case, want), case["tag"]
        ac.check(case, want, want)
