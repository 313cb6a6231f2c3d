"""CPU-side checks of tests/window_cases.py, on the oracle alone (no GPU needed): the non-vacuity test of
tests/test_gpu_large_windows.py.

A volume comparison at window w proves that the kernel ran window w only if the oracle's volume at w is not the volume of a smaller
window: for every case on the (6, 90) frame, the volume differs from the volume of the method's previous listed window (the next
one for the first), on the same pair, in at least 99 % of the entries that are finite in both -- measured 100 % on every textured
pair, and printed here.  A comparison also needs finite entries to compare, and the GPU tests stay quick only while every oracle
call stays below 2 s.  A case that misses a condition is replaced, never dropped."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asw_cases as ac  # noqa: E402
import window_cases as wc  # noqa: E402

ORACLE_SECONDS = 2.0
DIFFERENT_SHARE = 0.99


def _timed(oracle, case):
    t0 = time.perf_counter()
    want = wc.reference(oracle, case)
    return want, time.perf_counter() - t0


def test_the_tables_hold_what_they_are_meant_to():
    assert set(wc.LIMITS) == set(wc.RUN_METHODS) | {"wmedian", "geodesic", "geodist"} and len(wc.LIMITS) == 11
    for m, (last, refused, status, source) in wc.LIMITS.items():
        assert refused == last + (1 if m == "guided2" else 2) and refused % 2 == 1 and status == wc.ERR_BAD_ARGUMENT and source, m
    for m, wins in wc.FORM_WINDOWS.items():
        assert list(wins) == sorted(set(wins)) and wins[-1] == wc.LIMITS[m][0], m            # the last served window runs
        assert all(w % 2 == 1 for w in wins) or m == "guided2", m
    assert wc.FORM_WINDOWS["classic"] == wc.FORM_WINDOWS["direct8"] == (29, 31, 37, 61, 63)
    assert wc.FORM_WINDOWS["blo1"] == (23, 25, 49, 51, 63) and wc.FORM_WINDOWS["guided2"] == (36, 37, 63, 64)
    assert wc.FRAMES == ((6, 90, 0), (3, 20, 0), (9, 130, 5))
    runs = wc.run_ids()
    assert len(runs) == sum(len(w) + 4 for w in wc.FORM_WINDOWS.values())                   # every window once, the extremes on two more frames
    for m in wc.RUN_METHODS:
        all_cases = [c for (mm, w, f) in runs if mm == m for c in wc.cases(m, w, f)]
        assert {c["dt"] for c in all_cases} == set(wc.directions(m)), m
        assert {c["kind"] for c in all_cases} == {"textured", "periodic"} and {c["numD"] for c in all_cases} == {5, 18}, m
        assert {c["minD"] for c in all_cases} == ({0} if m == "blo1" else {0, 3}), m
        assert {c["params"] for c in all_cases} == {wc.TABLE_PARAMS[m]}, m
        assert any(c["L"].strides[0] > c["L"].shape[1] * 3 for c in all_cases), m            # padded rows
        for c in all_cases:
            again = ac.build_case(m, c["tag"])
            assert np.array_equal(again["L"], c["L"]) and np.array_equal(again["R"], c["R"]) and again["win"] == c["win"], c["tag"]


def test_limits_follow_from_the_launchers_expressions():
    derived = wc.derived_limits()
    assert set(derived) == set(wc.RUN_METHODS)
    for m, last in derived.items():
        assert wc.LIMITS[m][0] == last, m
    # the figures the table quotes, and the switches the listed windows straddle
    assert (wc.bilateral_lds(63), wc.bilateral_lds(65)) == (160160, 166912)
    assert (wc.bilateral_lds(29), wc.bilateral_lds(31)) == (62656, 67360) and wc.bilateral_lds(29) <= 64 * 1024 < wc.bilateral_lds(31)
    assert (wc.ncc_lds(59), wc.ncc_lds(61)) == (64232, 67328)
    assert [wc.blo1_chunk(w) for w in wc.FORM_WINDOWS["blo1"]] == [4, 2, 2, 1, 1]
    assert wc.blo1_lds(133, 1) <= wc.LDS_PER_WORKGROUP < wc.blo1_lds(135, 1)
    assert 45 * 45 <= 2048 < 47 * 47                                                        # the weighted median's slots


def test_sad_d_views_border_the_other_view():
    case = wc.cases("sad", 37, (3, 20, 0))[0]
    L, Rb, d = wc.sad_d_views(case, 2)
    max_off = case["minD"] + case["numD"] - 1
    assert d == case["minD"] + 2 and L is case["L"] and Rb.shape[1] == 20 + max_off
    assert np.array_equal(Rb[:, max_off:], case["R"]) and np.array_equal(Rb[:, max_off - 1], case["R"][:, 0])
    right = [c for c in wc.cases("sad", 37, (3, 20, 0)) if c["dt"] == wc.RIGHT][0]
    Lb, R, d = wc.sad_d_views(right, 0)
    assert R is right["R"] and np.array_equal(Lb[:, :20], right["L"]) and np.array_equal(Lb[:, 20], right["L"][:, 19])
    assert Lb.shape[1] == 20 + 17 and np.array_equal(Lb[:, 36], right["L"][:, 3])           # hgfedcb: column 2 * 20 - 1 - 36


@pytest.mark.parametrize("method", wc.RUN_METHODS)
def test_every_window_has_a_volume_of_its_own(oracle, method):
    wins = wc.FORM_WINDOWS[method]
    slowest, lowest = 0.0, 1.0
    vols = {}
    for win in wins:
        for frame in wc.frames(method, win):
            for case in wc.cases(method, win, frame):
                want, dt = _timed(oracle, case)
                slowest = max(slowest, dt)
                assert dt < ORACLE_SECONDS, (case["tag"], dt)
                vol = want["vol"]
                planes = case["numD"] if method == "sad" else ac.planes(method, case["numD"])
                assert vol.shape == (planes,) + case["L"].shape[:2], case["tag"]
                assert np.isfinite(vol).any(), case["tag"]
                if frame == wc.FRAMES[0]:
                    vols[case["tag"]] = vol
    for tag, vol in vols.items():
        win = tag[3]
        i = wins.index(win)
        other = list(tag)
        other[3] = wins[i - 1] if i > 0 else wins[1]
        prev = vols[tuple(other)]
        both = np.isfinite(vol) & np.isfinite(prev)
        if tag[0] == "periodic":
            # a candidate congruent to the pair's shift matches exactly, at a cost of 0 whatever the window: those planes cannot
            # tell two windows apart, and the claim is made of the others
            p, shift = wc.periodic_parameters(tag[9])
            exact = np.array([(tag[4] + k) % p == shift % p for k in range(vol.shape[0])])
            assert 0 < exact.sum() < vol.shape[0], tag
            both[exact] = False
        assert both.any(), tag
        share = float((vol[both] != prev[both]).mean())
        lowest = min(lowest, share)
        assert share >= DIFFERENT_SHARE, (tag, other[3], share)
    print("%s: slowest oracle call %.2f s, lowest share of entries that differ from the neighbouring window %.4f" % (method, slowest, lowest))


@pytest.mark.parametrize("method", [m for m in wc.LIMITS if m not in ("sad", "geodist")])
def test_small_case_after_a_refusal_is_served_by_the_oracle(oracle, method):
    case = wc.small_case(method)
    want, dt = _timed(oracle, case)
    assert dt < ORACLE_SECONDS and np.isfinite(want["vol"]).any() and want["disp"].shape == (6, 40), (case["tag"], dt)
    ac.check(case, want, want)
