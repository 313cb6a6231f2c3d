"""The confidence rule on the CPU (tests/confidence_ref.py): its two restatements against each other and
against hand-written answers for every branch, the properties the header promises (range, sign of zero, no NaN, power-of-two
scaling), that the measure separates right from wrong disparities on the CPU oracle's volumes, and that the header and the Python
signatures carry the feature.  No GPU."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import confidence_ref as cr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def col(*values):
    """one pixel's column as a volume [n][1][1]"""
    return np.array(values, np.float32).reshape(-1, 1, 1)


def both(V):
    a, b = cr.confidence_vec(V), cr.confidence_loop(V)
    assert cr.same_bits(a, b)
    return a


def one(*values):
    return float(both(col(*values))[0, 0])


# ---------------------------------------------------------------- the two forms agree
@pytest.mark.parametrize("n", range(1, 10))
def test_the_two_forms_are_bit_equal(n):
    rng = np.random.default_rng(900 + n)
    hit = {"nan": 0, "inf": 0, "tie": 0, "zero": 0, "positive": 0}
    for _ in range(6):
        V = cr.random_volume(rng, n, 9, 13)
        c = both(V)
        hit["nan"] += int(np.isnan(V).any())
        hit["inf"] += int(np.isinf(V).any())
        lo = np.where(np.isfinite(V), V, INF)
        hit["tie"] += int(((lo == lo.min(axis=0)) & np.isfinite(V)).sum(axis=0).max() > 1)
        hit["zero"] += int((c == 0).any())
        hit["positive"] += int((c > 0).any())
    assert hit["nan"] and hit["inf"] and hit["zero"] and (hit["tie"] or n == 1)  # the planted cases are there
    assert hit["positive"] or n <= 2


# ---------------------------------------------------------------- known answers, branch by branch
def test_no_finite_candidate():
    assert one(NAN) == 0 and one(NAN, INF, -INF, NAN, INF) == 0 and one(INF, INF, INF, INF) == 0


def test_no_candidate_beside_the_neighbours():
    assert one(3.0) == 0 and one(1.0, 2.0) == 0 and one(2.0, 1.0) == 0      # n <= 2
    assert one(5.0, 1.0, 7.0) == 0                                           # n = 3, the winner in the middle
    assert one(1.0, 5.0, 7.0) == np.float32(1.0)                             # n = 3, the winner at an end: G = {2}, c2 == cmax
    assert one(1.0, 2.0, NAN, INF) == 0 and one(NAN, 4.0, 2.0, 3.0, -INF) == 0  # the only candidates of G are not finite


def test_flat_column():
    assert one(2.5, 2.5, 2.5, 2.5, 2.5) == 0 and one(0.0, -0.0, 0.0, -0.0) == 0 and one(NAN, 7.0, INF, 7.0, 7.0) == 0


def test_winner_at_either_end():
    # k1 = 0: G = {2, 3, 4}; (3 - 1) / (9 - 1)
    assert one(1.0, 2.0, 3.0, 9.0, 5.0) == np.float32(0.25)
    # k1 = n - 1: G = {0, 1, 2}; (4 - 1) / (7 - 1)
    assert one(7.0, 4.0, 6.0, 2.0, 1.0) == np.float32(0.5)
    # an interior winner with a closer neighbour on each side: (6 - 2) / (10 - 2)
    assert one(10.0, 3.0, 2.0, 2.5, 6.0) == np.float32(0.5)
    # negative costs: (-1 - -3) / (5 - -3)
    assert one(-3.0, 5.0, -1.0, 0.0) == np.float32(0.25)
    # the quotient is rounded once, from f64: (0.3f - 0.1f) / (0.7f - 0.1f)
    a, b, c = np.float32(0.1), np.float32(0.3), np.float32(0.7)
    assert one(a, c, b, c) == np.float32((np.float64(b) - np.float64(a)) / (np.float64(c) - np.float64(a)))


def test_a_non_adjacent_tie_gives_zero():
    assert one(1.0, 4.0, 1.0, 9.0) == 0 and one(5.0, 2.0, 8.0, 8.0, 2.0) == 0
    assert one(-0.0, 3.0, 0.0, 1.0) == 0 and one(0.0, 3.0, -0.0, 1.0) == 0  # zeros of either sign tie
    assert not np.signbit(both(col(0.0, 3.0, -0.0, 1.0))).any()


def test_an_adjacent_tie_is_ignored():
    # k1 = 1 (the first of the two), its neighbour k = 2 ties with it and is left out: (5 - 1) / (9 - 1)
    assert one(9.0, 1.0, 1.0, 5.0, 6.0) == np.float32(0.5)
    assert one(1.0, 1.0, 5.0, 9.0) == np.float32(0.5)      # k1 = 0, G = {2, 3}
    assert one(9.0, 5.0, 1.0, 1.0) == np.float32(1.0)      # k1 = 2, G = {0}: c2 == cmax
    assert one(9.0, 5.0, 3.0, 1.0, 1.0) == np.float32(0.5)  # k1 = 3, G = {0, 1}


def test_non_finite_candidates_are_skipped():
    assert one(NAN, 1.0, INF, 3.0, -INF, 9.0) == np.float32(0.25)  # F = {1, 3, 5}
    assert one(-INF, 1.0, 2.0, 3.0, 9.0) == np.float32(0.25)       # -inf never wins here: it is not finite


# ---------------------------------------------------------------- properties
def test_range_sign_and_scaling():
    rng = np.random.default_rng(77)
    for n in (3, 4, 5, 8, 17, 65):
        V = cr.random_volume(rng, n, 11, 17)
        c = cr.confidence_vec(V)
        assert not np.isnan(c).any() and (c >= 0).all() and (c <= 1).all()
        assert not np.signbit(c).any()  # no -0
        for e in (-40, -3, 5, 60):  # a power of two within f32's normal range for these values (|V| < 2^20, steps >= 2^-40 or so)
            scaled = np.ldexp(V, e).astype(np.float32)
            assert np.array_equal(np.ldexp(scaled, -e).astype(np.float32), V, equal_nan=True)  # nothing was lost on the way
            assert cr.same_bits(cr.confidence_vec(scaled), c)


def test_the_winner_is_wta():
    """k1 is k_wta's winner wherever a finite candidate exists and no -inf / +inf comes before it"""
    rng = np.random.default_rng(5)
    V = rng.standard_normal((9, 20, 30)).astype(np.float32)
    assert np.array_equal(cr.wta(V, 3), 3 + V.argmin(axis=0))


# ---------------------------------------------------------------- the measure separates right from wrong, on the oracle alone
@pytest.mark.parametrize("method", ["classic", "guided2"])
def test_confident_half_is_more_often_right(oracle, method):
    from aswstereomatch_amd.synth import make_pair

    L, R, gt = make_pair(60, 160, 12, seed=5)
    if method == "classic":  # 16 candidates: entry 2's range is inclusive
        rc, disp, vol = oracle.asw_classic(L, R, 30.0, 20.0, 0, 7, 0, 15, want_vol=True)
    else:
        rc, disp, vol = oracle.asw_guided2(L, R, 0, 1e-6, 7, 0, 16, want_vol=True)
    assert rc == 0 and vol.shape == (16, 60, 160)
    conf = both(vol)
    assert np.isfinite(vol).all() and np.array_equal(disp, vol.argmin(axis=0))  # the map is min_d + k1
    wrong = np.abs(disp - gt) > 1
    order = np.argsort(-conf, axis=None, kind="stable")
    top = order[: order.size // 2]
    e_all, e_top = float(wrong.mean()), float(wrong.ravel()[top].mean())
    print("%s: error rate of the whole map %.4f, of the more confident half %.4f" % (method, e_all, e_top))
    assert e_top < e_all


# ---------------------------------------------------------------- the interface carries it
def test_the_header_states_the_rule():
    text = " ".join(open(os.path.join(ROOT, "include", "asw_mi355x.h")).read().split())
    for phrase in ("F = { k : V[k] finite }", "G = { k in F : |k - k1| >= 2 }",
                   "conf = (float)(((double)c2 - (double)c1) / ((double)cmax - (double)c1))", "2 channels", "step >= cols * 8",
                   "ASW_ERR_NO_FRAME without one", "DESIGN.md section 4.24"):
        assert phrase in text, phrase
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.24" in design and "k_confidence" in design


def test_the_python_signatures_carry_the_keyword():
    import aswstereomatch_amd as asw

    names = ["stereoMatching"] + [n for n in dir(asw.Context) if n.startswith("computeAdaptiveWeight")]
    assert len(names) == 14
    for n in names:
        p = inspect.signature(getattr(asw.Context, n)).parameters
        assert "return_confidence" in p and p["return_confidence"].default is False, n
        assert list(p)[-1] == "return_confidence", n  # appended: no positional argument moved
    p = inspect.signature(asw.Context.download_disparity).parameters
    assert list(p) == ["self", "slot", "shape", "confidence"] and p["confidence"].default is False
    src = open(os.path.join(ROOT, "aswstereomatch_amd", "_lib.py")).read()
    assert "confidence" not in src  # no new symbol: the request travels in the image's channel count
