"""The smoothing rule on the CPU (tests/smooth_ref.py): its two restatements against each other and against
hand-written answers, the properties the rule has by construction (identity on a line of one pixel, pass-through of a frame without
a confident pixel, constants stay constant, the result stays inside the confident inputs' range), how the request is encoded, and
that the smoothed map of the CPU oracle's matches is no worse than the raw one.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import confidence_ref as cr  # noqa: E402
import smooth_ref as sm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = np.float64


def both(G, d, c, sigma_c, lam, T):
    a, b = sm.smooth_vec(G, d, c, sigma_c, lam, T), sm.smooth_loop(G, d, c, sigma_c, lam, T)
    assert sm.same_bits(a, b)
    return a


# ---------------------------------------------------------------- the two forms agree
@pytest.mark.parametrize("seed", range(12))
def test_the_two_forms_are_bit_equal(seed):
    rng = np.random.default_rng(4250 + seed)
    case = sm.random_case(rng)
    H, W = case["d"].shape
    if H * W > 700:  # the loop form works on Python scalars: keep it in the tenths of a second
        tag = list(case["tag"])
        tag[0] = max(1, 700 // W)
        case = sm.build_case(tuple(tag))
    both(case["G"], case["d"], case["c"], case["sigma_c"], case["lam"], case["T"])


def test_the_seeded_set_reaches_the_planted_cases():
    rng = np.random.default_rng(4250)
    cases = [sm.random_case(rng) for _ in range(60)]
    assert any(np.isnan(c["d"]).any() for c in cases) and any(np.isinf(c["d"]).any() for c in cases)
    assert any((c["c"] < 0).any() for c in cases) and any(np.isnan(c["c"]).any() for c in cases) and any((c["c"] > 1).any() for c in cases)
    assert any(not c["c"].any() for c in cases)  # a whole frame of zero confidence
    assert any(c["G"].strides[0] != c["G"].shape[1] * (1 if c["G"].ndim == 2 else 3) for c in cases)  # padded rows
    assert {c["G"].ndim for c in cases} == {2, 3}
    assert {1, 2, 3, 8} <= {c["T"] for c in cases}


# ---------------------------------------------------------------- known answers
def test_table():
    Wt = sm.table(8.0, 3)
    assert Wt.shape == (766,) and Wt[0] == 1.0 and Wt[-1] == 0.0
    assert np.array_equal(Wt * 65536, np.floor(Wt * 65536))  # multiples of 2^-16
    assert Wt[8] == np.floor(65536 * np.exp(-1.0) + 0.5) / 65536
    assert (np.diff(Wt) <= 0).all()


def test_lam_t_sums_to_the_paper_s_variance():
    # the T iterations' lambdas are in ratio 4 : 1 and sum to 1.5 * lambda * (4^T - 1) / 3 / (4^T - 1) = lambda / 2
    for T in range(1, 9):
        assert abs(sum(sm.lam_t(900.0, T, t) for t in range(1, T + 1)) - 450.0) < 1e-9
        assert sm.lam_t(900.0, T, T) == F64(1.5) * F64(900.0) / F64((1 << 2 * T) - 1)


def test_a_line_of_two():
    """1 x 2, T = 1, constant guide (w = 1), lambda = 1: lam_1 = 1.5 * 1 * 1 / 3 = 0.5; the row system is [[1.5, -0.5], [-0.5, 1.5]],
    its inverse [[0.75, 0.25], [0.25, 0.75]]; the column pass works on lines of length 1.  With c = (1, 1), d = (0, 8):
    N = (2, 6), D = (1, 1)."""
    G = np.zeros((1, 2), np.uint8)
    out = both(G, np.array([[0, 8]], np.float32), np.ones((1, 2), np.float32), 8.0, 1.0, 1)
    # by the recurrences: r0 = 1/1.5, cp0 = -0.5 * r0, fp0 = 0; m1 = 1.5 - 0.5 * 0.5 * r0 ...: every value below is what they give
    r0 = F64(1.0) / F64(1.5)
    cp0 = F64(-0.5) * r0
    m1 = F64(1.5) - F64(-0.5) * cp0
    r1 = F64(1.0) / m1
    n1 = (F64(8.0) - F64(-0.5) * (F64(0.0) * r0)) * r1
    d1 = (F64(1.0) - F64(-0.5) * (F64(1.0) * r0)) * r1
    n0, d0 = F64(0.0) * r0 - cp0 * n1, F64(1.0) * r0 - cp0 * d1
    assert out[0, 1] == np.float32(n1 / d1) and out[0, 0] == np.float32(n0 / d0)
    assert np.allclose(out, [[2.0, 6.0]], rtol=1e-7)
    # a hole takes its neighbour's value whatever lambda is: N = (0, 8 c), D = (0, c) smoothed by the same matrix
    out = both(G, np.array([[np.nan, 8]], np.float32), np.array([[1, 0.25]], np.float32), 8.0, 1.0, 1)
    assert np.allclose(out, [[8.0, 8.0]], rtol=1e-7)
    # a cut link (w = 0 between the two pixels): both keep their own value, and the hole keeps its input bits
    Gc = np.array([[0, 255]], np.uint8)
    d = np.array([[np.nan, 8]], np.float32)
    out = both(Gc, d, np.array([[1, 0.25]], np.float32), 0.05, 1.0, 1)
    assert sm.same_bits(out, d)


def test_a_line_of_three():
    """1 x 3, T = 1, constant guide, lambda = 2: lam_1 = 1; the matrix is [[2, -1, 0], [-1, 3, -1], [0, -1, 2]] with determinant 8
    and inverse [[5, 2, 1], [2, 4, 2], [1, 2, 5]] / 8.  c = 1: D stays 1, the result is the inverse applied to d."""
    G = np.full((1, 3, 3), 9, np.uint8)
    out = both(G, np.array([[8, 0, 16]], np.float32), np.ones((1, 3), np.float32), 8.0, 2.0, 1)
    assert np.allclose(out, [[7.0, 6.0, 11.0]], rtol=1e-7)
    # the same as a column: the row pass is the identity
    out = both(np.full((3, 1), 9, np.uint8), np.array([[8], [0], [16]], np.float32), np.ones((3, 1), np.float32), 8.0, 2.0, 1)
    assert np.allclose(out.ravel(), [7.0, 6.0, 11.0], rtol=1e-7)


def test_a_line_of_one_is_the_identity():
    for v in (3.25, -0.0, 1e-30, 1e30):
        for c in (1.0, 0.125, 3.5):
            d = np.array([[v]], np.float32)
            out = both(np.zeros((1, 1), np.uint8), d, np.array([[c]], np.float32), 8.0, 900.0, 3)
            # N / D = (c * v) / c: exact in f64 for f32 inputs (a 48-bit product), so the f32 result is v itself
            assert sm.same_bits(out, d)
    solved = sm.solve_line_loop([[F64(0.3)], [F64(-7.0)]], [F64(0.0)], F64(5.0))
    assert solved == [[F64(0.3)], [F64(-7.0)]]
    vec = sm.solve_lines_vec([np.array([[0.3]]), np.array([[-7.0]])], np.zeros((1, 1)), F64(5.0))
    assert vec[0][0, 0] == 0.3 and vec[1][0, 0] == -7.0


def test_a_frame_of_holes_returns_the_input_bits():
    rng = np.random.default_rng(3)
    G = sm.make_guide(rng, 7, 9, 3, "noise")
    d = sm.make_map(rng, 7, 9, bad=0.2)
    d[0, 0] = np.frombuffer(np.uint32(0x7FC12345).tobytes(), np.float32)[0]  # a NaN with a payload
    assert np.isnan(d).any() and np.isinf(d).any()
    for c in (np.zeros((7, 9), np.float32), np.full((7, 9), -1, np.float32), np.full((7, 9), np.nan, np.float32)):
        assert sm.same_bits(both(G, d, c, 8.0, 900.0, 3), d)
    # every finite pixel untrusted, every trusted pixel non-finite
    c = np.where(np.isfinite(d), 0, 1).astype(np.float32)
    assert sm.same_bits(both(G, d, c, 8.0, 900.0, 2), d)


# ---------------------------------------------------------------- properties
# The solve is the inverse of a strictly diagonally dominant M-matrix whose rows sum to 1: the inverse is non-negative with unit row
# sums, in exact arithmetic.  In f64 a step of the recurrences commits a few roundings of relative size 2^-53 on values no larger
# than the inputs (|cp| < 1, r <= 1), and a value passes through at most rows + cols steps per pass and 2 T passes: below
# 2 * 8 * (rows + cols) * 8 * 2^-53 < 1e-11 relative for the frames here, before the one f32 rounding (2^-24 = 6e-8) of the result.
# 1e-9 relative on the f64 planes and 1e-7 on the f32 map are therefore bounds with room, derived, not measured.
@pytest.mark.parametrize("value", [17.0, 0.375, -3.0])
def test_a_constant_map_stays_constant(value):
    rng = np.random.default_rng(11)
    for kind in sm.GUIDES:
        G = sm.make_guide(rng, 20, 33, 3, kind)
        c = sm.make_conf(rng, 20, 33, "unit")
        d = np.full((20, 33), value, np.float32)
        out = sm.smooth_vec(G, d, c, 8.0, 900.0, 3)
        assert np.abs(out.astype(F64) - value).max() <= 1e-7 * abs(value)
        # the f64 planes before the last rounding: within 1e-9 relative
        N, D = sm.start_planes(d, c)
        kh, kv = sm.links(G)
        Wt = sm.table(8.0, 3)
        for t in range(1, 4):
            N, D = sm.solve_lines_vec([N, D], Wt[kh], sm.lam_t(900.0, 3, t))
            NT, DT = sm.solve_lines_vec([N.T.copy(), D.T.copy()], Wt[kv].T.copy(), sm.lam_t(900.0, 3, t))
            N, D = NT.T.copy(), DT.T.copy()
        assert (D > 0).all() and np.abs(N / D - value).max() <= 1e-9 * abs(value)


def test_the_result_stays_inside_the_confident_inputs():
    rng = np.random.default_rng(12)
    for _ in range(12):
        case = sm.random_case(rng)
        d, c = case["d"], case["c"]
        out = sm.smooth_vec(case["G"], d, c, case["sigma_c"], case["lam"], case["T"])
        ok = np.isfinite(d) & np.isfinite(c) & (c > 0)
        filled = out.view(np.uint32) != d.view(np.uint32)
        if not ok.any():
            assert not filled.any()
            continue
        lo, hi = float(d[ok].min()), float(d[ok].max())
        slack = 1e-7 * max(abs(lo), abs(hi), 1e-30)
        changed = out[filled]
        assert np.isfinite(changed).all() and (changed >= lo - slack).all() and (changed <= hi + slack).all()


# ---------------------------------------------------------------- the encoding
def test_the_constant_and_the_symbol_table():
    import aswstereomatch_amd as asw
    from aswstereomatch_amd import _lib

    assert asw.REFINE_SMOOTH == 0x40000000 == 1 << 30
    assert (asw.SMOOTH_SIGMA_C, asw.SMOOTH_LAMBDA, asw.SMOOTH_ITERATIONS) == (8.0, 900.0, 3)
    assert (sm.DEFAULTS["sigma_c"], sm.DEFAULTS["lam"], sm.DEFAULTS["iterations"]) == (8.0, 900.0, 3)
    assert len(_lib.ABI_SYMBOLS) == 46 and not [s for s in _lib.ABI_SYMBOLS if "smooth" in s]
    for T in range(1, 9):
        assert asw._smooth_word(T) == (1 << 30) | T
    for T in (0, -1, 9, 1 << 30):
        assert asw._smooth_word(T) == 1 << 30  # the invalid word: T = 0
    header = " ".join(open(os.path.join(ROOT, "include", "asw_mi355x.h")).read().split())
    for phrase in ("enum { ASW_REFINE_SMOOTH = 0x40000000 };", "static inline int asw_smooth_disparity(", "static inline int asw_match_smoothed_resident(",
                   "static inline int asw_stereo_match_smoothed(", "Wt[k] = floor(65536 * exp(-k / sigma_c) + 0.5) / 65536",
                   "b_i = (1.0 - a_i) - c_i", "DESIGN.md section 4.25"):
        assert phrase in header, phrase
    for name in ("smoothDisparity", "match_smoothed_resident", "stereoMatchingSmoothed"):
        assert hasattr(asw.Context, name)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.25" in design and "k_smooth" in design


def test_the_selector_words_are_untouched():
    """the request travels beside the two packed selector words, not in them: the program that prints every decoding of those words
    (pinned to tests/golden/selector_words_v1.txt.xz by tests/test_selector_words_cpu.py) knows nothing of it, and neither does the decoder"""
    for path in (("tests", "cpp", "selector_words.cpp"), ("aswstereomatch_amd", "csrc", "asw_selector.h")):
        src = open(os.path.join(ROOT, *path)).read()
        assert "SMOOTH" not in src and "smooth" not in src, path


# ---------------------------------------------------------------- usefulness, on the oracle alone
@pytest.mark.parametrize("method", ["classic", "guided2"])
def test_error_rates_on_the_synthetic_pair(oracle, method):
    """The oracle's integer map and the restated confidence of its volume, smoothed by the restatement at the default parameters,
    against the synthetic pair's ground truth: the share of pixels more than one level off.

    Measured on the CPU before anything was asserted (DESIGN.md section 4.25 records the rates): classic 0.0950 raw, 0.1050 smoothed;
    guided2 0.1020 raw, 0.1101 smoothed.  "smoothed <= raw" holds for NEITHER method on this pair, and for no other parameters
    either: over sigma_c in 1..1000, lambda in 0.05..900 and T in 1..3 the rate only approaches the raw one from above as the
    smoothing vanishes.  The pair's left image is low-pass filtered random texture, so its colour edges have nothing to do with the
    block edges of the true disparity: an edge-aware smoother has no edge to align to here, it pulls 10 to 20 wrong pixels right and
    blurs about a hundred across the block edges.  So the defaults stay the paper's and this test asserts only what it measured
    with: both rates exist and the smoothed map lies inside the candidate range.  What the smoother does when the guide's edges
    are the map's is asserted below, on a case where the answer follows from the rule."""
    from aswstereomatch_amd.synth import make_pair

    L, R, gt = make_pair(60, 160, 12, seed=5)
    if method == "classic":  # 16 candidates: entry 2's range is inclusive
        rc, disp, vol = oracle.asw_classic(L, R, 30.0, 20.0, 0, 7, 0, 15, want_vol=True)
    else:
        rc, disp, vol = oracle.asw_guided2(L, R, 0, 1e-6, 7, 0, 16, want_vol=True)
    assert rc == 0
    conf = cr.confidence_vec(vol)
    out = sm.smooth_vec(L, disp.astype(np.float32), conf)
    e_raw, e_smooth = float((np.abs(disp - gt) > 1).mean()), float((np.abs(out - gt) > 1).mean())
    print("%s: error rate of the raw map %.4f, of the smoothed map %.4f" % (method, e_raw, e_smooth))
    assert np.isfinite(out).all() and out.min() >= 0 and out.max() <= 15 * (1 + 1e-7)
    assert 0 < e_raw < 0.5 and 0 < e_smooth < 0.5  # a match and a smoothing took place: neither map is all right or all wrong


def test_unreliable_pixels_take_the_value_of_their_region():
    """Two flat regions of the guide, 255 levels apart in every channel: Wt[765] = floor(65536 * exp(-765 / 8) + 0.5) / 65536 = 0, so
    no link crosses the edge and each region is a system of its own.  The map is each region's constant with a fifth of the pixels
    replaced by outliers; the outliers carry confidence 0.  Every pixel of a region is then an average, with non-negative weights
    that sum to 1, of that region's confident inputs, which all hold the constant: the error rate goes from about 0.2 to exactly 0."""
    rng = np.random.default_rng(21)
    H, W = 24, 40
    G = np.zeros((H, W, 3), np.uint8)
    G[:, 23:] = 255
    truth = np.where(np.arange(W)[None, :] < 23, np.float32(5), np.float32(12)) * np.ones((H, 1), np.float32)
    bad = rng.random((H, W)) < 0.2
    d = np.where(bad, rng.integers(0, 16, (H, W)).astype(np.float32), truth).astype(np.float32)
    c = np.where(bad, np.float32(0), (1.0 - rng.random((H, W)) * 0.9).astype(np.float32))
    out = sm.smooth_vec(G, d, c)
    assert sm.table(8.0, 3)[765] == 0.0
    assert (np.abs(d - truth) > 1).mean() > 0.1
    assert np.abs(out.astype(F64) - truth).max() <= 1e-6  # the bound of the constant-map test above, at |value| <= 12
