"""The table of exactness bounds of tests/extreme_cases.py and the cases of tests/test_gpu_extreme_values.py, on the CPU alone.

The table is held to the source text: the constants every bound is made of are read from the .hip / .h files by pattern and must
equal the restated ones, so a changed constant fails here instead of leaving the table stale.  Non-vacuity, on the restatements
alone: each case drives its quantity to the value the table names, so a kernel that is exact only below that value cannot pass the
GPU file by never meeting it.

Three facts of the definitions that shape the cases:
  geodesic on opposed_flat is NaN in every plane: its support weights ARE the geodesic distances (no exponential), all 0 on a flat
  image, so den == 0.  Its largest cost, 765 = 3 * 255, is met on opposed_edges and checker;
  the AD-Census product 254 * 1225 cannot be reached on `complement`: a 35 x 35 window of x + 9 y spans 340 > 251 values, so it
  holds pixels with |2 L - 255| <= 1 and pixels whose census window wraps.  `checker` with lambdas (1, 1) reaches it;
  a refine call with minD = +-(1 << 20) has every disparity pointing outside any frame the call accepts: every pixel is unfillable.
  The median's votes take the ends 0 and 1024 in a case of their own (minD -520, 560 columns)."""
import os
import re
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extreme_cases as ec  # noqa: E402
import refine_ref  # noqa: E402
import sgbm_ref  # noqa: E402
import twopass_ref  # noqa: E402
from test_xq_scaled_domain_cpu import lut_classic, lut_ok  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "aswstereomatch_amd", "csrc")
LEFT, RIGHT = ec.LEFT, ec.RIGHT


def _src(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


def _one(text, pattern):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return m[0]


# ---------------------------------------------------------------- the constants, from the source text
def test_refine_constants():
    m = _src("asw_methods.hip")
    assert float(_one(m, r"tc\[c\] = \(unsigned\)floor\(([\d.]+) \* exp\(")) == ec.REFINE_TC_SCALE
    assert float(_one(m, r"= \(unsigned\)floor\(([\d.]+) \* exp\(-sqrt\(")) == ec.REFINE_TS_SCALE
    n, lo, hi = _one(m, r"if \(p\.n < 1 \|\| p\.n > (\d+) \|\| p\.minD < -\(1 << (\d+)\) \|\| p\.minD > \(1 << (\d+)\)\) return ASW_ERR_BAD_ARGUMENT;")
    assert int(n) == ec.REFINE_MAX_N and 1 << int(lo) == 1 << int(hi) == ec.REFINE_MAX_MIND
    assert int(_one(m, r"if \(p\.win < 1 \|\| p\.win > (\d+) \|\| p\.win % 2 == 0\) return ASW_ERR_BAD_ARGUMENT;")) == ec.REFINE_MAX_WIN
    k = _src("k_refine.hip")
    assert int(_one(k, r"if \(a\.win < 1 \|\| a\.win > (\d+)\) return ASW_ERR_BAD_ARGUMENT;")) == ec.REFINE_MAX_WIN
    assert "if (2u * below >= T)" in k and "unsigned T = 0;" in k and "unsigned below = 0;" in k
    # the claim: T fits 31 bits, 2 * T does not, and fits 32
    assert 1 << 30 < ec.REFINE_T_MAX < 1 << 31 < 2 * ec.REFINE_T_MAX < 1 << 32
    assert float(np.float32(ec.REFINE_MAX_MIND + ec.REFINE_MAX_N)) == ec.REFINE_MAX_MIND + ec.REFINE_MAX_N < 1 << 24


def test_cross_and_adcensus_constants():
    k = _src("k_cross.hip")
    assert int(_one(k, r"constexpr int MAX_L = (\d+);")) == ec.CROSS_MAX_L
    assert "S <= 255 * %d^2 < 2^24" % ec.CROSS_MAX_WIN in k
    m = _src("asw_methods.hip")
    assert m.count("if (mp.win < 1 || mp.win > %d) return ASW_ERR_BAD_ARGUMENT;" % ec.CROSS_MAX_WIN) >= 1
    assert "mp.cross_trunc < 1 || mp.cross_trunc > 255" in m
    assert "(uint8_t)floor(127.0 * (1.0 - exp(-(double)h / lambda_census)) + 0.5)" in m
    assert ec.ADCENSUS_E_MAX * ec.CROSS_MAX_WIN ** 2 < ec.CROSS_S_MAX < 1 << 24


def test_wmedian_constants():
    for name in ("k_wmedian.hip", "k_wmedian_tile.hip", "k_wmedian_tile_gen.hip"):
        assert int(_one(_src(name), r"constexpr uint32_t COST_BASE_BITS = (0x[0-9a-fA-F]+)u;"), 16) == ec.COST_BASE_BITS
    assert np.uint32(ec.COST_BASE_BITS).view(np.float32) == np.float32(4096.0)
    assert "- COST_BASE_BITS) << %d) | (uint32_t)e;" % ec.WM_KEY_SHIFT_32 in _src("k_wmedian.hip")
    t, g = _src("k_wmedian_tile.hip"), _src("k_wmedian_tile_gen.hip")
    assert "- COST_BASE_BITS) * %d.0 + " % ec.WM_KEY_MUL_TILE in t and "- COST_BASE_BITS) * %d.0 + " % ec.WM_KEY_MUL_GEN in g
    assert float(_one(t, r"constexpr double KEY_PAD = ([\d.]+);")) == ec.WM_KEY_PAD_TILE
    assert float(_one(g, r"constexpr double KEY_PAD = ([\d.]+);")) == ec.WM_KEY_PAD_GEN
    assert "build_similarity_volume(ctx, dL, dR, H, W, mp.minD, n, 0.4, 10, 50, raw.as<float>())" in _src("asw_methods.hip")
    assert ec.SIM_PARAMS == (0.4, 10.0, 50.0)
    # every cost of [4096, 16384) has key bits below 2^24: 16384.0f is 2^24 bit patterns above 4096.0f
    assert int(np.float32(16384.0).view(np.uint32)) - ec.COST_BASE_BITS == 1 << 24
    assert (1 << 24) * ec.WM_KEY_MUL_TILE == ec.WM_KEY_PAD_TILE / 256 and (1 << 24) * ec.WM_KEY_MUL_GEN <= ec.WM_KEY_PAD_GEN / 1024


def test_sgbm_and_bm_constants():
    k = _src("k_sgbm.hip")
    assert int(_one(k, r"constexpr int SGBM_BIG = (0x[0-9a-fA-F]+);"), 16) == ec.SGBM_BIG
    m = _src("asw_methods.hip")
    assert float(_one(m, r"if \(bound >= ([\d.]+)\) return ASW_ERR_BAD_ARGUMENT;")) == ec.SGBM_INT_BOUND == 2.0 ** 31
    assert float(_one(m, r"if \(want_volume && bound >= ([\d.]+)\) return ASW_ERR_BAD_ARGUMENT;")) == ec.SGBM_F32_BOUND == 2.0 ** 24
    assert "(double)cn * (2.0 * a.ftzero + %d.0) * k * k" % ec.SGBM_RAW_MAX in m and "62.0 * k * k" in m
    assert "(double)__builtin_popcount(p.paths) * (cmax + a.P2)" in m
    assert sgbm_ref.cost_bound(3, 11, 63) == 3 * (2 * 63 + ec.SGBM_RAW_MAX) * 121
    # BIG + P1 < 2^31 for every accepted P1 (P1 < P2, 3 * (C_max + P2) < 2^31)
    assert ec.SGBM_BIG + int(ec.SGBM_INT_BOUND) // 3 < 1 << 31
    cap = int(_one(m, r"if \(p\.pre_filter_cap < 1 \|\| p\.pre_filter_cap > (\d+)\) return ASW_ERR_BAD_ARGUMENT;"))
    blk = int(_one(m, r"if \(p\.block_size < 5 \|\| p\.block_size > (\d+) \|\| p\.block_size % 2 == 0 \|\| p\.block_size > std::min\(H, W\)\)"))
    assert (cap, blk) == (ec.BM_MAX_CAP, ec.BM_MAX_BLOCK)
    assert "a block SAD is below %d * %d^2 < 2^23" % (2 * cap, blk) in _src("k_bm.hip")
    assert ec.BM_SAD_MAX == 2 * cap * blk * blk < 1 << 23


def test_xq_scharr_and_flag_constants():
    assert int(_one(_src("asw_internal.h"), r"constexpr int XQ_LUT_SCALE_LOG2 = (\d+);")) == ec.XQ_LUT_SCALE_LOG2
    import test_xq_scaled_domain_cpu as xq
    assert xq.SCALE == ec.XQ_LUT_SCALE_LOG2
    c = _src("k_cost.hip")
    assert "|v| <= %d -> int16" % ec.SCHARR_MAX in c
    a, b, a2 = _one(c, r"int v = (\d+) \* \(\(int\)r0\[cp \* 3 \+ ch\] - \(int\)r0\[cm \* 3 \+ ch\]\) \+ (\d+) \* \(\(int\)r1\[cp \* 3 \+ ch\] - "
                       r"\(int\)r1\[cm \* 3 \+ ch\]\) \+\s+(\d+) \* ")
    assert (int(a) + int(b) + int(a2)) * 255 == ec.SCHARR_MAX < 1 << 15
    import scanline_ref as sl
    import cross_scale_ref as cs
    assert sl.encode(*ec.SCANLINE_MAX) != sl.FLAG and sl.encode(128, 7, 8) == sl.FLAG and sl.encode(127, 8, 8) == sl.FLAG
    assert sl.encode(*ec.SCANLINE_MIN) != sl.FLAG and sl.encode(0, 0, 1) == sl.FLAG
    assert float(sl.penalties(*ec.SCANLINE_MAX)[1]) == 127 * 16 * 8 and float(sl.penalties(*ec.SCANLINE_MIN)[0]) == 4.0 ** -5
    assert cs.encode(3, 255) >> 13 & 7 == 3 and cs.encode(3, 256) >> 13 & 7 == 0


EXACT_ROWS = ("T, the total weight of a window", "S of entry 12", "S of AD-Census", "a block SAD", "the Scharr response",
              "ab * cost, the volume", "e and E of the f64 scans", "P2 of the largest code")


def test_table_rows_are_complete_and_reach_what_they_say():
    """a row either computes its reached value on a restatement (value and reached both set) or says that it has no numeric reach
    (both None: the row names the cases the GPU file runs)"""
    reached = {}
    for row in ec.TABLE:
        assert set(row) == {"kernel", "quantity", "bound", "value", "reach", "reached", "held"} and row["held"] in ("gpu", "host")
        assert (row["value"] is None) == (row["reached"] is None), row["quantity"]
        if row["reached"] is None:
            print("%-50s %-40s no numeric reach (%s)" % (row["kernel"], row["quantity"], row["held"]))
            continue
        t0 = time.perf_counter()
        got = reached[row["quantity"]] = row["reached"]()
        print("%-50s %-40s bound %-12s reached %s (%s) in %.2f s" % (row["kernel"], row["quantity"], row["value"], got, row["held"],
                                                                     time.perf_counter() - t0))
        if row["quantity"] == "the smallest nonzero weight product":
            assert got >= row["value"], row       # a lower bound
        else:
            assert got <= row["value"], row
    assert len(reached) == len({r["quantity"] for r in ec.TABLE if r["reached"] is not None})
    values = {r["quantity"]: r["value"] for r in ec.TABLE}
    assert set(EXACT_ROWS) <= set(reached) and all(reached[q] == values[q] for q in EXACT_ROWS), reached
    assert reached["2u * below of the bisection"] >= 1 << 31 and reached["S with the volume handed back"] >= 1 << 23


# ---------------------------------------------------------------- the pairs
@pytest.mark.parametrize("cn", [1, 3])
def test_pairs_are_what_they_say(cn):
    H, W = 9, 70
    for kind in ec.KINDS:
        L, R = ec.pair(kind, H, W, cn)
        assert L.shape == R.shape == ((H, W) if cn == 1 else (H, W, 3)) and L.dtype == R.dtype == np.uint8
        assert np.array_equal(R, 255 - L)
        Ls, Rs = ec.pair(kind, H, W, cn, swap=True)
        assert np.array_equal(Ls, R) and np.array_equal(Rs, L)
        Lp, Rp = ec.pair(kind, H, W, cn, pad=3)
        assert np.array_equal(Lp, L) and np.array_equal(Rp, R) and Lp.strides[0] == (W + 3) * (1 if cn == 1 else 3)
        assert [v[0] for v in ec.variants(kind, H, W, cn)] == ["plain", "swapped", "padded"]
    L, R = ec.opposed_flat(H, W, cn)
    assert (L == 255).all() and (R == 0).all()
    for bar in (1, 2, 40):
        L, _ = ec.opposed_edges(H, W, cn, bar)
        g = L if cn == 1 else L[:, :, 0]
        assert set(np.unique(g)) <= {0, 255} and (g[:, :bar] == 0).all() and (bar >= W or (g[:, bar:2 * bar] == 255).all())
    L, _ = ec.checker(H, W, cn)
    g = (L if cn == 1 else L[:, :, 1]).astype(int)
    assert (np.abs(np.diff(g, axis=0)) == 255).all() and (np.abs(np.diff(g, axis=1)) == 255).all()


def test_complement_census_windows_hold_no_equal_pixels():
    import adcensus_ref as ar
    H, W = 30, 80
    L, R = ec.complement(H, W, 1)
    for y in range(3, H - 3, 5):
        for x in range(4, W - 4, 7):
            assert len(np.unique(L[y - 3:y + 4, x - 4:x + 5])) == 63
    ham = ar.hamming(L, R, LEFT, 0, 1)[0]
    assert (ham[3:H - 3, 4:W - 4] == 62).all() and ham.max() == 62
    L3, R3 = ec.complement(H, W, 3)
    assert np.array_equal(ar.gray_pair(L3, R3)[0], L) and np.array_equal(ar.hamming(L3, R3, LEFT, 0, 1)[0], ham)
    assert ar.ad(L, R, LEFT, 0, 1).max() == 255


# ---------------------------------------------------------------- non-vacuity: refine
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("case", [ec.REFINE_T_CASE, ec.REFINE_ENDS_CASE])
def test_refine_total_weight_at_its_maximum(case, cn):
    H, W, minD, n, win = case
    dl, dr = ec.refine_two_level_maps(H, W, minD, n)
    F, mask = ec.refine_fill(dl, dr, minD)
    assert set(np.unique(F)) == {0, n - 1} and (mask == 2).sum() == 0      # every tap votes; the votes are the ends of the range
    G = np.full((H, W) if cn == 1 else (H, W, 3), 255, np.uint8)
    tc, ts = refine_ref.tables(win, ec.REFINE_GAMMA, ec.REFINE_GAMMA, cn)
    assert (tc == ec.REFINE_TC_SCALE).all() and (ts == ec.REFINE_TS_SCALE).all()
    T, below = ec.refine_totals(G, F, win, ec.REFINE_GAMMA, ec.REFINE_GAMMA, (n - 1) >> 1)
    full = (mask == 1) & (T == ec.REFINE_T_MAX)
    over = full & (2 * below >= 1 << 31)
    print("filled pixels with T == %d: %d; of these with 2 * below >= 2^31 at the first bisection step: %d (largest %d)" % (
        ec.REFINE_T_MAX, full.sum(), over.sum(), 2 * below[full].max()))
    assert full.sum() >= 20 and over.sum() >= 20 and (below[over] >= 1 << 30).all()
    want = refine_ref.refine_vec(G, dl, dr, minD, n, 1.0, win, ec.REFINE_GAMMA, ec.REFINE_GAMMA)
    assert set(np.unique(want["out"][full])) == {minD, minD + n - 1}       # the medians take both levels
    assert (want["out"] != want["fill"]).any()                             # and move something
    # a signed 2 * below would be negative at these pixels: the comparison with T then takes the other branch there
    wrong = (2 * below[over]).astype(np.int32).astype(np.int64) >= T[over]
    assert not wrong.any() and (2 * below[over] >= T[over]).all()


@pytest.mark.parametrize("win", ec.REFINE_T_WINDOWS)
def test_refine_smaller_windows_reach_their_own_maximum(win):
    H, W, minD, n, _ = ec.REFINE_T_CASE
    dl, dr = ec.refine_two_level_maps(H, W, minD, n)
    F, mask = ec.refine_fill(dl, dr, minD)
    T, _ = ec.refine_totals(np.full((H, W), 255, np.uint8), F, win, ec.REFINE_GAMMA, ec.REFINE_GAMMA, 0)
    assert ((mask == 1) & (T == win * win * ec.REFINE_TC_SCALE * ec.REFINE_TS_SCALE)).sum() >= 20


@pytest.mark.parametrize("minD", [-ec.REFINE_MAX_MIND, ec.REFINE_MAX_MIND])
def test_refine_ends_of_min_disparity_leave_every_pixel_unfillable(minD):
    (H, W), n = ec.REFINE_MIND_FRAME, ec.REFINE_MAX_N
    dl = ec.refine_mind_end_map(minD)
    assert dl.min() == minD and dl.max() == minD + n - 1
    want = refine_ref.refine_vec(np.full((H, W), 255, np.uint8), dl, dl, minD, n, 1.0, 15, 60.0, 9.0)
    assert (want["mask"] == 2).all() and (want["out"] == np.float32(minD - 1)).all() and want["n_unfillable"] == H * W
    assert float(np.float32(minD - 1)) == minD - 1


# ---------------------------------------------------------------- non-vacuity: cross, AD-Census
def test_cross_sum_at_its_maximum():
    H, W = ec.CROSS_FRAME
    L, R = ec.opposed_flat(H, W, 1)
    for dt in (LEFT, RIGHT):
        S, N, E, disp = ec.cross_sums(L, R, dt, 20, 255, ec.CROSS_MAX_WIN, 0, 3)
        assert S.max() == 255 * 35 ** 2 == ec.CROSS_S_MAX == 312375 and N.max() == 1225
        assert (E[:, N == 1225] == np.float32(255.0)).all() and (E == np.float32(255.0)).all()
    L, R = ec.checker(H, W, 1)
    S, N, E, disp = ec.cross_sums(L, R, LEFT, 0, 255, ec.CROSS_MAX_WIN, 0, 3)
    assert (N == 1).all() and set(np.unique(S)) == {0, 255}      # tau 0: every arm 0


def test_adcensus_sum_at_its_maximum_on_checker_and_what_complement_reaches():
    import adcensus_ref as ar
    ta, tc = ar.tables(*ec.ADCENSUS_LAMBDAS)
    assert ta.max() + tc.max() == ec.ADCENSUS_E_MAX == 254
    H, W = ec.ADCENSUS_FRAME
    L, R = ec.checker(H, W, 1)
    for dt in (LEFT, RIGHT):
        S, N, E, disp, e = ec.adcensus_sums(L, R, dt, 255, ec.CROSS_MAX_WIN, 0, 3)
        assert e.max() == 254 and S.max() == 254 * 1225 and (S[0] == 254 * 1225).any()
    Lc, Rc = ec.complement(H, W, 1)
    S, N, E, disp, e = ec.adcensus_sums(Lc, Rc, LEFT, 255, ec.CROSS_MAX_WIN, 0, 3)
    share = S.max() / (254 * 1225)
    print("AD-Census on complement, tau 255, lambdas (1, 1): e.max %d, largest S %d = %.4f of 254 * 1225" % (e.max(), S.max(), share))
    assert e.max() == 254 and N.max() == 1225 and 0.9 < share < 1.0   # 254 on most taps, never on all 1225 (this file's header)


# ---------------------------------------------------------------- non-vacuity: SGBM, StereoBM
def test_sgbm_volume_case_passes_half_of_the_f32_bound():
    H, W, cn, minD, D, w, cap = ec.SGBM_VOLUME_CASE
    for paths in ec.SGBM_MASKS:
        P2 = ec.sgbm_largest_p2(cn, w, cap, paths)
        n = bin(paths).count("1")
        assert n * (sgbm_ref.cost_bound(cn, w, cap) + P2) < 1 << 24 <= n * (sgbm_ref.cost_bound(cn, w, cap) + P2 + 1)
    smax, lmax, cbound, cmax = ec.sgbm_reached(0xFF)
    print("8 paths: largest S %d = %.3f * 2^24, largest single L %d, largest C %d of the host's C_max %d" % (
        smax, smax / 2.0 ** 24, lmax, cmax, cbound))
    assert 1 << 23 <= smax < 1 << 24
    # what no small frame reaches: L grows by at most C_max a step, so S of a frame of 100 columns stays below 8 * 100 * C_max,
    # a 400th of 2^31; the int32 bound is held by the host check alone
    assert lmax <= cmax + ec.sgbm_largest_p2(cn, w, cap, 0xFF) and smax < (1 << 31) // 200
    s3 = ec.sgbm_reached(0x07)[0]
    print("3 paths: largest S %d = %.3f * 2^24" % (s3, s3 / 2.0 ** 24))
    assert s3 > 1 << 22


def test_stereobm_block_sad_at_its_maximum():
    out = ec.bm_reached()
    H, W, minD, D, w = ec.BM_CASE
    assert w == ec.BM_MAX_BLOCK and ec.BM_SETTINGS[0] == ec.BM_MAX_CAP
    assert np.nanmax(out["vol"]) == 2 * 63 * 255 ** 2 == ec.BM_SAD_MAX and np.nanmin(out["vol"]) < ec.BM_SAD_MAX
    assert np.isfinite(out["vol"]).any(axis=0).sum() >= 2


# ---------------------------------------------------------------- non-vacuity: the TAD C+G cost, Scharr
def test_tad_cost_reaches_both_ends_of_its_range(oracle):
    import similarity_ref as sr
    lo, hi = ec.tad_cost_range()
    assert 4096 <= lo < hi < 16384 and 0 <= ec.key_bits(lo) < ec.key_bits(hi) < 1 << 24
    assert (lo, hi) == (5100.0, 8452.0)     # 0.4 * 255 * 50 and 0.6 * (170 + 10) + 0.4 * (254 * 50 + 8160)
    H, W = ec.WMEDIAN_FRAME
    L, R = ec.opposed_edges(H, W, 3, 2)
    rc, vol = oracle.compute_similarity(L, R, *ec.SIM_PARAMS, 0, 0, 5)
    assert rc == 0 and float(vol.min()) == lo and float(vol.max()) == hi
    lit = sr.similarity_literal(L, R, *ec.SIM_PARAMS, 0, 5)
    assert np.array_equal(lit, vol)
    # a random pair stays inside: the ends are the ends
    rng = np.random.default_rng(3)
    A, B = rng.integers(0, 256, (9, 40, 3)).astype(np.uint8), rng.integers(0, 256, (9, 40, 3)).astype(np.uint8)
    v = oracle.compute_similarity(A, B, *ec.SIM_PARAMS, 0, 0, 5)[1]
    assert lo <= v.min() and v.max() <= hi


def test_scharr_takes_both_extremes():
    L, R = ec.opposed_edges(9, 70, 1, 2)
    for img in (L, R):
        g = ec.scharr_x(img)
        assert g.max() == ec.SCHARR_MAX and g.min() == -ec.SCHARR_MAX
    gl, gr = ec.scharr_x(L), ec.scharr_x(R)
    assert (np.abs(gl - gr)[:, 1:-1] == 2 * ec.SCHARR_MAX).all()      # +4080 meets -4080 at candidate 0
    assert (ec.scharr_x(ec.opposed_edges(9, 70, 1, 1)[0])[:, 1:-1] == 0).all()


# ---------------------------------------------------------------- non-vacuity: the float families
def test_bilateral_family_on_opposed_flat_and_checker(oracle):
    H, W = ec.FLOAT_FRAME
    L, R = ec.opposed_flat(H, W, 3)
    for dt in (LEFT, RIGHT):
        for win in (15, 35):
            rc, d, v = oracle.asw_classic(L, R, 30, 20, dt, win, 0, 4, want_vol=True)
            assert rc == 0 and (v == np.float32(255.0)).all()
            E, vol, disp = twopass_ref.twopass(L[:, :, 0], R[:, :, 0], 30, 20, win, 0, 4, dt)
            assert (vol == np.float32(255.0)).all()
    rc, d, v = oracle.asw_direct8(L, R, LEFT, 15, 0, 4, want_vol=True)
    assert rc == 0 and (v == np.float32(255.0)).all()
    rc, d, v = oracle.asw_geodesic(L, R, LEFT, 15, 0, 4, want_vol=True)
    assert rc == 0 and np.isnan(v).all()                         # den == 0: this file's header
    for kind in ("opposed_edges", "checker"):
        rc, d, v = oracle.asw_geodesic(*ec.pair(kind, H, W, 3), LEFT, 15, 0, 4, want_vol=True)
        assert rc == 0 and np.isfinite(v).all() and v.max() == np.float32(765.0)
    L, R = ec.checker(H, W, 3)
    rc, d, v = oracle.asw_classic(L, R, *ec.CHECKER_GAMMAS_NAN, LEFT, 15, 0, 4, want_vol=True)
    assert rc == 0 and np.isnan(v).all()
    rc, d, v = oracle.asw_classic(L, R, *ec.CHECKER_GAMMAS_FINITE, LEFT, 15, 0, 4, want_vol=True)
    assert rc == 0 and np.isfinite(v).all() and v.max() == np.float32(255.0) and v.min() < 255


def test_xq_gammas_pass_the_guard():
    assert lut_ok(lut_classic(*ec.XQ_GAMMAS))
