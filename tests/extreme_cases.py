"""Two-level image pairs that drive the quantities behind every exactness claim of the kernels to the ends of their ranges, and the
table of those claims, shared by tests/test_extreme_cases_cpu.py (the table, the source constants and the restatements alone) and
tests/test_gpu_extreme_values.py (the kernels).  Plain numpy: nothing here needs a GPU.  TEST INFRASTRUCTURE ONLY.

Almost every kernel is compared bit for bit with the oracle or a restatement, and can be, because each rests on an argument of the
form "this sum is exact because its operands are bounded".  The other pair kinds of the suite (tests/matcher_cases.py,
tests/asw_cases.py) are near copies of each other or noise: costs are small, or the support weights are tiny wherever costs are
large.  The pairs here are built so that the largest weight and the largest cost meet on every tap of the largest window.

Parts:

  the pairs `opposed_flat`, `opposed_edges`, `checker`, `complement`, each (H, W, cn) -> (L, R), and `pair(kind, H, W, cn, swap,
  pad)`: the swapped form exchanges L and R, the padded form is matcher_cases.padded_view of both;

  the source constants the bounds are made of (`REFINE_TC_SCALE` ... `XQ_LUT_SCALE_LOG2`): tests/test_extreme_cases_cpu.py reads each
  back from the .hip / .h text, so a changed constant fails there instead of leaving the table stale;

  the cases (`REFINE_T_CASE`, `SGBM_VOLUME_CASE`, `BM_CASE`, ...) and the functions that compute the reached value of each quantity
  on the restatement alone (`refine_totals`, `cross_sums`, `adcensus_sums`, `sgbm_reached`, `bm_reached`, `tad_cost_range`, `scharr_x`);

  `TABLE`: one row per claim: the kernel, the quantity, its bound as an expression of the source constants and as a number, the
  parameters and the smallest frame that reach it, the function of the reached value, and how the bound is held ("gpu": the GPU
  test reaches it; "host": no small frame can approach it, the host check alone holds it, and the row says what is reached).  A
  row whose claim is about rounding order and not about a magnitude has no numeric reach: value and function are None.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matcher_cases as mc  # noqa: E402

LEFT, RIGHT = 0, 1


# ---------------------------------------------------------------- the pairs
def _shape(H, W, cn):
    return (H, W) if cn == 1 else (H, W, 3)


def _expand(plane, cn):
    plane = np.ascontiguousarray(plane.astype(np.uint8))
    return plane if cn == 1 else np.ascontiguousarray(np.repeat(plane[:, :, None], 3, axis=2))


def opposed_flat(H, W, cn):
    """L = 255 everywhere, R = 0 everywhere: every support weight at its maximum (colour distance 0 on every tap of both views) and
    every AD cost at its maximum (255 gray; the 3-channel mean3 rule tops out at 170)"""
    return np.full(_shape(H, W, cn), 255, np.uint8), np.zeros(_shape(H, W, cn), np.uint8)


def opposed_edges(H, W, cn, bar=2):
    """vertical bars of 0 / 255, `bar` columns wide, starting with 0; R is the complement of L.  At bar = 2 every column of L has
    x-1 and x+1 in different bars: Scharr +-4080 against -+4080 in R, the prefiltered values of StereoBM / SGBM are 0 against
    2 * cap, and the colour distance is 255 at every candidate that is a multiple of 2 * bar (0 at the odd multiples of bar)"""
    row = (np.arange(W) // bar % 2 * 255)
    L = _expand(np.broadcast_to(row[None, :], (H, W)), cn)
    return L, (255 - L).astype(np.uint8)


def checker(H, W, cn):
    """period-1 checkerboard against its complement: half the taps of every window carry the last LUT column (colour distance 255),
    the other half colour distance 0, with cost 255 on all of them at the even candidates"""
    ys, xs = np.mgrid[0:H, 0:W]
    L = _expand((ys + xs) % 2 * 255, cn)
    return L, (255 - L).astype(np.uint8)


COMPLEMENT_A, COMPLEMENT_B, COMPLEMENT_MOD = 1, 9, 251


def complement(H, W, cn):
    """L(y, x) = (x + 9 y) mod 251, R = 255 - L.  Two pixels of a census window differ by dx + 9 dy with |dx| <= 8, |dy| <= 6: it
    is 0 only for dx = dy = 0 and its magnitude stays below 251, so no two pixels of a 9 x 7 window are equal; in R every order is
    reversed, so away from the clamped border the census Hamming distance is 62 at candidate 0.  AD = |2 L - 255|"""
    ys, xs = np.mgrid[0:H, 0:W]
    L = _expand((COMPLEMENT_A * xs + COMPLEMENT_B * ys) % COMPLEMENT_MOD, cn)
    return L, (255 - L).astype(np.uint8)


KINDS = ("opposed_flat", "opposed_edges", "checker", "complement")
_MAKERS = {"opposed_flat": opposed_flat, "opposed_edges": opposed_edges, "checker": checker, "complement": complement}


def pair(kind, H, W, cn, swap=False, pad=0, **kw):
    """the pair of `kind`; swap: L and R exchanged; pad: both as views into rows `pad` pixels longer (the padding holds 0 / 255, the
    opposite of nothing in particular: no kernel may read it)"""
    L, R = _MAKERS[kind](H, W, cn, **kw)
    if swap:
        L, R = R, L
    return mc.padded_view(L, pad, 0), mc.padded_view(R, pad, 255)


def variants(kind, H, W, cn, **kw):
    """[(label, L, R)]: the pair, its swapped form and its padded-view form"""
    return [("plain",) + pair(kind, H, W, cn, **kw), ("swapped",) + pair(kind, H, W, cn, swap=True, **kw),
            ("padded",) + pair(kind, H, W, cn, pad=3, **kw)]


# ---------------------------------------------------------------- the constants of the source text (held by the CPU test)
REFINE_TC_SCALE, REFINE_TS_SCALE = 4096, 256     # ensure_refine_tables (asw_methods.hip)
REFINE_MAX_WIN, REFINE_MAX_N, REFINE_MAX_MIND = 35, 1025, 1 << 20   # check_refine_params
CROSS_MAX_L = 17                                 # k_cross.hip MAX_L: win <= 35
CROSS_MAX_WIN = 2 * CROSS_MAX_L + 1
COST_BASE_BITS = 0x45800000                      # k_wmedian*.hip: the bits of 4096.0f
WM_KEY_SHIFT_32, WM_KEY_MUL_TILE, WM_KEY_MUL_GEN = 8, 1024, 4096   # key = cost bits << 8 | index; * 1024 + index; * 4096 + index
WM_KEY_PAD_TILE, WM_KEY_PAD_GEN = 2.0 ** 42, 2.0 ** 46
SGBM_BIG = 0x3fffffff                            # k_sgbm.hip
SGBM_INT_BOUND, SGBM_F32_BOUND = 2147483648.0, 16777216.0   # sgbm_prepare
SGBM_RAW_MAX = 63                                # the raw plane >> 2
BM_MAX_CAP, BM_MAX_BLOCK = 63, 255               # bm_prepare
XQ_LUT_SCALE_LOG2 = 60                           # asw_internal.h
SCHARR_MAX = 4080                                # k_cost.hip: (3 + 10 + 3) * 255
SCANLINE_MAX, SCANLINE_MIN = (127, 7, 8), (1, 0, 1)   # the largest and the smallest penalty code (a, u, ratio)
CROSS_SCALE_Q = (255, 1)

REFINE_T_MAX = REFINE_MAX_WIN ** 2 * REFINE_TC_SCALE * REFINE_TS_SCALE   # 1 284 505 600: above 2^30, below 2^31
CROSS_S_MAX = 255 * CROSS_MAX_WIN ** 2                                   # 312 375 < 2^24
ADCENSUS_E_MAX = 127 + 127                                               # TA and TC both end at 127
BM_SAD_MAX = 2 * BM_MAX_CAP * BM_MAX_BLOCK ** 2                          # 8 193 150 < 2^23


# ---------------------------------------------------------------- refine: T at its maximum
# H, W, minD, n, win: a flat guide and gammas of 1e9 make every entry of both tables its scale, so a filled pixel whose 35 x 35 taps
# all vote has T = 1225 * 4096 * 256.  The map has two levels, the ends 0 and n - 1 of the vote range: the first bisection step of
# k_refine_median then has `below` = the weight of the votes at 0, and 2 * below passes 2^31 where more than 1024 taps vote 0.
# minD = -(n // 2) keeps both levels pointing inside a 70-column frame.  The high level minD + n - 1 = h points inside only at
# x >= h and the low level only at x < W + minD, so the fill makes the frame low left of x = h and high right of it whatever the
# draw; the share of the low level falls from 0.98 to 0.02 over the eight columns from h on to match, and the medians of the pixels
# around x = h take both values.  REFINE_ENDS_CASE is the same with n = 1025: the votes are 0 and 1024, the ends of the vote range.
REFINE_GAMMA = 1e9
REFINE_T_CASE = (40, 70, -30, 61, 35)
REFINE_ENDS_CASE = (40, 560, -520, 1025, 35)
REFINE_T_WINDOWS = (35, 15, 3)


def refine_two_level_maps(H, W, minD, n, seed=5, p_reject=0.5):
    """(dl, dr): dl takes minD or h = minD + n - 1, the lower one with a probability that falls from 0.98 (x <= h) to 0.02
    (x >= h + 8); dr agrees with dl where dl points inside the frame, except on a random half of the pixels (NaN there: rejected,
    then filled)"""
    rng = np.random.default_rng(seed)
    p_low = np.clip((minD + n - 1 + 8 - np.arange(W)) / 8.0, 0.02, 0.98)
    low = rng.random((H, W)) < p_low[None, :]
    dl = np.where(low, minD, minD + n - 1).astype(np.float32)
    xr = np.arange(W)[None, :] - dl.astype(np.int64)
    dr = np.full((H, W), np.nan, np.float32)
    ys, xs = np.nonzero((xr >= 0) & (xr < W))
    dr[ys, xr[ys, xs]] = dl[ys, xs]
    dr[rng.random((H, W)) < p_reject] = np.nan
    return dl, dr


REFINE_MIND_FRAME = (15, 70)   # 1050 pixels: every one of the 1025 values occurs


def refine_mind_end_map(minD):
    """a left map that takes every value of [minD, minD + 1025) on REFINE_MIND_FRAME: with |minD| = 1 << 20 each points outside"""
    H, W = REFINE_MIND_FRAME
    return (minD + np.arange(H * W).reshape(H, W) % REFINE_MAX_N).astype(np.float32)


def refine_equal_maps(H, W, d):
    """an all-equal map d >= 0 whose first d columns point outside (rejected, filled from the right); dr agrees elsewhere"""
    dl = np.full((H, W), d, np.float32)
    return dl, dl.copy()


def refine_totals(G, F, win, gamma_c, gamma_s, mid):
    """(T, below): per pixel the total weight of the voting taps and the weight of the votes <= mid, in Python-sized integers
    (int64; the kernel keeps both in 32 unsigned bits), from refine_ref's tables and the fill F alone"""
    import refine_ref as ref
    g = ref._guide(G)
    H, W = F.shape
    k = win // 2
    tc, ts = ref.tables(win, gamma_c, gamma_s, g.shape[2])
    gp = np.zeros((H + 2 * k, W + 2 * k, g.shape[2]), np.int64)
    gp[k:k + H, k:k + W] = g
    fp = np.full((H + 2 * k, W + 2 * k), -1, np.int64)
    fp[k:k + H, k:k + W] = F
    T, below = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    for j in range(-k, k + 1):
        for i in range(-k, k + 1):
            f = fp[k + j:k + j + H, k + i:k + i + W]
            dc = np.abs(g - gp[k + j:k + j + H, k + i:k + i + W]).sum(axis=2)
            w = np.where(f >= 0, tc[dc] * ts[abs(j), abs(i)], 0)
            T += w
            below += np.where(f <= mid, w, 0)
    return T, below


def refine_fill(dl, dr, minD, max_diff=1.0):
    """(F, mask) of refine_ref's steps 1 and 2"""
    import refine_ref as ref
    dl, dr = np.asarray(dl, np.float32), np.asarray(dr, np.float32)
    return ref.fill_vec(dl, ref.cross_check_vec(dl, dr, max_diff), minD)


# ---------------------------------------------------------------- cross: S at its maximum
CROSS_FRAME = (40, 70)           # rows 17 .. 22 and columns 17 .. 52 hold a whole 35 x 35 region
CROSS_WINDOWS = (35, 3)
# AD-Census: the table's largest cost is TA[255] + TC[62] = 254 at lambdas (1, 1).  On `complement` every 35 x 35 window of the ramp
# x + 9 y spans 340 > 251 values, so it holds pixels with |2 L - 255| <= 1 (TA <= 80) and pixels whose census window wraps: the
# product 254 * 1225 cannot be reached there, and the CPU test states what is.  `checker` reaches it: AD 255 and Hamming 31 (the
# odd-parity half of the window), TC[31] = 127 at lambda_census 1, on every pixel four columns and three rows off the border.
ADCENSUS_FRAME = (43, 72)        # 35 + 2 * 4 rows, 35 + 2 * 4 columns and some more: one whole region off the clamped census border
ADCENSUS_LAMBDAS = (1, 1)


def adcensus_sums(L, R, dt, tau, win, minD, D, lambdas=ADCENSUS_LAMBDAS):
    """(S, N, E, disp, e) of adcensus_ref.match with the u8 cost volume e"""
    import adcensus_ref as ar
    e = ar.cost(L, R, dt, lambdas[0], lambdas[1], minD, D)
    return ar.match(L, R, dt, tau, lambdas[0], lambdas[1], win, minD, D, e=e) + (e,)


def cross_sums(L, R, dt, tau, trunc, win, minD, D):
    """(S, N, E, disp) of cross_ref.aggregate over adcensus_ref.ad (computeAD's value, restated there)"""
    import adcensus_ref as ar
    import cross_ref as cr
    return cr.aggregate(ar.ad(L, R, dt, minD, D), cr.arms(R if dt else L, tau, win // 2), trunc, minD)


# ---------------------------------------------------------------- SGBM with a kept volume
# H, W, cn, minD, D, block, preFilterCap: complementary 2-pixel bars.  P2 is the largest the host accepts with the volume handed
# back for eight paths, P1 = P2 - 1: L(p, d) - min L grows by C(d) - C(min) a step until it meets P2, so S needs paths of a few
# dozen steps in every direction to pass 2^23 (24 rows reach 0.40 * 2^24, 64 rows 0.57 * 2^24).
SGBM_VOLUME_CASE = (64, 100, 3, 0, 16, 11, 63)
SGBM_MASKS = (0x07, 0xFF)


def sgbm_largest_p2(cn, w, cap, paths, want_volume=True, census=False):
    """the largest P2 sgbm_prepare accepts: popcount(paths) * (C_max + P2) < 2^24 with a volume, < 2^31 without"""
    import sgbm_census_ref as cref
    import sgbm_ref as ref
    n = bin(paths).count("1")
    cmax = cref.cost_bound(w) if census else ref.cost_bound(cn, w, max(cap, 15) | 1)
    bound = int(SGBM_F32_BOUND if want_volume else SGBM_INT_BOUND)
    p2 = (bound - 1) // n - cmax
    assert n * (cmax + p2) < bound <= n * (cmax + p2 + 1)
    return p2


def sgbm_volume_args(paths):
    """(L, R, positional arguments of sgbm_paths_ref.sgbm_paths / ctx.sgbm_paths after the images)"""
    H, W, cn, minD, D, w, cap = SGBM_VOLUME_CASE
    L, R = opposed_edges(H, W, cn, 2)
    P2 = sgbm_largest_p2(cn, w, cap, paths)
    return L, R, (minD, D, w, P2 - 1, P2, 1, cap, 0, 0, 0, paths)


def sgbm_reached(paths):
    """(largest S, largest single L, C_max of the host's bound, largest C) of the case, on sgbm_paths_ref alone"""
    import sgbm_paths_ref as pref
    import sgbm_ref as ref
    H, W, cn, minD, D, w, cap = SGBM_VOLUME_CASE
    L, R, a = sgbm_volume_args(paths)
    C = ref.block_cost(L, R, minD, D, w, max(cap, 15) | 1)
    lmax = max(int(pref.path(C, a[3], a[4], dx, dy).max()) for bit, (dx, dy) in pref.DIRS.items() if paths & bit)
    S = pref.aggregate_paths(C, a[3], a[4], paths)
    return int(S.max()), lmax, ref.cost_bound(cn, w, max(cap, 15) | 1), int(C.max())


# ---------------------------------------------------------------- StereoBM
# H, W, minD, D, block: the largest block the host accepts (255), cap 63: complementary 2-pixel bars prefilter to 0 against 2 * cap
# on every column but the first and the last, so a block SAD is 2 * cap * w^2 = 8 193 150 at every candidate = 0 mod 4 whose window
# stays off those two columns.  H is even: with an odd H the last prefiltered row is all cap.  The restatement takes 0.04 s.
BM_CASE = (256, 300, 0, 16, 255)
BM_SETTINGS = (63, 10, 15, 0, 0, -1)  # preFilterCap, textureThreshold, uniquenessRatio, speckleWindowSize, speckleRange, disp12MaxDiff


def bm_pair():
    H, W = BM_CASE[:2]
    return opposed_edges(H, W, 1, 2)


def bm_reached():
    """the restatement's result dict of the case (disp, vol, raw)"""
    import stereobm_ref as bm
    H, W, minD, D, w = BM_CASE
    cap, tex, U, sw, sr, M = BM_SETTINGS
    return bm.stereo_bm(*bm_pair(), minD, D, w, cap, tex, U, sw, sr, M)


# ---------------------------------------------------------------- the TAD C+G cost and the weighted median's keys
SIM_PARAMS = (0.4, 10.0, 50.0)   # regularity, thresC, thresG of run_wmedian (M.cpp:3250)
WMEDIAN_FRAME = (20, 70)
WMEDIAN_WINDOWS = {"k_wmedian": 39, "k_wmedian_tile": 15, "k_wmedian_tile_gen": 17}   # run_wmedian: per-pixel sort from 39 on


def tad_cost_range():
    """(min, max) of the TAD C+G cost with the weighted median's literals over all uint8 inputs, from the lines of
    similarity_ref.similarity_literal after the differences, on the ends of its inputs: channel differences all 0 and all 255 (the
    colour mean saturates: (min(255, 255 + 255) + 255) / 3 = 170; the colour term is not decreasing in it: 0 up to thresC, then
    c + 10), Scharr differences all 0 and all 8160 = 2 * 4080 (the gradient term is 255 * thresG up to thresG and 254 * thresG + g
    above it, and 12700 + g > 12750 there)"""
    import cvlite as cv
    F32 = np.float32
    reg, thresC, thresG = SIM_PARAMS
    out = []
    for diff, grad in ((0, 0.0), (255, 2.0 * SCHARR_MAX)):
        c = np.array([[diff]], np.uint8)
        color_ = cv.addWeighted_u8(cv.add_u8(c, c), 1.0 / 3.0, c, 1.0 / 3.0)
        cmp_c = cv.compare_gt(color_, thresC)
        m1 = cv.mul_u8(color_, cmp_c, 1.0 / 255.0)
        cost_c = cv.addWeighted_u8(m1, 1.0, cmp_c, thresC * (1.0 / 255.0)).astype(F32)
        g = np.array([[grad]], F32)
        cur = cv.addWeighted_f32(g + g, 1.0 / 3.0, g, 1.0 / 3.0)
        bit = cv.scale_u8(cv.compare_gt(cur, thresG), 1.0 / 255.0)
        cost_g = np.bitwise_not(bit).astype(F32) * F32(thresG) + cur * bit.astype(F32)
        out.append(float((cost_c * F32(1 - reg) + cost_g * F32(reg))[0, 0]))
    return tuple(out)


def key_bits(cost):
    """the f32 bits of a cost minus those of 4096.0f: the weighted median's keys hold this in 24 bits"""
    return int(np.float32(cost).view(np.uint32)) - COST_BASE_BITS


def scharr_x(img):
    """the x-Scharr response (3, 10, 3) of a u8 plane with replicated borders, int64: only its extremes are used here"""
    a = np.pad(np.asarray(img).astype(np.int64), 1, mode="edge")
    d = a[:, 2:] - a[:, :-2]
    return 3 * d[:-2] + 10 * d[1:-1] + 3 * d[2:]


# ---------------------------------------------------------------- the float families
FLOAT_FRAME = (20, 70)
CHECKER_GAMMAS_NAN, CHECKER_GAMMAS_FINITE = (30.0, 0.01), (30.0, 20.0)   # gamma_g 0.01: exp(-sqrt(2) / 0.01) is 0 in f32
XQ_FRAME = (17, 130)
XQ_GAMMAS = (30.0, 20.0)


# ---------------------------------------------------------------- the table
def _row(kernel, quantity, bound, value, reach, reached, held):
    return {"kernel": kernel, "quantity": quantity, "bound": bound, "value": value, "reach": reach, "reached": reached, "held": held}


def _refine_reached():
    H, W, minD, n, win = REFINE_T_CASE
    dl, dr = refine_two_level_maps(H, W, minD, n)
    F, mask = refine_fill(dl, dr, minD)
    T, below = refine_totals(np.full((H, W), 255, np.uint8), F, win, REFINE_GAMMA, REFINE_GAMMA, (n - 1) >> 1)
    return int(T[mask == 1].max()), int(2 * below[mask == 1].max())


def _cross_reached():
    H, W = CROSS_FRAME
    L, R = opposed_flat(H, W, 1)
    return int(cross_sums(L, R, LEFT, 20, 255, CROSS_MAX_WIN, 0, 2)[0].max())


def _adcensus_reached():
    H, W = ADCENSUS_FRAME
    L, R = checker(H, W, 1)
    return int(adcensus_sums(L, R, LEFT, 255, CROSS_MAX_WIN, 0, 2)[0].max())


def _bm_reached():
    return int(np.nanmax(bm_reached()["vol"]))


def _scharr_reached():
    L, R = opposed_edges(9, 70, 1, 2)
    return int(scharr_x(L).max()), int(scharr_x(L).min())


def _twopass_reached():
    import twopass_ref as tp
    H, W = FLOAT_FRAME
    L, R = opposed_flat(H, W, 1)
    return float(tp.twopass(L, R, 30, 20, 35, 0, 4, LEFT)[1].max())


def _xq_reached():
    from test_xq_scaled_domain_cpu import lut_classic
    lut = lut_classic(*XQ_GAMMAS).astype(np.float64)
    return float(lut[lut > 0].min() ** 2)


def _permeability_reached():
    import adcensus_ref as ar
    import permeability_ref as pm
    H, W = FLOAT_FRAME
    L, R = opposed_flat(H, W, 1)
    e = ar.ad(L, R, LEFT, 0, 3)
    return float(min(int(e.max()), pm.aggregate(e, L, 255, 255, 0)[0].max()))


def _scanline_reached():
    import scanline_ref as sl
    return float(sl.penalties(*SCANLINE_MAX)[1])


TABLE = [
    _row("k_refine.hip k_refine_median", "T, the total weight of a window",
         "REFINE_MAX_WIN^2 * REFINE_TC_SCALE * REFINE_TS_SCALE < 2^31", REFINE_T_MAX,
         "win 35, gamma_c = gamma_s = 1e9, flat guide, %r" % (REFINE_T_CASE,), lambda: _refine_reached()[0], "gpu"),
    _row("k_refine.hip k_refine_median", "2u * below of the bisection", "2 * T < 2^32: fits only because it is unsigned",
         2 * REFINE_T_MAX, "the same case: more than 1024 taps vote 0 at the first step", lambda: _refine_reached()[1], "gpu"),
    _row("k_refine.hip k_refine_check / k_refine_fill", "(float)(minD + n), minD - 1",
         "|minD| <= REFINE_MAX_MIND, n <= REFINE_MAX_N: below 2^24, exact in f32", REFINE_MAX_MIND + REFINE_MAX_N,
         "n 1025, minD -(1 << 20) and (1 << 20): every disparity points outside any frame, so every pixel is unfillable",
         lambda: int(refine_mind_end_map(REFINE_MAX_MIND).max()) + 1, "gpu"),   # the largest value of the map, plus one: minD + n
    _row("k_cross.hip", "S of entry 12", "255 * (2 * MAX_L + 1)^2 < 2^24", CROSS_S_MAX,
         "gray opposed_flat, trunc 255, win 35, %r" % (CROSS_FRAME,), _cross_reached, "gpu"),
    _row("k_cross.hip", "S of AD-Census", "(127 + 127) * (2 * MAX_L + 1)^2 < 2^24", ADCENSUS_E_MAX * CROSS_MAX_WIN ** 2,
         "gray checker, tau 255, lambdas (1, 1), win 35, %r" % (ADCENSUS_FRAME,), _adcensus_reached, "gpu"),
    _row("k_sgbm.hip, sgbm_prepare", "S with the volume handed back", "n * (C_max + P2) < 16777216", int(SGBM_F32_BOUND),
         "opposed_edges(2), %r, 8 paths, the largest P2, P1 = P2 - 1" % (SGBM_VOLUME_CASE,), lambda: sgbm_reached(0xFF)[0], "gpu"),
    _row("k_sgbm.hip, sgbm_prepare", "S and L without a volume; SGBM_BIG + P1", "n * (C_max + P2) < 2147483648; BIG + P1 < 2^31",
         int(SGBM_INT_BOUND), "L grows by at most C_max a step: no small frame approaches it, and on the periodic pairs a penalty of 7e8 "
         "enters no sum.  sgbm / sgbm_census are served at their largest accepted P2 and refused at one more: the host check alone", lambda: sgbm_reached(0xFF)[1], "host"),
    _row("k_bm.hip", "a block SAD", "2 * 63 * 255^2 < 2^23", BM_SAD_MAX,
         "opposed_edges(2), %r, cap 63" % (BM_CASE,), _bm_reached, "gpu"),
    _row("k_wmedian.hip, k_wmedian_tile*.hip", "the TAD C+G cost and its key bits",
         "[4096, 16384): bits - COST_BASE_BITS < 2^24; keys below 2^32, 2^42, 2^46", 1 << 24,
         "opposed_edges(2): candidate 0 = 0 mod 4 gives the maximum, candidate 2 the minimum", lambda: key_bits(tad_cost_range()[1]), "gpu"),
    _row("k_cost.hip", "the Scharr response", "(3 + 10 + 3) * 255 = 4080 -> int16", SCHARR_MAX,
         "opposed_edges(2), 9 x 70", lambda: _scharr_reached()[0], "gpu"),
    _row("k_bilateral.hip, k_twopass.hip, k_geodesic*.hip", "ab * cost, the volume",
         "24 x 8 bits: exact in f64; E <= 255", 255.0, "opposed_flat: every plane is 255.0 (two-pass restatement, window 35)",
         _twopass_reached, "gpu"),
    _row("k_bilateral_xq.hip", "the smallest nonzero weight product", "nonzero products >= 2^-68, (max * 2^XQ_LUT_SCALE_LOG2)^2 < 2^128",
         2.0 ** -68, "gammas %r on opposed_edges, checker, complement at %r" % (XQ_GAMMAS, XQ_FRAME), _xq_reached, "gpu"),
    _row("k_permeability.hip", "e and E of the f64 scans", "e <= trunc <= 255, permeability <= 1: E <= 255", 255.0,
         "sigma 255, trunc 255 on gray opposed_flat (permeability_ref on the AD of adcensus_ref)", _permeability_reached, "gpu"),
    _row("k_scanline.hip", "P2 of the largest code", "ratio * a * 4^(u - 5) = 8 * 127 * 16, exact in f32", 127.0 * 16 * 8,
         "codes (127, 7, 8) and (1, 0, 1) over volumes whose planes are all equal", _scanline_reached, "gpu"),
    # rows without a numeric reach: the GPU file runs the named cases, the claim is about rounding order, not about a magnitude
    _row("k_cross_scale.hip", "the f64 weights and sum", "q in 1..255", None, "q 255 and 1 over the same volumes", None, "gpu"),
    _row("k_subpixel.hip", "zero denominators", "one IEEE operation a statement", None,
         "parabola and equiangular over volumes whose planes are all equal", None, "gpu"),
    _row("k_bilgrid.hip, k_ncc.hip, k_blo1.hip", "integer bin sums, f32 / f64 sums in the oracle's order", "bit-equal to the oracle", None,
         "the four pairs at the default and the largest served window", None, "gpu"),
    _row("k_guided.hip", "the cancellation var = E[I^2] - E[I]^2 at intensity 255", "asw_cases.tolerance", None,
         "opposed_flat, opposed_edges, checker; eps 1e-6 and 1e-8; fused walk against two passes", None, "gpu"),
    _row("k_prep.hip", "the saturating V + 2 (V - blur), normalize with max == min", "u8 saturation; scale 0", None,
         "preprocess_pair with the detail boost on opposed_edges and checker; a constant map", None, "gpu"),
]
