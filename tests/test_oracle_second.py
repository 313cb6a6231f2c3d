"""Second restatements: every function below re-states one reference function Mat operation by Mat
operation on numpy arrays, building the intermediate Mats the way aswMethods.cpp does and calling one tests/cvlite.py
primitive per cv:: call.  The C oracle states the same functions fused per pixel.  Neither can be pinned by the reference
(it ships no fixtures and needs OpenCV 4.1.0) -- so the known-answer test is that the two agree BIT FOR BIT on seeded frames:
a transcription error in either shows up as a mismatch.  CPU only; sizes chosen for seconds."""
import numpy as np
import pytest

from aswstereomatch_amd.synth import make_pair

from tests import cvlite as cv
from tests.similarity_ref import similarity_literal  # shared with tests/test_geometry_cases_cpu.py

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------
# getGuidedFilter, M.cpp:2766-2854 (+ multiChl_to_oneChl_mul 2727-2764, operator* 22-31)
# ------------------------------------------------------------------------------------------------------------------
def dot_channels(a, b):
    """multiChl_to_oneChl_mul: operator*(Vec3f / Vec6f): products added left to right (M.cpp:22-31)."""
    acc = a[..., 0] * b[..., 0]
    for c in range(1, a.shape[2]):
        acc = acc + a[..., c] * b[..., c]
    return acc


def guided_filter_literal(guidedImg, inputP, r, eps, box_mode=0):
    assert guidedImg.shape[:2] == inputP.shape and guidedImg.shape[2] in (3, 6)
    I = cv.normalize_minmax(guidedImg)                        # :2774 (global over all channels)
    P = cv.normalize_minmax(inputP)                           # :2775 (per call = per disparity slice)
    meanGuid = cv.boxFilter(I, r, box_mode)                   # :2778
    meanP = cv.boxFilter(P, r, box_mode)                      # :2780
    corrGuidP = np.stack([cv.boxFilter(I[..., c] * P, r, box_mode) for c in range(I.shape[2])], axis=2)  # :2785-2792
    corrGuid = cv.boxFilter(I * I, r, box_mode)               # :2796
    varGuid = corrGuid - meanGuid * meanGuid                  # :2799
    meanGuidmulP = np.stack([meanGuid[..., c] * meanP for c in range(I.shape[2])], axis=2)  # :2806-2812
    covGuidP = corrGuidP - meanGuidmulP                       # :2815
    ones = np.ones(varGuid.shape, F32)
    a = covGuidP / (ones * F32(eps) + varGuid)                # :2846  (varGuid + mergeOnes*eps -> scaleAdd(ones, eps, var))
    b = meanP - dot_channels(a, meanGuid)                     # :2847
    a = cv.boxFilter(a, r, box_mode)                          # :2849
    b = cv.boxFilter(b, r, box_mode)                          # :2850
    return dot_channels(a, I) + b                             # :2852


def test_guided_filter_second_restatement(oracle):
    rng = np.random.default_rng(41)
    for (H, W, r, C) in ((23, 37, 5, 3), (19, 30, 7, 6), (12, 9, 15, 3), (9, 14, 4, 6)):
        guide = rng.integers(0, 256, (H, W, C)).astype(np.uint8)
        P = (rng.random((H, W), dtype=F32) * 300 + 4000).astype(F32)
        rc, q = oracle.guided_filter(guide, P, r, 1e-6)
        assert rc == 0 and np.array_equal(q, guided_filter_literal(guide, P, r, 1e-6)), (H, W, r, C)
    # OpenCV's literal sliding RowSum / ColumnSum form: both restatements again agree with each other bit for bit
    guide = rng.integers(0, 256, (21, 26, 3)).astype(np.uint8)
    P = rng.random((21, 26), dtype=F32)
    oracle.set_box_mode(1)
    try:
        rc, q1 = oracle.guided_filter(guide, P, 5, 1e-6)
    finally:
        oracle.set_box_mode(0)
    assert np.array_equal(q1, guided_filter_literal(guide, P, 5, 1e-6, box_mode=1))


# ------------------------------------------------------------------------------------------------------------------
# computeSimilarity ("TAD C+G"), M.cpp:415-487 (the only branch that can execute) and the padded overload 651-668
# ------------------------------------------------------------------------------------------------------------------
def test_similarity_second_restatement(oracle):
    for seed, (H, W, minD, numD) in enumerate(((14, 31, 0, 9), (9, 12, 2, 17), (6, 40, 1, 5))):
        L, R, _ = make_pair(H, W, min(numD, W // 2), seed=60 + seed, block=6)
        rc, v = oracle.compute_similarity(L, R, 0.4, 10, 50, 0, minD, numD)
        assert rc == 0 and np.array_equal(v, similarity_literal(L, R, 0.4, 10, 50, minD, numD)), (H, W, minD, numD)
        # other literals: fractional / large thresholds exercise the compare and saturation paths
        rc, v = oracle.compute_similarity(L, R, 0.25, 37.5, 1200.0, 0, minD, numD)
        assert rc == 0 and np.array_equal(v, similarity_literal(L, R, 0.25, 37.5, 1200.0, minD, numD))
    # padded overload: copyMakeBorder(plane, h, h, h, h, BORDER_REFLECT) of every plane (M.cpp:662-667)
    L, R, _ = make_pair(10, 17, 4, seed=66, block=5)
    rc, vp = oracle.compute_similarity(L, R, 0.4, 10, 50, 0, 0, 4, win=7)
    want = np.stack([cv.copyMakeBorder(p, 3, 3, 3, 3, cv.BORDER_REFLECT) for p in similarity_literal(L, R, 0.4, 10, 50, 0, 4)])
    assert rc == 0 and np.array_equal(vp, want)


# ------------------------------------------------------------------------------------------------------------------
# geodesic windows (getWinGeoDist / getGeodesicDist, M.cpp:1328-1424) and aggregation (M.cpp:1436-1534)
# ------------------------------------------------------------------------------------------------------------------
def color_dist(a, b):   # getColorDist, M.cpp:1321-1326 (exact small integers)
    return float(abs(int(a[0]) - int(b[0])) + abs(int(a[1]) - int(b[1])) + abs(int(a[2]) - int(b[2])))


def geodesic_windows_literal(img, win, iter_time=3):
    H, W = img.shape[:2]
    h = win // 2
    ext = cv.copyMakeBorder(img, h + 1, h + 1, h + 1, h + 1, cv.BORDER_REFLECT)     # :1404
    FLT_MAX = np.finfo(F32).max
    out = {}
    for i in range(h + 1, W + h + 1):                                               # :1410
        for j in range(h + 1, H + h + 1):
            o = ext[j - h - 1:j + h + 2, i - h - 1:i + h + 2]
            d = np.full((win + 2, win + 2), FLT_MAX, F32)                           # :1416
            d[h + 1, h + 1] = 0                                                     # :1417
            for it in range(iter_time):                                             # getWinGeoDist, :1339
                if it // 2 == 1:        # forward pass: L, UL, U, UR                  :1341-1363
                    for r in range(1, win + 1):
                        for c in range(1, win + 1):
                            for (dr, dc) in ((0, -1), (-1, -1), (-1, 0), (-1, 1)):
                                d[r, c] = min(d[r, c], F32(d[r + dr, c + dc] + F32(color_dist(o[r + dr, c + dc], o[r, c]))))
                elif it // 2 == 0:      # backward pass: R, BR, B, BL (iterations 0 AND 1, App. B-8)   :1365-1387
                    for r in range(win, 0, -1):
                        for c in range(win, 0, -1):
                            for (dr, dc) in ((0, 1), (1, 1), (1, 0), (1, -1)):
                                d[r, c] = min(d[r, c], F32(d[r + dr, c + dc] + F32(color_dist(o[r + dr, c + dc], o[r, c]))))
            out[(i - h - 1, j - h - 1)] = d[1:win + 1, 1:win + 1].copy()            # :1420-1421, key Point(x, y)
    return out


def geodesic_asw_literal(L, R, disp_type, win, minD, numD):
    H, W = L.shape[:2]
    h = win // 2
    wl, wr = geodesic_windows_literal(L, win), geodesic_windows_literal(R, win)     # :1464-1465
    vol = np.zeros((numD + 1, H, W), F64)
    for off in range(minD, minD + numD + 1):                                        # :1467 (inclusive)
        for y in range(H):
            for x in range(W):
                num = den = 0.0
                for j in range(win):
                    for i in range(win):
                        if disp_type == 0:                                          # :1482-1492
                            nx, ny = min(max(0, x - h + i), W - 1), min(max(0, y - h + j), H - 1)
                            a, b = wl[(x, y)][j, i], wr[(max(0, x - off), y)][j, i]
                            c = F32(color_dist(L[ny, nx], R[ny, max(0, nx - off)]))
                        else:                                                       # :1503-1516
                            nx, ny = min(max(0, x + i - h), W - 1), min(max(0, y + j - h), H - 1)
                            a, b = wl[(min(x + off, W - 1), y)][j, i], wr[(x, y)][j, i]
                            c = F32(color_dist(R[ny, nx], L[ny, min(W - 1, nx + off)]))
                        with np.errstate(over="ignore", invalid="ignore"):
                            ab = F32(a * b)
                            num += float(F32(ab * c))                               # float * float * float, then += double
                            den += float(ab)
                with np.errstate(invalid="ignore", divide="ignore"):
                    vol[off - minD, y, x] = np.float64(num) / np.float64(den)
    return vol


def test_geodesic_second_restatement(oracle):
    L, R, _ = make_pair(7, 11, 3, seed=71, block=4)
    L[2:5, 3:8] = L[2, 3]      # a flat patch: zero distances, 0/0 windows
    for win in (3, 5):
        rc, w = oracle.geodesic_dist(L, win, 3)
        lit = geodesic_windows_literal(L, win)
        assert rc == 0 and all(np.array_equal(w[y, x], lit[(x, y)]) for y in range(7) for x in range(11))
        for dt in (0, 1):
            rc, d, v = oracle.asw_geodesic(L, R, dt, win, 1, 3, want_vol=True)
            want = geodesic_asw_literal(L, R, dt, win, 1, 3)
            assert rc == 0 and np.array_equal(v, want.astype(F32), equal_nan=True), (win, dt)
            # WTA: strict '<' in ascending d on the f64 values, NaN never selected, untouched pixels = 0 (M.cpp:1523-1528)
            best = np.full((7, 11), np.finfo(F64).max)
            dd = np.zeros((7, 11), F32)
            for k in range(want.shape[0]):
                m = want[k] < best
                best[m] = want[k][m]
                dd[m] = 1 + k
            assert np.array_equal(d, dd)


# ------------------------------------------------------------------------------------------------------------------
# weighted median, M.cpp:3139-3308 (DISPARITY_LEFT)
# ------------------------------------------------------------------------------------------------------------------
def color_weight_gau_literal(src, rateR, win):                                       # computeColorWeightGau, :3139-3205
    H, W = src.shape[:2]
    h = win // 2
    b = cv.copyMakeBorder(src, h, h, h, h, cv.BORDER_REFLECT)                        # :3156
    out = np.zeros((H, W, win, win), F32)
    al = (1.0 / rateR) * (-1.0)                                                      # MatExpr: (..)/rateR*(-1): scalars folded in double
    for y in range(H):
        for x in range(W):
            w = b[y:y + win, x:x + win]                                              # :3164
            d = [cv.absdiff(w[..., c], w[h, h, c]).astype(F32) for c in range(3)]    # :3168-3175
            # (d0 + d1 + d2) / rateR * (-1): d0 + d1 materialised, then addWeighted(t, al, d2, al)   :3177
            rangeDiff = cv.addWeighted_f32(d[0] + d[1], al, d[2], al)
            out[y, x] = cv.cv_exp_f32(rangeDiff)                                     # :3179
    return out


def space_weight_gau_literal(win, rateS):                                            # computeSpaceWeightGau, :3207-3226
    h = win // 2
    k = np.zeros((win, win), F32)
    for y in range(win):
        yDist = F32((y - h) * (y - h))
        for x in range(win):
            k[x, y] = F32((x - h) * (x - h)) + yDist                                 # :3221 (written as at(x, y))
    return cv.cv_exp_f32(k * F32((1.0 / rateS) * (-1.0)))                            # :3225


def wmedian_literal(L, R, win, rateS, rateR, minD, numD):
    H, W = L.shape[:2]
    h = win // 2
    max_offset = minD + numD - 1
    rightImg_border = cv.copyMakeBorder(R, 0, 0, max_offset, 0, cv.BORDER_REFLECT)   # :3246
    costs = [cv.copyMakeBorder(p, h, h, h, h, cv.BORDER_REFLECT) for p in similarity_literal(L, R, 0.4, 10, 50, minD, numD)]  # :3250
    weightDist = space_weight_gau_literal(win, rateS)                                # :3255
    wL = color_weight_gau_literal(L, rateR, win)                                     # :3262
    wR = color_weight_gau_literal(rightImg_border, rateR, win)                       # :3263
    vol = np.zeros((numD, H, W), F32)
    for offset in range(numD):                                                       # :3264
        for y in range(H):
            for x in range(W):
                cost_win = costs[offset][y:y + win, x:x + win]                       # :3273
                weight_win = wL[y, x] * weightDist * wR[y, x - offset + numD - 1]    # :3274
                pairs = sorted(((float(cost_win[wy, wx]), wy * win + wx, float(weight_win[wy, wx]))
                                for wy in range(win) for wx in range(win)), key=lambda t: (t[0], t[1]))  # multimap: key, then insertion order
                half = cv.sum_f64_rowmajor(weight_win) / 2                           # :3284
                partial = 0.0
                for idx, (c, _, w) in enumerate(pairs):                              # :3288-3304
                    partial += w
                    if partial > half:
                        vol[offset, y, x] = pairs[idx][0] if idx == 0 else pairs[idx - 1][0]
                        break
    return vol


def test_wmedian_second_restatement(oracle):
    L, R, _ = make_pair(6, 9, 3, seed=81, block=4)
    for win, minD, numD in ((3, 0, 4), (5, 0, 3)):
        rc, d, v = oracle.asw_wmedian(L, R, 0, win, 10, 10, minD, numD, want_vol=True)
        want = wmedian_literal(L, R, win, 10, 10, minD, numD)
        assert rc == 0 and np.array_equal(v, want), (win, minD, numD)
        assert np.array_equal(d, np.argmin(want.astype(F64), axis=0).astype(F32) + minD)   # strict '<': first minimum


# ------------------------------------------------------------------------------------------------------------------
# getCostSAD_d (M.cpp:2442-2503) and computeAdaptiveWeight_BLO1 (M.cpp:2505-2725)
# ------------------------------------------------------------------------------------------------------------------
def cost_sad_d_literal(left, right, disparity, disp_type, win):
    """left / right: gray u8; the non-reference view already bordered by the caller (M.cpp:2877-2878, 2522-2523)."""
    if disp_type == 0:
        H, W = left.shape
        roi = right[:, right.shape[1] - W - disparity:right.shape[1] - disparity]    # :2478
        diff = cv.absdiff(left, roi).astype(F32)                                     # :2478-2479
    else:
        H, W = right.shape
        diff = cv.absdiff(left[:, disparity:disparity + W], right).astype(F32)      # :2493-2494
    return cv.boxFilter(diff, win)                                                   # :2480 / 2495


def blo1_literal(L, R, disp_type, sampleRateR, win, numD):
    H, W = L.shape[:2]
    gl, gr = cv.cvtColor_BGR2GRAY(L), cv.cvtColor_BGR2GRAY(R)                         # :2514-2521
    max_offset = numD - 1                                                            # minDisparity = 0
    lb = cv.copyMakeBorder(gl, 0, 0, 0, max_offset, cv.BORDER_REFLECT)               # :2522
    rb = cv.copyMakeBorder(gr, 0, 0, max_offset, 0, cv.BORDER_REFLECT)               # :2523
    costs = [cost_sad_d_literal(gl, rb, i, 0, win) if disp_type == 0 else cost_sad_d_literal(lb, gr, i, 1, win)
             for i in range(0, max_offset + 1)]                                      # :2529-2547
    step = int(256 * sampleRateR)                                                    # :2550
    keys = list(range(0, 256, step))                                                 # :2551-2556
    if 255 not in keys:
        keys.append(255)                                                             # :2557-2560
    JB = {}
    for k in keys:                                                                   # :2568 / 2596
        fixed = cv.absdiff(gl if disp_type == 0 else gr, np.uint8(k)).astype(F32)    # abs(img - k) == absdiff, :2571 / 2599
        Js = []
        for i in range(numD):
            if disp_type == 0:
                other = cv.absdiff(rb[:, max_offset - i:max_offset - i + W], np.uint8(k)).astype(F32)   # :2577
                M = other * fixed                                                    # M_k_y_r.mul(M_k_y_l), :2579
            else:
                other = cv.absdiff(lb[:, i:i + W], np.uint8(k)).astype(F32)          # :2605
                M = fixed * other                                                    # :2607
            Js.append(cv.boxFilter(M * costs[i], win))                               # :2581-2583
        Mb = cv.boxFilter(M, win)                                                    # :2587: the LAST disparity's M only
        with np.errstate(divide="ignore", invalid="ignore"):
            JB[k] = [J / Mb for J in Js]                                             # :2593
    ref = gl if disp_type == 0 else gr
    vol = np.zeros((numD, H, W), F64)
    for y in range(H):
        for x in range(W):
            cur = int(ref[y, x])
            for off in range(numD):                                                  # :2645
                if cur not in JB:                                                    # :2650-2661
                    lower = cur // step * step
                    upper = min(lower + step, 255)
                    with np.errstate(invalid="ignore", over="ignore"):
                        t = F32(F32(cur - lower) * JB[lower][off][y, x]) + F32(F32(upper - cur) * JB[upper][off][y, x])
                    vol[off, y, x] = float(F32(t))
                else:
                    vol[off, y, x] = float(JB[cur][off][y, x])                        # :2665
    return vol


def test_blo1_second_restatement(oracle):
    L, R, _ = make_pair(11, 16, 4, seed=91, block=5)
    for dt in (0, 1):
        rc, d, v = oracle.asw_blo1(L, R, dt, 0.015, 5, 0, 4, want_vol=True)
        want = blo1_literal(L, R, dt, 0.015, 5, 4)
        assert rc == 0 and np.array_equal(v, want.astype(F32), equal_nan=True), dt
    # getCostSAD_d alone, as M.cpp:2884-2889 loops it
    gl, gr = cv.cvtColor_BGR2GRAY(L), cv.cvtColor_BGR2GRAY(R)
    rb = cv.copyMakeBorder(gr, 0, 0, 5, 0, cv.BORDER_REFLECT)
    rc, sad = oracle.cost_sad(L, R, 0, 7, 0, 6)
    assert rc == 0 and all(np.array_equal(sad[i], cost_sad_d_literal(gl, rb, i, 0, 7)) for i in range(6))


# ------------------------------------------------------------------------------------------------------------------
# the two BGR2GRAY constant sets: one switch in the oracle, both self-consistent
# ------------------------------------------------------------------------------------------------------------------
def test_gray_constants_switch(oracle):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (40, 50, 3)).astype(np.uint8)
    g14 = oracle.bgr2gray(img)
    assert np.array_equal(g14, cv.cvtColor_BGR2GRAY(img, 14))
    oracle.set_gray_bits(15)
    try:
        g15 = oracle.bgr2gray(img)
        assert np.array_equal(g15, cv.cvtColor_BGR2GRAY(img, 15))
        L, R, _ = make_pair(12, 30, 5, seed=3, block=6)
        rc, d15, v15 = oracle.asw_classic(L, R, 30, 20, 0, 5, 0, 5, want_vol=True)
    finally:
        oracle.set_gray_bits(14)
    diff = g14.astype(int) - g15.astype(int)
    assert np.abs(diff).max() <= 1 and 0 < (diff != 0).mean() < 0.2      # +-1 on a small fraction of inputs
    rc, d14, v14 = oracle.asw_classic(L, R, 30, 20, 0, 5, 0, 5, want_vol=True)
    assert v14.shape == v15.shape and not np.array_equal(v14, v15)       # the choice does reach the cost volume
    for bits, e in ((14, (29, 150, 76)), (15, (29, 150, 76))):           # pure B, G, R: both sets round to the same values
        assert tuple(cv.cvtColor_BGR2GRAY(np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255]]], np.uint8), bits)[0]) == e


def test_f3_primitives_second_restatement(oracle):
    """resize / BGR<->HSV / bilateralFilter / detail boost / u8 output (aswStereoMatch.cpp:30-31, 67-89, 97-98): the numpy
    whole-array forms of tests/cvlite.py against the per-pixel C oracle, bit for bit."""
    O = oracle
    rng = np.random.default_rng(2024)
    for (sh, sw), (dw, dh) in [((37, 53), (29, 21)), ((40, 64), (32, 20)), ((31, 45), (90, 70)), ((64, 48), (24, 32)),
                               ((50, 70), (70, 50)), ((9, 13), (5, 4))]:
        src = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
        np.testing.assert_array_equal(cv.resize_linear_u8(src, (dw, dh)), O.resize_linear(src, (dw, dh)),
                                      err_msg=f"resize {sh}x{sw} -> {dh}x{dw}")
    img = rng.integers(0, 256, (48, 80, 3), dtype=np.uint8)
    img[:6] = rng.integers(0, 256, (6, 80, 1), dtype=np.uint8)  # grey rows: S = 0, H = 0
    img[6:12, :, 1] = img[6:12, :, 2]                           # ties between the maxima
    hsv = cv.cvtColor_BGR2HSV(img)
    np.testing.assert_array_equal(hsv, O.bgr2hsv(img))
    every = np.stack(np.meshgrid(np.arange(0, 256, 5), np.arange(0, 256, 3), np.arange(0, 256, 7), indexing="ij"),
                     axis=-1).reshape(1, -1, 3).astype(np.uint8)  # includes H >= 180, which HSV2BGR must wrap
    np.testing.assert_array_equal(cv.cvtColor_HSV2BGR(every), O.hsv2bgr(every))
    np.testing.assert_array_equal(cv.cvtColor_HSV2BGR(hsv), O.hsv2bgr(hsv))
    plane = rng.integers(0, 256, (40, 56), dtype=np.uint8)
    smooth = (np.add.outer(np.arange(40), np.arange(56)) * 2 % 256).astype(np.uint8)
    for pl in (plane, smooth):
        np.testing.assert_array_equal(cv.bilateralFilter_u8(pl, 7, 10.0, 3.0), O.bilateral_u8(pl, 7, 10.0, 3.0))
    np.testing.assert_array_equal(cv.detail_boost(img), O.detail_boost(img))
    disp = (rng.random((30, 40)) * 300 - 20).astype(np.float32)
    disp[3, 3] = 12.5
    disp[3, 4] = 13.5
    for nrm in (True, False):
        np.testing.assert_array_equal(cv.disparity_to_u8(disp, nrm), O.disparity_to_u8(disp, nrm))
    np.testing.assert_array_equal(cv.disparity_to_u8(np.full((4, 4), 7, np.float32)), O.disparity_to_u8(np.full((4, 4), 7, np.float32)))
