"""Restatement of StereoBM (OpenCV 4.1.0 stereobm.cpp, PREFILTER_XSOBEL) and of cv::validateDisparity as this project states
them, in numpy integer arithmetic.  TEST INFRASTRUCTURE ONLY.

Two independent statements live here: `stereo_bm` works on whole arrays (per candidate plane, per block of rows) and is the one
the GPU tests compare against; `stereo_bm_scalar` copies OpenCV's loop structure (prefilter by row pairs, the sliding hsad / cbuf
ring with clamped column pointers, htext, dy0 / dy1, the validateDisparity passes) for tiny frames, and the CPU tests pin the two
to each other.  filterSpeckles and the 16S -> 8U conversion are shared with tests/sgbm_ref.py.

Conventions: images uint8 [H][W] (one channel); k is OpenCV's candidate index 0..D-1, disparity minD + D - 1 - k; the SAD volume
is returned [D][H][W] with plane p <-> disparity minD + p, NaN outside the pixels OpenCV computes (the valid rows
[w/2, H - w/2) x the columns [minD + D - 1, W))."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sgbm_ref import disp16_to_u8, filter_speckles  # noqa: E402,F401

I64 = np.int64
PREFILTER_NORMALIZED_RESPONSE, PREFILTER_XSOBEL = 0, 1


def check_params(H, W, minD, D, w, pre_filter_type, pre_filter_size, cap, texture, uniqueness):
    """StereoBM::compute's assertions (step 0) plus what this library does not serve: None when the call is served, else the
    name of the failing rule"""
    if pre_filter_type not in (PREFILTER_NORMALIZED_RESPONSE, PREFILTER_XSOBEL):
        return "preFilterType"
    if not (5 <= pre_filter_size <= 255 and pre_filter_size % 2 == 1):
        return "preFilterSize"
    if not 1 <= cap <= 63:
        return "preFilterCap"
    if not (5 <= w <= 255 and w % 2 == 1 and w <= min(H, W)):
        return "blockSize"
    if D <= 0 or D % 16 != 0:
        return "numDisparities"
    if texture < 0 or uniqueness < 0:
        return "textureThreshold/uniquenessRatio"
    return None


def prefilter_xsobel(img, cap):
    """Step 1: x-Sobel with rows y-1 / y+1 reflected (BORDER_REFLECT_101), clamped to [-cap, cap] and offset by cap; columns 0
    and W-1 hold cap; with an odd H the last row is all cap (OpenCV works on row pairs)."""
    I = np.asarray(img).astype(I64)
    H, W = I.shape
    out = np.full((H, W), cap, I64)
    if H < 2 or W < 3:
        return out
    yp = np.arange(H) - 1
    yp[0] = 1
    yn = np.arange(H) + 1
    yn[-1] = H - 2
    v = (I[yp, 2:] - I[yp, :-2]) + 2 * (I[:, 2:] - I[:, :-2]) + (I[yn, 2:] - I[yn, :-2])
    out[:, 1:-1] = np.clip(v, -cap, cap) + cap
    if H % 2:
        out[-1] = cap
    return out


def valid_roi(H, W, minD, D, w):
    """Step 2, getValidDisparityROI: (y0, y1, x0, x1) or None when empty"""
    h = w // 2
    y0, y1, x0, x1 = h, H - h, minD + D - 1 + h, W - h
    return (y0, y1, x0, x1) if (y1 > y0 and x1 > x0) else None


def _box_rows(P, h, y0, y1):
    """vertical window sums over rows [y - h, y + h] of P [rows][cols], for y in [y0, y1) (the windows lie inside P)"""
    c = np.concatenate([np.zeros((1,) + P.shape[1:], I64), np.cumsum(P, axis=0)])
    return c[y0 + h + 1:y1 + h + 1] - c[y0 - h:y1 - h]


def _box_cols(P, h, n):
    """horizontal window sums of width 2h+1 of P [..][n + 2h] -> [..][n]"""
    c = np.concatenate([np.zeros(P.shape[:-1] + (1,), I64), np.cumsum(P, axis=-1)], axis=-1)
    return c[..., 2 * h + 1:2 * h + 1 + n] - c[..., :n]


def _window_columns(W, minD, D, h):
    """the window columns c of every computed column X in [lofs, W) (c in [lofs - h, W + h)), with the clamped left column
    and the clamped base of the right column (OpenCV's lptr / rptr): right column = rbase + k"""
    lofs = minD + D - 1
    c = np.arange(lofs - h, W + h)
    return np.clip(c, 0, W - 1), np.clip(c - lofs, 0, W - D)


def sad_and_texture(Lp, Rp, minD, D, w, cap, y0, y1):
    """Step 3 on the rows [y0, y1) (inside the valid rows): SAD [D][y1-y0][W - lofs] (index k) and the texture sums
    [y1-y0][W - lofs] at the columns X in [lofs, W)"""
    H, W = Lp.shape
    h = w // 2
    lofs = minD + D - 1
    n = W - lofs
    lc, rb = _window_columns(W, minD, D, h)
    rows = slice(y0 - h, y1 + h)
    Lw = Lp[rows][:, lc]
    tex = _box_cols(_box_rows(np.abs(Lw - cap), h, h, h + y1 - y0), h, n)
    S = np.empty((D, y1 - y0, n), I64)
    for k in range(D):
        P = np.abs(Lw - Rp[rows][:, rb + k])
        S[k] = _box_cols(_box_rows(P, h, h, h + y1 - y0), h, n)
    return S, tex


def _cdiv(a, b):
    """C integer division (truncation toward zero)"""
    q = np.abs(a) // np.abs(b)
    return np.where((a < 0) != (b < 0), -q, q)


def winner(S, tex, minD, texture, uniqueness):
    """Step 4 on S [D][..]: (disp16 with FILTERED where a rule fails, cost = sad[mind])"""
    D = S.shape[0]
    FILTERED = 16 * (minD - 1)
    minsad = S.min(axis=0)
    mind = S.argmin(axis=0)  # first occurrence: the smallest k, i.e. the largest disparity
    bad = tex < texture
    if uniqueness > 0:
        thresh = minsad + (minsad * uniqueness) // 100
        k = np.arange(D).reshape((D,) + (1,) * (S.ndim - 1))
        far = np.abs(k - mind[None]) > 1
        bad |= (far & (S <= thresh[None])).any(axis=0)
    ext = np.concatenate([S[1:2], S, S[D - 2:D - 1]])  # sad[-1] = sad[1], sad[D] = sad[D-2]
    p = np.take_along_axis(ext, (mind + 2)[None], 0)[0]
    n = np.take_along_axis(ext, mind[None], 0)[0]
    d = p + n - 2 * minsad + np.abs(p - n)
    frac = np.where(d != 0, _cdiv((p - n) * 256, np.where(d != 0, d, 1)), 0)
    disp = ((D - mind - 1 + minD) * 256 + frac + 15) >> 4
    return np.where(bad, FILTERED, disp), minsad


def validate_row(disp, cost, minD, D, M):
    """Step 6 on one row (validateDisparity, CV_16S map, int cost): returns the new row"""
    W = disp.shape[0]
    INVALID = 16 * (minD - 1)
    minX1 = max(minD + D, 0)
    M16 = 16 * M
    disp2 = np.full(W, INVALID, I64)
    xs = np.arange(minX1, W)
    xs = xs[disp[xs] != INVALID]
    if len(xs):
        x2 = xs - ((disp[xs] + 8) >> 4)
        order = np.lexsort((xs, cost[xs], x2))  # per target column: the smallest cost, the first x on a tie
        first = np.ones(len(order), bool)
        first[1:] = x2[order][1:] != x2[order][:-1]
        sel = order[first]
        disp2[x2[sel]] = disp[xs[sel]]
    out = disp.copy()
    d = disp[xs]

    def disagrees(t):
        xx = xs - t
        inside = (xx >= 0) & (xx < W)
        v = disp2[np.clip(xx, 0, W - 1)]
        return inside & (v > INVALID) & (np.abs(v - d) > M16)

    out[xs[disagrees(d >> 4) & disagrees((d + 15) >> 4)]] = INVALID
    return out


def stereo_bm(left, right, minD, D, w, pre_filter_cap=31, texture_threshold=10, uniqueness_ratio=15, speckle_window_size=0,
              speckle_range=0, disp12_max_diff=-1, row_block=64, want_volume=True):
    """Steps 1-7 (PREFILTER_XSOBEL).  Returns dict(disp=int16 [H][W], vol=float32 [D][H][W] or None, raw=int16 before step 6)."""
    L, R = np.asarray(left), np.asarray(right)
    H, W = L.shape
    FILTERED = 16 * (minD - 1)
    lofs = minD + D - 1
    h = w // 2
    disp = np.full((H, W), FILTERED, I64)
    vol = np.full((D, H, W), np.nan, np.float32) if want_volume else None
    roi = valid_roi(H, W, minD, D, w)
    if roi is None:
        return {"disp": disp.astype(np.int16), "vol": vol, "raw": disp.astype(np.int16)}
    y0, y1, x0, x1 = roi
    Lp, Rp = prefilter_xsobel(L, pre_filter_cap), prefilter_xsobel(R, pre_filter_cap)
    cost = np.zeros((H, W), I64)
    for yb in range(y0, y1, row_block):
        ye = min(yb + row_block, y1)
        S, tex = sad_and_texture(Lp, Rp, minD, D, w, pre_filter_cap, yb, ye)
        dd, cc = winner(S, tex, minD, texture_threshold, uniqueness_ratio)
        disp[yb:ye, lofs:] = dd
        cost[yb:ye, lofs:] = cc
        if want_volume:
            vol[:, yb:ye, lofs:] = S[::-1].astype(np.float32)
    raw = disp.astype(np.int16)
    if disp12_max_diff >= 0:
        for y in range(y0, y1):
            disp[y] = validate_row(disp[y], cost[y], minD, D, disp12_max_diff)
    out = np.full((H, W), FILTERED, I64)
    out[y0:y1, x0:x1] = disp[y0:y1, x0:x1]
    out = out.astype(np.int16)
    if speckle_range >= 0 and speckle_window_size > 0:
        out = filter_speckles(out, FILTERED, speckle_window_size, speckle_range).astype(np.int16)
    return {"disp": out, "vol": vol, "raw": raw}


def get_disparity_bm(gray_left, gray_right, win, minD, D):
    """getDisparity_BM (aswMethods.cpp:100-146) on gray images: u8 map, or None where the reference raises CV_Error"""
    H, W = np.asarray(gray_left).shape
    w = win if win > 0 else 9
    if D % 16 != 0 or win % 2 == 0 or check_params(H, W, minD, D, w, 1, 9, 31, 10, 15) is not None:
        return None
    return disp16_to_u8(stereo_bm(gray_left, gray_right, minD, D, w, 31, 10, 15, 100, 32, 1, want_volume=False)["disp"])


# ---------------------------------------------------------------- the second statement: OpenCV's loops (tiny frames)
def prefilter_xsobel_scalar(img, cap):
    """prefilterXSobel: rows in pairs (y, y+1) with srow0..srow3, the table tab[], the odd last row filled with val0"""
    src = np.asarray(img).tolist()
    H, W = len(src), len(src[0])
    OFS = 256 * 4
    tab = [0 if x - OFS < -cap else 2 * cap if x - OFS > cap else x - OFS + cap for x in range(OFS * 2 + 256)]
    val0 = tab[OFS]
    dst = [[0] * W for _ in range(H)]
    y = 0
    while y < H - 1:
        srow1 = src[y]
        srow0 = src[y - 1] if y > 0 else (src[y + 1] if H > 1 else srow1)
        srow2 = src[y + 1] if y < H - 1 else (src[y - 1] if H > 1 else srow1)
        srow3 = src[y + 2] if y < H - 2 else srow1
        d0r, d1r = dst[y], dst[y + 1]
        d0r[0] = d0r[W - 1] = d1r[0] = d1r[W - 1] = val0
        for x in range(1, W - 1):
            d0 = srow0[x + 1] - srow0[x - 1]
            d1 = srow1[x + 1] - srow1[x - 1]
            d2 = srow2[x + 1] - srow2[x - 1]
            d3 = srow3[x + 1] - srow3[x - 1]
            d0r[x] = tab[d0 + d1 * 2 + d2 + OFS]
            d1r[x] = tab[d1 + d2 * 2 + d3 + OFS]
        y += 2
    while y < H:
        dst[y] = [val0] * W
        y += 1
    return dst


def _find_correspondence_scalar(left, right, row0, row1, minD, D, wsz, cap, texture, uniqueness):
    """findStereoCorrespondenceBM (the scalar form) on the rows [row0, row1) of the prefiltered images as one stripe:
    _dy0 = row0, _dy1 = rows - row1.  Returns (disp rows, cost rows, sad rows [y][X] -> list over k or None)."""
    rows, width = len(left), len(left[0])
    height = row1 - row0
    wsz2 = wsz // 2
    dy0, dy1 = min(row0, wsz2 + 1), min(rows - row1, wsz2 + 1)
    ndisp, mindisp = D, minD
    lofs = max(ndisp - 1 + mindisp, 0)
    rofs = -min(ndisp - 1 + mindisp, 0)
    width1 = width - rofs - ndisp + 1
    FILTERED = (mindisp - 1) << 4
    tab = [abs(x - cap) for x in range(256)]

    def L(y, c):  # lptr0 = left.ptr(row0) + lofs
        return left[row0 + y][lofs + c]

    def Rv(y, c):  # rptr0 = right.ptr(row0) + rofs
        return right[row0 + y][rofs + c]

    hsad = {y: [0] * ndisp for y in range(-dy0, height + dy1)}
    htext = {y: 0 for y in range(-wsz2 - 1, height + wsz2 + 1)}
    cbuf = [{y: [0] * ndisp for y in range(-dy0, height + dy1)} for _ in range(wsz + 1)]
    for x in range(-wsz2 - 1, wsz2):
        cb = cbuf[x + wsz2 + 1]
        lx = min(max(x, -lofs), width - lofs - 1)
        rx = min(max(x, -rofs), width - rofs - ndisp)
        for y in range(-dy0, height + dy1):
            lval = L(y, lx)
            for d in range(ndisp):
                diff = abs(lval - Rv(y, rx + d))
                cb[y][d] = diff
                hsad[y][d] += diff
            htext[y] += tab[lval]

    disp = [[FILTERED] * width for _ in range(height)]
    cost = [[0] * width for _ in range(height)]
    sads = [[None] * width for _ in range(height)]
    for x in range(width1):
        X = lofs + x
        x0, x1 = x - wsz2 - 1, x + wsz2
        cb_sub = cbuf[(x0 + wsz2 + 1) % (wsz + 1)]
        cb = cbuf[(x1 + wsz2 + 1) % (wsz + 1)]
        lx_sub = min(max(x0, -lofs), width - 1 - lofs)
        lx = min(max(x1, -lofs), width - 1 - lofs)
        rx = min(max(x1, -rofs), width - ndisp - rofs)
        for y in range(-dy0, height + dy1):
            lval = L(y, lx)
            for d in range(ndisp):
                diff = abs(lval - Rv(y, rx + d))
                hsad[y][d] = hsad[y][d] + diff - cb_sub[y][d]
                cb[y][d] = diff
            htext[y] += tab[lval] - tab[L(y, lx_sub)]
        for y in range(dy1, wsz2 + 1):
            htext[height + y] = htext[height + dy1 - 1]
        for y in range(-wsz2 - 1, -dy0):
            htext[y] = htext[-dy0]
        sad = [hsad[-dy0][d] * (wsz2 + 2 - dy0) for d in range(ndisp)]
        for y in range(1 - dy0, wsz2):
            for d in range(ndisp):
                sad[d] += hsad[y][d]
        tsum = sum(htext[y] for y in range(-wsz2 - 1, wsz2))
        for y in range(height):
            hs = hsad[min(y + wsz2, height + dy1 - 1)]
            hs_sub = hsad[max(y - wsz2 - 1, -dy0)]
            minsad, mind = None, -1
            for d in range(ndisp):
                sad[d] = sad[d] + hs[d] - hs_sub[d]
                if minsad is None or sad[d] < minsad:
                    minsad, mind = sad[d], d
            if X < width:
                sads[y][X] = list(sad)
            tsum += htext[y + wsz2] - htext[y - wsz2 - 1]
            if X >= width:  # OpenCV's loop runs to column width + minD - 1; those columns are not part of the map here
                continue
            if tsum < texture:
                disp[y][X] = FILTERED
                continue
            if uniqueness > 0:
                thresh = minsad + (minsad * uniqueness // 100)
                if any((d < mind - 1 or d > mind + 1) and sad[d] <= thresh for d in range(ndisp)):
                    disp[y][X] = FILTERED
                    continue
            ext = {d: sad[d] for d in range(ndisp)}
            ext[-1], ext[ndisp] = sad[1], sad[ndisp - 2]
            p, n = ext[mind + 1], ext[mind - 1]
            dd = p + n - 2 * ext[mind] + abs(p - n)
            num = (p - n) * 256
            frac = (abs(num) // dd * (1 if num >= 0 else -1)) if dd != 0 else 0
            disp[y][X] = ((ndisp - mind - 1 + mindisp) * 256 + frac + 15) >> 4
            cost[y][X] = minsad
    return disp, cost, sads


def _validate_scalar(disp, cost, minD, D, M):
    """validateDisparity (int cost), in place on a list of rows"""
    cols = len(disp[0])
    minX1, maxX1 = max(minD + D, 0), cols + min(minD, 0)
    INVALID = (minD - 1) * 16
    M16 = M * 16
    for y in range(len(disp)):
        dptr, cptr = disp[y], cost[y]
        disp2buf, disp2cost = [INVALID] * cols, [2 ** 31 - 1] * cols
        for x in range(minX1, maxX1):
            d, c = dptr[x], cptr[x]
            if d == INVALID:
                continue
            x2 = x - ((d + 8) >> 4)
            if disp2cost[x2] > c:
                disp2cost[x2] = c
                disp2buf[x2] = d
        for x in range(minX1, maxX1):
            d = dptr[x]
            if d == INVALID:
                continue
            d0, d1 = d >> 4, (d + 15) >> 4
            x0, x1 = x - d0, x - d1
            if (0 <= x0 < cols and disp2buf[x0] > INVALID and abs(disp2buf[x0] - d) > M16) and \
               (0 <= x1 < cols and disp2buf[x1] > INVALID and abs(disp2buf[x1] - d) > M16):
                dptr[x] = INVALID


def stereo_bm_scalar(left, right, minD, D, w, pre_filter_cap=31, texture_threshold=10, uniqueness_ratio=15,
                     disp12_max_diff=-1):
    """StereoBM::compute's steps 1-6 in OpenCV's loop form, one stripe.  Returns (disp int16 [H][W], SAD volume [D][H][W]
    float32 with NaN where nothing is computed)."""
    L, R = np.asarray(left), np.asarray(right)
    H, W = L.shape
    FILTERED = 16 * (minD - 1)
    disp = np.full((H, W), FILTERED, np.int16)
    vol = np.full((D, H, W), np.nan, np.float32)
    roi = valid_roi(H, W, minD, D, w)
    if roi is None:
        return disp, vol
    y0, y1, x0, x1 = roi
    Lp, Rp = prefilter_xsobel_scalar(L, pre_filter_cap), prefilter_xsobel_scalar(R, pre_filter_cap)
    d, c, sads = _find_correspondence_scalar(Lp, Rp, y0, y1, minD, D, w, pre_filter_cap, texture_threshold, uniqueness_ratio)
    if disp12_max_diff >= 0:
        _validate_scalar(d, c, minD, D, disp12_max_diff)
    for y in range(y1 - y0):
        for x in range(W):
            if x0 <= x < x1:
                disp[y0 + y, x] = d[y][x]
            if sads[y][x] is not None:
                vol[:, y0 + y, x] = sads[y][x][::-1]
    return disp, vol
