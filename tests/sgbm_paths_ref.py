"""Restatement of semi-global matching over a chosen set of path directions (asw_sgbm_paths), in numpy
integer arithmetic.  TEST INFRASTRUCTURE ONLY.

Steps 0-3 and 5-9 are those of tests/sgbm_ref.py, used as they are; only step 4 (the aggregation) is stated here:
S = sum over the directions r in `paths` of L_r, L_r the recurrence of sgbm_ref._path_step along every line of direction r over the
valid columns [minD + D, W) and all rows.  A pixel whose predecessor p - r lies outside that rectangle starts its line with
previous L = 0 and m = 0.

Two statements: `sgbm_paths` steps all lines of a direction at once (row by row, the previous row shifted by dx; column by column
for the two horizontal directions) and is the one the GPU tests compare against; `sgbm_paths_scalar` follows every line pixel by
pixel from the pixels that have no predecessor, for tiny frames.  The CPU tests pin the two to each other."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgbm_ref as ref  # noqa: E402

I64 = np.int64

PATH_LR, PATH_RL, PATH_TB, PATH_BT, PATH_TLBR, PATH_TRBL, PATH_BRTL, PATH_BLTR = (1 << i for i in range(8))
PATHS_3WAY, PATHS_HH4, PATHS_SGBM, PATHS_HH = 0x07, 0x0F, 0x37, 0xFF
# the step (dx, dy) from a pixel's predecessor to the pixel
DIRS = {PATH_LR: (1, 0), PATH_RL: (-1, 0), PATH_TB: (0, 1), PATH_BT: (0, -1), PATH_TLBR: (1, 1), PATH_TRBL: (-1, 1),
        PATH_BRTL: (-1, -1), PATH_BLTR: (1, -1)}
NEW_BITS = (PATH_BT, PATH_TLBR, PATH_TRBL, PATH_BRTL, PATH_BLTR)


def _swap(mask, pairs):
    out = mask
    for a, b in pairs:
        out &= ~(a | b)
        out |= (b if mask & a else 0) | (a if mask & b else 0)
    return out


def vflip(mask):
    """the mask of the same paths seen in the frame turned upside down"""
    return _swap(mask, ((PATH_TB, PATH_BT), (PATH_TLBR, PATH_BLTR), (PATH_TRBL, PATH_BRTL)))


def hflip(mask):
    """the mask of the same paths seen in the mirrored frame"""
    return _swap(mask, ((PATH_LR, PATH_RL), (PATH_TLBR, PATH_TRBL), (PATH_BRTL, PATH_BLTR)))


def _shift(a, dx):
    """a[x - dx] along the first axis, 0 where x - dx is outside"""
    if dx == 0:
        return a
    out = np.zeros_like(a)
    if dx > 0:
        out[dx:] = a[:-dx]
    else:
        out[:dx] = a[-dx:]
    return out


def path(C, P1, P2, dx, dy):
    """L_r of the direction (dx, dy) on C [H][Wv][D] (int64)"""
    H, Wv, D = C.shape
    L = np.zeros_like(C)
    if dy == 0:
        prev, m = np.zeros((H, D), I64), np.zeros(H, I64)
        for x in (range(Wv) if dx > 0 else range(Wv - 1, -1, -1)):
            prev, m = ref._path_step(C[:, x], prev, m, P1, P2)
            L[:, x] = prev
        return L
    prev, m = np.zeros((Wv, D), I64), np.zeros(Wv, I64)
    for y in (range(H) if dy > 0 else range(H - 1, -1, -1)):
        prev, m = ref._path_step(C[y], _shift(prev, dx), _shift(m, dx), P1, P2)
        L[y] = prev
    return L


def aggregate_paths(C, P1, P2, paths):
    """Step 4: S = sum of L_r over the directions of `paths`, [H][Wv][D] int64"""
    C = np.asarray(C, I64)
    S = np.zeros_like(C)
    for bit, (dx, dy) in DIRS.items():
        if paths & bit:
            S += path(C, P1, P2, dx, dy)
    return S


def sgbm_paths(left, right, minD, D, block_size, P1, P2, disp12_max_diff, pre_filter_cap, uniqueness_ratio, speckle_window_size,
               speckle_range, paths):
    """sgbm_ref.sgbm with step 4 over `paths`: the same dict (S [H][W][D] int64, raw, med, disp)."""
    w, ftzero, P1, P2, M, U = ref.effective_params(block_size, P1, P2, disp12_max_diff, pre_filter_cap, uniqueness_ratio)
    a = ref._planes(left)
    H, W = a.shape[:2]
    INVALID = 16 * (minD - 1)
    x0 = minD + D
    S_full = np.zeros((H, W, D), I64)
    disp = np.full((H, W), INVALID, I64)
    if x0 < W:
        C = ref.block_cost(left, right, minD, D, w, ftzero)
        S = aggregate_paths(C, P1, P2, paths)
        S_full[:, x0:] = S
        v, valid, best, minS = ref.winner(S, minD, U)
        for y in range(H):
            row = np.full(W, INVALID, I64)
            row[x0:] = np.where(valid[y], v[y], INVALID)
            disp[y] = ref.lr_check_row(row, valid[y], best[y], minS[y], x0, W, minD, M)
    raw = disp.astype(np.int16)
    med = raw if x0 >= W else ref.median3(raw)
    out = med
    if speckle_window_size > 0 and x0 < W:
        out = ref.filter_speckles(med, INVALID, speckle_window_size, 16 * speckle_range)
    return {"S": S_full, "raw": raw, "med": med, "disp": out.astype(np.int16)}


def get_disparity_sgbm_paths(left, right, win, minD, D, paths=PATHS_HH):
    """getDisparity_SGBM_paths of the C++ shim: getDisparity_SGBM's settings over `paths`, u8 map"""
    cn = ref._planes(left).shape[2]
    return ref.disp16_to_u8(sgbm_paths(left, right, minD, D, paths=paths, **ref.selector_params(cn, win))["disp"])


# ---------------------------------------------------------------- the second, scalar statement of steps 4-6 (tiny frames)
def lines(H, x_lo, x_hi, dx, dy):
    """every line of direction (dx, dy) in the rectangle [0, H) x [x_lo, x_hi): lists of (y, x) in walking order, each starting at
    a pixel whose predecessor (y - dy, x - dx) is outside"""
    inside = lambda y, x: 0 <= y < H and x_lo <= x < x_hi  # noqa: E731
    out = []
    for ys in range(H):
        for xs in range(x_lo, x_hi):
            if inside(ys - dy, xs - dx):
                continue
            y, x, pts = ys, xs, []
            while inside(y, x):
                pts.append((y, x))
                y, x = y + dy, x + dx
            out.append(pts)
    return out


def sgbm_paths_scalar(left, right, minD, D, block_size, P1, P2, disp12_max_diff, pre_filter_cap, uniqueness_ratio, paths):
    """Literal per-pixel loops of steps 4-6 on the block cost of steps 1-3 (sgbm_ref.block_cost, which tests/test_sgbm_cpu.py pins
    to its own scalar form).  Returns (S [H][W][D] as nested lists, int16-valued disp [H][W] as lists)."""
    w, ftzero, P1, P2, M, U = ref.effective_params(block_size, P1, P2, disp12_max_diff, pre_filter_cap, uniqueness_ratio)
    H, W = ref._planes(left).shape[:2]
    INVALID = 16 * (minD - 1)
    minX1, maxX1 = minD + D, W
    S = [[[0] * D for _ in range(W)] for _ in range(H)]
    disp = [[INVALID] * W for _ in range(H)]
    if minX1 >= maxX1:
        return S, disp
    Cv = ref.block_cost(left, right, minD, D, w, ftzero).tolist()
    C = {(y, x): Cv[y][x - minX1] for y in range(H) for x in range(minX1, maxX1)}

    def walk(points):
        Lp, out = [0] * D, {}
        for p in points:
            m = min(Lp)
            cur = []
            for d in range(D):
                best = Lp[d]
                if d > 0:
                    best = min(best, Lp[d - 1] + P1)
                if d < D - 1:
                    best = min(best, Lp[d + 1] + P1)
                best = min(best, m + P2)
                cur.append(C[p][d] + best - m)
            out[p] = cur
            Lp = cur
        return out

    for bit, (dx, dy) in DIRS.items():
        if not paths & bit:
            continue
        for pts in lines(H, minX1, maxX1, dx, dy):
            for (y, x), L in walk(pts).items():
                for d in range(D):
                    S[y][x][d] += L[d]

    for y in range(H):
        cost2 = [None] * W
        disp2 = [minD - 1] * W
        for x in range(minX1, maxX1):
            s = S[y][x]
            minS = min(s)
            best = s.index(minS)
            if any(abs(d - best) > 1 and s[d] * (100 - U) < minS * 100 for d in range(D)):
                continue
            if 0 < best < D - 1:
                den = max(s[best - 1] + s[best + 1] - 2 * minS, 1)
                num = 16 * (s[best - 1] - s[best + 1]) + den
                q = abs(num) // (2 * den)
                v = 16 * best + (q if num >= 0 else -q)
            else:
                v = 16 * best
            disp[y][x] = v + 16 * minD
            x2 = x - (best + minD)
            if cost2[x2] is None or cost2[x2] > minS:
                cost2[x2] = minS
                disp2[x2] = best + minD
        for x in range(W):
            d1 = disp[y][x]
            if d1 == INVALID:
                continue
            lo, hi = d1 >> 4, (d1 + 15) >> 4
            bad = [0 <= x - t < W and disp2[x - t] >= minD and abs(disp2[x - t] - t) > M for t in (lo, hi)]
            if all(bad):
                disp[y][x] = INVALID
    return S, disp
