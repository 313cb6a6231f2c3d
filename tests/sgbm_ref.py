"""Restatement of StereoSGBM (MODE_SGBM_3WAY, OpenCV 4.1.0 stereosgbm.cpp as this project states it: DESIGN.md section 4.8)
and of cv::filterSpeckles, in numpy integer arithmetic.  TEST INFRASTRUCTURE ONLY.

Two independent statements of steps 1-6 live here: `sgbm` works on whole arrays (per disparity plane, per path step) and is the
one the GPU tests compare against; `sgbm_scalar` is a literal per-pixel loop for tiny frames, and the CPU tests pin the two to
each other.  Steps 7-9 (median, speckles, 16S -> 8U) are shared.

Conventions: images uint8 [H][W] or [H][W][C]; d is the candidate INDEX 0..D-1 (absolute disparity minD + d); S is returned
[H][W][D] over every column, 0 outside the valid columns [minX1, maxX1) = [minD + D, W)."""
from collections import deque

import numpy as np

I64 = np.int64


def effective_params(block_size, P1, P2, disp12_max_diff, pre_filter_cap, uniqueness_ratio):
    """Step 0: (w, ftzero, P1, P2, M, U) as StereoSGBM::compute derives them."""
    ftzero = max(pre_filter_cap, 15) | 1
    P1 = P1 if P1 > 0 else 2
    P2 = max(P2 if P2 > 0 else 5, P1 + 1)
    U = 10 if uniqueness_ratio < 0 else uniqueness_ratio
    M = 1 if disp12_max_diff <= 0 else disp12_max_diff
    w = 5 if block_size <= 0 else block_size
    return w, ftzero, P1, P2, M, U


def cost_bound(cn, w, ftzero):
    """C_max: the largest block cost (Sobel planes <= 2*ftzero, raw planes >> 2 <= 63) over the (2*(w//2)+1)^2 window."""
    k = 2 * (w // 2) + 1
    return cn * (2 * ftzero + 63) * k * k


def _planes(img):
    a = np.asarray(img)
    return a[:, :, None] if a.ndim == 2 else a


def prefilter(img, ftzero):
    """Step 1: [sobel_c ...] + [raw_c ...] planes, int64 [2cn][H][W]; columns 0 and W-1 hold ftzero in both kinds."""
    a = _planes(img).astype(I64)
    H, W, cn = a.shape
    out = np.full((2 * cn, H, W), ftzero, I64)
    yn = np.maximum(np.arange(H) - 1, 0)
    ys = np.minimum(np.arange(H) + 1, H - 1)
    for c in range(cn):
        I = a[:, :, c]
        if W >= 3:
            s = 2 * (I[:, 2:] - I[:, :-2]) + I[yn, 2:] - I[yn, :-2] + I[ys, 2:] - I[ys, :-2]
            out[c, :, 1:-1] = np.clip(s, -ftzero, ftzero) + ftzero
            out[cn + c, :, 1:-1] = I[:, 1:-1]
    return out


def bt_minmax(p):
    """Birchfield-Tomasi half-neighbour interval of a plane [..][W]: (min, max); a neighbour outside the row is the pixel."""
    l = np.concatenate([p[..., :1], p[..., :-1]], axis=-1)
    r = np.concatenate([p[..., 1:], p[..., -1:]], axis=-1)
    hl, hr = (p + l) >> 1, (p + r) >> 1
    return np.minimum(np.minimum(p, hl), hr), np.maximum(np.maximum(p, hl), hr)


def bt_cost(u, um, up, v, vm, vp):
    return np.minimum(np.maximum(np.maximum(0, u - vp), vm - u), np.maximum(np.maximum(0, v - up), um - v))


def _box(P, h):
    """sum over |i|,|j| <= h with edge clamping, of a 2-D int64 array"""
    Q = np.pad(P, h, mode="edge")
    c = np.cumsum(np.cumsum(Q, axis=0), axis=1)
    c = np.pad(c, ((1, 0), (1, 0)))
    k = 2 * h + 1
    return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]


def block_cost(left, right, minD, D, w, ftzero):
    """Steps 1-3: C [H][maxX1-minX1][D] (int64) over the valid columns."""
    pl, pr = prefilter(left, ftzero), prefilter(right, ftzero)
    cn = pl.shape[0] // 2
    H, W = pl.shape[1:]
    x0, Wv = minD + D, W - (minD + D)
    lm, lp = bt_minmax(pl)
    rm, rp = bt_minmax(pr)
    C = np.zeros((H, Wv, D), I64)
    xs = slice(x0, W)
    for d in range(D):
        xr = slice(x0 - (minD + d), W - (minD + d))
        pix = np.zeros((H, Wv), I64)
        for k in range(2 * cn):
            c = bt_cost(pl[k, :, xs], lm[k, :, xs], lp[k, :, xs], pr[k, :, xr], rm[k, :, xr], rp[k, :, xr])
            pix += c if k < cn else c >> 2
        C[:, :, d] = _box(pix, w // 2)
    return C


def _path_step(Cs, prev, m, P1, P2):
    """one step of L(p,d) = C + min(L(p-r,d), L(p-r,d+-1) + P1, m + P2) - m over the last axis"""
    big = np.iinfo(I64).max // 4
    nb = np.full_like(prev, big)
    nb[..., 1:] = np.minimum(nb[..., 1:], prev[..., :-1] + P1)
    nb[..., :-1] = np.minimum(nb[..., :-1], prev[..., 1:] + P1)
    L = Cs + np.minimum(np.minimum(prev, nb), (m + P2)[..., None]) - m[..., None]
    return L, L.min(axis=-1)


def aggregate(C, P1, P2):
    """Step 4: S = L_lr + L_rl + L_tb, [H][Wv][D]."""
    H, Wv, D = C.shape
    S = np.zeros_like(C)
    prev, m = np.zeros((Wv, D), I64), np.zeros(Wv, I64)
    for y in range(H):
        prev, m = _path_step(C[y], prev, m, P1, P2)
        S[y] += prev
    for xs in (range(Wv), range(Wv - 1, -1, -1)):
        prev, m = np.zeros((H, D), I64), np.zeros(H, I64)
        for x in xs:
            prev, m = _path_step(C[:, x], prev, m, P1, P2)
            S[:, x] += prev
    return S


def _cdiv(a, b):
    """C integer division (truncation toward zero)"""
    q = np.abs(a) // np.abs(b)
    return np.where((a < 0) != (b < 0), -q, q)


def winner(S, minD, U):
    """Step 5 on S [H][Wv][D]: (disp [H][Wv] scaled by 16, valid mask, best, minS)"""
    H, Wv, D = S.shape
    minS = S.min(axis=-1)
    best = S.argmin(axis=-1)  # first occurrence: the smallest d
    d = np.arange(D)
    far = np.abs(d[None, None, :] - best[..., None]) > 1
    bad = (far & (S * (100 - U) < (minS * 100)[..., None])).any(axis=-1)
    v = 16 * best.astype(I64)
    inner = (best > 0) & (best < D - 1)
    bi = np.clip(best, 1, max(D - 2, 1))
    if D >= 3:
        sm = np.take_along_axis(S, (bi - 1)[..., None], -1)[..., 0]
        sp = np.take_along_axis(S, (bi + 1)[..., None], -1)[..., 0]
        den = np.maximum(sm + sp - 2 * minS, 1)
        v = np.where(inner, v + _cdiv(16 * (sm - sp) + den, 2 * den), v)
    return v + 16 * minD, ~bad, best, minS


def lr_check_row(disp, valid, best, minS, x0, W, minD, M):
    """Step 6 on one row: disp [W] (int64, scaled), valid/best/minS over the valid columns [x0, W).  Returns the new disp row."""
    INVALID = 16 * (minD - 1)
    cost2 = np.full(W, np.iinfo(I64).max, I64)
    disp2 = np.full(W, minD - 1, I64)
    xs = np.nonzero(valid)[0]
    # ascending x, strict '>': per target column the smallest minS wins, the smallest x on a tie
    x2 = (xs + x0) - (best[xs] + minD)
    order = np.lexsort((xs, minS[xs], x2))
    first = np.ones(len(order), bool)
    first[1:] = x2[order][1:] != x2[order][:-1]
    sel = order[first]
    cost2[x2[sel]] = minS[xs[sel]]
    disp2[x2[sel]] = best[xs[sel]] + minD
    out = disp.copy()
    for x in range(W):
        d1 = out[x]
        if d1 == INVALID:
            continue
        lo, hi = d1 >> 4, (d1 + 15) >> 4
        a, b = x - lo, x - hi
        bad_lo = 0 <= a < W and disp2[a] >= minD and abs(disp2[a] - lo) > M
        bad_hi = 0 <= b < W and disp2[b] >= minD and abs(disp2[b] - hi) > M
        if bad_lo and bad_hi:
            out[x] = INVALID
    return out


def median3(disp):
    """Step 7: medianBlur(ksize 3) with replicated borders"""
    H, W = disp.shape
    p = np.pad(disp, 1, mode="edge")
    st = np.stack([p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    return np.sort(st, axis=0)[4]


def filter_speckles(img, new_val, max_speckle_size, max_diff):
    """cv::filterSpeckles by breadth-first search: 4-connected components of pixels != new_val whose neighbours differ by at
    most max_diff; every component of <= max_speckle_size pixels becomes new_val.  Returns a new array."""
    a = np.asarray(img)
    H, W = a.shape
    v = a.astype(I64).ravel().tolist()
    out = a.copy().ravel()
    seen = bytearray(H * W)
    for s in range(H * W):
        if seen[s] or v[s] == new_val:
            continue
        seen[s] = 1
        comp = [s]
        q = deque([s])
        while q:
            p = q.popleft()
            y, x = divmod(p, W)
            vp = v[p]
            for n, ok in ((p - 1, x > 0), (p + 1, x < W - 1), (p - W, y > 0), (p + W, y < H - 1)):
                if ok and not seen[n] and v[n] != new_val and abs(v[n] - vp) <= max_diff:
                    seen[n] = 1
                    comp.append(n)
                    q.append(n)
        if len(comp) <= max_speckle_size:
            out[comp] = new_val
    return out.reshape(H, W)


def disp16_to_u8(disp):
    """Step 9: convertTo(CV_8U, 1/16) -- round half to even, saturate to 0..255"""
    return np.clip(np.rint(np.asarray(disp, np.float64) / 16.0), 0, 255).astype(np.uint8)


def sgbm(left, right, minD, D, block_size, P1, P2, disp12_max_diff, pre_filter_cap, uniqueness_ratio, speckle_window_size,
         speckle_range):
    """Steps 0-8.  Returns dict(S=[H][W][D] int64, raw=int16 after step 6, med=after step 7, disp=int16 after step 8)."""
    w, ftzero, P1, P2, M, U = effective_params(block_size, P1, P2, disp12_max_diff, pre_filter_cap, uniqueness_ratio)
    a = _planes(left)
    H, W = a.shape[:2]
    INVALID = 16 * (minD - 1)
    x0 = minD + D
    S_full = np.zeros((H, W, D), I64)
    disp = np.full((H, W), INVALID, I64)
    if x0 < W:
        C = block_cost(left, right, minD, D, w, ftzero)
        S = aggregate(C, P1, P2)
        S_full[:, x0:] = S
        v, valid, best, minS = winner(S, minD, U)
        for y in range(H):
            row = np.full(W, INVALID, I64)
            row[x0:] = np.where(valid[y], v[y], INVALID)
            disp[y] = lr_check_row(row, valid[y], best[y], minS[y], x0, W, minD, M)
    raw = disp.astype(np.int16)
    med = raw if x0 >= W else median3(raw)
    out = med
    if speckle_window_size > 0 and x0 < W:
        out = filter_speckles(med, INVALID, speckle_window_size, 16 * speckle_range)
    return {"S": S_full, "raw": raw, "med": med, "disp": out.astype(np.int16)}


def selector_params(cn, win):
    """getDisparity_SGBM (aswMethods.cpp:158-194): the StereoSGBM settings for an image of cn channels and window win"""
    w = win if win > 0 else 3
    return dict(block_size=w, P1=8 * cn * w * w, P2=32 * cn * w * w, disp12_max_diff=200, pre_filter_cap=10,
                uniqueness_ratio=10, speckle_window_size=175, speckle_range=32)


def get_disparity_sgbm(left, right, win, minD, D):
    """the selector's SGBM entry: u8 map"""
    cn = _planes(left).shape[2]
    return disp16_to_u8(sgbm(left, right, minD, D, **selector_params(cn, win))["disp"])


# ---------------------------------------------------------------- the second, scalar statement of steps 1-6 (tiny frames)
def sgbm_scalar(left, right, minD, D, block_size, P1, P2, disp12_max_diff, pre_filter_cap, uniqueness_ratio):
    """Literal per-pixel loops of steps 0-6.  Returns (S [H][W][D] as nested lists, int16-valued disp [H][W] as lists)."""
    w, ftzero, P1, P2, M, U = effective_params(block_size, P1, P2, disp12_max_diff, pre_filter_cap, uniqueness_ratio)
    L, R = _planes(left).tolist(), _planes(right).tolist()
    H, W, cn = len(L), len(L[0]), len(L[0][0])
    INVALID = 16 * (minD - 1)
    minX1, maxX1 = minD + D, W

    def pre(img, k, y, x):
        if x == 0 or x == W - 1:
            return ftzero
        if k >= cn:
            return img[y][x][k - cn]
        yn, ys = max(y - 1, 0), min(y + 1, H - 1)
        c = k
        s = (2 * (img[y][x + 1][c] - img[y][x - 1][c]) + img[yn][x + 1][c] - img[yn][x - 1][c] + img[ys][x + 1][c]
             - img[ys][x - 1][c])
        return min(max(s, -ftzero), ftzero) + ftzero

    def lohi(img, k, y, x):
        a = pre(img, k, y, x)
        l = pre(img, k, y, x - 1) if x > 0 else a
        r = pre(img, k, y, x + 1) if x < W - 1 else a
        cands = (a, (a + l) >> 1, (a + r) >> 1)
        return a, min(cands), max(cands)

    def pix(x, y, d):
        tot = 0
        for k in range(2 * cn):
            u, um, up = lohi(L, k, y, x)
            v, vm, vp = lohi(R, k, y, x - (minD + d))
            c = min(max(0, u - vp, vm - u), max(0, v - up, um - v))
            tot += c if k < cn else c >> 2
        return tot

    S = [[[0] * D for _ in range(W)] for _ in range(H)]
    disp = [[INVALID] * W for _ in range(H)]
    if minX1 >= maxX1:
        return S, disp
    h = w // 2
    P = {}
    for y in range(H):
        for x in range(minX1, maxX1):
            for d in range(D):
                P[y, x, d] = pix(x, y, d)
    C = {}
    for y in range(H):
        for x in range(minX1, maxX1):
            for d in range(D):
                C[y, x, d] = sum(P[min(max(y + j, 0), H - 1), min(max(x + i, minX1), maxX1 - 1), d]
                                 for j in range(-h, h + 1) for i in range(-h, h + 1))

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
                cur.append(C[p + (d,)] + best - m)
            out[p] = cur
            Lp = cur
        return out

    for y in range(H):
        lr = walk([(y, x) for x in range(minX1, maxX1)])
        rl = walk([(y, x) for x in range(maxX1 - 1, minX1 - 1, -1)])
        for x in range(minX1, maxX1):
            for d in range(D):
                S[y][x][d] = lr[y, x][d] + rl[y, x][d]
    for x in range(minX1, maxX1):
        tb = walk([(y, x) for y in range(H)])
        for y in range(H):
            for d in range(D):
                S[y][x][d] += tb[y, x][d]

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
