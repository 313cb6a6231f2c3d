"""Restatement of the left-right refinement rule (include/asw_mi355x.h asw_refine_disparity) for the tests.

There is no reference implementation of this step; the rule is the library's own and is stated in integers, so both forms here
and the kernels must agree to the last bit (np.array_equal).  Two forms:

  refine_loop   the literal per-pixel loop of the rule;
  refine_vec    tap loop over arrays of filled pixels + cumulative histogram, fast enough for a 1080p frame.

Both return a dict: out (f32), mask (u8: 0 valid, 1 filled, 2 unfillable), fill (f32: the map after step 2, before the median),
n_rejected, n_unfillable.  A left map outside the domain of step 0 raises DomainError.
"""
import math

import numpy as np


class DomainError(ValueError):
    pass


def tables(win, gamma_c, gamma_s, channels):
    k = win // 2
    tc = np.array([math.floor(4096.0 * math.exp(-c / gamma_c) + 0.5) for c in range(255 * channels + 1)], np.int64)
    ts = np.array([[math.floor(256.0 * math.exp(-math.sqrt(i * i + j * j) / gamma_s) + 0.5) for i in range(k + 1)]
                   for j in range(k + 1)], np.int64)
    return tc, ts


def _guide(G):
    G = np.asarray(G)
    assert G.dtype == np.uint8
    return (G[:, :, None] if G.ndim == 2 else G).astype(np.int64)


def check_domain(dl, minD, n):
    with np.errstate(invalid="ignore"):
        ok = (dl >= minD) & (dl < minD + n) & (dl == np.floor(dl))
    if not ok.all():
        raise DomainError("disp_left leaves [%d, %d) or is not an integer" % (minD, minD + n))


# ---------------------------------------------------------------------------------------------------------------------------
# the literal form
# ---------------------------------------------------------------------------------------------------------------------------
def cross_check_loop(dl, dr, max_diff):
    H, W = dl.shape
    valid = np.zeros((H, W), bool)
    md = np.float32(max_diff)
    for y in range(H):
        for x in range(W):
            d = dl[y, x]
            xr = x - int(d)
            if 0 <= xr < W:
                diff = np.float32(d) - np.float32(dr[y, xr])
                valid[y, x] = bool(abs(diff) <= md)  # a NaN compares false
    return valid


def fill_loop(dl, valid, minD):
    """-> (F as int64 offsets d - minD, -1 = unfillable; mask)"""
    H, W = dl.shape
    F = np.full((H, W), -1, np.int64)
    mask = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            if valid[y, x]:
                F[y, x] = int(dl[y, x]) - minD
                continue
            a = b = None
            for xl in range(x - 1, -1, -1):
                if valid[y, xl]:
                    a = int(dl[y, xl]) - minD
                    break
            for xr in range(x + 1, W):
                if valid[y, xr]:
                    b = int(dl[y, xr]) - minD
                    break
            if a is None and b is None:
                mask[y, x] = 2
            else:
                mask[y, x] = 1
                F[y, x] = b if a is None else a if b is None else min(a, b)
    return F, mask


def median_loop(G, F, mask, win, gamma_c, gamma_s):
    g = _guide(G)
    H, W = F.shape
    k = win // 2
    tc, ts = tables(win, gamma_c, gamma_s, g.shape[2])
    M = F.copy()
    for y in range(H):
        for x in range(W):
            if mask[y, x] != 1:
                continue
            votes = {}
            T = 0
            for j in range(-k, k + 1):
                for i in range(-k, k + 1):
                    yy, xx = y + j, x + i
                    if not (0 <= yy < H and 0 <= xx < W) or F[yy, xx] < 0:
                        continue
                    dc = int(np.abs(g[y, x] - g[yy, xx]).sum())
                    w = int(tc[dc]) * int(ts[abs(j), abs(i)])
                    votes[int(F[yy, xx])] = votes.get(int(F[yy, xx]), 0) + w
                    T += w
            assert 0 < T < 2 ** 31
            c = 0
            for v in sorted(votes):
                c += votes[v]
                if 2 * c >= T:
                    M[y, x] = v
                    break
    return M


def _finish(dl, F, M, mask, minD, valid):
    out = np.where(mask == 0, dl, np.where(mask == 1, (M + minD).astype(np.float32), np.float32(minD - 1))).astype(np.float32)
    fill = np.where(mask == 2, np.float32(minD - 1), (F + minD).astype(np.float32)).astype(np.float32)
    return {"out": out, "mask": mask, "fill": fill, "n_rejected": int((~valid).sum()), "n_unfillable": int((mask == 2).sum())}


def refine_loop(G, dl, dr, minD, n, max_diff, win, gamma_c, gamma_s):
    dl = np.asarray(dl, np.float32)
    dr = np.asarray(dr, np.float32)
    check_domain(dl, minD, n)
    valid = cross_check_loop(dl, dr, max_diff)
    F, mask = fill_loop(dl, valid, minD)
    M = median_loop(G, F, mask, win, gamma_c, gamma_s)
    return _finish(dl, F, M, mask, minD, valid)


# ---------------------------------------------------------------------------------------------------------------------------
# the vectorised form
# ---------------------------------------------------------------------------------------------------------------------------
def cross_check_vec(dl, dr, max_diff):
    H, W = dl.shape
    xr = np.arange(W)[None, :] - dl.astype(np.int64)
    inside = (xr >= 0) & (xr < W)
    other = np.take_along_axis(dr, np.clip(xr, 0, W - 1), axis=1)
    with np.errstate(invalid="ignore"):
        return inside & (np.abs(dl - other) <= np.float32(max_diff))


def fill_vec(dl, valid, minD):
    H, W = dl.shape
    rel = dl.astype(np.int64) - minD
    xs = np.broadcast_to(np.arange(W), (H, W))
    left = np.maximum.accumulate(np.where(valid, xs, -1), axis=1)
    right = np.minimum.accumulate(np.where(valid, xs, W)[:, ::-1], axis=1)[:, ::-1]
    big = np.int64(1 << 40)
    a = np.where(left >= 0, np.take_along_axis(rel, np.clip(left, 0, W - 1), axis=1), big)
    b = np.where(right < W, np.take_along_axis(rel, np.clip(right, 0, W - 1), axis=1), big)
    f = np.minimum(a, b)
    some = valid.any(axis=1)[:, None]
    mask = np.where(valid, 0, np.where(some, 1, 2)).astype(np.uint8)
    F = np.where(valid, rel, np.where(some, f, -1)).astype(np.int64)
    return F, mask


def median_vec(G, F, mask, n, win, gamma_c, gamma_s, chunk_cells=1 << 23):
    g = _guide(G)
    H, W = F.shape
    k = win // 2
    tc, ts = tables(win, gamma_c, gamma_s, g.shape[2])
    gp = np.zeros((H + 2 * k, W + 2 * k, g.shape[2]), np.int64)
    gp[k:k + H, k:k + W] = g
    fp = np.full((H + 2 * k, W + 2 * k), -1, np.int64)
    fp[k:k + H, k:k + W] = F
    M = F.copy()
    ys, xs = np.nonzero(mask == 1)  # row-major: chunks are row bands of the filled pixels
    step = max(256, chunk_cells // max(n, 1))
    for s in range(0, len(ys), step):
        y, x = ys[s:s + step], xs[s:s + step]
        m = len(y)
        rows = np.arange(m)
        hist = np.zeros((m, n), np.int64)
        g0 = gp[y + k, x + k]
        for j in range(-k, k + 1):
            for i in range(-k, k + 1):
                f = fp[y + k + j, x + k + i]
                votes = f >= 0
                dc = np.abs(g0 - gp[y + k + j, x + k + i]).sum(axis=1)
                w = np.where(votes, tc[dc] * ts[abs(j), abs(i)], 0)
                hist[rows, np.where(votes, f, 0)] += w
        cum = np.cumsum(hist, axis=1)
        T = cum[:, -1]
        assert (T > 0).all() and (T < 2 ** 31).all()
        M[y, x] = np.argmax(2 * cum >= T[:, None], axis=1)
    return M


def refine_vec(G, dl, dr, minD, n, max_diff, win, gamma_c, gamma_s):
    dl = np.asarray(dl, np.float32)
    dr = np.asarray(dr, np.float32)
    check_domain(dl, minD, n)
    valid = cross_check_vec(dl, dr, max_diff)
    F, mask = fill_vec(dl, valid, minD)
    M = median_vec(G, F, mask, n, win, gamma_c, gamma_s) if win > 1 else F
    return _finish(dl, F, M, mask, minD, valid)


def vacuity_shares(res):
    """(rejected share of the pixels, share of the filled pixels the median moved off the fill) -- the conditions that keep a
    parity test on matcher output from passing with a kernel that skipped a stage; computed on the restatement alone."""
    filled = res["mask"] == 1
    moved = int((res["out"][filled] != res["fill"][filled]).sum())
    return res["n_rejected"] / res["mask"].size, moved / max(1, int(filled.sum()))
