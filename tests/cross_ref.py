"""Restatement of cross-based support-region aggregation (Zhang, Lu, Lafruit 2009), twice and
independently: a literal loop over every pixel's region (arms_loop / aggregate_loop) and the vectorised integral form
(arms / aggregate).  All integer until the one f32 division.  The raw cost is an INPUT (the u8 AD volume of computeAD for the same
direction: the oracle's on the CPU, ctx.computeAD on the GPU), never restated here, so there is one border rule and it is computeAD's.

    arms(img, tau, L)               -> int64 [4][H][W]: left, right, up, down
    aggregate(e_u8, arms, trunc)    -> S int64 [D][H][W], N int64 [H][W], E float32 [D][H][W], disp float32 [H][W] (min_d + index)

Also the test pairs: region_pair (piece-wise constant colours + a weak texture: arms of every length at tau = 20) and the shares the
vacuity conditions of tests/test_cross_cpu.py are stated on."""
import numpy as np

from aswstereomatch_amd.synth import make_pair


def _img(img):
    a = np.asarray(img)
    assert a.dtype == np.uint8
    return (a[:, :, None] if a.ndim == 2 else a).astype(np.int64)


# ---------------------------------------------------------------- literal form
def arms_loop(img, tau, L):
    g = _img(img)
    H, W = g.shape[:2]
    out = np.zeros((4, H, W), np.int64)
    for y in range(H):
        for x in range(W):
            for u, (dx, dy) in enumerate(((-1, 0), (1, 0), (0, -1), (0, 1))):
                r = 0
                while r < L:
                    xx, yy = x + (r + 1) * dx, y + (r + 1) * dy
                    if not (0 <= xx < W and 0 <= yy < H):
                        break
                    if np.abs(g[yy, xx] - g[y, x]).max() > tau:  # against the anchor
                        break
                    r += 1
                out[u, y, x] = r
    return out


def aggregate_loop(e_u8, arms, trunc, min_d=0, rows=None):
    """rows: compute these rows only (the others come back as the region of one zero-cost pixel) -- for frames where the whole
    literal form would take a quarter of a minute"""
    e = np.minimum(np.asarray(e_u8).astype(np.int64), int(trunc))
    D, H, W = e.shape
    left, right, up, down = arms
    S = np.zeros((D, H, W), np.int64)
    N = np.zeros((H, W), np.int64) if rows is None else np.ones((H, W), np.int64)
    for y in (range(H) if rows is None else rows):
        N[y] = 0
        for x in range(W):
            for yy in range(y - up[y, x], y + down[y, x] + 1):
                a, b = x - left[yy, x], x + right[yy, x] + 1
                S[:, y, x] += e[:, yy, a:b].sum(axis=1)
                N[y, x] += b - a
    return _finish(S, N, min_d)


def _finish(S, N, min_d):
    assert S.max(initial=0) < 1 << 24 and N.min() >= 1
    E = S.astype(np.float32) / N.astype(np.float32)[None]  # one correctly rounded f32 division of two exact operands
    disp = (np.argmin(E, axis=0) + min_d).astype(np.float32)  # the first minimum: strict '<' in ascending d
    return S, N, E, disp


# ---------------------------------------------------------------- integral form
def arms(img, tau, L):
    g = _img(img)
    H, W = g.shape[:2]
    out = np.zeros((4, H, W), np.int64)
    ys, xs = np.mgrid[0:H, 0:W]
    for u, (dx, dy) in enumerate(((-1, 0), (1, 0), (0, -1), (0, 1))):
        alive = np.ones((H, W), bool)
        for k in range(1, L + 1):
            xx, yy = xs + k * dx, ys + k * dy
            inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            other = g[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
            alive = alive & inside & (np.abs(other - g).max(axis=2) <= tau)
            out[u] += alive
    return out


def _region_sums(e, arms):
    """e int64 [D][H][W] -> region sums by the two orthogonal integral steps"""
    D, H, W = e.shape
    left, right, up, down = arms
    xs = np.arange(W)[None, None, :]
    ys = np.arange(H)[None, :, None]
    P = np.zeros((D, H, W + 1), np.int64)
    np.cumsum(e, axis=2, out=P[:, :, 1:])
    hi = np.broadcast_to(xs + right[None] + 1, (D, H, W))
    lo = np.broadcast_to(xs - left[None], (D, H, W))
    EH = np.take_along_axis(P, hi, axis=2) - np.take_along_axis(P, lo, axis=2)
    V = np.zeros((D, H + 1, W), np.int64)
    np.cumsum(EH, axis=1, out=V[:, 1:])
    hi = np.broadcast_to(ys + down[None] + 1, (D, H, W))
    lo = np.broadcast_to(ys - up[None], (D, H, W))
    return np.take_along_axis(V, hi, axis=1) - np.take_along_axis(V, lo, axis=1)


def aggregate(e_u8, arms, trunc, min_d=0):
    e = np.minimum(np.asarray(e_u8).astype(np.int64), int(trunc))
    S = _region_sums(e, arms)
    N = _region_sums(np.ones((1,) + e.shape[1:], np.int64), arms)[0]
    return _finish(S, N, min_d)


# ---------------------------------------------------------------- test pairs and what they exercise
def region_pair(H, W, D, seed, cell=(9, 13), amp=0.12, block=16, noise=2):
    """Left image: block-constant random colours in cells of cell = (rows, columns) at a random offset, plus amp * (the texture of
    synth.make_pair - 128); right image: warped by a piece-wise constant disparity in [0, D), holes filled with noise, +-2 noise,
    exactly as synth.make_pair does.  make_pair itself is too contrasty for this method: at tau = 20 its arms are 97 % zero."""
    rng = np.random.default_rng(seed)
    tex = make_pair(H, W, D, seed=seed, block=block, noise=0)[0].astype(np.float64)
    ch, cw = cell
    oy, ox = int(rng.integers(0, ch)), int(rng.integers(0, cw))
    ny, nx = (H + oy + ch - 1) // ch + 1, (W + ox + cw - 1) // cw + 1
    colours = rng.integers(24, 232, size=(ny, nx, 3)).astype(np.float64)
    base = np.repeat(np.repeat(colours, ch, axis=0), cw, axis=1)[oy:oy + H, ox:ox + W]
    L = np.clip(np.floor(base + (tex - 128.0) * amp + 0.5), 0, 255).astype(np.uint8)

    by, bx = (H + block - 1) // block, (W + block - 1) // block
    dmax = max(1, min(D, W // 2))
    gt = np.repeat(np.repeat(rng.integers(0, dmax, size=(by, bx)), block, axis=0), block, axis=1)[:H, :W].astype(np.int32)
    R = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)  # occlusion filler
    ys, xs = np.mgrid[0:H, 0:W]
    order = np.argsort(gt, axis=None, kind="stable")  # far to near
    yy, xx, dd = ys.ravel()[order], xs.ravel()[order], gt.ravel()[order]
    xr = xx - dd
    ok = xr >= 0
    R[yy[ok], xr[ok]] = L[yy[ok], xx[ok]]
    if noise:
        n = rng.integers(-noise, noise + 1, size=R.shape)
        R = np.clip(R.astype(np.int32) + n, 0, 255).astype(np.uint8)
    return L, R, gt


# H, W, D, cell, seed, amp, win: the region_pair cases of tests/test_gpu_cross.py at win 7, 15 and 35 (65 rows: two 32-row bands of
# the aggregation kernel and one row); tests/test_cross_cpu.py holds them to the vacuity conditions in both directions
REGION_CASES = [
    (20, 70, 12, (9, 13), 8, 0.16, 7),
    (37, 130, 17, (9, 13), 3, 0.12, 15),
    (65, 150, 17, (25, 40), 9, 0.10, 35),
]


def arm_shares(a, L):
    """shares of the arm values equal to 0, strictly between, equal to L"""
    a = np.asarray(a)
    return float((a == 0).mean()), float(((a > 0) & (a < L)).mean()), float((a == L).mean())


def tie_share(E):
    """share of the pixels whose two smallest E are equal (needs two candidates)"""
    s = np.sort(E, axis=0)
    return float((s[0] == s[1]).mean())


# ---------------------------------------------------------------- random cases (tools/fuzz_parity.py, leg "cross")
def random_case(rng, n=0):
    """A random case of the method: frames from one pixel up, every window, both directions, 1 and 3 channels, candidates past the
    image, padded rows, constant rectangles (long arms, ties).  case["tag"] rebuilds it: build_case(tag)."""
    H = int(rng.choice([1, 2, 31, 32, 33, 64, 65, int(rng.integers(1, 80))]))
    W = int(rng.choice([1, 2, 63, 64, 65, 128, 129, int(rng.integers(1, 280))]))
    win = int(rng.choice([1, 3, 5, 7, 9, 15, 21, 33, 35]))
    minD = int(rng.choice([0, 0, 0, 1, 3, 17, max(0, W - 2)]))
    D = int(rng.choice([1, 2, 3, 4, 5, 8, 9, 17, int(rng.integers(1, 40))]))
    tag = (H, W, int(rng.choice([1, 3])), win, minD, D, int(rng.integers(0, 2)), int(rng.choice([0, 5, 20, 20, 60, 255])),
           int(rng.choice([1, 7, 20, 20, 100, 255])), int(rng.integers(0, 1 << 30)), int(rng.choice([0, 0, 0, 3])),
           int(rng.choice([0, 0, 1])))
    return build_case(tag)


def build_case(tag):
    H, W, cn, win, minD, D, dt, tau, trunc, seed, pad, flat = tag
    rng = np.random.default_rng(seed)
    cell = (int(rng.integers(2, 30)), int(rng.integers(2, 45)))
    L, R, _ = region_pair(H, W + pad, max(2, D), seed, cell, float(rng.choice([0.05, 0.12, 0.2])), block=int(rng.choice([4, 8, 16])))
    if flat:
        for img in (L, R):
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            img[y0:y0 + int(rng.integers(1, 40)), x0:x0 + int(rng.integers(1, 60))] = rng.integers(0, 256, 3).astype(np.uint8)
    if cn == 1:
        L, R = np.ascontiguousarray(L[:, :, 1]), np.ascontiguousarray(R[:, :, 1])
    return {"tag": tag, "L": L[:, :W], "R": R[:, :W], "win": win, "minD": minD, "D": D, "dt": dt, "tau": tau, "trunc": trunc}


def gpu_result(ctx, case):
    """((volume, map) of the library with the volume kept, map without it) and the restatement's (volume, map)"""
    c = case
    e = np.stack(ctx.computeAD(c["L"], c["R"], c["dt"], c["minD"], c["D"]))
    S, N, E, disp = aggregate(e, arms(c["R"] if c["dt"] else c["L"], c["tau"], c["win"] // 2), c["trunc"], c["minD"])
    d, v = ctx.computeAdaptiveWeight_cross(c["L"], c["R"], c["dt"], c["tau"], c["trunc"], c["win"], c["minD"], c["D"],
                                           return_cost_volume=True)
    d2 = ctx.computeAdaptiveWeight_cross(c["L"], c["R"], c["dt"], c["tau"], c["trunc"], c["win"], c["minD"], c["D"])
    return (v, d, d2), (E, disp)
