"""Restatement of scanline optimisation (include/asw_mi355x.h asw_disparity_scanline) for the tests.

There is no reference implementation of this step; the rule is the library's own and is fixed completely, in f32 with one IEEE
operation per statement, so the kernels must agree to the last bit (np.array_equal).  The volume V the step starts from is not
restated here: it is what the method returns without the flag.

    c = V where V is finite, else +inf;  paths LR (predecessor x-1), RL (x+1), TB (y-1), BT (y+1), minq = min_k L(q,k)
    q outside the frame or minq == +inf:  L(p,k) = c(p,k)
    else  t0 = L(q,k); t1 = L(q,k-1) + P1; t2 = L(q,k+1) + P1; t3 = minq + P2; m = min(t0..t3); L(p,k) = c(p,k) + (m - minq)
    S = ((L_LR + L_RL) + L_TB) + L_BT;  out = V finite ? S : V;  map = wta(out)

The sign of a zero may differ between implementations of min(): np.minimum and the loops below keep the first of two equal zeros,
the kernel whichever its reduction meets.  It is invisible to == (and to np.array_equal) and to the value of every later addition.
"""
import numpy as np

from cross_scale_ref import METHODS, algorithm, textured_pair, wta  # noqa: F401  (one copy of k_wta's rule and of the method list)

LEFT, RIGHT = 0, 1
FLAG = 0x01000000
DEFAULT = (8, 5, 4)  # a, u, ratio: P1 = 8, P2 = 32
INF = np.float32(np.inf)

# (a, u, ratio) for the volumes of three methods on textured pairs: P1 about a fifth of the standard deviation of the method's costs
# (classic 19, geodesic 62, GuidedF_2 0.12 on the CPU test's pair), P2 four times that.  The CPU test holds them to the oracle's
# volumes: at least 1 % of the winners move.
CODES = {"classic": (4, 5, 4), "geodesic": (9, 5, 4), "guided2": (26, 0, 4)}


def encode(a, u, ratio):
    """asw_disparity_scanline(a, u, ratio): bit 24, a in bits 1..7, u in bits 25..27, ratio - 1 in bits 28..30; an argument out of
    range gives the flag alone"""
    a, u, ratio = int(a), int(u), int(ratio)
    if a < 1 or a > 127 or u < 0 or u > 7 or ratio < 1 or ratio > 8:
        return FLAG
    return FLAG | (a << 1) | (u << 25) | ((ratio - 1) << 28)


def penalties(a, u, ratio):
    """(P1, P2) as f32: a * 4^(u-5) and ratio * a * 4^(u-5), both exact (at most 10 significant bits times a power of two)"""
    unit = 4.0 ** (u - 5)
    p1, p2 = np.float32(a * unit), np.float32(ratio * a * unit)
    assert float(p1) == a * unit and float(p2) == ratio * a * unit
    return p1, p2


def _costs(V):
    V = np.asarray(V, np.float32)
    assert V.ndim == 3
    return V, np.where(np.isfinite(V), V, INF).astype(np.float32)


def _path(c, P1, P2, axis, backward):
    """L of one path: c [n][H][W], the path runs along `axis` (1 = y, 2 = x); every pixel of the other axis at once"""
    cm = np.moveaxis(c, axis, 0)  # [T][n][M]
    T, n, M = cm.shape
    L = np.empty_like(cm)
    order = range(T - 1, -1, -1) if backward else range(T)
    prev = None
    for t in order:
        if prev is None:
            L[t] = cm[t]
        else:
            q = L[prev]
            minq = q.min(axis=0)
            t1 = np.full((n, M), INF, np.float32)
            t2 = np.full((n, M), INF, np.float32)
            t1[1:] = q[:-1] + P1
            t2[:-1] = q[1:] + P1
            t3 = minq + P2
            m = np.minimum(np.minimum(np.minimum(q, t1), t2), t3[None])
            d = m - minq[None]  # inf - inf where the path restarts: not used there
            L[t] = np.where((minq < INF)[None], cm[t] + d, cm[t])
        prev = t
    assert L.dtype == np.float32
    return np.moveaxis(L, 0, axis)


def optimise(V, P1, P2):
    """-> out [n][H][W] f32"""
    V, c = _costs(V)
    P1, P2 = np.float32(P1), np.float32(P2)
    with np.errstate(invalid="ignore", over="ignore"):
        S = _path(c, P1, P2, 2, False) + _path(c, P1, P2, 2, True)
        S = S + _path(c, P1, P2, 1, False)
        S = S + _path(c, P1, P2, 1, True)
    assert S.dtype == np.float32
    return np.where(np.isfinite(V), S, V)


def starts_sum(V):
    """the four unregularised starts summed in the rule's order: ((c + c) + c) + c, kept where V is finite"""
    V, c = _costs(V)
    with np.errstate(over="ignore"):
        return np.where(np.isfinite(V), ((c + c) + c) + c, V)


def optimise_literal(V, P1, P2):
    """the same statements in plain loops over np.float32 scalars (tiny volumes)"""
    V, c = _costs(V)
    n, H, W = V.shape
    P1, P2 = np.float32(P1), np.float32(P2)
    S = None
    with np.errstate(invalid="ignore", over="ignore"):
        for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):  # the predecessor's offset: LR, RL, TB, BT
            L = np.zeros((n, H, W), np.float32)
            ys = range(H) if dy <= 0 else range(H - 1, -1, -1)
            xs = range(W) if dx <= 0 else range(W - 1, -1, -1)
            for y in ys:
                for x in xs:
                    qy, qx = y + dy, x + dx
                    minq = INF
                    if 0 <= qy < H and 0 <= qx < W:
                        for k in range(n):
                            if L[k, qy, qx] < minq:
                                minq = L[k, qy, qx]
                    for k in range(n):
                        if not minq < INF:
                            L[k, y, x] = c[k, y, x]
                            continue
                        m = L[k, qy, qx]
                        if k > 0:
                            t1 = np.float32(L[k - 1, qy, qx] + P1)
                            m = t1 if t1 < m else m
                        if k < n - 1:
                            t2 = np.float32(L[k + 1, qy, qx] + P1)
                            m = t2 if t2 < m else m
                        t3 = np.float32(minq + P2)
                        m = t3 if t3 < m else m
                        d = np.float32(m - minq)
                        L[k, y, x] = np.float32(c[k, y, x] + d)
            S = L if S is None else (S + L).astype(np.float32)
    return np.where(np.isfinite(V), S, V)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def build_case(tag):
    """the case of a tag (method, dt, H, W, cn, win, minD, numD, a, u, ratio, subpixel, shift, seed), as random_case draws and prints it"""
    method, dt, H, W, cn, win, minD, numD, a, u, ratio, sub, shift, seed = tag
    L, R = textured_pair(H, W, cn, shift, seed)
    return {"method": method, "alg": algorithm(method), "extra": METHODS[method][1], "dt": dt, "win": win, "minD": minD, "numD": numD,
            "a": a, "u": u, "ratio": ratio, "subpixel": sub, "L": L, "R": R, "tag": tuple(tag)}


def random_case(rng, n=0):
    """One seeded scanline case: a method, a direction it serves, a small frame (at most about 2500 pixels; widths and heights on
    both sides of the kernels' tile constants 4, 8, 16 and 32), a candidate range on both sides of a wavefront's 64 lanes now and
    then, a code triple over the whole encodable range and sometimes a sub-pixel flag."""
    method = list(METHODS)[int(rng.integers(len(METHODS)))]
    sel, extra, right, gray, wins, min0 = METHODS[method]
    W = int((1, 2, 3, 5, 8, 9, 31, 32, 33, 63, 64, 65, 72, 100)[int(rng.integers(14))])
    H = int(rng.integers(1, max(2, min(40, 2500 // W)) + 1))
    cn = 1 if (gray and rng.integers(3) == 0) else 3
    dt = RIGHT if (right and rng.integers(2)) else LEFT
    minD = 0 if min0 else int(rng.integers(0, 8))
    numD = int(rng.integers(1, 25)) if rng.integers(6) else int((62, 63, 64, 65, 66)[int(rng.integers(5))])
    if numD > 30 and H * W > 600:
        H = max(1, 600 // W)
    a = int((1, 8, 127, int(rng.integers(1, 128)))[int(rng.integers(4))])
    u = int(rng.integers(0, 8))
    ratio = int(rng.integers(1, 9))
    sub = int((0, 0, 0x100, 0x200)[int(rng.integers(4))])
    shift = minD + int(rng.integers(min(numD, 24)))
    win = int(wins[int(rng.integers(len(wins)))])
    return build_case((method, dt, H, W, cn, win, minD, numD, a, u, ratio, sub, shift, int(rng.integers(1 << 30))))


_ctx2 = []  # gpu_result's second context, created at first use


def gpu_result(ctx, case):
    """The leg scanline of tools/fuzz_parity.py: ((volume, map, map without a kept volume) of the flagged call, (volume, map) built
    from a second context's plain call).  NaN slots are compared as -1e30 and infinities as -2e30 / -3e30 (no method returns such a
    cost)."""
    import aswstereomatch_amd as asw
    import subpixel_ref as sp

    if not _ctx2:
        _ctx2.append(asw.Context(0))
    c = case
    plain = _ctx2[0].stereoMatching(c["L"], c["R"], c["dt"], c["alg"], c["win"], c["minD"], c["numD"], return_cost_volume=True)[1]
    vw = optimise(plain, *penalties(c["a"], c["u"], c["ratio"]))
    dw = wta(vw, c["minD"])
    if c["subpixel"]:
        dw = sp.subpixel_vec(dw, vw, c["minD"], c["subpixel"])[0]
    flag = encode(c["a"], c["u"], c["ratio"])
    d, v = ctx.stereoMatching(c["L"], c["R"], c["dt"], c["alg"], c["win"], c["minD"], c["numD"], return_cost_volume=True,
                              subpixel=c["subpixel"], scanline=flag)
    d2 = ctx.stereoMatching(c["L"], c["R"], c["dt"] | c["subpixel"] | flag, c["alg"], c["win"], c["minD"], c["numD"])

    def plainify(a):
        a = np.where(np.isnan(a), np.float32(-1e30), a)
        return np.where(np.isposinf(a), np.float32(-2e30), np.where(np.isneginf(a), np.float32(-3e30), a))

    return (plainify(v), d, d2), (plainify(vw), dw)
