"""Restatement of cross-scale cost aggregation (include/asw_mi355x.h asw_disparity_cross_scale) for the tests.

There is no reference implementation of this step; the rule is the library's own and is fixed completely: the pyramid in integers,
the weights by the Thomas algorithm in f64 (Python floats: one IEEE operation per statement, nothing fused), the combination in f64
in the order of the scales.  The kernel must agree to the last bit (np.array_equal).  The per-scale volumes V_s are not restated
here: they are what the method returns on the level-s pair with the level's candidate range (scale_ranges).
"""
import numpy as np

LEFT, RIGHT = 0, 1
FLAG = 0x1000
DEFAULT_SCALES, DEFAULT_Q = 3, 19


def encode(S, q):
    """asw_disparity_cross_scale(S, q): bit 12, S in bits 13..15, q in bits 16..23; an argument out of range leaves the S field 0"""
    S, q = int(S), int(q)
    bad = S < 2 or S > 5 or q < 1 or q > 255
    return FLAG | ((0 if bad else S) << 13) | ((q & 0xFF) << 16)


def down2(img):
    """one pyramid step of an 8U image [H][W] or [H][W][C]: ceil(H/2) x ceil(W/2), (a + b + c + d + 2) >> 2 of the 2x2 block with the
    last row / column repeated where the block leaves the image"""
    img = np.asarray(img, np.uint8)
    H, W = img.shape[:2]
    ys, xs = np.arange((H + 1) // 2) * 2, np.arange((W + 1) // 2) * 2
    y1, x1 = np.minimum(ys + 1, H - 1), np.minimum(xs + 1, W - 1)
    v = img.astype(np.int32)
    s = v[ys][:, xs] + v[ys][:, x1] + v[y1][:, xs] + v[y1][:, x1]
    return np.ascontiguousarray(((s + 2) >> 2).astype(np.uint8))


def scale_ranges(minD, n, extra, S):
    """[(minD_s, planes_s, numD_s)] for s = 0..S-1 of a method with n planes at the finest scale, n - extra of them numDisparity; None
    where a scale is left with numD_s < 1 (the library refuses the call)"""
    out = []
    for s in range(S):
        m = minD >> s
        planes = ((minD + n - 1) >> s) - m + 1
        if planes - extra < 1:
            return None
        out.append((m, planes, planes - extra))
    return out


def weights64(S, q):
    """w = A^-1 e_0 in f64, A the S x S tridiagonal matrix of the paper (diagonal 1 + lam at both ends and 1 + 2 lam between,
    off-diagonals -lam), lam = q / 64, by the Thomas algorithm written out statement by statement"""
    lam = float(q) / 64.0
    off = -lam
    cp, dp = [0.0] * S, [0.0] * S
    for i in range(S):
        b = 1.0 + lam if (i == 0 or i == S - 1) else 1.0 + 2.0 * lam
        rhs = 1.0 if i == 0 else 0.0
        if i == 0:
            cp[0] = off / b
            dp[0] = rhs / b
        else:
            t = off * cp[i - 1]
            den = b - t
            u = off * dp[i - 1]
            cp[i] = off / den
            dp[i] = (rhs - u) / den
    x = [0.0] * S
    x[S - 1] = dp[S - 1]
    for i in range(S - 2, -1, -1):
        t = cp[i] * x[i + 1]
        x[i] = dp[i] - t
    return np.array(x, np.float64)


def weights(S, q):
    return weights64(S, q).astype(np.float32)


def matrix(S, q):
    lam = q / 64.0
    A = np.zeros((S, S))
    for i in range(S):
        A[i, i] = 1 + lam if i in (0, S - 1) else 1 + 2 * lam
        if i:
            A[i, i - 1] = A[i - 1, i] = -lam
    return A


def combine(vols, minD, w, drop=None):
    """out[k][y][x] = (float)(sum over s in order of (double)w[s] * (double)vols[s][((minD + k) >> s) - (minD >> s)][y >> s][x >> s]),
    starting from 0.0; drop: a scale whose term is left out (the CPU test's sensitivity check)"""
    v0 = np.asarray(vols[0], np.float32)
    n, H, W = v0.shape
    k = minD + np.arange(n)
    ys, xs = np.arange(H), np.arange(W)
    acc = np.zeros((n, H, W), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for s, v in enumerate(vols):
            if s == drop:
                continue
            v = np.asarray(v, np.float32)
            term = v[(k >> s) - (minD >> s)][:, ys >> s][:, :, xs >> s].astype(np.float64)
            acc = acc + np.float64(np.float32(w[s])) * term
        return acc.astype(np.float32)


def wta(vol, minD):
    """k_wta's rule: strict '<' in ascending k against DBL_MAX, NaN never wins, a never-updated pixel is 0"""
    vol = np.asarray(vol, np.float32)
    best = np.full(vol.shape[1:], np.finfo(np.float64).max)
    disp = np.zeros(vol.shape[1:], np.float32)
    with np.errstate(invalid="ignore"):
        for k in range(vol.shape[0]):
            c = vol[k].astype(np.float64)
            better = c < best
            best = np.where(better, c, best)
            disp = np.where(better, np.float32(minD + k), disp)
    return disp


def pyramid(img, S):
    out = [np.ascontiguousarray(img)]
    for _ in range(S - 1):
        out.append(down2(out[-1]))
    return out


def textured_pair(H, W, cn, shift, seed):
    """a blocky noisy scene and its copy shifted by `shift` columns; cn = 1: [H][W], cn = 3: [H][W][3]"""
    rng = np.random.default_rng(seed)
    Wb = W + shift + 4
    base = rng.integers(0, 256, (H // 5 + 2, Wb // 6 + 2, cn)).astype(np.float64)
    base = np.repeat(np.repeat(base, 5, axis=0), 6, axis=1)[:H, :Wb]
    img = np.clip(base * 0.85 + rng.integers(0, 40, (H, Wb, cn)), 0, 255)
    L = img[:, shift:shift + W]
    R = np.clip(img[:, :W] + rng.integers(-3, 4, (H, W, cn)), 0, 255)
    L, R = L.astype(np.uint8), R.astype(np.uint8)
    if cn == 1:
        L, R = L[:, :, 0], R[:, :, 0]
    return np.ascontiguousarray(L), np.ascontiguousarray(R)


# method name -> (selector value or the name of the aswstereomatch_amd function that forms it, extra planes, DISPARITY_RIGHT served,
#                 1-channel pairs served, windows, minD must be 0)
METHODS = {
    "classic": (2, 1, True, False, (1, 3, 5, 9), False),
    "direct8": (3, 1, False, False, (3, 5, 9), False),
    "geodesic": (4, 1, True, False, (3, 5, 7), False),
    "bilgrid": (5, 1, False, True, (1,), False),
    "blo1": (6, 0, True, True, (3, 5, 9), True),
    "guided": (7, 0, True, False, (3, 5, 9), False),
    "guided2": (8, 0, False, False, (3, 5, 9), False),
    "wmedian": (10, 0, False, False, (3, 5), False),
    "cross": (12, 0, True, True, (1, 3, 7, 15), False),
    "twopass": ("twopass_algorithm", 1, True, True, (1, 3, 7, 15), False),
    "cross_params": ("cross_algorithm", 0, True, True, (3, 7), False),
    "adcensus": ("adcensus_algorithm", 0, True, True, (3, 7), False),
    "permeability": ("permeability_algorithm", 0, True, True, (1,), False),
}


def algorithm(method):
    sel = METHODS[method][0]
    if isinstance(sel, str):
        import aswstereomatch_amd as asw
        return getattr(asw, sel)()
    return sel


def build_case(tag):
    """the case of a tag (method, dt, H, W, cn, win, minD, numD, S, q, subpixel, shift, seed), as random_case draws and prints it"""
    method, dt, H, W, cn, win, minD, numD, S, q, sub, shift, seed = tag
    L, R = textured_pair(H, W, cn, shift, seed)
    return {"method": method, "alg": algorithm(method), "extra": METHODS[method][1], "dt": dt, "win": win, "minD": minD, "numD": numD,
            "S": S, "q": q, "subpixel": sub, "L": L, "R": R, "tag": tuple(tag)}


_ctx2 = []  # gpu_result's second context, created at first use


def gpu_result(ctx, case):
    """The leg cross_scale of tools/fuzz_parity.py: ((volume, map, map without a kept volume) of the flagged call, (volume, map) built
    from a second context's plain calls on the pyramid).  NaN slots are compared as -1 (no method returns a negative cost)."""
    import aswstereomatch_amd as asw
    from aswstereomatch_amd import _lib
    import subpixel_ref as sp

    if not _ctx2:
        _ctx2.append(asw.Context(0))
    c = case
    n = _lib.lib().asw_volume_planes(int(c["alg"]), c["numD"])
    ranges = scale_ranges(c["minD"], n, n - c["numD"], c["S"])
    vols = [_ctx2[0].stereoMatching(Ls, Rs, c["dt"], c["alg"], c["win"], ranges[s][0], ranges[s][2], return_cost_volume=True)[1]
            for s, (Ls, Rs) in enumerate(zip(pyramid(c["L"], c["S"]), pyramid(c["R"], c["S"])))]
    vw = combine(vols, c["minD"], weights(c["S"], c["q"]))
    dw = wta(vw, c["minD"])
    if c["subpixel"]:
        dw = sp.subpixel_vec(dw, vw, c["minD"], c["subpixel"])[0]
    flag = encode(c["S"], c["q"])
    d, v = ctx.stereoMatching(c["L"], c["R"], c["dt"], c["alg"], c["win"], c["minD"], c["numD"], return_cost_volume=True,
                              subpixel=c["subpixel"], cross_scale=flag)
    d2 = ctx.stereoMatching(c["L"], c["R"], c["dt"] | c["subpixel"] | flag, c["alg"], c["win"], c["minD"], c["numD"])
    unnan = lambda a: np.where(np.isnan(a), np.float32(-1), a)  # noqa: E731
    return (unnan(v), d, d2), (unnan(vw), dw)


def random_case(rng, n=0):
    """One seeded cross-scale case: a method, a direction it serves, a small frame (at most about 2500 pixels; widths on both sides of
    64 and of a multiple of 4), an admissible candidate range (odd minD included) that holds the pair's shift, S, q and sometimes a
    sub-pixel flag."""
    method = list(METHODS)[int(rng.integers(len(METHODS)))]
    sel, extra, right, gray, wins, min0 = METHODS[method]
    S = int(rng.integers(2, 6))
    q = int((1, 19, 64, 255, int(rng.integers(1, 256)))[int(rng.integers(5))])
    W = int((1, 2, 3, 5, 9, 31, 60, 63, 64, 65, 66, 67, 68, 72, 100)[int(rng.integers(15))])
    H = int(rng.integers(1, max(2, min(24, 2500 // W)) + 1))
    cn = 1 if (gray and rng.integers(3) == 0) else 3
    dt = RIGHT if (right and rng.integers(2)) else LEFT
    minD = 0 if min0 else int(rng.integers(0, 8))
    numD = int(rng.integers(1, 25))
    while scale_ranges(minD, numD + extra, extra, S) is None:
        numD += 1
    sub = int((0, 0, 0x100, 0x200)[int(rng.integers(4))])
    shift = minD + int(rng.integers(numD))
    win = int(wins[int(rng.integers(len(wins)))])
    return build_case((method, dt, H, W, cn, win, minD, numD, S, q, sub, shift, int(rng.integers(1 << 30))))
