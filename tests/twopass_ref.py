"""Restatement of the two-pass (separable) adaptive-support-weight aggregation (Wang et al. 2006; DESIGN.md section 4.16;
k_twopass.hip), twice: vectorised over the frame with one array statement per tap (twopass), and as literal per-pixel loops
(twopass_loop).  The arithmetic is fixed completely -- f32 weights from one table, f32 weight product, f64 sums in ascending tap
order, the horizontal products rounded before they are added -- so the GPU is compared with np.array_equal.

    T[r][dc] = (float)exp(-((double)dc / gamma_c + (double)r / gamma_g)),   r = 0..win/2, dc = 0..255  (math.exp: libm, double)

DISPARITY_LEFT, xr = max(0, x - d), clamp to the image:
    vertical   j = -h..h, yy = clamp(y + j):   ab = T[|j|][|gL(yy,x) - gL(y,x)|] * T[|j|][|gR(yy,xr) - gR(y,xr)|]  (f32)
                                               vn += (double)ab * |gL(yy,x) - gR(yy,xr)|;  vd += (double)ab
    horizontal i = -h..h, xx = clamp(x + i), xri = clamp(xr + i):
                                               ab = T[|i|][|gL(y,xx) - gL(y,x)|] * T[|i|][|gR(y,xri) - gR(y,xr)|]  (f32)
                                               num = num + (double)ab * vn(xx,y,d);  den = den + (double)ab * vd(xx,y,d)
    E = num / den (f64); volume plane (float)E; map = first strict minimum of E over ascending d = minD .. minD + numD (inclusive).
DISPARITY_RIGHT is DISPARITY_LEFT of the x-mirrored, swapped pair, mirrored back."""
import math

import numpy as np

LEFT, RIGHT = 0, 1


def table(gamma_c, gamma_g, win):
    h = win // 2
    return np.array([[np.float32(math.exp(-(dc / float(gamma_c) + r / float(gamma_g)))) for dc in range(256)] for r in range(h + 1)],
                    np.float32)


def _left(gL, gR, T, win, minD, numD):
    H, W = gL.shape
    h = win // 2
    a = gL.astype(np.int32)
    b = gR.astype(np.int32)
    X, Y = np.arange(W), np.arange(H)
    E = np.empty((numD + 1, H, W), np.float64)
    for k in range(numD + 1):
        xr = np.maximum(0, X - (minD + k))
        bc = b[:, xr]  # the right image at every pixel's own right column
        vn = np.zeros((H, W), np.float64)
        vd = np.zeros((H, W), np.float64)
        for j in range(-h, h + 1):
            yy = np.clip(Y + j, 0, H - 1)
            ab = T[abs(j)][np.abs(a[yy] - a)] * T[abs(j)][np.abs(bc[yy] - bc)]  # f32 * f32 -> f32
            vn = vn + ab.astype(np.float64) * np.abs(a[yy] - bc[yy])
            vd = vd + ab.astype(np.float64)
        num = np.zeros((H, W), np.float64)
        den = np.zeros((H, W), np.float64)
        for i in range(-h, h + 1):
            xx = np.clip(X + i, 0, W - 1)
            xri = np.clip(xr + i, 0, W - 1)
            ab = T[abs(i)][np.abs(a[:, xx] - a)] * T[abs(i)][np.abs(b[:, xri] - bc)]
            num = num + ab.astype(np.float64) * vn[:, xx]  # the product is rounded, then added
            den = den + ab.astype(np.float64) * vd[:, xx]
        E[k] = num / den
    return E


def _left_loop(gL, gR, T, win, minD, numD):
    H, W = gL.shape
    h = win // 2
    gl = [[int(v) for v in row] for row in gL]
    gr = [[int(v) for v in row] for row in gR]
    Tl = [[float(v) for v in row] for row in T]  # f32 values held in Python floats

    def f32(v):
        return float(np.float32(v))

    E = np.empty((numD + 1, H, W), np.float64)
    for k in range(numD + 1):
        d = minD + k
        vn = [[0.0] * W for _ in range(H)]
        vd = [[0.0] * W for _ in range(H)]
        for y in range(H):
            for x in range(W):
                xr = max(0, x - d)
                n = 0.0
                s = 0.0
                for j in range(-h, h + 1):
                    yy = min(max(y + j, 0), H - 1)
                    ab = f32(Tl[abs(j)][abs(gl[yy][x] - gl[y][x])] * Tl[abs(j)][abs(gr[yy][xr] - gr[y][xr])])
                    n += ab * abs(gl[yy][x] - gr[yy][xr])
                    s += ab
                vn[y][x] = n
                vd[y][x] = s
        for y in range(H):
            for x in range(W):
                xr = max(0, x - d)
                num = 0.0
                den = 0.0
                for i in range(-h, h + 1):
                    xx = min(max(x + i, 0), W - 1)
                    xri = min(max(xr + i, 0), W - 1)
                    ab = f32(Tl[abs(i)][abs(gl[y][xx] - gl[y][x])] * Tl[abs(i)][abs(gr[y][xri] - gr[y][xr])])
                    num = num + ab * vn[y][xx]
                    den = den + ab * vd[y][xx]
                E[k, y, x] = num / den
    return E


def _run(left_fn, gL, gR, gamma_c, gamma_g, win, minD, numD, dt):
    gL, gR = np.asarray(gL), np.asarray(gR)
    assert gL.ndim == 2 and gL.shape == gR.shape and gL.dtype == np.uint8 and gR.dtype == np.uint8 and win % 2 == 1
    T = table(gamma_c, gamma_g, win)
    if int(dt) & 1:
        E = left_fn(gR[:, ::-1], gL[:, ::-1], T, win, minD, numD)[:, :, ::-1]
    else:
        E = left_fn(gL, gR, T, win, minD, numD)
    E = np.ascontiguousarray(E)
    disp = (np.argmin(E, axis=0) + minD).astype(np.float32)  # first minimum == strict '<' over ascending d (no NaN: den >= 1)
    return E, E.astype(np.float32), disp


def twopass(gL, gR, gamma_c=30, gamma_g=20, win=15, minD=0, numD=64, dt=LEFT):
    """-> E f64 [numD + 1][H][W], the volume (float)E, the map f32 [H][W]."""
    return _run(_left, gL, gR, gamma_c, gamma_g, win, minD, numD, dt)


def twopass_loop(gL, gR, gamma_c=30, gamma_g=20, win=15, minD=0, numD=64, dt=LEFT):
    return _run(_left_loop, gL, gR, gamma_c, gamma_g, win, minD, numD, dt)


def tie_share(E):
    """share of the pixels whose f64 minimum is reached, bit for bit, at two or more candidates"""
    return float(((E == E.min(axis=0)).sum(axis=0) >= 2).mean())


# ---------------------------------------------------------------- inputs
def textured_pair(H, W, cn, shift, seed):
    """A smooth-plus-noise scene and its copy shifted by `shift` columns with a little noise of its own: the gray differences span
    the table, and the minimum is neither flat nor everywhere the same."""
    rng = np.random.default_rng(seed)
    Wb = W + shift + 4
    base = rng.integers(0, 256, (H // 4 + 2, Wb // 4 + 2, cn)).astype(np.float64)
    base = np.repeat(np.repeat(base, 4, axis=0), 4, axis=1)[:H, :Wb]
    img = np.clip(base * 0.7 + rng.integers(0, 90, (H, Wb, cn)), 0, 255)
    L = img[:, shift:shift + W]
    R = np.clip(img[:, :W] + rng.integers(-6, 7, (H, W, cn)), 0, 255)
    L, R = L.astype(np.uint8), R.astype(np.uint8)
    if cn == 1:
        L, R = L[:, :, 0], R[:, :, 0]
    return np.ascontiguousarray(L), np.ascontiguousarray(R)


def periodic_pair(H, W, period=8, shift=3, seed=3):
    """Horizontally periodic, 1 channel, the left view `shift` columns ahead: candidates a period apart (period - shift, 2 period -
    shift, ...) see the same windows away from the borders -> tied minima at candidates other than the first."""
    rng = np.random.default_rng(seed)
    cell = rng.integers(0, 256, (H, period)).astype(np.uint8)
    img = np.tile(cell, (1, (W + shift) // period + 2))
    return np.ascontiguousarray(img[:, shift:shift + W]), np.ascontiguousarray(img[:, :W])


def constant_pair(H, W, value=77):
    img = np.full((H, W), value, np.uint8)
    return img, img.copy()


# name -> (L, R, win, minD, numD): the tie-dense inputs of tests/test_twopass_cpu.py and tests/test_gpu_twopass.py
def tie_cases():
    return {
        "periodic": periodic_pair(20, 150) + (15, 0, 17),
        "constant": constant_pair(9, 70) + (7, 3, 8),
    }


def kernel_lds(win):
    """Layout::total of k_twopass.hip: the {vn, vd} pairs of a chunk (4 rows, 8 candidates, 64 + 2h columns, 16 bytes each), the
    table, the two gray tiles with rows padded to 16 bytes"""
    def up16(v):
        return (v + 15) // 16 * 16
    h = win // 2
    return 4 * 8 * (64 + 2 * h) * 16 + (h + 1) * 256 * 4 + (4 + 2 * h) * (up16(64 + 2 * h) + up16(64 + 2 * h + 7))


def max_window():
    """the largest odd window whose layout fits a workgroup's 160 KB: twopass_max_window() restated"""
    win = 1
    while kernel_lds(win + 2) <= 160 * 1024:
        win += 2
    return win


ROW_TILE = 4                       # rows of the kernel's tile
WINDOWS = (1, 3, 7, 15, 35)        # 25 | 27: the dynamic-LDS opt-in above 64 KB (63744 / 66656 bytes); max_window(): the last served
NUMDS = (1, 2, 4, 8, 16, 17, 32, 33)
GAMMAS = ((30, 20), (1, 1), (255, 255), (7, 36))


def random_case(rng, n=0):
    """A random case for the seeded sweep and the fuzz leg: frames from one pixel up, windows to 35, both directions, 1 and 3
    channels, candidates past the image, padded rows, constant rectangles (ties).  case["tag"] rebuilds it: build_case(tag)."""
    H = int(rng.choice([1, 3, 4, 5, 8, int(rng.integers(1, 41))]))
    W = int(rng.choice([1, 2, 63, 64, 65, 129, int(rng.integers(1, 141))]))
    win = int(rng.choice([1, 3, 5, 7, 9, 11, 15, 21, 25, 27, 35]))
    numD = int(rng.choice([1, 2, 3, 4, 7, 8, 9, 16, 17, 20]))
    minD = int(rng.choice([0, 0, 0, 1, 3, 11, max(0, W - 2)]))
    if rng.random() < 0.3:
        gamma_c, gamma_g = int(rng.integers(1, 256)), int(rng.integers(1, 256))
    else:
        gamma_c, gamma_g = GAMMAS[int(rng.integers(0, len(GAMMAS)))]
    tag = (H, W, int(rng.choice([1, 3])), win, minD, numD, int(rng.integers(0, 2)), gamma_c, gamma_g, int(rng.integers(0, 1 << 30)),
           int(rng.choice([0, 0, 0, 3])), int(rng.choice([0, 0, 1])))
    return build_case(tag)


def build_case(tag):
    H, W, cn, win, minD, numD, dt, gamma_c, gamma_g, seed, pad, flat = tag
    rng = np.random.default_rng(seed)
    L, R = textured_pair(H, W + pad, cn, int(rng.integers(0, 8)), seed)
    if flat:
        for img in (L, R):
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            img[y0:y0 + int(rng.integers(1, 40)), x0:x0 + int(rng.integers(1, 60))] = int(rng.integers(0, 256))
    return {"tag": tag, "L": L[:, :W], "R": R[:, :W], "gamma_c": gamma_c, "gamma_g": gamma_g, "win": win, "minD": minD, "numD": numD,
            "dt": dt}


def gpu_result(ctx, case):
    """((volume, map) of the library with the volume kept, map without it) and the restatement's (volume, map); the gray pair is
    ctx.bgr2gray of the inputs"""
    c = case
    gL, gR = (ctx.bgr2gray(c["L"]), ctx.bgr2gray(c["R"])) if c["L"].ndim == 3 else (c["L"], c["R"])
    E, vol, disp = twopass(gL, gR, c["gamma_c"], c["gamma_g"], c["win"], c["minD"], c["numD"], c["dt"])
    args = (c["L"], c["R"], c["gamma_c"], c["gamma_g"], c["dt"], c["win"], c["minD"], c["numD"])
    d, v = ctx.computeAdaptiveWeight_twopass(*args, return_cost_volume=True)
    d2 = ctx.computeAdaptiveWeight_twopass(*args)
    return (v, d, d2), (vol, disp)
