"""Restatement of the confidence-weighted edge-aware smoothing (include/asw_mi355x.h "Smoothing") for the tests.

There is no reference implementation the library is held to: the rule is the fast global smoother of Min et al. (TIP 2014) as the
header words it, a fixed sequence of IEEE f64 operations (numpy's float64 arithmetic performs each of them as one correctly rounded
operation and never fuses two), so the kernels must agree to the last bit.

    ce = c if (d, c finite and c > 0) else 0;  N = ce * d (0 in a hole), D = ce
    Wt[k] = floor(65536 * exp(-k / sigma_c) + 0.5) / 65536;  wh / wv = Wt[sum over channels |G(p) - G(left / upper neighbour)|]
    for t = 1..T: lam_t = 1.5 * lambda * 4^(T - t) / (4^T - 1); every row, then every column: solve (N, D) along the line
    out = float32(N / D) where D > 0, else d

Two forms: smooth_vec (a pass over all its lines at once, one numpy operation per written operation) and smooth_loop (the rule,
line by line and step by step, on Python scalars of type numpy.float64)."""
import math

import numpy as np

F64 = np.float64
DEFAULTS = {"sigma_c": 8.0, "lam": 900.0, "iterations": 3}  # the Python wrappers' defaults


def table(sigma_c, channels):
    """step 3, with libm's exp as the host builds it"""
    return np.array([math.floor(65536.0 * math.exp(-float(k) / float(sigma_c)) + 0.5) / 65536.0 for k in range(255 * channels + 1)], F64)


def links(G):
    """step 4's table indices: (kh, kv), int [H][W]; kh[:, 0] and kv[0, :] are unused (0)"""
    G = np.asarray(G)
    g = (G if G.ndim == 3 else G[:, :, None]).astype(np.int64)
    kh = np.zeros(g.shape[:2], np.int64)
    kv = np.zeros(g.shape[:2], np.int64)
    kh[:, 1:] = np.abs(g[:, 1:] - g[:, :-1]).sum(axis=2)
    kv[1:, :] = np.abs(g[1:, :] - g[:-1, :]).sum(axis=2)
    return kh, kv


def start_planes(d, c):
    """steps 1-2"""
    d = np.asarray(d, np.float32)
    c = np.asarray(c, np.float32)
    ok = np.isfinite(d) & np.isfinite(c) & (c > 0)
    ce = np.where(ok, c, np.float32(0)).astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        N = np.where(ok, ce * np.where(ok, d, np.float32(0)).astype(F64), F64(0))
    return N, ce


def lam_t(lam, T, t):
    return (F64(1.5) * F64(lam) * F64(1 << 2 * (T - t))) / F64((1 << 2 * T) - 1)


def solve_lines_vec(fs, w, lam):
    """fs: a list of right-hand sides, each f64 [lines][n]; w: f64 [lines][n], w[:, i] the link between steps i - 1 and i (column 0
    unused) -> the solutions, in the same shapes"""
    lines, n = w.shape
    zero = np.zeros(lines, F64)
    cp = np.zeros((lines, n), F64)
    fp = [np.zeros((lines, n), F64) for _ in fs]
    for i in range(n):
        a = -(lam * w[:, i]) if i >= 1 else zero
        c = -(lam * w[:, i + 1]) if i + 1 < n else zero
        b = (F64(1.0) - a) - c
        m = b - a * cp[:, i - 1] if i >= 1 else b
        r = F64(1.0) / m
        cp[:, i] = c * r
        for f, p in zip(fs, fp):
            p[:, i] = (f[:, i] - a * p[:, i - 1]) * r if i >= 1 else f[:, i] * r
    us = [np.zeros((lines, n), F64) for _ in fs]
    for p, u in zip(fp, us):
        u[:, n - 1] = p[:, n - 1]
        for i in range(n - 2, -1, -1):
            u[:, i] = p[:, i] - cp[:, i] * u[:, i + 1]
    return us


def solve_line_loop(fs, w, lam):
    """one line: fs a list of sequences of numpy.float64, w[i] the link between steps i - 1 and i (w[0] unused)"""
    n = len(w)
    if n == 1:
        return [[F64(f[0])] for f in fs]  # a line of length 1 returns its input
    a = [F64(0.0)] + [-(F64(lam) * F64(w[i])) for i in range(1, n)]
    c = [-(F64(lam) * F64(w[i + 1])) for i in range(n - 1)] + [F64(0.0)]
    b = [(F64(1.0) - a[i]) - c[i] for i in range(n)]
    cp, r = [], []
    for i in range(n):
        m = b[0] if i == 0 else b[i] - a[i] * cp[i - 1]
        r.append(F64(1.0) / m)
        cp.append(c[i] * r[i])
    out = []
    for f in fs:
        fp = []
        for i in range(n):
            fp.append(F64(f[0]) * r[0] if i == 0 else (F64(f[i]) - a[i] * fp[i - 1]) * r[i])
        u = [None] * n
        u[n - 1] = fp[n - 1]
        for i in range(n - 2, -1, -1):
            u[i] = fp[i] - cp[i] * u[i + 1]
        out.append(u)
    return out


def finish(N, D, d):
    """step 6"""
    d = np.asarray(d, np.float32)
    ok = D > 0
    with np.errstate(over="ignore"):
        q = (np.where(ok, N, F64(0)) / np.where(ok, D, F64(1))).astype(np.float32)
    return np.where(ok, q.view(np.uint32), d.view(np.uint32)).view(np.float32)  # the input's bits, a NaN's payload included


def smooth_vec(G, d, c, sigma_c=DEFAULTS["sigma_c"], lam=DEFAULTS["lam"], iterations=DEFAULTS["iterations"]):
    G = np.asarray(G)
    Wt = table(sigma_c, 1 if G.ndim == 2 else G.shape[2])
    kh, kv = links(G)
    wh, wvT = Wt[kh], np.ascontiguousarray(Wt[kv].T)
    N, D = start_planes(d, c)
    T = int(iterations)
    for t in range(1, T + 1):
        lt = lam_t(lam, T, t)
        N, D = solve_lines_vec([N, D], wh, lt)
        NT, DT = solve_lines_vec([np.ascontiguousarray(N.T), np.ascontiguousarray(D.T)], wvT, lt)
        N, D = np.ascontiguousarray(NT.T), np.ascontiguousarray(DT.T)
    return finish(N, D, d)


def smooth_loop(G, d, c, sigma_c=DEFAULTS["sigma_c"], lam=DEFAULTS["lam"], iterations=DEFAULTS["iterations"]):
    """the rule as the header words it, one line and one step at a time"""
    G = np.asarray(G)
    g = G if G.ndim == 3 else G[:, :, None]
    H, W, C = g.shape
    Wt = table(sigma_c, C)
    d = np.asarray(d, np.float32)
    c = np.asarray(c, np.float32)
    N = [[F64(0.0)] * W for _ in range(H)]
    D = [[F64(0.0)] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            ce = F64(c[y, x]) if (np.isfinite(d[y, x]) and np.isfinite(c[y, x]) and c[y, x] > 0) else F64(0.0)
            N[y][x] = ce * F64(d[y, x]) if ce > 0 else F64(0.0)
            D[y][x] = ce

    def wlink(y, x, yp, xp):
        return Wt[sum(abs(int(g[y, x, ch]) - int(g[yp, xp, ch])) for ch in range(C))]

    T = int(iterations)
    for t in range(1, T + 1):
        lt = lam_t(lam, T, t)
        for y in range(H):
            w = [F64(0.0)] + [wlink(y, x, y, x - 1) for x in range(1, W)]
            N[y], D[y] = solve_line_loop([N[y], D[y]], w, lt)
        for x in range(W):
            w = [F64(0.0)] + [wlink(y, x, y - 1, x) for y in range(1, H)]
            un, ud = solve_line_loop([[N[y][x] for y in range(H)], [D[y][x] for y in range(H)]], w, lt)
            for y in range(H):
                N[y][x], D[y][x] = un[y], ud[y]
    return finish(np.array(N, F64).reshape(H, W), np.array(D, F64).reshape(H, W), d)


def same_bits(a, b):
    """equal shapes and equal f32 bit patterns: tells -0 from +0 and one NaN from another"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- case makers: tests/test_gpu_smooth.py, tests/test_smooth_cpu.py and the leg `smooth` of tools/fuzz_parity.py ----
GUIDES = ("noise", "constant", "edges", "smooth", "blocks")


def make_guide(rng, H, W, cn, kind, pad=0):
    """an 8U guide [H][W] or [H][W][3]; pad > 0: a view into rows that carry `pad` more pixels (the C-ABI reads it through its step)"""
    shape = (H, W + pad) if cn == 1 else (H, W + pad, cn)
    if kind == "constant":
        full = np.full(shape, int(rng.integers(256)), np.uint8)
    elif kind == "edges":  # one vertical and one horizontal step edge
        full = np.full(shape, 40, np.uint8)
        full[:, (W + 1) // 2:] = 200
        full[(H + 1) // 2:] = 255 - full[(H + 1) // 2:]
    elif kind == "smooth":  # neighbours differ by a few levels: every link carries weight
        yy, xx = np.mgrid[0:H, 0:W + pad]
        base = (3 * xx + 5 * yy + rng.integers(0, 4, (H, W + pad))) % 256
        full = (base if cn == 1 else np.stack([base, (base + 7) % 256, (base * 2) % 256], axis=2)).astype(np.uint8)
    elif kind == "blocks":  # constant blocks with strong edges between them
        by, bx = int(rng.integers(2, 9)), int(rng.integers(2, 9))
        small = rng.integers(0, 256, ((H + by - 1) // by, (W + pad + bx - 1) // bx) + shape[2:])
        full = np.repeat(np.repeat(small, by, axis=0), bx, axis=1)[:H, :W + pad].astype(np.uint8)
    else:
        full = rng.integers(0, 256, shape).astype(np.uint8)
    if pad:
        full[:, W:] = 255 - full[:, W - 1:W]  # what a kernel that ignored the step would read
        return full[:, :W]
    return np.ascontiguousarray(full)


def make_map(rng, H, W, bad=0.0):
    """a disparity-like f32 map: integers, fractions, zeros of both signs; `bad`: the share of NaN / +inf / -inf pixels (each)"""
    d = rng.integers(0, 64, (H, W)).astype(np.float32)
    d = np.where(rng.random((H, W)) < 0.3, d + rng.random((H, W)).astype(np.float32), d).astype(np.float32)
    d = np.where(rng.random((H, W)) < 0.05, np.float32(-0.0), d)
    d = np.where(rng.random((H, W)) < 0.05, -d, d)
    for v in (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)):
        d = np.where(rng.random((H, W)) < bad, v, d)
    return np.ascontiguousarray(d, np.float32)


def make_conf(rng, H, W, kind="mixed"):
    """a confidence plane.  mixed: values in (0, 1] with zeros, negatives, NaN, inf and values above 1 planted; mask: 0 / 1; zero: all 0;
    unit: values in (0, 1] only"""
    if kind == "zero":
        return np.zeros((H, W), np.float32)
    if kind == "mask":
        return (rng.random((H, W)) < 0.6).astype(np.float32)
    c = (1.0 - rng.random((H, W))).astype(np.float32)
    if kind == "mixed":
        for v, share in ((0.0, 0.15), (-0.0, 0.03), (-0.5, 0.05), (np.nan, 0.04), (np.inf, 0.02), (-np.inf, 0.02), (3.5, 0.05), (1e-30, 0.02)):
            c = np.where(rng.random((H, W)) < share, np.float32(v), c)
    return np.ascontiguousarray(c, np.float32)


def build_case(tag):
    """the case of a tag (H, W, cn, guide kind, pad, conf kind, bad share in 1/100, T, lambda, sigma_c, seed), as random_case draws
    and prints it"""
    H, W, cn, kind, pad, ckind, bad, T, lam, sigma_c, seed = tag
    rng = np.random.default_rng(seed)
    G = make_guide(rng, H, W, cn, kind, pad)
    return {"G": G, "d": make_map(rng, H, W, bad / 100.0), "c": make_conf(rng, H, W, ckind), "T": T, "lam": lam, "sigma_c": sigma_c,
            "tag": tuple(tag)}


SIZES = (1, 2, 3, 5, 15, 16, 17, 31, 32, 33, 47, 63, 64, 65, 70, 100, 129)  # around the kernels' 16, 32 and 64
LAMBDAS = (2.0 ** -10, 1.0, 30.0, 900.0, 2.0 ** 20)
SIGMAS = (0.05, 0.7, 8.0, 25.0, 1000.0)


def random_case(rng, n=0):
    """One seeded smoothing case: a small frame (at most about 5000 pixels) with sides around the kernels' tile constants, a guide of
    one of the kinds of GUIDES with 1 or 3 channels and sometimes padded rows, a map with or without non-finite pixels, a confidence
    of one of make_conf's kinds, T in 1..8 and lambda / sigma_c from the lists above."""
    W = int(SIZES[int(rng.integers(len(SIZES)))])
    H = int(SIZES[int(rng.integers(len(SIZES)))])
    if H * W > 5000:
        H = max(1, 5000 // W)
    cn = 3 if rng.integers(3) else 1
    kind = GUIDES[int(rng.integers(len(GUIDES)))]
    pad = int(rng.integers(1, 9)) if rng.integers(5) == 0 else 0
    ckind = ("mixed", "mixed", "unit", "mask", "zero")[int(rng.integers(5))]
    bad = int((0, 0, 3, 10)[int(rng.integers(4))])
    T = int((1, 2, 3, 3, 4, 8)[int(rng.integers(6))])
    lam = float(LAMBDAS[int(rng.integers(len(LAMBDAS)))])
    sigma_c = float(SIGMAS[int(rng.integers(len(SIGMAS)))])
    return build_case((H, W, cn, kind, pad, ckind, bad, T, lam, sigma_c, int(rng.integers(1 << 30))))


def gpu_result(ctx, case):
    """The leg smooth of tools/fuzz_parity.py, in the form of its other legs: ((v, d, d2), (vw, dw)), all as u32 bit patterns (a NaN
    that passes through must keep its bits): v the context's result, d the same call again (the tables and scratch are warm), d2 a
    fresh context's; vw = dw = the restatement."""
    import aswstereomatch_amd as asw

    c = case
    args = (c["G"], c["d"], c["c"], c["sigma_c"], c["lam"], c["T"])
    want = smooth_vec(*args).view(np.uint32)
    v = ctx.smoothDisparity(*args).view(np.uint32)
    d = ctx.smoothDisparity(*args).view(np.uint32)
    fresh = asw.Context(0)
    try:
        d2 = fresh.smoothDisparity(*args).view(np.uint32)
    finally:
        fresh.close()
    return (v, d, d2), (want, want)
