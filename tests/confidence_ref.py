"""Restatement of the per-pixel confidence (include/asw_mi355x.h "Confidence") for the tests.

There is no reference implementation of this measure; the rule is the library's own and is fixed completely: comparisons of f32
values, two f64 subtractions and one f64 division, each one IEEE operation, rounded to f32.  The kernel must agree to the last bit
(np.array_equal).  The volume V the rule starts from is not restated here: it is what the same call returns.

    F = {k : V[k] finite};  F empty -> 0
    c1 = min over F, k1 = the smallest k with V[k] == c1, cmax = max over F
    G = {k in F : |k - k1| >= 2};  G empty, cmax == c1 or c2 == c1 -> 0 (+0)
    c2 = min over G;  conf = (float)(((double)c2 - (double)c1) / ((double)cmax - (double)c1))

Two forms: confidence_vec (numpy over the whole volume) and confidence_loop (the rule, pixel by pixel, candidate by candidate)."""
import numpy as np

import cross_scale_ref as cs
import scanline_ref as sr
from cross_scale_ref import METHODS, algorithm, textured_pair, wta  # noqa: F401  (one copy of the method list and of k_wta's rule)

LEFT, RIGHT = 0, 1
INF = np.float32(np.inf)


def confidence_vec(V):
    """V: f32 [n][...] -> f32 [...]"""
    V = np.asarray(V, np.float32)
    n = V.shape[0]
    fin = np.isfinite(V)
    lo = np.where(fin, V, INF)
    c1 = lo.min(axis=0)
    k1 = lo.argmin(axis=0)  # the first occurrence
    cmax = np.where(fin, V, -INF).max(axis=0)
    k = np.arange(n).reshape((n,) + (1,) * (V.ndim - 1))
    in_g = fin & (np.abs(k - k1[None]) >= 2)
    c2 = np.where(in_g, V, INF).min(axis=0)
    ok = fin.any(axis=0) & in_g.any(axis=0) & (cmax != c1) & (c2 != c1)
    c1d, c2d, cmd = (np.where(ok, a, 0).astype(np.float64) for a in (c1, c2, cmax))
    den = np.where(ok, cmd - c1d, 1.0)
    return np.where(ok, (c2d - c1d) / den, 0.0).astype(np.float32)


def confidence_loop(V):
    """the rule as the header words it, one pixel and one candidate at a time"""
    V = np.asarray(V, np.float32)
    n = V.shape[0]
    flat = V.reshape(n, -1)
    out = np.zeros(flat.shape[1], np.float32)
    for p in range(flat.shape[1]):
        col = flat[:, p]
        F = [k for k in range(n) if np.isfinite(col[k])]
        if not F:
            continue
        k1 = F[0]
        for k in F:
            if col[k] < col[k1]:  # strict '<' in ascending k
                k1 = k
        c1 = col[k1]
        cmax = col[F[0]]
        for k in F:
            if col[k] > cmax:
                cmax = col[k]
        G = [k for k in F if abs(k - k1) >= 2]
        if not G or cmax == c1:
            continue
        c2 = col[G[0]]
        for k in G:
            if col[k] < c2:
                c2 = col[k]
        if c2 == c1:
            continue
        num = np.float64(c2) - np.float64(c1)
        den = np.float64(cmax) - np.float64(c1)
        out[p] = np.float32(num / den)
    return out.reshape(V.shape[1:])


def same_bits(a, b):
    """equal shapes and equal f32 bit patterns: tells -0 from +0 and one NaN from another"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def random_volume(rng, n, H, W):
    """a volume for the rule's own tests: a few distinct values per column (ties, adjacent and not), zeros of both signs, and NaN,
    +inf and -inf planted in a share of the slots, a share of the columns and a share of the pixels entirely"""
    levels = rng.standard_normal(int(rng.integers(2, 7))).astype(np.float32) * np.float32(10.0 ** int(rng.integers(-3, 4)))
    levels[int(rng.integers(len(levels)))] = 0.0
    V = levels[rng.integers(0, len(levels), (n, H, W))]
    fine = rng.random((n, H, W)) < 0.5
    V = np.where(fine, V + rng.standard_normal((n, H, W)).astype(np.float32), V).astype(np.float32)
    V = np.where(rng.random((n, H, W)) < 0.05, np.float32(-0.0), V)
    for bad in (np.float32(np.nan), INF, -INF):
        V = np.where(rng.random((n, H, W)) < 0.08, bad, V)
    V = np.where((rng.random((H, W)) < 0.1)[None], np.float32(np.nan), V)
    return np.ascontiguousarray(V, np.float32)


# ---- seeded GPU cases: tests/test_gpu_confidence.py and the leg `confidence` of tools/fuzz_parity.py ----
def build_case(tag):
    """the case of a tag (method, dt, H, W, cn, win, minD, numD, step, subpixel, shift, seed), as random_case draws and prints it;
    step: 0, or a cross_scale_ref.encode() / scanline_ref.encode() value"""
    method, dt, H, W, cn, win, minD, numD, step, sub, shift, seed = tag
    L, R = textured_pair(H, W, cn, shift, seed)
    return {"method": method, "alg": algorithm(method), "extra": METHODS[method][1], "dt": dt, "win": win, "minD": minD, "numD": numD,
            "step": step, "subpixel": sub, "L": L, "R": R, "tag": tuple(tag)}


def random_case(rng, n=0):
    """One seeded confidence case: a method, a direction it serves, a small frame (at most about 2500 pixels; rows * cols of every
    residue mod 4, on both sides of the kernel's 256 and 1024 pixels per workgroup), a candidate range around the kernel's unroll
    width (4) and now and then around 64, no step flag, the cross-scale flag or the scanline flag, and sometimes a sub-pixel flag."""
    method = list(METHODS)[int(rng.integers(len(METHODS)))]
    sel, extra, right, gray, wins, min0 = METHODS[method]
    W = int((1, 2, 3, 5, 7, 16, 31, 32, 33, 63, 64, 65, 72, 100)[int(rng.integers(14))])
    H = int(rng.integers(1, max(2, min(40, 2500 // W)) + 1))
    cn = 1 if (gray and rng.integers(3) == 0) else 3
    dt = RIGHT if (right and rng.integers(2)) else LEFT
    minD = 0 if min0 else int(rng.integers(0, 8))
    numD = int(rng.integers(1, 25)) if rng.integers(6) else int((62, 63, 64, 65, 66)[int(rng.integers(5))])
    if numD > 30 and H * W > 600:
        H = max(1, 600 // W)
    kind = int(rng.integers(4))  # 0, 1: no step flag
    step = 0
    if kind == 2:
        S = int(rng.integers(2, 6))
        while cs.scale_ranges(minD, numD + extra, extra, S) is None:
            numD += 1
        step = cs.encode(S, int(rng.integers(1, 256)))
    elif kind == 3:
        step = sr.encode(int(rng.integers(1, 128)), int(rng.integers(0, 8)), int(rng.integers(1, 9)))
    sub = int((0, 0, 0x100, 0x200)[int(rng.integers(4))])
    shift = minD + int(rng.integers(min(numD, 24)))
    win = int(wins[int(rng.integers(len(wins)))])
    return build_case((method, dt, H, W, cn, win, minD, numD, step, sub, shift, int(rng.integers(1 << 30))))


_ctx2 = []  # gpu_result's second context, created at first use


def gpu_result(ctx, case):
    """The leg confidence of tools/fuzz_parity.py, in the form of its other legs: ((volume, {map, confidence}, the same without a
    kept volume) of the 2-channel call, (volume, {map, confidence})): volume and map of a second context's 1-channel call with the
    same flags, the confidence the restatement applied to the volume the 2-channel call returned.  NaN slots are compared as -1e30
    and infinities as -2e30 / -3e30 (no method returns such a cost)."""
    import aswstereomatch_amd as asw

    if not _ctx2:
        _ctx2.append(asw.Context(0))
    c = case
    dt = c["dt"] | c["subpixel"] | c["step"]
    args = (c["L"], c["R"], dt, c["alg"], c["win"], c["minD"], c["numD"])
    d, v, conf = ctx.stereoMatching(*args, return_cost_volume=True, return_confidence=True)
    d2, conf2 = ctx.stereoMatching(*args, return_confidence=True)
    d0, v0 = _ctx2[0].stereoMatching(*args, return_cost_volume=True)

    def plainify(a):
        a = np.where(np.isnan(a), np.float32(-1e30), a)
        return np.where(np.isposinf(a), np.float32(-2e30), np.where(np.isneginf(a), np.float32(-3e30), a))

    return (plainify(v), np.stack([d, conf]), np.stack([d2, conf2])), (plainify(v0), np.stack([d0, confidence_vec(v)]))
