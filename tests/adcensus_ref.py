"""Restatement of the AD-Census cost (Mei et al. 2011; census of Zabih & Woodfill 1994), twice and
independently: a literal loop over every pixel (census_loop / cost_loop) and a vectorised form (census / hamming / ad / cost).
All integer; the two tables come from numpy's double exp.  The aggregation is tests/cross_ref.py's, with trunc 255.

    gray_pair(L, R, bits)                 -> the two gray images (cvlite.cvtColor_BGR2GRAY for 3 channels, the images themselves for 1)
    census(G)                             -> uint64 [H][W]: bit (dy + 3) * 9 + dx + 4 set when G[clamp][clamp] < G[y][x]
    hamming(L, R, dt, minD, D, bits)      -> uint8 [D][H][W], 0..62
    ad(L, R, dt, minD, D)                 -> uint8 [D][H][W]: computeAD's value (mean3 rule, BORDER_REFLECT)
    tables(lambda_ad, lambda_census)      -> TA int64 [256], TC int64 [63]
    cost(L, R, dt, lam_ad, lam_c, minD, D, bits) -> uint8 [D][H][W] = TA[ad] + TC[hamming]
    match(L, R, dt, tau, lam_ad, lam_c, win, minD, D, bits) -> S, N, E, disp of cross_ref.aggregate over cost
    table_margin(lam, n)                  -> the smallest distance of 127 (1 - exp(-v / lam)), v < n, from a half-integer"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cross_ref as cr  # noqa: E402
import cvlite  # noqa: E402

RY, RX = 3, 4  # the 9-wide, 7-high window


def gray_pair(L, R, bits=14):
    L, R = np.asarray(L), np.asarray(R)
    if L.ndim == 3:
        return cvlite.cvtColor_BGR2GRAY(L, bits), cvlite.cvtColor_BGR2GRAY(R, bits)
    return L, R


def reflect(p, n):
    """BORDER_REFLECT index (reflect_idx of asw_device.h), repeated until inside"""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p - 1 if p < 0 else 2 * n - 1 - p
    return p


def _reflect_vec(p, n):
    if n == 1:
        return np.zeros_like(p)
    q = np.mod(p, 2 * n)  # the pattern abc|cba has period 2 n
    return np.where(q < n, q, 2 * n - 1 - q)


def tables(lambda_ad, lambda_census):
    ta = np.floor(127.0 * (1.0 - np.exp(-np.arange(256, dtype=np.float64) / float(lambda_ad))) + 0.5).astype(np.int64)
    tc = np.floor(127.0 * (1.0 - np.exp(-np.arange(63, dtype=np.float64) / float(lambda_census))) + 0.5).astype(np.int64)
    return ta, tc


def table_margin(lam, n):
    v = 127.0 * (1.0 - np.exp(-np.arange(n, dtype=np.float64) / float(lam)))
    return float(np.abs(v - np.floor(v) - 0.5).min())


# ---------------------------------------------------------------- literal form
def census_loop(G):
    G = np.asarray(G)
    H, W = G.shape
    out = [[0] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            code = 0
            for dy in range(-RY, RY + 1):
                for dx in range(-RX, RX + 1):
                    if (dy or dx) and G[min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)] < G[y, x]:
                        code |= 1 << ((dy + RY) * (2 * RX + 1) + dx + RX)
            out[y][x] = code
    return out


def cost_loop(L, R, dt, lambda_ad, lambda_census, minD, D, bits=14):
    """(hamming, ad, cost), each uint8 [D][H][W], pixel by pixel"""
    L, R = np.asarray(L), np.asarray(R)
    A, B = (R, L) if dt else (L, R)
    gA, gB = gray_pair(A, B, bits)
    cA, cB = census_loop(gA), census_loop(gB)
    ta, tc = tables(lambda_ad, lambda_census)
    H, W = gA.shape
    s = 1 if dt else -1
    ham = np.zeros((D, H, W), np.uint8)
    adv = np.zeros((D, H, W), np.uint8)
    e = np.zeros((D, H, W), np.uint8)
    for k in range(D):
        for y in range(H):
            for x in range(W):
                xb = reflect(x + s * (minD + k), W)
                h = bin(cA[y][x] ^ cB[y][xb]).count("1")
                if A.ndim == 3:
                    c = [abs(int(A[y, x, i]) - int(B[y, xb, i])) for i in range(3)]
                    a = (min(255, c[0] + c[1]) + c[2] + 1) // 3  # mean3_u8
                else:
                    a = abs(int(A[y, x]) - int(B[y, xb]))
                ham[k, y, x], adv[k, y, x], e[k, y, x] = h, a, ta[a] + tc[h]
    return ham, adv, e


# ---------------------------------------------------------------- vectorised form
def census(G):
    G = np.asarray(G).astype(np.int64)
    H, W = G.shape
    P = np.pad(G, ((RY, RY), (RX, RX)), mode="edge")
    code = np.zeros((H, W), np.uint64)
    for dy in range(-RY, RY + 1):
        for dx in range(-RX, RX + 1):
            if dy == 0 and dx == 0:
                continue
            less = P[RY + dy:RY + dy + H, RX + dx:RX + dx + W] < G
            code |= less.astype(np.uint64) << np.uint64((dy + RY) * (2 * RX + 1) + dx + RX)
    return code


def _popcount64(v):
    b = np.ascontiguousarray(v).view(np.uint8).reshape(v.shape + (8,))
    return np.unpackbits(b, axis=-1).sum(axis=-1)


def _partners(W, dt, minD, D):
    s = 1 if dt else -1
    return [_reflect_vec(np.arange(W) + s * (minD + k), W) for k in range(D)]


def hamming(L, R, dt, minD, D, bits=14):
    A, B = (R, L) if dt else (L, R)
    gA, gB = gray_pair(A, B, bits)
    cA, cB = census(gA), census(gB)
    return np.stack([_popcount64(cA ^ cB[:, xb]) for xb in _partners(gA.shape[1], dt, minD, D)]).astype(np.uint8)


def ad(L, R, dt, minD, D):
    L, R = np.asarray(L), np.asarray(R)
    A, B = ((R, L) if dt else (L, R))
    A, B = A.astype(np.int64), B.astype(np.int64)
    out = []
    for xb in _partners(A.shape[1], dt, minD, D):
        c = np.abs(A - B[:, xb])
        out.append((np.minimum(255, c[..., 0] + c[..., 1]) + c[..., 2] + 1) // 3 if A.ndim == 3 else c)
    return np.stack(out).astype(np.uint8)


def cost(L, R, dt, lambda_ad, lambda_census, minD, D, bits=14):
    ta, tc = tables(lambda_ad, lambda_census)
    e = ta[ad(L, R, dt, minD, D)] + tc[hamming(L, R, dt, minD, D, bits)]
    assert e.max(initial=0) <= 254
    return e.astype(np.uint8)


def match(L, R, dt, tau, lambda_ad, lambda_census, win, minD, D, bits=14, e=None):
    """S, N, E, disp of the cross-based aggregation (trunc 255: a no-op) over the AD-Census cost (or over e, a u8 volume)"""
    if e is None:
        e = cost(L, R, dt, lambda_ad, lambda_census, minD, D, bits)
    return cr.aggregate(e, cr.arms(R if dt else L, tau, win // 2), 255, minD)


# ---------------------------------------------------------------- random cases (tools/fuzz_parity.py, leg "adcensus")
def random_case(rng, n=0):
    """cross_ref.random_case plus random lambdas; case["tag"] rebuilds it: build_case(tag)"""
    c = cr.random_case(rng, n)
    lam = (int(rng.choice([1, 5, 10, 10, 17, 31])), int(rng.choice([1, 12, 30, 30, 45, 255])))
    return build_case(tuple(c["tag"]) + lam)


def build_case(tag):
    c = cr.build_case(tuple(tag[:-2]))
    c["tag"], c["lambda_ad"], c["lambda_census"] = tuple(tag), int(tag[-2]), int(tag[-1])
    return c


def gpu_result(ctx, case):
    """((volume, map) of the library with the volume kept, map without it) and the restatement's (volume, map)"""
    c = case
    args = (c["L"], c["R"], c["dt"], c["tau"], c["lambda_ad"], c["lambda_census"], c["win"], c["minD"], c["D"])
    S, N, E, disp = match(*args)
    d, v = ctx.computeAdaptiveWeight_adcensus(*args, return_cost_volume=True)
    d2 = ctx.computeAdaptiveWeight_adcensus(*args)
    return (v, d, d2), (E, disp)
