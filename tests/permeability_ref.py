"""Restatement of the recursive (information-permeability) cost aggregation over the whole image (Cigla & Alatan 2013; DESIGN.md
section 4.17; k_permeability.hip), twice: vectorised over the frame with one array statement per scan step (aggregate), and as
literal per-pixel loops (aggregate_loop).  The arithmetic is fixed completely -- f64 scans, every product rounded before it is
added, one f64 division -- so the GPU is compared with np.array_equal.  The raw cost is an INPUT (the u8 AD volume of computeAD for
the same direction: the oracle's on the CPU, ctx.computeAD on the GPU), never restated here.

    P[k] = (double)(float)exp(-(double)k / sigma), k = 0..255                                      (math.exp: libm, double)
    ph(x,y) = P[max_c |I_c(x,y) - I_c(x-1,y)|], x >= 1;  pv(x,y) = P[max_c |I_c(x,y) - I_c(x,y-1)|], y >= 1;  I = the view image
    e = min(trunc, AD)
    per row and plane:  LR(0) = e(0), LR(x) = e(x) + ph(x) LR(x-1);  RL(W-1) = e(W-1), RL(x) = e(x) + ph(x+1) RL(x+1);
                        Hs(x) = (LR(x) + RL(x)) - e(x)
    per column and plane: the same with Hs for e and pv for ph -> S
    N = the same two passes over e == 1;  E = S / N;  volume (float)E;  map = min_d + first strict minimum of E over ascending d."""
import math

import numpy as np

LEFT, RIGHT = 0, 1


def table(sigma):
    return np.array([float(np.float32(math.exp(-float(k) / float(sigma)))) for k in range(256)], np.float64)


def _img(img):
    a = np.asarray(img)
    assert a.dtype == np.uint8
    return (a[:, :, None] if a.ndim == 2 else a).astype(np.int64)


def permeabilities(img, sigma):
    """-> ph, pv f64 [H][W]; column 0 of ph and row 0 of pv are not part of the definition (left 0, never read)"""
    g, P = _img(img), table(sigma)
    H, W = g.shape[:2]
    ph, pv = np.zeros((H, W), np.float64), np.zeros((H, W), np.float64)
    ph[:, 1:] = P[np.abs(g[:, 1:] - g[:, :-1]).max(axis=2)]
    pv[1:, :] = P[np.abs(g[1:] - g[:-1]).max(axis=2)]
    return ph, pv


# ---------------------------------------------------------------- vectorised form: one array statement per scan step
def _scan_rows(e, ph):
    """e [D][H][W] f64, ph [H][W] -> Hs"""
    W = e.shape[2]
    LR, RL = np.empty_like(e), np.empty_like(e)
    LR[:, :, 0] = e[:, :, 0]
    for x in range(1, W):
        LR[:, :, x] = e[:, :, x] + ph[None, :, x] * LR[:, :, x - 1]  # the product is rounded, then added
    RL[:, :, W - 1] = e[:, :, W - 1]
    for x in range(W - 2, -1, -1):
        RL[:, :, x] = e[:, :, x] + ph[None, :, x + 1] * RL[:, :, x + 1]
    return (LR + RL) - e


def _two_passes(e, ph, pv):
    hs = _scan_rows(e, ph)
    return _scan_rows(hs.transpose(0, 2, 1), pv.T).transpose(0, 2, 1)  # columns as rows: the same three statements


# ---------------------------------------------------------------- literal form
def _scan_line(e, p):
    n = len(e)
    lr, rl = [0.0] * n, [0.0] * n
    lr[0] = e[0]
    for i in range(1, n):
        lr[i] = e[i] + p[i] * lr[i - 1]
    rl[n - 1] = e[n - 1]
    for i in range(n - 2, -1, -1):
        rl[i] = e[i] + p[i + 1] * rl[i + 1]
    return [(lr[i] + rl[i]) - e[i] for i in range(n)]


def _two_passes_loop(e, ph, pv):
    D, H, W = e.shape
    out = np.empty((D, H, W), np.float64)
    phl, pvl = ph.tolist(), pv.T.tolist()
    for d in range(D):
        hs = [_scan_line(e[d, y].tolist(), phl[y]) for y in range(H)]
        for x in range(W):
            out[d, :, x] = _scan_line([hs[y][x] for y in range(H)], pvl[x])
    return out


def _run(passes, e_u8, img, sigma, trunc, min_d):
    e_u8 = np.asarray(e_u8)
    assert e_u8.dtype == np.uint8 and e_u8.ndim == 3 and 1 <= sigma <= 255 and 1 <= trunc <= 255
    e = np.minimum(e_u8.astype(np.int64), int(trunc)).astype(np.float64)
    ph, pv = permeabilities(img, sigma)
    S = passes(e, ph, pv)
    N = passes(np.ones((1,) + e.shape[1:], np.float64), ph, pv)[0]
    E = np.ascontiguousarray(S / N[None])
    disp = (np.argmin(E, axis=0) + min_d).astype(np.float32)  # first minimum == strict '<' over ascending d (no NaN: N >= 1)
    return E, E.astype(np.float32), disp, N


def aggregate(e_u8, img, sigma=8, trunc=20, min_d=0):
    """e_u8 [D][H][W], img = the view image -> E f64 [D][H][W], the volume (float)E, the map f32 [H][W], N f64 [H][W]"""
    return _run(_two_passes, e_u8, img, sigma, trunc, min_d)


def aggregate_loop(e_u8, img, sigma=8, trunc=20, min_d=0):
    return _run(_two_passes_loop, e_u8, img, sigma, trunc, min_d)


def tie_share(E):
    """share of the pixels whose f64 minimum is reached, bit for bit, at two or more candidates"""
    return float(((E == E.min(axis=0)).sum(axis=0) >= 2).mean())


# ---------------------------------------------------------------- inputs
def textured_pair(H, W, cn, shift, seed, flat=0.5):
    """A blocky scene with mild noise and its copy shifted by `shift` columns: colour steps from 0 (inside the flat blocks: permeability
    1) to well past 103 (barriers at sigma 1), so every part of the table is met."""
    rng = np.random.default_rng(seed)
    Wb = W + shift + 4
    base = rng.integers(0, 256, (H // 5 + 2, Wb // 6 + 2, cn)).astype(np.float64)
    base = np.repeat(np.repeat(base, 5, axis=0), 6, axis=1)[:H, :Wb]
    noise = rng.integers(0, 7, (H, Wb, cn)) * (rng.random((H, Wb, 1)) > flat)
    img = np.clip(base * 0.9 + noise, 0, 255)
    L = img[:, shift:shift + W]
    R = np.clip(img[:, :W] + rng.integers(-3, 4, (H, W, cn)), 0, 255)
    L, R = L.astype(np.uint8), R.astype(np.uint8)
    if cn == 1:
        L, R = L[:, :, 0], R[:, :, 0]
    return np.ascontiguousarray(L), np.ascontiguousarray(R)


def constant_pair(H=9, W=70, cn=1, value=77):
    img = np.full((H, W) if cn == 1 else (H, W, cn), value, np.uint8)
    return img, img.copy()


def row_constant_pair(H=11, W=70, cn=1, seed=5):
    """every row one colour, the same in both views: AD is 0 everywhere, every plane is equal"""
    col = np.random.default_rng(seed).integers(0, 256, (H, 1) if cn == 1 else (H, 1, cn)).astype(np.uint8)
    img = np.ascontiguousarray(np.broadcast_to(col, (H, W) if cn == 1 else (H, W, cn)))
    return img, img.copy()


def barrier_pair(cn=1, H=12, W=160, seed=3):
    """R is x-periodic with period 8 and values below 100; L is R rolled by 5 with columns 60-61 and 120-121 set to 255: at sigma 1
    they are hard barriers (steps above 155 > 103.28), and between them (columns 62..119) candidates 5, 13 and 21 see the same costs
    and the same permeabilities -> bit-equal minima, the first one wins.  -> L, R, D = 24, sigma = 1, trunc = 60"""
    rng = np.random.default_rng(seed)
    cell = rng.integers(0, 100, (H, 8) if cn == 1 else (H, 8, cn)).astype(np.uint8)
    R = np.concatenate([cell] * (W // 8), axis=1)
    L = np.roll(R, 5, axis=1)
    L[:, 60:62] = 255
    L[:, 120:122] = 255
    return np.ascontiguousarray(L), np.ascontiguousarray(R), 24, 1, 60


SIGMAS = (1, 8, 255)
TRUNCS = (1, 20, 255)
SEGMENT = 16   # k_permeability.hip: steps per register segment = checkpoint spacing (both passes)
COST_TILE = 64  # columns of the horizontal pass's cost tile; also the candidates of one wavefront
COLUMNS_PER_WORKGROUP = 8  # columns of the vertical pass's workgroup


def random_case(rng, n=0):
    """A random case for the seeded sweep and the fuzz leg: frames from one pixel up, both directions, 1 and 3 channels, candidates
    past the image, padded rows, constant rectangles (permeability 1, ties).  case["tag"] rebuilds it: build_case(tag)."""
    H = int(rng.choice([1, 2, 15, 16, 17, 33, int(rng.integers(1, 50))]))
    W = int(rng.choice([1, 2, 7, 8, 9, 63, 64, 65, 129, int(rng.integers(1, 150))]))
    D = int(rng.choice([1, 2, 3, 5, 8, 17, int(rng.integers(1, 30))]))
    minD = int(rng.choice([0, 0, 0, 1, 3, 11, max(0, W - 2)]))
    if rng.random() < 0.3:
        sigma, trunc = int(rng.integers(1, 256)), int(rng.integers(1, 256))
    else:
        sigma, trunc = int(rng.choice(SIGMAS + (8,))), int(rng.choice(TRUNCS + (20,)))
    tag = (H, W, int(rng.choice([1, 3])), minD, D, int(rng.integers(0, 2)), sigma, trunc, int(rng.integers(0, 1 << 30)),
           int(rng.choice([0, 0, 0, 3])), int(rng.choice([0, 0, 1])))
    return build_case(tag)


def build_case(tag):
    H, W, cn, minD, D, dt, sigma, trunc, seed, pad, flat = tag
    rng = np.random.default_rng(seed)
    L, R = textured_pair(H, W + pad, cn, int(rng.integers(0, 8)), seed)
    if flat:
        for img in (L, R):
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            img[y0:y0 + int(rng.integers(1, 40)), x0:x0 + int(rng.integers(1, 60))] = int(rng.integers(0, 256))
    return {"tag": tag, "L": L[:, :W], "R": R[:, :W], "sigma": sigma, "trunc": trunc, "minD": minD, "D": D, "dt": dt}


def gpu_result(ctx, case):
    """((volume, map) of the library with the volume kept, map without it) and the restatement's (volume, map)"""
    c = case
    e = np.stack(ctx.computeAD(c["L"], c["R"], c["dt"], c["minD"], c["D"]))
    E, vol, disp, N = aggregate(e, c["R"] if c["dt"] else c["L"], c["sigma"], c["trunc"], c["minD"])
    args = (c["L"], c["R"], c["dt"], c["sigma"], c["trunc"], c["minD"], c["D"])
    d, v = ctx.computeAdaptiveWeight_permeability(*args, return_cost_volume=True)
    d2 = ctx.computeAdaptiveWeight_permeability(*args)
    return (v, d, d2), (vol, disp)
