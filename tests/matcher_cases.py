"""Inputs on which winner-take-all matchers go wrong first, and a seeded case generator for the integer kernels (SGBM, SGBM over a
mask of path directions, StereoBM, filterSpeckles, the left-right refinement, the sub-pixel flag).  Plain numpy: nothing here needs
a GPU.  TEST INFRASTRUCTURE ONLY.

Three parts:

  the tie-dense pair generators (`constant`, `periodic`, `row_constant`, `quantised`, `flat_rects`; `textured` is plain
  make_pair) and `tie_share`, which measures on a cost volume how often the minimum is shared; `tie_pair`, `noise` and
  `SGBM_TINY_FRAMES` are the fixed inputs that the degenerate-input files of SGBM and of SGBM over path masks share;

  `random_case(rng, family, index)` / `build_case(family, tag)`: a case is rebuilt from its tag alone, so the tuple an assertion
  prints is enough to run that case again;

  `reference(case)` and `gpu_result(ctx, case)`: the restatement's answer and the library's, in the same layout, for
  tests/test_gpu_matcher_degenerate.py and tools/fuzz_parity.py alike (`ctx` is an aswstereomatch_amd.Context).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import refine_ref  # noqa: E402
import sgbm_paths_ref  # noqa: E402
import sgbm_ref  # noqa: E402
import stereobm_ref  # noqa: E402
import subpixel_ref  # noqa: E402
from aswstereomatch_amd.synth import make_pair  # noqa: E402

FAMILIES = ("sgbm", "bm", "speckles", "refine", "subpixel", "sgbm_paths")
KINDS = ("constant", "periodic", "row_constant", "quantised", "flat_rects", "textured")
# the seeds and case counts of the sweep in tests/test_gpu_matcher_degenerate.py; tests/test_matcher_cases_cpu.py runs the
# restatements over the same cases
SWEEP_SEEDS = (20261, 20262)
SWEEP_COUNTS = {"sgbm": 30, "bm": 30, "speckles": 30, "refine": 12, "subpixel": 12, "sgbm_paths": 30}

# selector value, DISPARITY_RIGHT served (the nine methods that take the sub-pixel flag; tests/test_gpu_subpixel.py METHODS)
SUBPIXEL_METHODS = {
    "classic": (2, True), "direct8": (3, False), "geodesic": (4, True), "bilgrid": (5, False), "BLO1": (6, True),
    "GuidedF": (7, True), "GuidedF_2": (8, False), "GuidedF_3": (9, True), "median": (10, False),
}


# ---------------------------------------------------------------- tie-dense pairs: (L, R) uint8 [H][W] or [H][W][3]
def _channels(img3, cn):
    return np.ascontiguousarray(img3[:, :, 1]) if cn == 1 else np.ascontiguousarray(img3)


def _shape(H, W, cn):
    return (H, W) if cn == 1 else (H, W, 3)


def constant(H, W, cn, value=90):
    """one value in both images"""
    L = np.full(_shape(H, W, cn), value, np.uint8)
    return L, L.copy()


def periodic(H, W, cn, p, shift):
    """a random pattern of period p along x; R is L rolled by `shift` columns: every disparity = shift (mod p) matches equally"""
    base = np.random.default_rng(p).integers(0, 256, _shape(H, p, cn))
    reps = (W + p - 1) // p
    L = np.tile(base, (1, reps) if cn == 1 else (1, reps, 1))[:, :W].astype(np.uint8)
    return np.ascontiguousarray(L), np.ascontiguousarray(np.roll(L, -shift, axis=1))


def row_constant(H, W, cn, seed=0):
    """every row one value, identical pair: no horizontal gradient anywhere"""
    v = np.random.default_rng(seed).integers(0, 256, (H, 1) if cn == 1 else (H, 1, 3))
    L = np.ascontiguousarray(np.broadcast_to(v, _shape(H, W, cn)).astype(np.uint8))
    return L, L.copy()


def textured(H, W, cn, seed=0, D=16):
    L, R, _ = make_pair(H, W, max(2, min(D, max(W // 3, 1)) // 2), seed=seed, block=16)
    return _channels(L, cn), _channels(R, cn)


def quantised(H, W, cn, seed=0, D=16):
    """make_pair reduced to four grey levels: wide plateaus, saturated prefilter values"""
    L, R = textured(H, W, cn, seed, D)
    return (L // 64 * 64).astype(np.uint8), (R // 64 * 64).astype(np.uint8)


def flat_rects(H, W, cn, seed=0, D=16):
    """make_pair with one to three constant rectangles pasted into each image (as tools/fuzz_parity.py --flat does)"""
    L, R, _ = make_pair(H, W, max(2, min(D, max(W // 3, 1)) // 2), seed=seed, block=16)
    rng = np.random.default_rng(seed + 1)
    for img in (L, R):
        for _ in range(int(rng.integers(1, 4))):
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            img[y0:y0 + int(rng.integers(1, 12)), x0:x0 + int(rng.integers(1, 40))] = rng.integers(0, 256, 3).astype(np.uint8)
    return _channels(L, cn), _channels(R, cn)


_PERIODS = (2, 3, 4, 5, 8, 16)


def make_input(kind, H, W, cn, seed, D=16):
    """the pair of `kind`; the free parameters of a kind (value, period and shift, row values, texture) follow from `seed`"""
    if kind == "constant":
        return constant(H, W, cn, seed % 256)
    if kind == "periodic":
        return periodic(H, W, cn, _PERIODS[seed % len(_PERIODS)], (seed // len(_PERIODS)) % 8)
    if kind == "row_constant":
        return row_constant(H, W, cn, seed)
    if kind == "quantised":
        return quantised(H, W, cn, seed, D)
    if kind == "flat_rects":
        return flat_rects(H, W, cn, seed, D)
    if kind == "textured":
        return textured(H, W, cn, seed, D)
    raise ValueError(kind)


# the tie table of tests/test_gpu_matcher_degenerate.py and tests/test_gpu_sgbm_paths_degenerate.py: "periodic4" and "periodic8" are
# periodic(4, 3) and periodic(8, 3)
TIE_KINDS = ["constant", "periodic4", "periodic8", "row_constant", "quantised", "flat_rects"]


def tie_pair(kind, H, W, cn):
    if kind == "constant":
        return constant(H, W, cn)
    if kind.startswith("periodic"):
        return periodic(H, W, cn, int(kind[8:]), 3)
    if kind == "row_constant":
        return row_constant(H, W, cn, seed=5)
    if kind == "quantised":
        return quantised(H, W, cn, seed=6, D=32)
    return flat_rects(H, W, cn, seed=7, D=32)


def noise(H, W, seed):
    """two unrelated uint8 noise images"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W)).astype(np.uint8), rng.integers(0, 256, (H, W)).astype(np.uint8)


# H, W, minD, D, block
SGBM_TINY_FRAMES = [
    (1, 17, 0, 16, 1), (1, 18, 0, 16, 3),                       # Wv = 1 and 2, one row
    (2, 80, 0, 16, 5),
    (3, 16 + 63, 0, 16, 7), (3, 16 + 64, 0, 16, 7), (3, 16 + 65, 0, 16, 7),   # Wv around one wavefront
    (4, 57, 7, 48, 3), (5, 81, 0, 80, 5),
]


def sgbm_tiny_settings(w):
    """(P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio): P1 = P2 = 0 with the uniqueness rule off; the binding's own defaults
    (all zero: the same penalties, uniqueness 0 in force); and the customary 8 w^2 / 32 w^2 with a left-right check and a prefilter
    cap, where the penalties and the later stages do work"""
    return ((0, 0, 0, 0, -1), (0, 0, 0, 0, 0), (8 * w * w, 32 * w * w, 1, 10, 0))


# Turning a pair upside down turns the result of SGBM over a path mask upside down when the mask is turned with it
# (sgbm_paths_ref.vflip): tests/test_sgbm_paths_cpu.py shows it on the restatement, tests/test_gpu_sgbm_paths_degenerate.py on the GPU
PATHS_FLIP_KINDS = ["textured", "flat_rects", "quantised"]
PATHS_FLIP_MASKS = [0x0F, 0x17, 0x27, 0x47, 0x87, 0x37, 0xFF]   # bottom->top, each diagonal alone, five paths, all eight


def paths_flip_pair(kind, cn):
    return make_input(kind, 23, 90, cn, seed=11, D=32)


def paths_flip_args(cn):
    """minD, D, block, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio, speckleWindowSize, speckleRange"""
    return (1, 32, 5, 8 * cn * 25, 32 * cn * 25, 1, 10, 10, 20, 2)


def padded_view(img, pad, fill):
    """the same pixels as a view into rows that are `pad` pixels longer (step > cols * channels); the padding holds `fill`"""
    if pad <= 0:
        return img
    shape = list(img.shape)
    shape[1] += pad
    wide = np.full(shape, fill, img.dtype)
    wide[:, :img.shape[1]] = img
    return wide[:, :img.shape[1]]


def tie_share(volume, axis):
    """Of the pixels whose costs are all finite: the share whose minimum over the candidate axis is reached by at least two
    candidates (0.0 when there is no such pixel)."""
    v = np.moveaxis(np.asarray(volume), axis, -1)
    v = v[np.isfinite(v).all(axis=-1)]
    if v.shape[0] == 0:
        return 0.0
    return float(((v == v.min(axis=-1, keepdims=True)).sum(axis=-1) >= 2).mean())


# ---------------------------------------------------------------- seeded cases
def _pick(rng, values):
    return values[int(rng.integers(0, len(values)))]


def _matcher_draws(rng, family, index):
    kind = KINDS[(int(rng.integers(0, len(KINDS))) if index is None else index) % len(KINDS)]
    w = 2 * int(rng.integers(0, 11)) + 1 if family == "sgbm" else 2 * int(rng.integers(2, 11)) + 1
    lo = 1 if family == "sgbm" else w
    H, W = int(rng.integers(lo, 41)), int(rng.integers(lo, 221))
    D = _pick(rng, (16, 32, 48, 64, 80, 128))
    minD = _pick(rng, (0, 1, 5, 17))
    pad = int(rng.integers(1, 9)) if rng.random() < 1.0 / 7 else 0
    seed = int(rng.integers(0, 1 << 30))
    return kind, H, W, minD, D, w, pad, seed


def _sgbm_tag(rng, kind, H, W, minD, D, w, pad, seed):
    cn = _pick(rng, (1, 3))
    pens = (0, 8 * cn * w * w, 32 * cn * w * w, 10, 100, 600, 2400)
    return (kind, H, W, cn, minD, D, w, _pick(rng, pens), _pick(rng, pens), _pick(rng, (-1, 0, 1, 3, 200)),
            _pick(rng, (0, 1, 10, 31, 63)), _pick(rng, (-1, 0, 5, 10, 50)), _pick(rng, (0, 10, 100)), _pick(rng, (0, 1, 2, 32)),
            pad, seed)


def random_case(rng, family, index=None):
    """One case of `family`, drawn from `rng`.  The input kind cycles with `index` over KINDS (drawn when index is None)."""
    if family == "sgbm":
        tag = _sgbm_tag(rng, *_matcher_draws(rng, family, index))
    elif family == "sgbm_paths":
        # the sgbm tag followed by a mask that contains the three paths.  The added directions work on the valid columns
        # [minD + D, W) only, so nine cases in ten get 1..120 of them whatever minD and D are; the tenth keeps any width from 1 up
        # (W <= minD + D included: the all-INVALID answer)
        kind = KINDS[(int(rng.integers(0, len(KINDS))) if index is None else index) % len(KINDS)]
        w = 2 * int(rng.integers(0, 11)) + 1
        H = int(rng.integers(1, 41))
        D = _pick(rng, (16, 32, 48, 64, 80, 128))
        minD = _pick(rng, (0, 1, 5, 17))
        Wv, anyW = int(rng.integers(1, 121)), int(rng.integers(1, 221))
        W = minD + D + Wv if rng.random() < 0.9 else anyW
        pad = int(rng.integers(1, 9)) if rng.random() < 1.0 / 7 else 0
        tag = _sgbm_tag(rng, kind, H, W, minD, D, w, pad, int(rng.integers(0, 1 << 30)))
        tag += (0x07 | (int(rng.integers(0, 32)) << 3),)
    elif family == "bm":
        kind, H, W, minD, D, w, pad, seed = _matcher_draws(rng, family, index)
        tag = (kind, H, W, minD, D, w, _pick(rng, (1, 5, 31, 63)), _pick(rng, (0, 10, 500)), _pick(rng, (0, 15, 100)),
               _pick(rng, (-1, 0, 1, 200)), _pick(rng, (0, 10, 100)), _pick(rng, (0, 1, 2, 32)), pad, seed)
    elif family == "speckles":
        tag = (int(rng.integers(1, 61)), int(rng.integers(1, 301)), int(rng.integers(0, 1 << 30)), _pick(rng, (-16, -16, 0, -1000)),
               _pick(rng, (0, 1, 20, 400)), _pick(rng, (0, 1, 16, 48)))
    elif family == "refine":
        H, W = int(rng.integers(1, 41)), int(rng.integers(1, 141))
        dead = tuple(sorted({int(rng.integers(0, H)) for _ in range(int(rng.integers(0, 3)))}))
        tag = (H, W, _pick(rng, (1, 3)), _pick(rng, (1, 3, 15, 35)), _pick(rng, (1, 2, 5, 17, 40, 64)), _pick(rng, (0, 2, 7)), dead,
               _pick(rng, (0.0, 1.0, 2.5)), _pick(rng, (60.0, 80.0, 150.0)), _pick(rng, (3.0, 6.0, 9.0, 20.0)),
               int(rng.integers(0, 1 << 30)))
    elif family == "subpixel":
        method = _pick(rng, tuple(SUBPIXEL_METHODS))
        kind = KINDS[(int(rng.integers(0, len(KINDS))) if index is None else index) % len(KINDS)]
        dt = int(rng.integers(0, 2)) if SUBPIXEL_METHODS[method][1] else 0
        tag = (method, kind, int(rng.integers(1, 31)), int(rng.integers(1, 121)), dt, _pick(rng, (3, 5, 7, 9, 11, 15)),
               0 if method == "BLO1" else _pick(rng, (0, 1, 3)), int(rng.integers(1, 25)), _pick(rng, subpixel_ref.MODES),
               int(rng.integers(0, 1 << 30)))
    else:
        raise ValueError(family)
    return build_case(family, tag)


def cases(family, seed, count=None):
    """the `count` cases of (family, seed), input kinds in rotation"""
    rng = np.random.default_rng(seed)
    return [random_case(rng, family, i) for i in range(SWEEP_COUNTS[family] if count is None else count)]


def _piecewise(H, W, seed, holes=0.1, block=6, levels=5, step=16):
    rng = np.random.default_rng(seed)
    by, bx = (H + block - 1) // block, (W + block - 1) // block
    base = rng.integers(0, levels, size=(by, bx)) * step * 3
    m = np.repeat(np.repeat(base, block, 0), block, 1)[:H, :W]
    m = m + rng.integers(-step, step + 1, size=(H, W)) * (rng.random((H, W)) < 0.3)
    m[rng.random((H, W)) < holes] = -16
    return m.astype(np.int16)


def _refine_maps(rng, H, W, cn, n, minD, dead_rows, p_reject=0.3):
    """random integer maps with random rejections (tests/test_gpu_refine.py), under a guide of four grey levels"""
    G = (rng.integers(0, 256, _shape(H, W, cn)) // 64 * 64).astype(np.uint8)
    levels = min(n, 40)
    stride = (n - 1) // (levels - 1) if levels > 1 else 1
    far = rng.integers(0, levels, (H, W)) * stride
    near = rng.integers(0, max(1, min(n, W // 3)), (H, W))
    dl = (minD + np.where(rng.random((H, W)) < (0.8 if n > W // 2 else 0.0), near, far)).astype(np.float32)
    xr = np.arange(W)[None, :] - dl.astype(np.int64)
    dr = np.full((H, W), -9.0, np.float32)
    ys, xs = np.nonzero((xr >= 0) & (xr < W))
    dr[ys, xr[ys, xs]] = dl[ys, xs]
    kill = rng.random((H, W)) < p_reject
    dr[kill] = np.where(rng.random(int(kill.sum())) < 0.5, np.float32(np.nan), np.float32(-5.0))
    for y in dead_rows:
        dr[y] = np.nan
    return G, dl, dr


def build_case(family, tag):
    """the case of `tag`: dict(family, tag, inputs and parameters)"""
    c = {"family": family, "tag": tuple(tag)}
    if family == "sgbm":
        kind, H, W, cn, minD, D, w, P1, P2, m12, cap, U, sw, sr, pad, seed = tag
        L, R = make_input(kind, H, W, cn, seed, D)
        c.update(L=padded_view(L, pad, 0), R=padded_view(R, pad, 255), args=(minD, D, w, P1, P2, m12, cap, U, sw, sr))
    elif family == "sgbm_paths":
        c.update(build_case("sgbm", tag[:-1]), family=family, tag=tuple(tag), paths=tag[-1])
    elif family == "bm":
        kind, H, W, minD, D, w, cap, tex, U, m12, sw, sr, pad, seed = tag
        L, R = make_input(kind, H, W, 1, seed, D)
        c.update(L=padded_view(L, pad, 0), R=padded_view(R, pad, 255), args=(minD, D, w, cap, tex, U, sw, sr, m12))
    elif family == "speckles":
        H, W, seed, new_val, size, diff = tag
        c.update(map=_piecewise(H, W, seed), args=(new_val, size, diff))
    elif family == "refine":
        H, W, cn, win, n, minD, dead, max_diff, gc, gs, seed = tag
        G, dl, dr = _refine_maps(np.random.default_rng(seed), H, W, cn, n, minD, dead)
        c.update(G=G, dl=dl, dr=dr, args=(minD, n, max_diff, win, gc, gs))
    elif family == "subpixel":
        method, kind, H, W, dt, win, minD, numD, mode, seed = tag
        L, R = make_input(kind, H, W, 3, seed, numD)
        c.update(L=L, R=R, alg=SUBPIXEL_METHODS[method][0], dt=dt, win=win, minD=minD, numD=numD, mode=mode)
    else:
        raise ValueError(family)
    return c


# ---------------------------------------------------------------- both sides of a case, in one layout
def reference(case):
    """the restatement's answer: a dict of arrays / counts (family `subpixel` has none of its own: see gpu_result)"""
    f = case["family"]
    if f == "sgbm":
        want = sgbm_ref.sgbm(case["L"], case["R"], *case["args"])
        return {"disp": want["disp"], "vol": np.moveaxis(want["S"], 2, 0).astype(np.float32)}
    if f == "sgbm_paths":
        want = sgbm_paths_ref.sgbm_paths(case["L"], case["R"], *case["args"], case["paths"])
        return {"disp": want["disp"], "vol": np.moveaxis(want["S"], 2, 0).astype(np.float32)}
    if f == "bm":
        minD, D, w, cap, tex, U, sw, sr, m12 = case["args"]
        want = stereobm_ref.stereo_bm(case["L"], case["R"], minD, D, w, cap, tex, U, sw, sr, m12)
        return {"disp": want["disp"], "vol": want["vol"]}
    if f == "speckles":
        return {"map": sgbm_ref.filter_speckles(case["map"], *case["args"])}
    if f == "refine":
        minD, n, max_diff, win, gc, gs = case["args"]
        want = refine_ref.refine_vec(case["G"], case["dl"], case["dr"], minD, n, max_diff, win, gc, gs)
        return {"out": want["out"], "mask": want["mask"], "counts": np.array([want["n_rejected"], want["n_unfillable"]])}
    raise ValueError(f)


def gpu_result(ctx, case):
    """-> (got, want): the library's answer and what it is compared with, as dicts of arrays with the same keys.  For `subpixel`
    `want` is the restatement applied to the call's own unflagged map and volume, and the flagged call's volume must be that
    volume."""
    f = case["family"]
    if f == "sgbm":
        disp, vol = ctx.sgbm(case["L"], case["R"], *case["args"], return_cost_volume=True)
        return {"disp": disp, "vol": vol}, reference(case)
    if f == "sgbm_paths":
        disp, vol = ctx.sgbm_paths(case["L"], case["R"], *case["args"], paths=case["paths"], return_cost_volume=True)
        return {"disp": disp, "vol": vol}, reference(case)
    if f == "bm":
        minD, D, w, cap, tex, U, sw, sr, m12 = case["args"]
        disp, vol = ctx.stereoBM(case["L"], case["R"], minD, D, w, 1, 9, cap, tex, U, sw, sr, m12, return_cost_volume=True)
        return {"disp": disp, "vol": vol}, reference(case)
    if f == "speckles":
        return {"map": ctx.filterSpeckles(case["map"], *case["args"])}, reference(case)
    if f == "refine":
        minD, n, max_diff, win, gc, gs = case["args"]
        out, nrej, nunf, mask = ctx.refineDisparity(case["G"], case["dl"], case["dr"], minD, n, max_diff, win, gc, gs, return_mask=True)
        return {"out": out, "mask": mask, "counts": np.array([nrej, nunf])}, reference(case)
    if f == "subpixel":
        a = (case["L"], case["R"], case["dt"], case["alg"], case["win"], case["minD"], case["numD"])
        d0, v0 = ctx.stereoMatching(*a, return_cost_volume=True)
        d1, v1 = ctx.stereoMatching(*a, return_cost_volume=True, subpixel=case["mode"])
        want, _ = subpixel_ref.subpixel_vec(d0, v0, case["minD"], case["mode"])
        return {"disp": d1, "vol": v1.view(np.uint32)}, {"disp": want, "vol": v0.view(np.uint32)}
    raise ValueError(f)


def same(got, want):
    """exact equality of every array (NaN equal to NaN: BM's volume)"""
    return all(np.array_equal(got[k], want[k], equal_nan=np.issubdtype(np.asarray(want[k]).dtype, np.floating)) for k in want)
