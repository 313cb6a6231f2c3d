"""Restatement of the sub-pixel rule (include/asw_mi355x.h ASW_DISPARITY_SUBPIXEL_*) for the tests.

There is no reference implementation of this step; the rule is the library's own.  Every operation is one IEEE f64 operation
(numpy's and Python's floats are f64, their division is correctly rounded, nothing is fused), so both forms here and the kernel
must agree to the last bit (np.array_equal):

  subpixel_vec   on whole arrays;
  subpixel_loop  the literal per-pixel loop, for small crops.

Both take the integer winner-take-all map (f32, absolute disparities), the aggregated volume (f32 [n][H][W], plane k <-> disparity
minD + k) and return (sub-pixel map f32, refined mask bool).  slanted_plane_pair builds the pair of the value tests.
"""
import math

import numpy as np

PARABOLA, EQUIANGULAR = 0x100, 0x200
MODES = (PARABOLA, EQUIANGULAR)


def subpixel_vec(disp, vol, minD, mode):
    assert mode in MODES
    disp = np.ascontiguousarray(disp, np.float32)
    vol = np.ascontiguousarray(vol, np.float32)
    n = vol.shape[0]
    assert vol.shape[1:] == disp.shape
    with np.errstate(invalid="ignore"):
        inside = (disp > np.float32(minD)) & (disp < np.float32(minD + n - 1))  # 0 < k < n - 1; NaN compares false
    if not inside.any():
        return disp.copy(), inside
    k = np.where(inside, disp, np.float32(minD + 1)).astype(np.int64) - minD
    inside &= (k >= 1) & (k <= n - 2)
    k = np.clip(k, 1, max(1, n - 2))[None]
    c0 = np.take_along_axis(vol, k, 0)[0].astype(np.float64)
    cm = np.take_along_axis(vol, k - 1, 0)[0].astype(np.float64)
    cp = np.take_along_axis(vol, k + 1, 0)[0].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = inside & np.isfinite(c0) & np.isfinite(cm) & np.isfinite(cp)
        ok &= (cm >= c0) & (cp >= c0)
        den = (cm - c0) + (cp - c0) if mode == PARABOLA else np.maximum(cm, cp) - c0
        ok &= den > 0.0
        off = (cm - cp) / (2.0 * den)
        off = np.where(off < -0.5, -0.5, np.where(off > 0.5, 0.5, off))
        moved = (disp.astype(np.float64) + off).astype(np.float32)
    return np.where(ok, moved, disp), ok


def subpixel_loop(disp, vol, minD, mode):
    assert mode in MODES
    disp = np.asarray(disp, np.float32)
    vol = np.asarray(vol, np.float32)
    n, H, W = vol.shape
    out = disp.copy()
    ok = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            d = float(disp[y, x])
            if not (d > minD and d < minD + n - 1):
                continue
            k = int(d) - minD
            if k < 1 or k > n - 2:
                continue
            c0, cm, cp = float(vol[k, y, x]), float(vol[k - 1, y, x]), float(vol[k + 1, y, x])
            if not (math.isfinite(c0) and math.isfinite(cm) and math.isfinite(cp)):
                continue
            if not (cm >= c0 and cp >= c0):
                continue
            den = (cm - c0) + (cp - c0) if mode == PARABOLA else max(cm, cp) - c0
            if not den > 0.0:
                continue
            off = (cm - cp) / (2.0 * den)
            off = -0.5 if off < -0.5 else (0.5 if off > 0.5 else off)
            out[y, x] = np.float32(d + off)
            ok[y, x] = True
    return out, ok


def refined_share(disp, vol, minD, mode=PARABOLA):
    return float(subpixel_vec(disp, vol, minD, mode)[1].mean())


def slanted_plane_pair(H=72, W=240, seed=11, block=32):
    """Left image of make_pair(H, W, 16, seed, block); the right view of the plane d(x) = 3 + 6 x / W:
    R[:, x'] = round(lerp(L, (x' + 3) / (1 - 6 / W))), columns clamped.  -> (L, R, ground truth of the left view, f64 [H][W])."""
    from aswstereomatch_amd.synth import make_pair

    L, _, _ = make_pair(H, W, 16, seed=seed, block=block)
    xs = (np.arange(W, dtype=np.float64) + 3.0) / (1.0 - 6.0 / W)
    x0 = np.floor(xs)
    t = (xs - x0)[None, :, None]
    a = np.clip(x0.astype(np.int64), 0, W - 1)
    b = np.clip(x0.astype(np.int64) + 1, 0, W - 1)
    Lf = L.astype(np.float64)
    R = np.rint(Lf[:, a] * (1.0 - t) + Lf[:, b] * t).astype(np.uint8)
    gt = np.broadcast_to(3.0 + 6.0 * np.arange(W, dtype=np.float64) / W, (H, W)).copy()
    return L, np.ascontiguousarray(R), gt


def cropped_mae(disp, gt):
    H, W = gt.shape
    return float(np.abs(disp.astype(np.float64) - gt)[10:H - 10, 30:W - 30].mean())
