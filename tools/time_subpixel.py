"""What the sub-pixel flag costs, library event times (asw_get_timing total_ms) of asw_match_resident,
1920x1080 D=128 win=15, for the bilateral, GuidedF_2 and geodesic methods:

  K  unflagged, keep_volume=1   the baseline: it writes the same bytes as a flagged call
  N  unflagged, keep_volume=0   what the selector call costs today (bilateral / geodesic skip the volume write)
  P  flagged (parabola), keep_volume=0
  E  flagged (equiangular), keep_volume=0

P - K (E - K) is the gather kernel, P - N the price of the flag over today's call.  With --other-lib PATH the K form is also timed
on another build of the library (the parent commit's) in the same process, to show that the unflagged path did not move.  The forms
run in a freshly shuffled (seeded) order every repetition.  One JSON line per method.

    python tools/time_subpixel.py [--reps 30] [--warmup 3] [--other-lib PATH] [--out FILE] [--only-flagged]

--only-flagged runs P alone and, before it, one unflagged keep_volume=1 match whose volume goes through asw_wta's kernel path
(for a rocprofv3 --kernel-trace --stats run of its own: k_subpixel beside the methods' kernels)."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aswstereomatch_amd as asw  # noqa: E402
from aswstereomatch_amd import _lib  # noqa: E402
from aswstereomatch_amd.synth import make_pair  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, warmup, other, out_path = arg("--reps", 30), arg("--warmup", 3), arg("--other-lib", ""), arg("--out", "")
H, W, D = 1080, 1920, 128
L, R, _ = make_pair(H, W, D, seed=1234, block=48)
ctx = asw.Context(0)
ctx.upload_pair(0, L, R)


class Other:
    """asw_upload_pair / asw_match_resident / asw_get_timing of another build of the library, through ctypes alone."""

    def __init__(self, path):
        self.l = C.CDLL(path)
        self.l.asw_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        self.l.asw_upload_pair.argtypes = [C.c_void_p, C.c_int, C.POINTER(_lib.AswImage), C.POINTER(_lib.AswImage)]
        self.l.asw_match_resident.argtypes = [C.c_void_p] + [C.c_int] * 7
        self.l.asw_get_timing.argtypes = [C.c_void_p, C.POINTER(_lib.AswTiming)]
        self.l.asw_destroy.argtypes = [C.c_void_p]
        self.l.asw_destroy.restype = None
        self.h = C.c_void_p()
        assert self.l.asw_create(0, C.byref(self.h)) == 0
        li, la = asw._image(L)
        ri, ra = asw._image(R)
        assert self.l.asw_upload_pair(self.h, 0, C.byref(li), C.byref(ri)) == 0

    def match(self, alg, keep):
        assert self.l.asw_match_resident(self.h, 0, 0, alg, 15, 0, D, keep) == 0
        t = _lib.AswTiming()
        self.l.asw_get_timing(self.h, C.byref(t))
        return t.total_ms


oth = Other(other) if other else None


def stats(v):
    v = np.sort(np.asarray(v))
    return {"median": round(float(np.median(v)), 4), "min": round(float(v[0]), 4), "p10": round(float(v[len(v) // 10]), 4),
            "p90": round(float(v[(len(v) * 9) // 10]), 4)}


def match(alg, keep, subpixel=None):
    ctx.match_resident(0, asw.DISPARITY_LEFT, alg, 15, 0, D, keep_volume=keep, subpixel=subpixel)
    return ctx.timing()["total_ms"]


lines = []
for name, alg in (("bilateral", 2), ("guided2", 8), ("geodesic", 4)):
    if "--only-flagged" in sys.argv:
        forms = {"P": lambda: match(alg, False, asw.SUBPIXEL_PARABOLA)}
        match(alg, True)
        ctx.winnerTakeAll(ctx.download_volume(0, (_lib.lib().asw_volume_planes(alg, D), H, W)))  # k_wta over the same volume
    else:
        forms = {"K": lambda: match(alg, True), "N": lambda: match(alg, False), "P": lambda: match(alg, False, asw.SUBPIXEL_PARABOLA),
                 "E": lambda: match(alg, False, asw.SUBPIXEL_EQUIANGULAR)}
        if oth:
            forms["K_other"] = lambda: oth.match(alg, 1)
            forms["N_other"] = lambda: oth.match(alg, 0)
    t = {k: [] for k in forms}
    order = np.random.default_rng(7)
    for i in range(warmup + reps):
        for k in order.permutation(list(forms)):
            ms = forms[k]()
            if i >= warmup:
                t[k].append(ms)
    rec = {"config": "%s 1920x1080 D=%d win=15 LEFT" % (name, D), "algorithm": alg, "reps": reps, "warmup": warmup,
           "event_total_ms": {k: stats(v) for k, v in t.items()}}
    if "K" in t:
        med = {k: float(np.median(v)) for k, v in t.items()}
        rec["P_minus_K_ms"] = round(med["P"] - med["K"], 4)
        rec["E_minus_K_ms"] = round(med["E"] - med["K"], 4)
        rec["K_minus_N_ms"] = round(med["K"] - med["N"], 4)
        rec["P_minus_N_ms"] = round(med["P"] - med["N"], 4)
        rec["P_over_K"] = round(med["P"] / med["K"], 4)
        rec["P_over_N"] = round(med["P"] / med["N"], 4)
        if "K_other" in med:
            rec["K_over_K_other"] = round(med["K"] / med["K_other"], 4)
            rec["N_over_N_other"] = round(med["N"] / med["N_other"], 4)
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
ctx.close()
