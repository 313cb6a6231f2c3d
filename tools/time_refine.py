"""What the left-right refinement costs, host clock around calls that end in a synchronise, 1920x1080 D=128:

  A  asw_match_refined_resident (both directions + cross-check + fill + weighted median, everything stays in HBM)
  B  two plain asw_match_resident calls (LEFT, RIGHT)
  C  what a caller did before for the cross-check alone: B + two asw_download_disparity + asw_lr_check on the host maps

A - B is the refinement's cost, C - B the earlier cost of a lesser result.  With --other-lib PATH the same B is also timed on
another build of the library (the parent commit's) in the same process, alternating with this one, to show that the plain path
did not move.  The forms run in a freshly shuffled (seeded) order every repetition, so no form owes its number to what ran before it.
One JSON line per configuration.

    python tools/time_refine.py [--reps 50] [--warmup 4] [--other-lib PATH] [--out FILE] [--only-refined]

--only-refined runs A alone (for a rocprofv3 --kernel-trace --stats run of its own)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aswstereomatch_amd as asw  # noqa: E402
from aswstereomatch_amd import _lib  # noqa: E402
from aswstereomatch_amd.synth import make_pair  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, warmup, other, out_path = arg("--reps", 50), arg("--warmup", 4), arg("--other-lib", ""), arg("--out", "")
H, W, D = 1080, 1920, 128
L, R, _ = make_pair(H, W, D, seed=1234, block=48)
ctx = asw.Context(0)
ctx.upload_pair(0, L, R)


class Other:
    """asw_upload_pair / asw_match_resident of another build of the library, through ctypes alone."""

    def __init__(self, path):
        self.l = C.CDLL(path)
        self.l.asw_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        self.l.asw_upload_pair.argtypes = [C.c_void_p, C.c_int, C.POINTER(_lib.AswImage), C.POINTER(_lib.AswImage)]
        self.l.asw_match_resident.argtypes = [C.c_void_p] + [C.c_int] * 7
        self.l.asw_destroy.argtypes = [C.c_void_p]
        self.l.asw_destroy.restype = None
        self.h = C.c_void_p()
        assert self.l.asw_create(0, C.byref(self.h)) == 0
        li, la = asw._image(L)
        ri, ra = asw._image(R)
        assert self.l.asw_upload_pair(self.h, 0, C.byref(li), C.byref(ri)) == 0

    def match(self, dt, alg):
        assert self.l.asw_match_resident(self.h, 0, dt, alg, 15, 0, D, 0) == 0


oth = Other(other) if other else None


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    v = np.sort(np.asarray(v))
    return {"median": round(float(np.median(v)), 4), "min": round(float(v[0]), 4), "p10": round(float(v[len(v) // 10]), 4),
            "p90": round(float(v[(len(v) * 9) // 10]), 4)}


lines = []
for name, alg, rwin in (("classic", 2, 15), ("classic", 2, 35), ("guided", 7, 15)):
    n = _lib.lib().asw_volume_planes(alg, D)

    def fa():
        return ctx.match_refined_resident(0, alg, 15, 0, D, 1.0, rwin, 150.0, 9.0)

    def fb():
        ctx.match_resident(0, 0, alg, 15, 0, D)
        ctx.match_resident(0, 1, alg, 15, 0, D)

    def fb_other():
        oth.match(0, alg)
        oth.match(1, alg)

    def fc():
        ctx.match_resident(0, 0, alg, 15, 0, D)
        dl = ctx.download_disparity(0, (H, W))
        ctx.match_resident(0, 1, alg, 15, 0, D)
        dr = ctx.download_disparity(0, (H, W))
        ctx.leftRightCheck(dl, dr, 1.0, -1.0)

    forms = {"A": fa} if "--only-refined" in sys.argv else {"B": fb, "A": fa, "C": fc}
    if oth and "B" in forms:
        forms["B_other"] = fb_other
    t = {k: [] for k in forms}
    refine_ms = []
    order = np.random.default_rng(7)
    for i in range(warmup + reps):
        for k in order.permutation(list(forms)):  # a fresh order every repetition: no form owes its number to its predecessor
            ms = clock(forms[k])
            if i >= warmup:
                t[k].append(ms)
            if k == "A" and i >= warmup:
                tm = ctx.timing()
                refine_ms.append(tm["total_ms"])
    nrej, nunf = fa()
    rec = {"config": "%s 1920x1080 D=%d win=15 refine_win=%d gamma 150/9" % (name, D, rwin), "algorithm": alg, "reps": reps,
           "warmup": warmup, "num_values": n, "rejected": nrej, "unfillable": nunf, "host_ms": {k: stats(v) for k, v in t.items()},
           "A_event_total_ms": stats(refine_ms)}
    if "B" in t:
        a, b, c = (np.median(t[k]) for k in ("A", "B", "C"))
        rec["A_minus_B_ms"] = round(float(a - b), 4)
        rec["C_minus_B_ms"] = round(float(c - b), 4)
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
ctx.close()
