"""Per-call times (HIP events of the library, asw_get_timing) of asw_sgbm_paths at the two shapes of DESIGN.md sections 4.8 / 4.8b,
1920x1080x3 D=128 block 15 and 1242x375x3 D=64 block 5 (the frames and settings of tools/time_sgbm.py), for the masks 0x07, 0x0F,
0x37 and 0xFF, with asw_sgbm next to the 0x07 call.  Best of N by total time; the maps of 0x07 and asw_sgbm are compared.
Per-kernel times: rocprofv3 --kernel-trace --stats -f csv -- python tools/time_sgbm_paths.py (profiles/sgbm_paths_kernel_stats.csv)

    python tools/time_sgbm_paths.py [--reps N]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aswstereomatch_amd as asw  # noqa: E402
from aswstereomatch_amd.synth import make_pair  # noqa: E402

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
ctx = asw.Context(0)


def best_of(call):
    ts = []
    for i in range(reps + 1):  # the first call warms up
        out = call()
        ts.append(ctx.timing())
    return out, min(ts[1:], key=lambda t: t["total_ms"])


# (label, frame, maxDisp of the synthetic pair, seed, numDisparities, blockSize, the other StereoSGBM settings)
SHAPES = [
    ("1920x1080x3 D=128 block=15", (1080, 1920), 64, 1, 128, 15, (8 * 3 * 225, 32 * 3 * 225, 200, 10, 10, 175, 32)),
    ("1242x375x3 D=64 block=5", (375, 1242), 32, 2, 64, 5, (8 * 3 * 25, 32 * 3 * 25, 1, 15, 10, 100, 2)),
]
for label, (H, W), maxd, seed, D, w, rest in SHAPES:
    L, R, _ = make_pair(H, W, maxd, seed=seed)
    ref_map, t = best_of(lambda: ctx.sgbm(L, R, 0, D, w, *rest))
    print("%s  asw_sgbm          : total %.3f ms  paths %.3f ms  launches %d" % (label, t["total_ms"], t["aggregate_ms"],
                                                                              t["aggregate_launches"]), flush=True)
    base = None
    for paths in (asw.SGBM_PATHS_3WAY, asw.SGBM_PATHS_HH4, asw.SGBM_PATHS_SGBM, asw.SGBM_PATHS_HH):
        disp, t = best_of(lambda: ctx.sgbm_paths(L, R, 0, D, w, *rest, paths=paths))
        base = base or t
        note = ""
        if paths == asw.SGBM_PATHS_3WAY:
            note = "  map == asw_sgbm: %s" % np.array_equal(disp, ref_map)
        print("%s  asw_sgbm_paths 0x%02X: total %.3f ms  paths %.3f ms  launches %d  paths / 3-way %.2f%s" % (
            label, paths, t["total_ms"], t["aggregate_ms"], t["aggregate_launches"], t["aggregate_ms"] / base["aggregate_ms"], note),
            flush=True)
ctx.close()
