"""Per-call times (HIP events of the library, asw_get_timing) of asw_sgbm_census next to asw_sgbm_paths of the same build, at the two
shapes of DESIGN.md sections 4.8 / 4.8b / 4.8c, 1920x1080x3 D=128 block 15 and 1242x375x3 D=64 block 5 (the frames of
tools/time_sgbm_paths.py), for the masks 0x07 and 0xFF.  Best of N by total time.  Per call: total, aggregate_ms (the path
kernels), and the cost stage = total - aggregate of the same call with the speckle filter off: what runs in front of the path
kernels (BT: prefilter + hcost; census: gray pair + two census transforms + hcost_census), plus the left-right rule and the median,
two plane-sized kernels that are the same in both.  The census penalties are those of one plane (8 w^2, 32 w^2).
Per-kernel times: rocprofv3 --kernel-trace --stats -f csv -- python tools/time_sgbm_census.py

    python tools/time_sgbm_census.py [--reps N]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aswstereomatch_amd as asw  # noqa: E402
from aswstereomatch_amd.synth import make_pair  # noqa: E402

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
ctx = asw.Context(0)


def best_of(call):
    ts = []
    for i in range(reps + 1):  # the first call warms up
        call()
        ts.append(ctx.timing())
    return min(ts[1:], key=lambda t: t["total_ms"])


# (label, frame, maxDisp of the synthetic pair, seed, numDisparities, blockSize, disp12MaxDiff, uniqueness, speckle window / range)
SHAPES = [
    ("1920x1080x3 D=128 block=15", (1080, 1920), 64, 1, 128, 15, 200, 10, 175, 32),
    ("1242x375x3 D=64 block=5", (375, 1242), 32, 2, 64, 5, 1, 10, 100, 2),
]
for label, (H, W), maxd, seed, D, w, m12, U, sw, sr in SHAPES:
    L, R, _ = make_pair(H, W, maxd, seed=seed)
    for paths in (asw.SGBM_PATHS_3WAY, asw.SGBM_PATHS_HH):
        calls = {
            "asw_sgbm_paths ": lambda s: ctx.sgbm_paths(L, R, 0, D, w, 8 * 3 * w * w, 32 * 3 * w * w, m12, 10, U, s, sr, paths=paths),
            "asw_sgbm_census": lambda s: ctx.sgbm_census(L, R, 0, D, w, 8 * w * w, 32 * w * w, m12, U, s, sr, paths=paths),
        }
        for name, call in calls.items():
            t = best_of(lambda: call(sw))
            t0 = best_of(lambda: call(0))
            print("%s  %s 0x%02X: total %.3f ms  paths %.3f ms  launches %d  cost stage %.3f ms" % (
                label, name, paths, t["total_ms"], t["aggregate_ms"], t["aggregate_launches"], t0["total_ms"] - t0["aggregate_ms"]),
                flush=True)
ctx.close()
