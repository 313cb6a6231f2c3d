"""Per-call kernel times (HIP events of the library, asw_get_timing) of semi-global block matching at the two shapes of
DESIGN.md section 4.8: the selector's SGBM at 1920x1080 D=128 win 15 (3 channels) and asw_sgbm at KITTI 1242x375 D=64 block 5.
Per-kernel times: rocprofv3 --kernel-trace --stats -f csv -- python tools/time_sgbm.py (profiles/sgbm_kernel_stats.csv)

    python tools/time_sgbm.py [--reps N]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aswstereomatch_amd as asw  # noqa: E402
from aswstereomatch_amd.synth import make_pair  # noqa: E402

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
ctx = asw.Context(0)

L, R, _ = make_pair(1080, 1920, 64, seed=1)
ctx.upload_pair(0, L, R)
ts = []
for i in range(reps + 1):
    ctx.match_resident(0, asw.DISPARITY_LEFT, asw.StereoMatchingAlgorithms.SGBM, 15, 0, 128)
    ts.append(ctx.timing())
best = min(ts[1:], key=lambda t: t["total_ms"])
print("selector SGBM 1920x1080x3 D=128 win=15: total %.3f ms  paths %.3f ms  (best of %d)" % (best["total_ms"], best["aggregate_ms"], reps),
      flush=True)

L, R, _ = make_pair(375, 1242, 32, seed=2)
ts = []
for i in range(reps + 1):
    ctx.sgbm(L, R, 0, 64, 5, 8 * 3 * 25, 32 * 3 * 25, 1, 15, 10, 100, 2, return_cost_volume=(i == 0))
    ts.append(ctx.timing())
best = min(ts[1:], key=lambda t: t["total_ms"])
print("asw_sgbm 1242x375x3 D=64 block=5: total %.3f ms  paths %.3f ms  (best of %d, no volume)" % (best["total_ms"], best["aggregate_ms"], reps),
      flush=True)
ctx.close()
