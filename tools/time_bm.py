"""Per-call times (HIP events of the library, asw_get_timing) of block matching at the two shapes of DESIGN.md section 4.9:
getDisparity_BM at 640x360 D=64 win 15 (the reference driver's shape) and at 1920x1080 D=128 win 15, 3-channel input.
total_ms covers the gray conversion, every kernel and the u8 conversion (not the host copies); match_ms is k_bm_match alone.
Per-kernel times: rocprofv3 --kernel-trace --stats -f csv -- python tools/time_bm.py (profiles/bm_kernel_stats.csv)

    python tools/time_bm.py [--reps N]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aswstereomatch_amd as asw  # noqa: E402
from aswstereomatch_amd.synth import make_pair  # noqa: E402

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
ctx = asw.Context(0)
for H, W, D in ((360, 640, 64), (1080, 1920, 128)):
    L, R, _ = make_pair(H, W, D // 2, seed=H, block=16)
    ts = []
    for i in range(reps + 1):
        ctx.getDisparity_BM(L, R, 15, 0, D)
        ts.append(ctx.timing())
    ts = ts[1:]
    best = min(ts, key=lambda t: t["total_ms"])
    med = sorted(t["total_ms"] for t in ts)[len(ts) // 2]
    print("getDisparity_BM %dx%dx3 D=%d win=15: total %.3f ms (median %.3f)  match %.3f ms  (best of %d)"
          % (W, H, D, best["total_ms"], med, best["aggregate_ms"], reps), flush=True)
ctx.close()
