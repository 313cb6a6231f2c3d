#!/usr/bin/env python3
"""Benchmark of the hot path: disparity Mpix/s on synthetic 1920x1080 pairs, D=128 (BASELINE.json).

    python bench.py --gpus N --steps K --warmup W [--workload bilateral|guided2|guided|geodesic|wmedian]
                    [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times K steps, writes its outputs if --dump-outputs is given and prints the line.  The
secondary legs (the batch API, the PCIe-inclusive one-call rate, the CPU baseline) run only under --full.

A "step" is one pass of the hot path over one batch of `--frames` stereo pairs that are already
resident in HBM (uploaded before the timed region).  One process per GPU; frames are independent,
so ranks never exchange data: torch.distributed is used only for the barrier around the
timed region and the MAX over ranks of the elapsed time.  Rank 0 prints ONE JSON line.

N > 1: under `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...` every process is one
rank (RANK / LOCAL_RANK / WORLD_SIZE from the environment); a bare `python bench.py --gpus N` starts the N
ranks itself as child processes (launch_ranks: the parent never touches the GPU).  Either way WORLD_SIZE
must equal --gpus and every rank must find its own GPU, or the run fails loudly.  After the timed region the
ranks leave the process group; under --full rank 0 alone then drives all N devices from one process through the
library's own batch API (`asw_stereo_match_batch`, 64 frames, host buffers in and out) and reports it as `batch_api`.

--dump-outputs DIR: after the timed region every rank writes what the last timed step left for a caller of the resident
path, as float32 .npy files: `disparity` (every frame's disparity map, frames x H x W) and `cost_volume_last_frame` (the
kept cost volume of the last frame, planes x H x W).  An array larger than its share of DUMP_BYTES is replaced by a fixed,
seeded sample of its flattened values (sorted indices, numpy default_rng(DUMP_SEED)), so that two builds run with the same
arguments can be compared value for value.  With N > 1 ranks the names carry a `_rank<r>` suffix.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: 8.0 TB/s spec
F64_PEAK_TFLOPS = 78.6      # vector f64
DUMP_BYTES = 60 * 10**6     # --dump-outputs: all files of all ranks together (64 MB at most, headers included)
DUMP_SEED = 20261016        # --dump-outputs: the sample of an array too large to write whole

WORKLOADS = {
    # name: (algorithm enum, candidates(numD), label)
    "bilateral": (2, lambda n: n + 1, "classic bilateral ASW (computeAdaptiveWeight)"),
    "direct8": (3, lambda n: n + 1, "direct8 ASW (row + column + diagonal support)"),
    "geodesic": (4, lambda n: n + 1, "geodesic ASW"),
    "bilgrid": (5, lambda n: n + 1, "bilateral-grid ASW (rates 10, 10)"),
    "blo1": (6, lambda n: n, "O(1)-bilateral ASW (BLO1)"),
    "guided": (7, lambda n: n, "guided-filter ASW (SAD cost, 6-ch guide)"),
    "guided2": (8, lambda n: n, "guided-filter ASW (TAD C+G cost)"),
    "guided3": (9, lambda n: n, "guided-filter ASW (NCC cost, 6-ch guide)"),
    "wmedian": (10, lambda n: n, "weighted-median ASW"),
    "ncc": (11, lambda n: n, "NCC matching (computeNCC -> disparity)"),
}


from aswstereomatch_amd.roofline import algorithmic_bytes  # noqa: E402  (shared with tools/pmc_traffic.py)


def cpu_baseline(args, L, R, gpu_disp, alg):
    """The oracle (CPU restatement of the reference method) timed on this host on a bounded sample."""
    from oracle import asw_oracle as O

    cores = O.usable_cores()
    O.set_threads(cores)
    H, W = L.shape[:2]
    D, win = args.disp, args.win
    if alg == 2:
        # rows of the very frame the GPU just processed (classic ASW is local: a row needs only its window)
        y0 = H // 4
        t = time.time()
        O.asw_classic(L, R, 30, 20, 0, win, 0, D, rows=(y0, y0 + cores))
        per_row = (time.time() - t) / cores
        rows = int(max(cores, min(H - y0, args.cpu_seconds / max(per_row, 1e-9))))
        rows = max(cores, rows // cores * cores)
        t = time.time()
        rc, d, _ = O.asw_classic(L, R, 30, 20, 0, win, 0, D, rows=(y0, y0 + rows))
        dt = time.time() - t
        ok = bool(np.array_equal(d[y0:y0 + rows], gpu_disp[y0:y0 + rows])) if gpu_disp is not None else None
        # the reference itself has no threading: the same code on ONE thread, on a few rows
        O.set_threads(1)
        r1 = max(1, min(16, int(2.0 / max(per_row, 1e-9))))
        t = time.time()
        O.asw_classic(L, R, 30, 20, 0, win, 0, D, rows=(y0, y0 + r1))
        dt1 = time.time() - t
        O.set_threads(cores)
        return {"single_thread": {"value": round(r1 * W / dt1 / 1e6, 5), "unit": "Mpix/s", "sample": "%d rows, %.1f s" % (r1, dt1)},
                "value": round(rows * W / dt / 1e6, 5), "unit": "Mpix/s", "cores": cores, "kind": "port",
                "sample": "rows %d..%d (%d of %d) of one %dx%d D=%d win=%d frame, oracle/asw_oracle.c "
                          "orc_asw_classic_rows, OpenMP %d threads, %.1f s" % (y0, y0 + rows, rows, H, W, H, D, win, cores, dt),
                "gpu_rows_match_oracle": ok}
    # the other methods are not row-local (per-slice normalisation, whole-frame tables): time a smaller frame
    from aswstereomatch_amd.synth import make_pair

    fn = {3: lambda a, b: O.asw_direct8(a, b, 0, win, 0, D), 5: lambda a, b: O.asw_bilgrid(a, b, 0, 10, 10, 0, D), 9: lambda a, b: O.asw_guided3(a, b, 0, 1e-6, win, 0, D),
          11: lambda a, b: O.ncc_disparity(a, b, 0, win, 0, D),
          4: lambda a, b: O.asw_geodesic(a, b, 0, win, 0, D), 6: lambda a, b: O.asw_blo1(a, b, 0, 0.015, win, 0, D), 7: lambda a, b: O.asw_guided(a, b, 0, 1e-6, win, 0, D),
          8: lambda a, b: O.asw_guided2(a, b, 0, 1e-6, win, 0, D), 10: lambda a, b: O.asw_wmedian(a, b, 0, win, 10, 10, 0, D)}[alg]
    sw, sh = {3: (1280, 720), 5: (640, 360), 9: (640, 360), 11: (640, 360), 4: (1242, 375), 6: (480, 270), 7: (1280, 720), 8: (1920, 1080), 10: (621, 188)}[alg]  # sized for ~3-10 s on 16 cores
    sw, sh = min(sw, W), min(sh, H)
    Ls, Rs, _ = make_pair(sh, sw, min(D, sw // 2), seed=4321)
    t = time.time()
    reps = 0
    while True:  # whole frames until about cpu_seconds of CPU work have been timed
        rc = fn(Ls, Rs)[0]
        reps += 1
        dt = time.time() - t
        if dt >= 0.7 * args.cpu_seconds or reps >= 64:
            break
    return {"value": round(reps * sw * sh / dt / 1e6, 5), "unit": "Mpix/s", "cores": cores, "kind": "port",
            "sample": "%d x one %dx%d D=%d win=%d synthetic frame (full method, rc=%d), oracle/asw_oracle.c, OpenMP %d threads, %.1f s"
                      % (reps, sw, sh, D, win, rc, cores, dt)}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="bilateral", choices=sorted(WORKLOADS))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--disp", type=int, default=128)
    ap.add_argument("--win", type=int, default=15)
    ap.add_argument("--frames", type=int, default=8, help="frames per GPU per step (C5: 64 frames / 8 GPUs)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline line's work, also run the secondary legs: asw_stereo_match_batch (--batch-frames), "
                         "the PCIe-inclusive one-call rate and the CPU baseline (--no-cpu skips it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step to DIR/<name>.npy (float32, %d MB at most)" % (DUMP_BYTES // 10**6))
    ap.add_argument("--batch-frames", type=int, default=64,
                    help="--full: frames of the asw_stereo_match_batch leg over all --gpus devices (C5: 64); 0 skips it")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="--full: CPU time budget of the CPU baseline")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--backend", default="nccl", help="process-group backend for N>1 (nccl = RCCL; gloo for rehearsals: implied by --dry-run and --oversubscribe)")
    ap.add_argument("--oversubscribe", action="store_true",
                    help="rehearsal only: allow more ranks than visible GPUs (ranks wrap over the devices)")
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU, no HIP library: a trivial numpy stand-in for the hot path, to exercise the rank launcher, "
                         "the process group and the JSON contract on CPU (tests/test_bench_launcher.py); never a measurement")
    ap.add_argument("--fail-rank", type=int, default=-1, help=argparse.SUPPRESS)  # dry-run fault injection for the launcher test
    return ap.parse_args(argv)


def launch_ranks(args, argv):
    """`python bench.py --gpus N` without a launcher around it: start N child ranks of this very script.

    The parent never imports torch and never touches the GPU (a process that has initialised the GPU must not be
    replaced or forked into ranks); children are ordinary subprocesses with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set,
    exactly what `python -m torch.distributed.run --nproc-per-node N` would give them.  Rank 0 inherits stdout and prints the
    one JSON line.  The first non-zero exit ends the job: the other children are terminated (by PID) and the code is returned.
    """
    import socket
    import subprocess

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this pool (RCCL needs it)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    live = list(procs)
    while live and rc == 0:
        time.sleep(0.05)
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            if code != 0:
                rc = code
    for p in live:  # a rank failed: the others would wait in a barrier for ever
        p.terminate()
    for p in live:
        try:
            p.wait(timeout=10)
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()
    if rc != 0:
        sys.stderr.write("bench.py: a rank exited with code %d; job aborted\n" % rc)
    return rc


class DryEngine:
    """--dry-run: stands where the asw context stands, computes a checksum on the CPU.  Exercises launcher, group, JSON."""

    def __init__(self):
        self.frames = {}
        self.sums = {}

    def upload_pair(self, i, L, R):
        self.frames[i] = (L, R)

    def match(self, i):
        L, R = self.frames[i]
        self.sums[i] = int(np.abs(L.astype(np.int32) - R.astype(np.int32)).sum())
        return {"aggregate_ms": 0.0, "total_ms": 0.0, "aggregate_launches": 0}

    def outputs(self):
        return {"checksum": np.array([self.sums[i] for i in sorted(self.sums)], np.float64)}

    def synchronize(self):
        pass

    def close(self):
        pass


def dump_outputs(directory, arrays, budget_bytes, suffix=""):
    """Write each array as DIR/<name><suffix>.npy; an array over its equal share of budget_bytes becomes a seeded sample."""
    os.makedirs(directory, exist_ok=True)
    share = budget_bytes // max(1, len(arrays))
    for name, a in sorted(arrays.items()):
        n = share // a.itemsize
        if a.size > n:
            what = "a seeded sample of %d of the %d values of shape %s" % (n, a.size, a.shape)
            a = a.reshape(-1)[np.sort(np.random.default_rng(DUMP_SEED).choice(a.size, n, replace=False))]
        else:
            what = "shape %s" % (a.shape,)
        path = os.path.join(directory, name + suffix + ".npy")
        np.save(path, a)
        sys.stderr.write("bench.py: wrote %s (%s, %s)\n" % (path, a.dtype, what))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = parse_args(argv)
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args, argv))  # parent: spawn the ranks, touch nothing else

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d: launch one rank per GPU (or drop the launcher and let "
                         "--gpus N start the ranks)" % (args.gpus, world))
    if (args.dry_run or args.oversubscribe) and args.backend == "nccl" and not os.environ.get("ASW_BENCH_KEEP_BACKEND"):
        args.backend = "gloo"  # no GPU at all / ranks sharing a GPU (RCCL refuses two ranks on one device): rehearsals only
    if args.fail_rank >= 0 and not args.dry_run:
        raise SystemExit("--fail-rank is a --dry-run test hook")

    alg, ncand_fn, label = WORKLOADS[args.workload]
    W, H, D = args.width, args.height, args.disp
    ncand = ncand_fn(D)

    from aswstereomatch_amd.dist import Group
    from aswstereomatch_amd.synth import make_pair

    torch = None
    device_index = -1
    if args.dry_run:
        group = Group(backend=args.backend)
        eng = DryEngine()
        ctx = None
    else:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        ndev = torch.cuda.device_count()
        if ndev < local_world and not args.oversubscribe:
            raise SystemExit("bench.py: %d ranks on this node but only %d GPU(s) visible; one process per GPU "
                             "(--oversubscribe only for rehearsals)" % (local_world, ndev))
        device_index = local_rank % ndev if args.oversubscribe else local_rank
        torch.cuda.set_device(device_index)
        import aswstereomatch_amd as asw

        group = Group(backend=args.backend, device=torch.device("cuda", device_index) if args.backend == "nccl" else None)
        ctx = asw.Context(device_index)

        class GpuEngine:
            def upload_pair(self, i, L, R):
                ctx.upload_pair(i, L, R)

            def match(self, i):
                ctx.match_resident(i, asw.DISPARITY_LEFT, alg, args.win, 0, D, keep_volume=True)
                return ctx.timing()

            def outputs(self):
                last = args.frames - 1
                planes = ctx._lib.asw_volume_planes(alg, D)
                return {"disparity": np.stack([ctx.download_disparity(i, (H, W)) for i in range(args.frames)]),
                        "cost_volume_last_frame": ctx.download_volume(last, (planes, H, W))}

            def synchronize(self):
                torch.cuda.synchronize()
                ctx._lib.asw_synchronize(ctx._h)

            def close(self):
                ctx.close()

        eng = GpuEngine()

    if rank == args.fail_rank:
        sys.stderr.write("bench.py: injected failure on rank %d\n" % rank)
        os._exit(3)

    # synthetic frames of the named shape, resident in HBM before the timed region
    frames = []
    for i in range(args.frames):
        L, R, _ = make_pair(H, W, D, seed=1234 + rank * args.frames + i)
        eng.upload_pair(i, L, R)
        if rank == 0:
            frames.append((L, R))

    def barrier():
        group.barrier()
        eng.synchronize()

    def step():
        agg = 0.0
        tot = 0.0
        launches = 0
        for i in range(args.frames):
            t = eng.match(i)
            agg += t["aggregate_ms"]
            tot += t["total_ms"]
            launches += t["aggregate_launches"]
        return agg, tot, launches

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    agg_ms = tot_ms = 0.0
    launches = 0
    for _ in range(args.steps):
        a, t, n = step()
        agg_ms += a
        tot_ms += t
        launches += n
    barrier()
    elapsed = time.perf_counter() - t0
    elapsed = group.max_over_ranks(elapsed)
    pids = group.gather_ints(os.getpid())  # one entry per rank: the line shows how many processes really ran
    devices = group.gather_ints(device_index)  # the device index every rank bound (-1: dry run)

    if rank == 0:
        frames_total = args.frames * args.steps * world
        value = W * H * frames_total / elapsed / 1e6
        n_frames_rank = args.frames * args.steps
        out = {
            "metric": "disparity Mpix/s, %dx%d D=%d %s" % (W, H, D, label),
            "value": round(value, 3), "unit": "Mpix/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64" if alg in (2, 4) else "f32", "data": "synthetic",
            "config": {"workload": "%dx%d D=%d win=%d %s, %d frames/GPU/step resident in HBM, cost volume kept"
                                   % (W, H, D, args.win, args.workload, args.frames),
                       "frames_per_gpu_per_step": args.frames, "candidates": ncand, "parallelism": "frames sharded, no collective",
                       "ranks": world, "rank_pids": pids, "backend": group.backend if world > 1 else "none",
                       # N > 1 on hardware: backend must read "nccl", rccl_ok true and devices 0..N-1, one process each -- a line
                       # whose rccl_ok is false was synchronised over gloo (aswstereomatch_amd/dist.py) and says why
                       "devices": devices,
                       "rccl_ok": (group.backend == "nccl") if (world > 1 and group.requested_backend == "nccl") else None,
                       "rccl_error": group.rccl_error},
        }
        if world > 1 and not args.dry_run and (out["config"]["rccl_ok"] is False or len(set(pids)) != world or sorted(devices) != list(range(world))):
            sys.stderr.write("bench.py: WARNING: this %d-GPU line is not one RCCL rank per device (backend %s, rccl_ok %s, %d processes, devices %s)\n"
                             % (world, group.backend, out["config"]["rccl_ok"], len(set(pids)), devices))
        if args.dry_run:
            out["dry_run"] = True
            out["data"] = "synthetic (dry run: CPU checksum stand-in, not a measurement)"
            print(json.dumps(out), flush=True)
        else:
            agg_per_frame_ms = agg_ms / n_frames_rank          # dominant aggregation kernel(s), HIP events
            balg = algorithmic_bytes(W, H, ncand)
            achieved = balg / (agg_per_frame_ms * 1e-3) / 1e9
            traffic = None
            traffic_source = None
            pmc = os.path.join(ROOT, "profiles", "pmc_%s.json" % args.workload)
            if os.path.exists(pmc):
                try:
                    rec = json.load(open(pmc))
                    # per FRAME, like algorithmic_bytes_per_launch below (the "launch" of this line is the frame's set of
                    # aggregation launches); only when the record was taken at this very shape
                    if rec.get("shape") == [W, H, D, args.win]:
                        traffic = rec.get("hbm_bytes_per_frame")
                        traffic_source = ("recorded: profiles/pmc_%s.json, bytes per frame over all aggregation launches (rocprofv3 --pmc "
                                          "FETCH_SIZE / WRITE_SIZE passes of this workload, FETCH_SIZE doubled per the gfx950 note); "
                                          "not re-measured in this run" % args.workload)
                except Exception:
                    traffic = None
            out["roofline"] = {"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic, "traffic_source": traffic_source,
                               "kernel": "aggregate (all aggregation launches of one frame)", "algorithmic_bytes_per_launch": balg,
                               "avg_launch_ms": round(agg_per_frame_ms / max(1, launches / n_frames_rank), 4),
                               "launches_per_frame": launches / n_frames_rank}
            out["kernel_ms_per_frame"] = {"aggregate": round(agg_per_frame_ms, 4), "all": round(tot_ms / n_frames_rank, 4)}
            if alg == 2:
                # this kernel is f64-VALU bound, not HBM bound: 1 f64 fma + 1 f64 add per (tap, d)
                taps = W * H * ncand * (args.win * args.win - 1)
                tf = taps * 3 / (agg_per_frame_ms * 1e-3) / 1e12  # fma = 2 flop, add = 1 flop, all f64
                out["valu_roofline"] = {"bound": "f64 valu", "achieved": round(tf, 3), "peak": F64_PEAK_TFLOPS,
                                        "unit": "TFLOP/s", "frac": round(tf / F64_PEAK_TFLOPS, 4),
                                        "note": "3 f64 flop per (pixel,d,tap); cvt/f32 work not counted"}

    # The process group has done its job (barrier around the timed region, MAX of the elapsed time): leave it now, all ranks
    # together.  Ranks other than 0 are finished and free their device; rank 0 goes on alone with the legs that are not part of
    # `value` -- no collective is pending, so nothing of RCCL can spin on a device meanwhile.
    group.close()
    if args.dump_outputs:  # every rank, before any secondary leg touches the context
        dump_outputs(args.dump_outputs, eng.outputs(), DUMP_BYTES // world, "_rank%d" % rank if world > 1 else "")
    if rank != 0:
        eng.close()
        return

    # ---- second leg (--full), rank 0 only, after the timed region: the product's own multi-GPU API.  asw_stereo_match_batch
    # shards --batch-frames frames (host buffers in and out) over ALL --gpus devices from ONE process.
    if args.full and not args.dry_run and args.batch_frames > 0:
        if rank == 0:
            import aswstereomatch_amd as asw

            try:
                devs = [k % torch.cuda.device_count() for k in range(world)] if args.oversubscribe else list(range(world))
                want = [ctx.download_disparity(i, (H, W)) for i in range(len(frames))]  # resident-path results of this rank's frames
                nb = args.batch_frames
                outs = [np.full((H, W), -1.0, np.float32) for _ in range(nb)]  # touched once, as a frame loop reusing buffers has them
                Lb = [frames[i % len(frames)][0] for i in range(nb)]
                Rb = [frames[i % len(frames)][1] for i in range(nb)]
                nw = min(nb, 2 * world)  # warm-up: creates the scheduler's contexts, scratch and pinned staging on every device
                asw.stereoMatchingBatch(Lb[:nw], Rb[:nw], asw.DISPARITY_LEFT, alg, args.win, 0, D, device_ids=devs)
                t1 = time.perf_counter()
                asw.stereoMatchingBatch(Lb, Rb, asw.DISPARITY_LEFT, alg, args.win, 0, D, device_ids=devs, out=outs)
                dt = time.perf_counter() - t1
                same = all(np.array_equal(outs[i], want[i % len(frames)]) for i in range(nb))
                out["batch_api"] = {"api": "asw_stereo_match_batch", "value": round(W * H * nb / dt / 1e6, 3), "unit": "Mpix/s",
                                    "frames": nb, "n_devices": world, "device_ids": devs, "ms_per_frame": round(dt / nb * 1e3, 3),
                                    "outputs_equal_resident_path": bool(same),
                                    "note": "one process, one host thread + context per device, pageable host buffers in and out "
                                            "(PCIe-inclusive); never the headline value"}
            except Exception as e:  # noqa: BLE001 -- a secondary leg must not cost the run its headline line
                out["batch_api"] = {"api": "asw_stereo_match_batch", "error": "%s: %s" % (type(e).__name__, e)}

    if rank == 0 and not args.dry_run:
        if args.full and world == 1:
            # the same method through the one-call host-buffer entry point (asw_stereo_match: H2D of both images, kernels,
            # D2H of the disparity) -- the PCIe-inclusive rate of sequential calls; never the headline value
            L, R = frames[0]
            try:
                ctx.stereoMatching(L, R, asw.DISPARITY_LEFT, alg, args.win, 0, D)
                t1 = time.perf_counter()
                nrep = 3
                for _ in range(nrep):
                    ctx.stereoMatching(L, R, asw.DISPARITY_LEFT, alg, args.win, 0, D)
                dt = (time.perf_counter() - t1) / nrep
                out["pcie_inclusive"] = {"value": round(W * H / dt / 1e6, 3), "unit": "Mpix/s", "ms_per_frame": round(dt * 1e3, 3),
                                         "note": "asw_stereo_match on pageable host buffers, no cost-volume download"}
            except Exception as e:  # noqa: BLE001
                out["pcie_inclusive"] = {"error": "%s: %s" % (type(e).__name__, e)}
            if not args.no_cpu:
                gpu_disp = ctx.download_disparity(0, (H, W))  # slot 0 still holds frame 0's result of the timed loop
                cb = cpu_baseline(args, L, R, gpu_disp, alg)
                if cb is not None:
                    out["cpu_baseline"] = cb
        print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
