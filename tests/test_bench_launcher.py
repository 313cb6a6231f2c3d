"""bench.py --gpus N must run N real processes.  No GPU here: `--dry-run` swaps the HIP hot path for a
numpy checksum and the process group runs on gloo, so the launcher, the rank environment, the barrier / MAX-over-ranks
timing and the one-JSON-line contract are exercised exactly as on the GPU box."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
SMALL = ["--dry-run", "--backend", "gloo", "--width", "96", "--height", "64", "--disp", "8", "--frames", "3", "--steps", "2",
         "--warmup", "1"]


def _clean_env():
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def _json_line(stdout):
    lines = stdout.strip().splitlines()
    # rank 0 prints ONE JSON line and NOTHING else on stdout (the banners gloo / RCCL print while a process group is built are
    # sent to stderr, aswstereomatch_amd/dist.py); the other ranks print nothing
    assert len(lines) == 1 and lines[0].startswith("{"), stdout
    return json.loads(lines[0])


def test_gpus_2_spawns_two_ranks_itself():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"] + SMALL, env=_clean_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _json_line(r.stdout)
    assert out["n_gpus"] == 2 and out["dry_run"] is True
    pids = out["config"]["rank_pids"]
    assert len(pids) == 2 and len(set(pids)) == 2 and os.getpid() not in pids  # two real child processes
    assert out["steps"] == 2 and out["warmup"] == 1 and out["scaling"] == "weak" and out["higher_is_better"] is True
    # whole-job value: W*H * frames * steps * ranks / elapsed
    assert abs(out["value"] - 96 * 64 * 3 * 2 * 2 / (out["ms_per_step"] * 2 / 1e3) / 1e6) <= 0.02 * out["value"] + 1e-3


def test_gpus_8_dry_run_is_eight_processes_and_says_how_it_was_synchronised():
    # the shape of the first real 8-GPU line, rehearsed on CPU: eight ranks, eight distinct processes; a dry run never claims RCCL
    r = subprocess.run([sys.executable, BENCH, "--gpus", "8"] + SMALL, env=_clean_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _json_line(r.stdout)
    cfg = out["config"]
    assert out["n_gpus"] == 8 and cfg["ranks"] == 8 and len(cfg["rank_pids"]) == 8 and len(set(cfg["rank_pids"])) == 8
    assert cfg["backend"] == "gloo" and cfg["rccl_ok"] is None and cfg["rccl_error"] is None  # gloo was asked for: nothing fell back
    assert cfg["devices"] == [-1] * 8  # no device in a dry run; on hardware: [0, 1, ..., 7]


def test_under_an_external_launcher_each_process_is_one_rank():
    # what `python -m torch.distributed.run --nproc-per-node 2 bench.py --gpus 2` gives every process
    procs = []
    for rank in range(2):
        env = dict(_clean_env(), RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", LOCAL_WORLD_SIZE="2",
                   MASTER_ADDR="127.0.0.1", MASTER_PORT="29547")
        procs.append(subprocess.Popen([sys.executable, BENCH, "--gpus", "2"] + SMALL, env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=300) for p in procs]
    assert [p.returncode for p in procs] == [0, 0], outs
    assert _json_line(outs[0][0])["n_gpus"] == 2
    assert "{" not in outs[1][0]  # rank 1 prints no JSON (gloo itself may print a connection notice)


def test_single_rank_default():
    r = subprocess.run([sys.executable, BENCH] + SMALL, env=_clean_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _json_line(r.stdout)
    assert out["n_gpus"] == 1 and len(out["config"]["rank_pids"]) == 1


def test_world_size_mismatch_fails_loudly():
    env = dict(_clean_env(), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"] + SMALL, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr and r.stdout.strip() == ""


def test_a_failing_rank_aborts_the_job():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--fail-rank", "1"] + SMALL, env=_clean_env(), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 3, (r.returncode, r.stderr[-2000:])
    assert "{" not in r.stdout  # no JSON line from a broken job


def test_without_a_gpu_the_real_bench_refuses():
    # the product path has no CPU fallback: on this GPU-less host the non-dry run must exit with a message, not a number.
    # Asked in a child process: torch brings its own copy of the HIP runtime, and once the library's copy is loaded here
    # (tests/test_abi_cpu.py), starting a second one in this process leaves the library without a device for the GPU tests.
    probe = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], env=_clean_env(),
                           capture_output=True, text=True, timeout=300)
    assert probe.returncode == 0, probe.stderr[-2000:]
    if probe.stdout.strip().splitlines()[-1] == "True":
        return
    r = subprocess.run([sys.executable, BENCH, "--steps", "1", "--warmup", "0"], env=_clean_env(), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "needs a GPU" in r.stderr and "{" not in r.stdout


def test_dump_outputs_are_the_same_from_run_to_run(tmp_path):
    sums = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, BENCH, "--dump-outputs", str(tmp_path / d)] + SMALL, env=_clean_env(), capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        _json_line(r.stdout)
        assert sorted(os.listdir(tmp_path / d)) == ["checksum.npy"]
        sums.append(np.load(tmp_path / d / "checksum.npy"))
    assert sums[0].dtype == np.float64 and sums[0].shape == (3,) and np.array_equal(sums[0], sums[1])


def test_dump_outputs_samples_an_array_over_its_share(tmp_path):
    import bench

    big = np.arange(1000, dtype=np.float32)
    small = np.ones((2, 3), np.float64)
    bench.dump_outputs(str(tmp_path), {"big": big, "small": small}, 2000, "_rank1")
    got = np.load(tmp_path / "big_rank1.npy")
    assert got.dtype == np.float32 and got.size == 1000 // 4 and np.all(np.diff(got) > 0)  # 1000 bytes: a sorted seeded sample
    assert np.array_equal(got, big[got.astype(np.int64)])
    bench.dump_outputs(str(tmp_path / "again"), {"big": big}, 1000)
    assert np.array_equal(np.load(tmp_path / "again" / "big.npy"), got)
    assert np.array_equal(np.load(tmp_path / "small_rank1.npy"), small)


@pytest.mark.gpu
def test_dump_outputs_are_what_the_resident_path_computed(tmp_path):
    import aswstereomatch_amd as asw
    from aswstereomatch_amd.synth import make_pair

    args = ["--width", "96", "--height", "64", "--disp", "8", "--frames", "2", "--steps", "2", "--warmup", "1"]
    r = subprocess.run([sys.executable, BENCH, "--dump-outputs", str(tmp_path)] + args, env=_clean_env(), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _json_line(r.stdout)
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and "cpu_baseline" not in out and "batch_api" not in out
    disp = np.load(tmp_path / "disparity.npy")
    vol = np.load(tmp_path / "cost_volume_last_frame.npy")
    assert disp.dtype == vol.dtype == np.float32 and disp.shape == (2, 64, 96) and vol.shape == (9, 64, 96)
    ctx = asw.Context(0)
    try:
        for i in range(2):
            L, R, _ = make_pair(64, 96, 8, seed=1234 + i)
            want, wvol = ctx.stereoMatching(L, R, asw.DISPARITY_LEFT, asw.StereoMatchingAlgorithms.ADAPTIVE_WEIGHT, 15, 0, 8,
                                            return_cost_volume=True)
            assert np.array_equal(disp[i], want)
        assert np.array_equal(vol, wvol, equal_nan=True)
    finally:
        ctx.close()
