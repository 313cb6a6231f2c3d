"""Sub-pixel disparity on the GPU (ASW_DISPARITY_SUBPIXEL_* in disparity_type; k_subpixel.hip) against the
restatement of tests/subpixel_ref.py.  The rule is stated in single IEEE f64 operations: every comparison is np.array_equal.

A kernel that moved nothing would pass wherever the guards refuse every pixel, so every parity case first asserts, on the
restatement applied to the GPU's own unflagged map and volume, the refined share of tests/test_subpixel_cpu.py (>= 0.75; the
bilateral grid, whose volume is almost all non-finite on these pairs, must come back unchanged instead)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib
from aswstereomatch_amd._lib import AswError
from aswstereomatch_amd.synth import make_pair

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subpixel_ref as sp  # noqa: E402
from shim_build import build_demo  # noqa: E402

A = asw.StereoMatchingAlgorithms
LEFT, RIGHT = asw.DISPARITY_LEFT, asw.DISPARITY_RIGHT
MODES = (asw.SUBPIXEL_PARABOLA, asw.SUBPIXEL_EQUIANGULAR)
PAIRS = {"a": (96, 260, 24, 11, 32), "b": (60, 160, 16, 5, 16)}
# method -> (selector value, DISPARITY_RIGHT served, pairs with a share requirement)
METHODS = {
    "classic": (A.ADAPTIVE_WEIGHT, True, "ab"), "geodesic": (A.ADAPTIVE_WEIGHT_GEODESIC, True, "ab"),
    "GuidedF": (A.ADAPTIVE_WEIGHT_GUIDED_FILTER, True, "ab"), "GuidedF_2": (A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2, False, "ab"),
    "GuidedF_3": (A.ADAPTIVE_WEIGHT_GUIDED_FILTER_3, True, "a"), "median": (A.ADAPTIVE_WEIGHT_MEDIAN, False, "ab"),
    "BLO1": (A.ADAPTIVE_WEIGHT_BLO1, True, "ab"), "direct8": (A.ADAPTIVE_WEIGHT_8DIRECT, False, "ab"),
    "bilgrid": (A.ADAPTIVE_WEIGHT_BILATERAL_GRID, False, "ab"),
}

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


def _planes(alg, D):
    return _lib.lib().asw_volume_planes(int(alg), D)


def _parity(ctx, L, R, dt, alg, win, minD, D, share=0.75, unchanged=False):
    """Flagged calls of both modes against the restatement on the unflagged call's own map and volume -> {mode: map}."""
    d0, v0 = ctx.stereoMatching(L, R, dt, alg, win, minD, D, return_cost_volume=True)
    assert v0.shape[0] == _planes(alg, D)
    got = {}
    for mode in MODES:
        want, ok = sp.subpixel_vec(d0, v0, minD, mode)
        print("alg %d dt %d mode %#x: refined share %.3f" % (int(alg), int(dt), mode, ok.mean()))
        if unchanged:
            assert want.tobytes() == d0.tobytes()
        else:  # share: the requirement of the CPU test where there is one; everywhere the kernel must have something to move
            assert share is None or ok.mean() >= share
            assert (want != d0).mean() >= 0.1
        d1, v1 = ctx.stereoMatching(L, R, dt, alg, win, minD, D, return_cost_volume=True, subpixel=mode)
        assert v1.tobytes() == v0.tobytes()  # the volume of a flagged call is the unflagged one, NaN slots included
        assert np.array_equal(d1, want), np.argwhere(d1 != want)[:5]
        assert (np.abs(d1 - d0) <= 0.5).all()
        # the flag OR-ed in by the caller is the same call
        assert np.array_equal(ctx.stereoMatching(L, R, int(dt) | mode, alg, win, minD, D), want)
        got[mode] = d1
    return d0, v0, got


# ---- parity per method, mode and direction ----
@pytest.mark.parametrize("pair", ["a", "b"])
@pytest.mark.parametrize("method", list(METHODS))
def test_parity_per_method(ctx, pair, method):
    alg, right, share_pairs = METHODS[method]
    H, W, D, seed, block = PAIRS[pair]
    L, R, _ = make_pair(H, W, D, seed=seed, block=block)
    share = 0.75 if pair in share_pairs else None
    _parity(ctx, L, R, LEFT, alg, 15, 0, D, share=share, unchanged=method == "bilgrid")
    if right:  # the share requirement is stated for the left view
        _parity(ctx, L, R, RIGHT, alg, 15, 0, D, share=None)


# ---- the oracle's bit-exact volumes ----
@pytest.mark.parametrize("method", ["classic", "geodesic"])
@pytest.mark.parametrize("dt", [LEFT, RIGHT])
def test_against_oracle_volumes(ctx, oracle, method, dt):
    H, W, D, seed, block = PAIRS["b"]
    L, R, _ = make_pair(H, W, D, seed=seed, block=block)
    if method == "classic":
        rc, dw, vw = oracle.asw_classic(L, R, 30.0, 20.0, int(dt), 15, 0, D, want_vol=True)
    else:
        rc, dw, vw = oracle.asw_geodesic(L, R, int(dt), 15, 0, D, want_vol=True)
    assert rc == 0
    for mode in MODES:
        want, ok = sp.subpixel_vec(dw, vw, 0, mode)
        assert ok.mean() >= 0.75  # measured on the oracle: 0.91 in either view
        assert np.array_equal(ctx.stereoMatching(L, R, dt, METHODS[method][0], 15, 0, D, subpixel=mode), want)


# ---- both kernel forms of the bilateral and the geodesic method ----
# (H, W, minD, numD, row padding in pixels): the xq forms need win 15 and >= 64 candidates
FORM_SHAPES = [(9, 200, 0, 128, 0), (4, 333, 48, 70, 0), (5, 131, 2, 100, 5), (3, 257, 3, 140, 0)]


@pytest.mark.parametrize("method,switch", [("classic", "ASW_BILATERAL_XQ"), ("geodesic", "ASW_GEODESIC_XQ")])
@pytest.mark.parametrize("H,W,minD,numD,pad", FORM_SHAPES)
def test_both_kernel_forms(ctx, method, switch, H, W, minD, numD, pad):
    alg = METHODS[method][0]
    L, R, _ = make_pair(H, W + pad, min(numD, W // 2), seed=H * 1000 + W, block=16)
    L, R = L[:, :W], R[:, :W]  # pad > 0: views whose rows carry padding (step > cols * 3)
    assert (L.strides[0] > W * 3) == (pad > 0)
    old = asw.Context(0, env={switch: "0"})  # the one-kernel form only
    try:
        for dt in (LEFT, RIGHT):
            ctx.stereoMatching(L, R, dt, alg, 15, minD, numD, subpixel=MODES[0])
            xq_launches = ctx.timing()["aggregate_launches"]
            old.stereoMatching(L, R, dt, alg, 15, minD, numD, subpixel=MODES[0])
            if method == "classic" and dt == LEFT:  # the two forms really ran (RIGHT with a large minD has the one-kernel form only)
                assert xq_launches > 1 and old.timing()["aggregate_launches"] == 1
            _, _, new = _parity(ctx, L, R, dt, alg, 15, minD, numD, share=None)
            _, _, one = _parity(old, L, R, dt, alg, 15, minD, numD, share=None)
            for mode in MODES:
                assert np.array_equal(new[mode], one[mode])
    finally:
        old.close()


# ---- without a kept volume; the resident slot ----
@pytest.mark.parametrize("method", ["classic", "geodesic", "BLO1", "bilgrid", "direct8", "GuidedF_2", "median"])
def test_no_kept_volume_and_resident(ctx, method):
    alg = METHODS[method][0]
    H, W, D, seed, block = PAIRS["b"]
    L, R, _ = make_pair(H, W, D, seed=seed, block=block)
    n = _planes(alg, D)
    d0, v0 = ctx.stereoMatching(L, R, LEFT, alg, 15, 0, D, return_cost_volume=True)
    ctx.upload_pair(11, L, R)
    for mode in MODES:
        want, _ = sp.subpixel_vec(d0, v0, 0, mode)
        assert np.array_equal(ctx.stereoMatching(L, R, LEFT, alg, 15, 0, D, subpixel=mode), want)  # cost_volume_out = NULL
        ctx.match_resident(11, LEFT, alg, 15, 0, D, keep_volume=True)  # a previous, unflagged result with a volume
        assert np.array_equal(ctx.download_disparity(11, (H, W)), d0)
        ctx.match_resident(11, LEFT, alg, 15, 0, D, keep_volume=False, subpixel=mode)
        assert np.array_equal(ctx.download_disparity(11, (H, W)), want)
        with pytest.raises(AswError) as e:
            ctx.download_volume(11, (n, H, W))
        assert e.value.status == asw.ERR_NO_FRAME
        t = ctx.timing()
        assert t["total_ms"] > 0 and t["total_ms"] >= t["aggregate_ms"] >= 0 and t["cost_ms"] > 0
        ctx.match_resident(11, int(LEFT) | mode, alg, 15, 0, D, keep_volume=True)
        assert np.array_equal(ctx.download_disparity(11, (H, W)), want)
        assert ctx.download_volume(11, (n, H, W)).tobytes() == v0.tobytes()
        l2, r2 = ctx.download_pair(11, L.shape)
        assert np.array_equal(l2, L) and np.array_equal(r2, R)
    # the unflagged call afterwards is the integer map again
    ctx.match_resident(11, LEFT, alg, 15, 0, D)
    assert np.array_equal(ctx.download_disparity(11, (H, W)), d0)


def test_per_method_entry_points_take_the_flag(ctx):
    H, W, D, seed, block = PAIRS["b"]
    L, R, _ = make_pair(H, W, D, seed=seed, block=block)
    calls = [
        lambda dt, **k: ctx.computeAdaptiveWeight(L, R, 30, 20, dt, 15, 0, D, **k),
        lambda dt, **k: ctx.computeAdaptiveWeight_direct8(L, R, dt, 15, 0, D, **k),
        lambda dt, **k: ctx.computeAdaptiveWeight_geodesic(L, R, dt, 15, 0, D, **k),
        lambda dt, **k: ctx.computeAdaptiveWeight_GuidedF(L, R, dt, 1e-6, 15, 0, D, **k),
        lambda dt, **k: ctx.computeAdaptiveWeight_GuidedF_2(L, R, dt, 1e-6, 15, 0, D, **k),
        lambda dt, **k: ctx.computeAdaptiveWeight_GuidedF_3(L, R, dt, 1e-6, 15, 0, D, **k),
        lambda dt, **k: ctx.computeAdaptiveWeight_BLO1(L, R, dt, 0.015, 15, 0, D, **k),
        lambda dt, **k: ctx.computeAdaptiveWeight_bilateralGrid(L, R, dt, 10, 10, 0, D, **k),
        lambda dt, **k: ctx.computeAdaptiveWeight_WeightedMedian(L, R, dt, 15, 10, 10, 0, D, **k),
    ]
    for call in calls:
        d0, v0 = call(LEFT, return_cost_volume=True)
        for mode in MODES:
            want, _ = sp.subpixel_vec(d0, v0, 0, mode)
            d1, v1 = call(int(LEFT) | mode, return_cost_volume=True)
            assert np.array_equal(d1, want) and v1.tobytes() == v0.tobytes()
            assert np.array_equal(call(int(LEFT) | mode), want)


# ---- batch ----
@pytest.mark.parametrize("alg", [A.ADAPTIVE_WEIGHT, A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2, A.ADAPTIVE_WEIGHT_GEODESIC])
def test_batch_equals_single_calls(ctx, alg):
    H, W, D = 40, 150, 20
    pairs = [make_pair(H, W, D, seed=100 + i, block=16)[:2] for i in range(5)]
    for mode in MODES:
        outs = asw.stereoMatchingBatch([p[0] for p in pairs], [p[1] for p in pairs], LEFT, alg, 15, 0, D, device_ids=[0], subpixel=mode)
        for (L, R), o in zip(pairs, outs):
            single = ctx.stereoMatching(L, R, LEFT, alg, 15, 0, D, subpixel=mode)
            assert o.tobytes() == single.tobytes()
            assert (o != np.floor(o)).mean() >= 0.3  # fractional maps: the non-syncing path enqueued the kernel
    outs = asw.stereoMatchingBatch([p[0] for p in pairs], [p[1] for p in pairs], LEFT, alg, 15, 0, D, device_ids=[0])
    assert all((o == np.floor(o)).all() for o in outs)


# ---- 8-bit download ----
def test_u8_download_rounds_half_to_even(ctx, oracle):
    H, W, D, seed, block = PAIRS["a"]
    L, R, _ = make_pair(H, W, D, seed=seed, block=block)
    ctx.upload_pair(12, L, R)
    # the median's costs are order statistics: a neighbour that ties with the winner gives an offset of exactly 0.5
    for alg, mode in ((A.ADAPTIVE_WEIGHT, asw.SUBPIXEL_PARABOLA), (A.ADAPTIVE_WEIGHT_MEDIAN, asw.SUBPIXEL_EQUIANGULAR)):
        ctx.match_resident(12, LEFT, alg, 15, 0, D, subpixel=mode)
        d = ctx.download_disparity(12, (H, W))
        assert (d != np.floor(d)).mean() >= 0.5
        frac = d - np.floor(d)
        print("pixels at exactly x.5: %d" % (frac == 0.5).sum())
        assert ((frac > 0) & (frac < 0.5)).mean() >= 0.1 and (frac > 0.5).mean() >= 0.1  # truncation or rounding up would show
        for normalize in (False, True):
            got = ctx.download_disparity_u8(12, (H, W), normalize=normalize)
            assert np.array_equal(got, oracle.disparity_to_u8(d, normalize=normalize))
        assert np.array_equal(ctx.download_disparity_u8(12, (H, W), normalize=False), np.clip(np.rint(d), 0, 255).astype(np.uint8))


# ---- statuses ----
def test_statuses(ctx):
    H, W, D, seed, block = PAIRS["b"]
    L, R, _ = make_pair(H, W, D, seed=seed, block=block)
    P, E = MODES
    ctx.upload_pair(13, L, R)

    def expect(status, dt, alg, win=15, numD=D):
        ctx.match_resident(13, LEFT, A.ADAPTIVE_WEIGHT, 15, 0, D, keep_volume=True)  # a previous result
        with pytest.raises(AswError) as e:
            ctx.match_resident(13, dt, alg, win, 0, numD, keep_volume=True)
        assert e.value.status == status, (dt, alg, e.value.status)
        for fetch in (lambda: ctx.download_disparity(13, (H, W)), lambda: ctx.download_volume(13, (D + 1, H, W))):
            with pytest.raises(AswError) as e:  # a failed flagged match drops the slot's results
                fetch()
            assert e.value.status == asw.ERR_NO_FRAME
        l2, r2 = ctx.download_pair(13, L.shape)
        assert np.array_equal(l2, L) and np.array_equal(r2, R)
        with pytest.raises(AswError) as e:  # the host-image call answers alike
            ctx.stereoMatching(L, R, dt, alg, win, 0, numD)
        assert e.value.status == status

    expect(asw.ERR_BAD_ARGUMENT, P | E, A.ADAPTIVE_WEIGHT)
    expect(asw.ERR_BAD_ARGUMENT, P | E | 1, A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2)
    expect(asw.ERR_BAD_ARGUMENT, 0x400, A.ADAPTIVE_WEIGHT)
    expect(asw.ERR_BAD_ARGUMENT, P | 0x400, A.ADAPTIVE_WEIGHT)
    expect(asw.ERR_BAD_ARGUMENT, E | 2, A.ADAPTIVE_WEIGHT_GEODESIC)
    expect(asw.ERR_UNSUPPORTED_METHOD, P, A.NCC)
    expect(asw.ERR_UNSUPPORTED_METHOD, E | 1, A.NCC)
    expect(asw.ERR_UNSUPPORTED_METHOD, P, A.BM, numD=16)
    # the low bit keeps its statuses
    for alg in (A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2, A.ADAPTIVE_WEIGHT_MEDIAN, A.ADAPTIVE_WEIGHT_8DIRECT, A.ADAPTIVE_WEIGHT_BILATERAL_GRID):
        expect(asw.ERR_UNSUPPORTED_LAYOUT, P | 1, alg)
    expect(asw.ERR_BAD_ARGUMENT, P, A.ADAPTIVE_WEIGHT, numD=0)
    with pytest.raises(AswError) as e:
        ctx.computeNCC(L, R, int(LEFT) | P, 15, 0, D)
    assert e.value.status == asw.ERR_UNSUPPORTED_METHOD
    assert ctx.stereoMatching(L, R, int(LEFT) | E, A.ADAPTIVE_WEIGHT, 14, 0, D) is None  # even window: the silent return, as unflagged
    assert asw.last_status() == asw.ERR_EVEN_WINDOW
    # SGBM ignores disparity_type altogether
    s0 = ctx.stereoMatching(L, R, LEFT, A.SGBM, 5, 0, 16)
    assert np.array_equal(ctx.stereoMatching(L, R, P | E | 0x400, A.SGBM, 5, 0, 16), s0)
    # the batch call returns the same statuses
    with pytest.raises(AswError) as e:
        asw.stereoMatchingBatch([L], [R], int(LEFT) | P | E, A.ADAPTIVE_WEIGHT, 15, 0, D, device_ids=[0])
    assert e.value.status == asw.ERR_BAD_ARGUMENT
    # and the slot works again afterwards
    ctx.match_resident(13, LEFT, A.ADAPTIVE_WEIGHT, 15, 0, D, subpixel=P)
    assert ctx.download_disparity(13, (H, W)).shape == (H, W)


# ---- value on the GPU: the slanted plane of tests/test_subpixel_cpu.py ----
@pytest.mark.parametrize("method", ["classic", "GuidedF_2"])
def test_slanted_plane_value(ctx, method):
    L, R, gt = sp.slanted_plane_pair()
    alg = METHODS[method][0]
    mae_int = sp.cropped_mae(ctx.stereoMatching(L, R, LEFT, alg, 15, 0, 16), gt)
    for mode in MODES:
        mae_sub = sp.cropped_mae(ctx.stereoMatching(L, R, LEFT, alg, 15, 0, 16, subpixel=mode), gt)
        print("%s mode %#x: MAE integer %.4f, sub-pixel %.4f, ratio %.3f" % (method, mode, mae_int, mae_sub, mae_sub / mae_int))
        assert mae_sub <= 0.6 * mae_int


# ---- one whole frame, the headline configuration ----
def test_full_frame_bilateral(ctx):
    H, W, D = 1080, 1920, 128
    L, R, _ = make_pair(H, W, D, seed=1234, block=48)
    ctx.upload_pair(0, L, R)
    ctx.match_resident(0, LEFT, A.ADAPTIVE_WEIGHT, 15, 0, D, keep_volume=True)
    d0 = ctx.download_disparity(0, (H, W))
    v0 = ctx.download_volume(0, (D + 1, H, W))
    want, ok = sp.subpixel_vec(d0, v0, 0, asw.SUBPIXEL_EQUIANGULAR)
    assert ok.mean() >= 0.75
    ctx.match_resident(0, LEFT, A.ADAPTIVE_WEIGHT, 15, 0, D, subpixel=asw.SUBPIXEL_EQUIANGULAR)
    assert np.array_equal(ctx.download_disparity(0, (H, W)), want)


# ---- the C++ shim ----
@pytest.mark.parametrize("cv", [False, True])
def test_shim_subpixel(ctx, tmp_path, cv):
    exe = build_demo("subpixel_demo.cpp", tmp_path / "subpixel_demo", cv)
    H, W, D, seed, block = PAIRS["b"]
    L, R, _ = make_pair(H, W, D, seed=seed, block=block)
    L.tofile(tmp_path / "l.raw")
    R.tofile(tmp_path / "r.raw")

    def run(dt, alg, mode):
        return subprocess.run([exe, str(H), str(W), "3", str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), str(int(dt)), str(int(alg)),
                               "15", "0", str(D), str(mode), str(tmp_path / "shim.raw"), str(tmp_path / "c.raw")],
                              capture_output=True, text=True, timeout=120)

    for dt, alg, mode in ((LEFT, A.ADAPTIVE_WEIGHT, MODES[0]), (RIGHT, A.ADAPTIVE_WEIGHT_GEODESIC, MODES[1]),
                          (LEFT, A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2, MODES[1])):
        d0, v0 = ctx.stereoMatching(L, R, dt, alg, 15, 0, D, return_cost_volume=True)
        want, ok = sp.subpixel_vec(d0, v0, 0, mode)
        assert (want != d0).mean() >= 0.3
        r = run(dt, alg, mode)
        assert r.returncode == 0 and r.stdout.strip() == "ok %d %d" % (H, W), (r.stdout, r.stderr)
        for name in ("shim.raw", "c.raw"):
            assert np.array_equal(np.fromfile(tmp_path / name, np.float32).reshape(H, W), want)
    r = run(LEFT, A.NCC, MODES[0])
    assert r.returncode == 0 and r.stdout.startswith("error"), (r.stdout, r.stderr)
    r = run(RIGHT, A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2, MODES[0])
    assert r.returncode == 0 and r.stdout.startswith("error"), (r.stdout, r.stderr)
