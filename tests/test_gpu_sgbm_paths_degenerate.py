"""asw_sgbm_paths (k_sgbm_line of k_sgbm.hip) where the textured pairs of tests/test_gpu_sgbm_paths.py never
take it: costs that tie under the added directions, every number of candidates per lane with a full, a partly filled and an empty
last register, frames of one or two rows or one valid column, padded rows, and identities between the GPU's own volumes that hold
whatever tests/sgbm_paths_ref.py says.  Every comparison with the restatement is np.array_equal, map and volume.

The identities: S is a sum of independent paths, so the volume of a mask minus the three-path volume is the sum of what each added
bit adds alone (this pins the forth-then-back walk of one wavefront, and several line launches in a row, to single walks); in a
frame of one row, or of one valid column, an added line has one pixel and adds the block cost C itself; and turning the pair upside
down turns the result upside down when the mask is turned with it, which for 0x0F ties the bottom->top path to the top->bottom path
of asw_sgbm (tests/test_gpu_sgbm.py, tests/test_gpu_matcher_degenerate.py)."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd import _lib
from aswstereomatch_amd.synth import make_pair

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matcher_cases as mc  # noqa: E402
import sgbm_paths_ref as pref  # noqa: E402

H, W, BLOCK = 20, 150, 5   # the tie pairs of tests/test_gpu_matcher_degenerate.py
DIAGONALS = (pref.PATH_TLBR, pref.PATH_TRBL, pref.PATH_BRTL, pref.PATH_BLTR)
FULL = (1, 10, 10, 20, 2)  # disp12MaxDiff, preFilterCap, uniquenessRatio, speckleWindowSize, speckleRange

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = asw.Context(0)
    yield c
    c.close()


def _check(ctx, L, R, minD, D, w, P1, P2, m12, cap, U, sw, sr, paths):
    want = pref.sgbm_paths(L, R, minD, D, w, P1, P2, m12, cap, U, sw, sr, paths)
    got, vol = ctx.sgbm_paths(L, R, minD, D, w, P1, P2, m12, cap, U, sw, sr, paths=paths, return_cost_volume=True)
    tag = (L.shape, minD, D, w, P1, P2, m12, cap, U, sw, sr, hex(paths))
    assert np.array_equal(vol, np.moveaxis(want["S"], 2, 0).astype(np.float32)), tag
    assert got.dtype == np.int16 and np.array_equal(got, want["disp"]), tag
    return want


def _textured(Hn, Wn, D, cn, seed):
    L, R, _ = make_pair(Hn, Wn, max(2, min(D, 64) // 2), seed=seed, block=16)
    if cn == 1:
        return np.ascontiguousarray(L[:, :, 1]), np.ascontiguousarray(R[:, :, 1])
    return L, R


# ---------------------------------------------------------------- a. ties
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("D", [32, 80])  # D = 80: two candidates per lane, a tie can sit in two registers of one lane
@pytest.mark.parametrize("kind", mc.TIE_KINDS)
def test_sgbm_paths_tied_costs(ctx, kind, D, cn):
    L, R = mc.tie_pair(kind, H, W, cn)
    for paths in (pref.PATHS_HH4, pref.PATHS_SGBM, pref.PATHS_HH):
        for cap, minD, U, m12 in itertools.product((10, 63), (0, 5), (0, 10), (-1, 1)):
            want = _check(ctx, L, R, minD, D, BLOCK, 200, 800, m12, cap, U, 0, 0, paths)
            # the floors of tests/test_sgbm_paths_cpu.py::test_tie_generators_tie_under_every_named_mask, on the restatement alone
            if (D, cn, cap, U, m12) != (32, 1, 10, 0, -1):
                continue
            ties = mc.tie_share(want["S"][:, minD + D:], 2)
            alive = float((want["disp"] != 16 * (minD - 1)).mean())
            if (kind, minD) == ("periodic4", 0):
                print("paths 0x%02X periodic(4, 3): tie share %.3f, not-invalid share %.3f" % (paths, ties, alive))
                assert ties >= 0.5 and alive >= 0.5
            if (kind, minD) == ("constant", 5):
                print("paths 0x%02X constant minD 5: tie share %.3f" % (paths, ties))
                assert ties >= 0.5
                assert (want["disp"][:, minD + D:] == 16 * minD).all()  # the smallest disparity


# ---------------------------------------------------------------- b. every lane form
# NPL = ceil(D / 64) rounded up to 1, 2, 4, 8, 16 registers per lane.  full: D = 64 NPL; partly filled last register: D % 64 != 0
# with ceil(D / 64) = NPL; a last register wholly beyond D: ceil(D / 64) < NPL
LANE_FORMS = [
    (16, 1), (64, 1),                                  # partial, full
    (80, 2), (128, 2),                                 # partial, full
    (144, 4), (192, 4), (256, 4),                      # three live registers of four (the third partial); three full; full
    (272, 8), (320, 8), (512, 8),                      # five live of eight (the fifth partial); five full; full
    (528, 16), (576, 16), (1024, 16),                  # nine live of sixteen (the ninth partial); nine full; full
]


def _lane_frame(ctx, D, paths):
    L, R = _textured(6, D + 9, D, 1, seed=D)
    want = _check(ctx, L, R, 0, D, 3, 20, 200, *FULL, paths)
    assert want["S"][:, D:].any()


@pytest.mark.parametrize("D,npl", LANE_FORMS)
def test_sgbm_paths_every_lane_form(ctx, D, npl):
    assert npl == next(n for n in (1, 2, 4, 8, 16) if n >= (D + 63) // 64)   # launch_sgbm's choice
    _lane_frame(ctx, D, pref.PATHS_HH)


@pytest.mark.parametrize("bit", pref.NEW_BITS)
def test_sgbm_paths_eight_registers_each_direction(ctx, bit):
    _lane_frame(ctx, 320, 0x07 | bit)


# ---------------------------------------------------------------- c. tiny and ragged frames
# the line count H + Wv - 1 of a diagonal launch at 3, 64, 65 and 128
LINE_COUNT_FRAMES = [(2, 16 + 2, 0, 16, 3), (2, 16 + 63, 0, 16, 3), (64, 16 + 2, 0, 16, 3), (65, 16 + 64, 0, 16, 3)]


@pytest.mark.parametrize("paths", [pref.PATHS_HH, 0x07 | pref.PATH_TRBL | pref.PATH_BLTR])
@pytest.mark.parametrize("Hn,Wn,minD,D,w", mc.SGBM_TINY_FRAMES + LINE_COUNT_FRAMES)
def test_sgbm_paths_tiny_and_ragged_frames(ctx, Hn, Wn, minD, D, w, paths):
    L, R = mc.noise(Hn, Wn, Hn * 1000 + Wn)
    assert Wn - minD - D >= 1
    for P1, P2, m12, cap, U in mc.sgbm_tiny_settings(w):
        want = _check(ctx, L, R, minD, D, w, P1, P2, m12, cap, U, 0, 0, paths)
        assert want["S"][:, minD + D:].any()
    L3 = np.ascontiguousarray(np.stack([L, R, L], axis=2))
    R3 = np.ascontiguousarray(np.stack([R, L, R[::-1]], axis=2))
    _check(ctx, L3, R3, minD, D, w, 0, 0, 0, 0, -1, 0, 0, paths)


# ---------------------------------------------------------------- d. identities between the GPU's own volumes
def _volume(ctx, L, R, args, paths):
    """(map, S as int64 [D][H][W]) of the GPU; the f32 volume holds integers below 2^24"""
    disp, vol = ctx.sgbm_paths(L, R, *args, paths=paths, return_cost_volume=True)
    out = vol.astype(np.int64)
    assert np.array_equal(out.astype(np.float32), vol) and vol.max() < 1 << 24
    return disp, out


def _deltas(ctx, L, R, args, masks):
    """V(0x07) and {m: V(m) - V(0x07)}"""
    base = _volume(ctx, L, R, args, pref.PATHS_3WAY)[1]
    return base, {m: _volume(ctx, L, R, args, m)[1] - base for m in masks}


@pytest.mark.parametrize("Hn,Wn,D,w", [(24, 40, 16, 3), (33, 100, 80, 5)])
def test_volume_of_a_mask_is_the_sum_of_its_parts(ctx, Hn, Wn, D, w):
    L, R = _textured(Hn, Wn, D, 3, seed=Hn + Wn)
    args = (0, D, w, 8 * 3 * w * w, 32 * 3 * w * w) + FULL
    both = (pref.PATH_TLBR | pref.PATH_BRTL, pref.PATH_TRBL | pref.PATH_BLTR)
    _, d = _deltas(ctx, L, R, args, [0x07 | b for b in pref.NEW_BITS] + [0x07 | b for b in both] + [pref.PATHS_HH])
    for b in pref.NEW_BITS:
        assert d[0x07 | b][:, :, D:].min() >= 0 and d[0x07 | b][:, :, D:].any(), hex(b)
    assert len({d[0x07 | b].tobytes() for b in pref.NEW_BITS}) == 5          # five different contributions
    assert np.array_equal(d[pref.PATHS_HH], sum(d[0x07 | b] for b in pref.NEW_BITS))
    # forth and back over the same line in one launch, against the two single walks
    assert np.array_equal(d[0x07 | both[0]], d[0x07 | pref.PATH_TLBR] + d[0x07 | pref.PATH_BRTL])
    assert np.array_equal(d[0x07 | both[1]], d[0x07 | pref.PATH_TRBL] + d[0x07 | pref.PATH_BLTR])


def test_one_row_every_added_line_is_one_pixel(ctx):
    """H = 1: each added direction starts and ends in its pixel, so it adds L = C + min(0, P1, P2) - 0 = C.  C is read back as the
    difference V(0x0F) - V(0x07); the three-path volume itself is then L_lr(C) + L_rl(C) + L_tb with L_tb = C (its line has one
    pixel as well), the two row recurrences taken over the C read back from the GPU.  In a frame of one row and one valid column
    every path is one pixel and the three-path volume is 3 C with no recurrence at all."""
    D, w = 16, 3
    L, R = _textured(1, 60, D, 3, seed=61)
    args = (0, D, w, 8 * 3 * w * w, 32 * 3 * w * w) + FULL
    base, d = _deltas(ctx, L, R, args, [0x07 | b for b in pref.NEW_BITS] + [pref.PATHS_HH])
    c = d[pref.PATHS_HH4]
    assert c[:, :, D:].any() and not c[:, :, :D].any()
    for b in pref.NEW_BITS:
        assert np.array_equal(d[0x07 | b], c), hex(b)
    assert np.array_equal(d[pref.PATHS_HH], 5 * c)
    Cv = np.ascontiguousarray(np.moveaxis(c[:, :, D:], 0, 2))     # [H][Wv][D]
    P1, P2 = args[3], args[4]
    rows = pref.path(Cv, P1, P2, 1, 0) + pref.path(Cv, P1, P2, -1, 0)
    assert np.array_equal(np.moveaxis(base[:, :, D:], 0, 2), rows + Cv)
    # one row, one valid column
    L1, R1 = np.ascontiguousarray(L[:, :D + 1]), np.ascontiguousarray(R[:, :D + 1])
    base, d = _deltas(ctx, L1, R1, args, [pref.PATHS_HH4, pref.PATHS_HH])
    assert d[pref.PATHS_HH4][:, :, D].any()
    assert np.array_equal(base, 3 * d[pref.PATHS_HH4]) and np.array_equal(d[pref.PATHS_HH], 5 * d[pref.PATHS_HH4])


def test_one_valid_column_every_diagonal_is_one_pixel(ctx):
    D = 16
    L, R = _textured(30, D + 1, D, 3, seed=47)
    args = (0, D, 3, 7, 50, 0, 10, 0, 0, 0)
    base, d = _deltas(ctx, L, R, args, [0x07 | b for b in DIAGONALS] + [pref.PATHS_HH4])
    c = d[0x07 | pref.PATH_TLBR]
    assert c[:, :, D].any()
    for b in DIAGONALS:
        assert np.array_equal(d[0x07 | b], c), hex(b)
    # the two row paths have one pixel as well, and the column paths start with L = C: top->bottom in row 0, bottom->top in row H-1
    assert np.array_equal(base[:, 0], 3 * c[:, 0]) and np.array_equal(d[pref.PATHS_HH4][:, -1], c[:, -1])
    assert not np.array_equal(d[pref.PATHS_HH4], c)


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("kind", mc.PATHS_FLIP_KINDS)
def test_vertical_flip_permutes_the_directions(ctx, kind, cn):
    """The result for mask m, turned upside down, is the result for vflip(m) on the pair turned upside down.  The library serves
    supersets of the three paths only, and vflip moves top->bottom to bottom->top, so vflip(m) is admissible only when m holds
    PATH_BT.  Each mask of the table is therefore taken twice.  With PATH_BT added (0x0F and 0xFF have it) the map and the volume
    are compared as they are.  Without it the diagonals it adds are compared through the volumes' differences from the three-path
    volume, flip(V(m) - V(0x07)) = V'(0x07 | vflip(m & 0xF0)) - V'(0x07), V' on the turned pair: both sides are admissible
    calls, and the three paths themselves, which do not flip into each other, drop out."""
    L, R = mc.paths_flip_pair(kind, cn)
    Lf, Rf = L[::-1].copy(), R[::-1].copy()
    args = mc.paths_flip_args(cn)
    base, basef = _volume(ctx, L, R, args, pref.PATHS_3WAY)[1], _volume(ctx, Lf, Rf, args, pref.PATHS_3WAY)[1]
    assert not np.array_equal(basef[:, ::-1], base)          # top->bottom alone is not symmetric
    for m in mc.PATHS_FLIP_MASKS:
        with_bt = m | pref.PATH_BT
        assert pref.vflip(with_bt) & 0x07 == 0x07
        disp, vol = _volume(ctx, L, R, args, with_bt)
        dispf, volf = _volume(ctx, Lf, Rf, args, pref.vflip(with_bt))
        assert np.array_equal(volf[:, ::-1], vol), hex(with_bt)
        assert np.array_equal(dispf[::-1], disp), hex(with_bt)
        assert 0.2 < float((disp == 16 * (args[0] - 1)).mean()) < 0.8, hex(with_bt)
        if pref.vflip(with_bt) != with_bt:   # the unturned mask on the turned pair is another volume: directions are told apart
            assert not np.array_equal(_volume(ctx, Lf, Rf, args, with_bt)[1][:, ::-1], vol), hex(with_bt)
        if m != with_bt:
            added = pref.vflip(m & 0xF0)
            delta = _volume(ctx, L, R, args, m)[1] - base
            assert delta.any() and np.array_equal((_volume(ctx, Lf, Rf, args, 0x07 | added)[1] - basef)[:, ::-1], delta), hex(m)
            assert not np.array_equal((_volume(ctx, Lf, Rf, args, m)[1] - basef)[:, ::-1], delta), hex(m)


# ---------------------------------------------------------------- e. padded views and launches
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("Wn", [97, 129])
def test_sgbm_paths_padded_views(ctx, Wn, cn):
    Hn = 31
    Lw, Rw = mc.textured(Hn, Wn + 37, cn, seed=Wn, D=32)
    L, R = Lw[:, 5:5 + Wn], Rw[:, 5:5 + Wn]            # padded rows: step = (Wn + 37) * cn
    assert L.strides[0] == (Wn + 37) * cn and not L.flags["C_CONTIGUOUS"]
    args = (1, 32, 7, 8 * cn * 49, 32 * cn * 49, 1, 10, 10, 20, 2)
    want = _check(ctx, L, R, *args, pref.PATHS_HH)
    assert (want["disp"] != 0).any()
    flat = ctx.sgbm_paths(np.ascontiguousarray(L), np.ascontiguousarray(R), *args, paths=pref.PATHS_HH)
    # a padded int16 output: rows of Wn + 3 shorts, the padding untouched
    out = np.full((Hn, Wn + 3), 12345, np.int16)
    li, _ = asw._image(L)
    ri, _ = asw._image(R)
    assert li.step == (Wn + 37) * cn
    oi = _lib.AswImage(out.ctypes.data, Hn, Wn, 1, 3, (Wn + 3) * 2)
    rc = _lib.lib().asw_sgbm(ctx._h, C.byref(li), C.byref(ri), C.byref(oi), *args, asw._SGBM_MODE_PATHS | pref.PATHS_HH, None, 0)
    assert rc == 0
    assert np.array_equal(out[:, :Wn], flat) and (out[:, Wn:] == 12345).all()
    assert np.array_equal(flat, want["disp"])


def test_aggregate_launches_count_the_line_geometries(ctx):
    L, R = _textured(20, 64, 16, 3, seed=3)
    for m, lines in ((0x07, 0), (0x0F, 1), (0x17, 1), (0x47, 1), (0x57, 1), (0x37, 2), (0xA7, 1), (0xFF, 3)):
        # columns (bottom->top), diagonals (TLBR, BRTL), anti-diagonals (TRBL, BLTR): one launch per geometry in the mask
        assert lines == bool(m & pref.PATH_BT) + bool(m & (pref.PATH_TLBR | pref.PATH_BRTL)) + bool(m & (pref.PATH_TRBL | pref.PATH_BLTR))
        ctx.sgbm_paths(L, R, 0, 16, 5, 100, 400, *FULL, paths=m)
        assert ctx.timing()["aggregate_launches"] == 2 + lines, hex(m)
