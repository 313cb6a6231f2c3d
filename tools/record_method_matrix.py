"""Which status a call returns, per method and per entry path -- recorded once, replayed by tests/test_gpu_method_matrix.py.

    python tools/record_method_matrix.py            # writes tests/golden/method_matrix.json (needs the GPU)
    python tools/record_method_matrix.py OUT.json

matrix() runs one table of calls through the package's public API (and, where the wrappers cannot express a fault -- a short
volume buffer, an output map of the wrong type or shape -- through the package's own ctypes binding) and returns
{row key: [fields]}.  A valid call records status 0, the number of volume planes it handed back (checked against
asw_volume_planes), timing()["aggregate_launches"] and a CRC-32 of the disparity bytes; a refused call records its status.

The selector table: algorithm values 0..12, one cross_algorithm() value and one invalid encoding; each through stereoMatching, the
resident path and the method's own entry point where it has one; a 9 x 24 3-channel pair, numDisparity 16, winSize 5; every fault
on its own, then the pairs of faults whose order of checks decides the status.  The disp16 table: sgbm, sgbm_paths, stereoBM,
getDisparity_BM, filterSpeckles on an 11 x 40 1-channel pair, numDisparities 16, block 5.

The golden file is a recording of the commit BEFORE a change to the host layer; regenerating it to make the test pass defeats it."""
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "method_matrix.json")

H, W, NUMD, WIN = 9, 24, 16, 5
H16, W16, BLOCK = 11, 40, 5

# case -> the arguments it replaces (win, ch, dt, minD, numD); the others keep their valid values
CASES = [
    ("valid", {}),
    ("even_win", dict(win=4)),
    ("win0", dict(win=0)),
    ("one_channel", dict(ch=1)),
    ("disptype2", dict(dt=2)),
    ("right", dict(dt=1)),
    ("minD-1", dict(minD=-1)),
    ("numD0", dict(numD=0)),
    ("numD15", dict(numD=15)),
    # the ordering probes: two faults in one call
    ("even_win+one_channel", dict(win=4, ch=1)),
    ("right+even_win", dict(dt=1, win=4)),
    ("numD0+even_win", dict(numD=0, win=4)),
]


def _crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def _pairs():
    rng = np.random.RandomState(20261018)
    L = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    R = np.roll(L, -3, axis=1)
    R[:, -3:] = rng.randint(0, 256, (H, 3, 3)).astype(np.uint8)
    L16 = rng.randint(0, 256, (H16, W16)).astype(np.uint8)
    R16 = np.roll(L16, -4, axis=1)
    return L, R, L16, R16


def _status(asw, call):
    """(status, result): a silent return leaves its status in last_status(), anything else raises AswError."""
    try:
        out = call()
    except asw.AswError as e:
        return e.status, None
    return asw.last_status(), out


def _planes(asw, alg, numD):
    return asw.Context._candidates(alg, numD)


def _valid_fields(asw, ctx, alg, numD, disp, vol):
    """[0, planes handed back, planes of asw_volume_planes, aggregate_launches, crc of the disparity]"""
    return [0, None if vol is None else int(vol.shape[0]), int(_planes(asw, alg, numD)) if alg is not None else None,
            int(ctx.timing()["aggregate_launches"]), _crc(disp)]


def _method_calls(asw, ctx):
    """algorithm value -> f(L, R, dt, win, minD, numD, want_volume): the method's own entry point (an argument the entry point
    lacks is dropped: the bilateral grid has no window, computeNCC no volume)."""
    A = asw.StereoMatchingAlgorithms
    return {
        int(A.BM): lambda L, R, dt, w, m, n, v: ctx.getDisparity_BM(L, R, w, m, n),
        int(A.SGBM): lambda L, R, dt, w, m, n, v: ctx.getDisparity_SGBM(L, R, w, m, n),
        int(A.ADAPTIVE_WEIGHT): lambda L, R, dt, w, m, n, v: ctx.computeAdaptiveWeight(L, R, 30, 20, dt, w, m, n, v),
        int(A.ADAPTIVE_WEIGHT_8DIRECT): lambda L, R, dt, w, m, n, v: ctx.computeAdaptiveWeight_direct8(L, R, dt, w, m, n, v),
        int(A.ADAPTIVE_WEIGHT_GEODESIC): lambda L, R, dt, w, m, n, v: ctx.computeAdaptiveWeight_geodesic(L, R, dt, w, m, n, v),
        int(A.ADAPTIVE_WEIGHT_BILATERAL_GRID):
            lambda L, R, dt, w, m, n, v: ctx.computeAdaptiveWeight_bilateralGrid(L, R, dt, 10, 10, m, n, v),
        int(A.ADAPTIVE_WEIGHT_BLO1): lambda L, R, dt, w, m, n, v: ctx.computeAdaptiveWeight_BLO1(L, R, dt, 0.015, w, m, n, v),
        int(A.ADAPTIVE_WEIGHT_GUIDED_FILTER): lambda L, R, dt, w, m, n, v: ctx.computeAdaptiveWeight_GuidedF(L, R, dt, 1e-6, w, m, n, v),
        int(A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2):
            lambda L, R, dt, w, m, n, v: ctx.computeAdaptiveWeight_GuidedF_2(L, R, dt, 1e-6, w, m, n, v),
        int(A.ADAPTIVE_WEIGHT_GUIDED_FILTER_3):
            lambda L, R, dt, w, m, n, v: ctx.computeAdaptiveWeight_GuidedF_3(L, R, dt, 1e-6, w, m, n, v),
        int(A.ADAPTIVE_WEIGHT_MEDIAN):
            lambda L, R, dt, w, m, n, v: ctx.computeAdaptiveWeight_WeightedMedian(L, R, dt, w, 10, 10, m, n, v),
        int(A.NCC): lambda L, R, dt, w, m, n, v: ctx.computeNCC(L, R, dt, w, m, n),
        int(A.ADAPTIVE_WEIGHT_CROSS): lambda L, R, dt, w, m, n, v: ctx.computeAdaptiveWeight_cross(L, R, dt, 20, 20, w, m, n, v),
    }


def _selector_rows(asw, ctx, L, R, out):
    from aswstereomatch_amd import _lib

    lib = _lib.lib()
    algs = [(str(a), a) for a in range(13)] + [("cross(12,30)", asw.cross_algorithm(12, 30)), ("cross(300,20)", asw.cross_algorithm(300, 20))]
    own = _method_calls(asw, ctx)
    for aname, alg in algs:
        for cname, c in CASES:
            win, dt, minD, numD = c.get("win", WIN), c.get("dt", 0), c.get("minD", 0), c.get("numD", NUMD)
            l, r = (L, R) if c.get("ch", 3) == 3 else (np.ascontiguousarray(L[:, :, 1]), np.ascontiguousarray(R[:, :, 1]))
            for vol in (False, True):
                tag = "%s/%s/%s" % (aname, cname, "vol" if vol else "novol")
                # 1. stereoMatching
                st, res = _status(asw, lambda: ctx.stereoMatching(l, r, dt, alg, win, minD, numD, return_cost_volume=vol))
                if st == 0:
                    disp, v = res if vol else (res, None)
                    out["host/" + tag] = _valid_fields(asw, ctx, alg, numD, disp, v)
                else:
                    out["host/" + tag] = [st]
                # 2. the resident path
                ctx.upload_pair(0, l, r)
                st, _ = _status(asw, lambda: ctx.match_resident(0, dt, alg, win, minD, numD, keep_volume=vol))
                if st == 0:
                    launches = int(ctx.timing()["aggregate_launches"])
                    disp = ctx.download_disparity(0, l.shape[:2])
                    planes = int(_planes(asw, alg, numD))
                    # asw_download_volume takes the exact size only: success pins the plane count, anything else its status
                    vst, _ = _status(asw, lambda: ctx.download_volume(0, (planes,) + l.shape[:2]))
                    out["resident/" + tag] = [0, planes if vst == 0 else "download status %d" % vst, planes, launches, _crc(disp)]
                else:
                    out["resident/" + tag] = [st]
                # 3. the method's own entry point
                if alg in own:
                    st, res = _status(asw, lambda: own[alg](l, r, dt, win, minD, numD, vol))
                    if st == 0:
                        disp, v = res if isinstance(res, tuple) else (res, None)
                        out["own/" + tag] = _valid_fields(asw, ctx, alg, numD, disp, v)
                    else:
                        out["own/" + tag] = [st]
        # a cost-volume buffer one float short, through stereoMatching's C entry point (the wrapper sizes its own)
        planes = int(_planes(asw, alg, NUMD))
        li, la = asw._image(L)
        ri, ra = asw._image(R)
        disp = np.zeros((H, W), np.float32)
        di, _ = asw._image(disp, 5)
        for short in (1, 0):
            buf = np.zeros(planes * H * W - short, np.float32)
            rc = lib.asw_stereo_match(ctx._h, C.byref(li), C.byref(ri), C.byref(di), 0, int(alg), WIN, 0, NUMD,
                                      buf.ctypes.data_as(C.c_void_p), buf.size)
            out["host/%s/volume_%s" % (aname, "short" if short else "exact")] = [int(rc)]


def _disp16_rows(asw, ctx, L, R, out):
    from aswstereomatch_amd import _lib

    lib = _lib.lib()

    def rec(key, call, alg=None):
        st, res = _status(asw, call)
        if st != 0:
            out[key] = [st]
            return None
        disp, v = res if isinstance(res, tuple) else (res, None)
        out[key] = [0, None if v is None else int(v.shape[0]), None, int(ctx.timing()["aggregate_launches"]), _crc(disp)]
        return disp

    for n, tag in ((NUMD, "valid"), (15, "numD15")):
        for vol in (False, True):
            v = "vol" if vol else "novol"
            d16 = rec("sgbm/%s/%s" % (tag, v), lambda: ctx.sgbm(L, R, 0, n, BLOCK, return_cost_volume=vol))
            rec("sgbm_paths/%s/%s" % (tag, v), lambda: ctx.sgbm_paths(L, R, 0, n, BLOCK, paths=asw.SGBM_PATHS_HH, return_cost_volume=vol))
            rec("stereoBM/%s/%s" % (tag, v), lambda: ctx.stereoBM(L, R, 0, n, BLOCK, return_cost_volume=vol))
        rec("getDisparity_BM/%s" % tag, lambda: ctx.getDisparity_BM(L, R, BLOCK, 0, n))
        if d16 is not None:
            rec("filterSpeckles/%s" % tag, lambda: ctx.filterSpeckles(d16, -16, 20, 16))
    # an output map of the wrong type (8-bit where int16 is due, int16 where 8-bit is due) or the wrong shape, alone and together
    # with numDisparities 15: the wrappers allocate their own map, so these go through the binding
    li, la = asw._image(L)
    ri, ra = asw._image(R)
    maps = {
        "u8": asw._image(np.zeros((H16, W16), np.uint8), 0),
        "s16": asw._image(np.zeros((H16, W16), np.int16), 3),
        "u8_short": asw._image(np.zeros((H16 - 1, W16), np.uint8), 0),
        "s16_short": asw._image(np.zeros((H16 - 1, W16), np.int16), 3),
    }
    for n in (NUMD, 15):
        for mname, (mi, _keep) in maps.items():
            m = C.byref(mi)
            if mname != "s16":
                out["sgbm/map_%s/numD%d" % (mname, n)] = [int(lib.asw_sgbm(ctx._h, C.byref(li), C.byref(ri), m, 0, n, BLOCK, 0, 0, 0, 0, 0, 0, 0,
                                                                          asw.MODE_SGBM_3WAY, None, 0))]
                out["sgbm_paths/map_%s/numD%d" % (mname, n)] = [int(lib.asw_sgbm(ctx._h, C.byref(li), C.byref(ri), m, 0, n, BLOCK, 0, 0, 0, 0, 0,
                                                                                0, 0, 0x40000000 | asw.SGBM_PATHS_HH, None, 0))]
                out["stereoBM/map_%s/numD%d" % (mname, n)] = [int(lib.asw_stereo_bm(ctx._h, C.byref(li), C.byref(ri), m, 0, n, BLOCK, 1, 9, 31, 10,
                                                                                   15, 0, 0, -1, None, 0))]
            if mname != "u8":
                out["getDisparity_BM/map_%s/numD%d" % (mname, n)] = [int(lib.asw_get_disparity_bm(ctx._h, C.byref(li), C.byref(ri), m, BLOCK, 0, n))]
    out["filterSpeckles/map_u8"] = [int(lib.asw_filter_speckles(ctx._h, C.byref(maps["u8"][0]), -16, 20, 16))]


def matrix(asw):
    L, R, L16, R16 = _pairs()
    ctx = asw.Context(0)
    out = {}
    try:
        _selector_rows(asw, ctx, L, R, out)
        _disp16_rows(asw, ctx, L16, R16, out)
    finally:
        ctx.close()
    return out


def main(argv):
    sys.path.insert(0, ROOT)
    import aswstereomatch_amd as asw

    path = argv[1] if len(argv) > 1 else GOLDEN
    rows = matrix(asw)
    with open(path, "w") as fh:
        json.dump(rows, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("%d rows -> %s" % (len(rows), path))


if __name__ == "__main__":
    main(sys.argv)
