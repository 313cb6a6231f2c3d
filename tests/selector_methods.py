"""The selector methods that arrive as an encoded `algorithm` value with a per-method wrapper (cross-based regions, AD-Census, two-pass
ASW), one descriptor each: what tests/test_gpu_selector_contract.py, tests/test_cpp_shim_selector.py and the legs of
tools/fuzz_parity.py vary between them, and nothing else.  A new method of this kind is a new row of METHODS.

Every callable takes the method's parameters as one tuple `params`, in the order of encode():
    call(ctx, L, R, dt, params, win, minD, numD, **kw)   the per-method wrapper, in its own argument order
    want(ctx, L, R, dt, params, win, minD, numD)         -> (volume, map) of the restatement
The *_input fields build (L, R, win, numD); rows of parameters are spelled out, never derived."""
import os
import sys
from types import SimpleNamespace

import numpy as np

import aswstereomatch_amd as asw
from aswstereomatch_amd.synth import make_pair

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adcensus_ref as ac  # noqa: E402
import cross_ref as cr  # noqa: E402
import twopass_ref as tp  # noqa: E402

CROSS = asw.StereoMatchingAlgorithms.ADAPTIVE_WEIGHT_CROSS
XA, ADC, TPA = asw.cross_algorithm, asw.adcensus_algorithm, asw.twopass_algorithm
TOP = tp.max_window()


def region_views(H, W, cn, D, seed=None, pad=0):
    """a region_pair of small cells, 1 or 3 channels; pad > 0: views whose rows carry padding"""
    L, R, _ = cr.region_pair(H, W + pad, max(2, D), H * 1000 + W if seed is None else seed, (5, 7), 0.12, block=8)
    if cn == 1:
        L, R = np.ascontiguousarray(L[:, :, 1]), np.ascontiguousarray(R[:, :, 1])
    return L[:, :W], R[:, :W]


def _region_case_1():
    H, W, D, cell, seed, amp, win = cr.REGION_CASES[1]
    return cr.region_pair(H, W, D, seed, cell, amp)[:2] + (win, D)


def _region_batch():
    H, W, D, cell, seed, amp, win = cr.REGION_CASES[1]
    return [_region_case_1()[:2]] + [cr.region_pair(H, W, D, s, (9, 13), 0.12)[:2] for s in (201, 202)], win, D


def _cross_want(ctx, L, R, dt, params, win, minD, numD):
    e = np.stack(ctx.computeAD(L, R, dt, minD, numD))  # pinned to the oracle elsewhere: its border rule is not stated a second time
    return cr.aggregate(e, cr.arms(R if int(dt) else L, params[0], win // 2), params[1], minD)[2:]


def _twopass_want(ctx, L, R, dt, params, win, minD, numD):
    gL, gR = (ctx.bgr2gray(L), ctx.bgr2gray(R)) if L.ndim == 3 else (L, R)  # pinned to the oracle elsewhere
    return tp.twopass(gL, gR, params[0], params[1], win, minD, numD, int(dt))[1:]


_XOK, _AOK, _TOK = XA(20, 20), ADC(20, 10, 30), TPA(30, 20)
_REGION_STATUS = lambda: cr.region_pair(20, 70, 12, 8, (9, 13), 0.16)[:2]  # noqa: E731

METHODS = [
    SimpleNamespace(
        name="cross", ref=cr, encode=XA, default=(20, 20), equivalents=(CROSS, 12, _XOK),
        call=lambda ctx, L, R, dt, p, win, minD, numD, **kw: ctx.computeAdaptiveWeight_cross(L, R, dt, *p, win, minD, numD, **kw),
        binding=asw.computeAdaptiveWeight_cross,
        want=_cross_want, planes=lambda numD: numD, other_plain=None,
        forms_input=_region_case_1, subpixel_input=_region_case_1, refined_input=_region_case_1, forms_alt=(7, 33),
        batch_input=lambda: ([cr.region_pair(40, 150, 12, 200 + i, (9, 13), 0.12)[:2] for i in range(5)], 15, 12),
        batch_algs=((CROSS, (20, 20)), (_XOK, (20, 20)), (XA(3, 9), (3, 9))),
        subpixel_rows=((CROSS, (20, 20), 0), (XA(12, 40), (12, 40), 3)),                       # alg, params, minD
        refined_rows=((CROSS, (20, 20), 0, 15, 150.0), (XA(10, 30), (10, 30), 3, 7, 60.0)),    # alg, params, minD, refine window, gamma_c
        launches_match=3, launches_refined=6, first_refused_window=37, even_window_above_top=None,
        status_input=_REGION_STATUS,
        bad_algs=(XA(256, 1), XA(5, 0), XA(-1, 7), 0x40000000 | 12, _XOK | 0x02000000, _XOK | 0x20000000),
        unsupported_algs=((_XOK & ~0xFF) | 11, (_XOK & ~0xFF) | 2, _XOK & ~0xFF, (_XOK & ~0xFF) | 13),
        bad_wrapper_params=(20, 256),
        sweep_seed=20262, sweep_count=100,
        # the C++ demo: three good rows (right, params, win, minD) with selector_same against the default encoding, and the throwing
        # rows (params, win)
        shim_input=lambda: cr.region_pair(37, 130, 17, 3, (9, 13), 0.12)[:2],
        shim_good=((0, (20, 20), 15, 0, 1), (1, (20, 20), 7, 3, 1), (0, (5, 60), 15, 0, 0)),
        shim_throwing=(((20, 0), 15), ((300, 20), 15), ((20, 20), 37)),
    ),
    SimpleNamespace(
        name="adcensus", ref=ac, encode=ADC, default=(20, 10, 30), equivalents=(_AOK,),
        call=lambda ctx, L, R, dt, p, win, minD, numD, **kw: ctx.computeAdaptiveWeight_adcensus(L, R, dt, *p, win, minD, numD, **kw),
        binding=asw.computeAdaptiveWeight_adcensus,
        want=lambda ctx, L, R, dt, p, win, minD, numD: ac.match(L, R, int(dt), *p, win, minD, numD)[2:],
        planes=lambda numD: numD, other_plain=12,  # the plain entry 12 is another method
        forms_input=_region_case_1, subpixel_input=_region_case_1, refined_input=_region_case_1, forms_alt=(7, 5, 12),
        batch_input=_region_batch,
        batch_algs=((ADC(), (20, 10, 30)), (ADC(3, 17, 45), (3, 17, 45))),
        subpixel_rows=((ADC(), (20, 10, 30), 0), (ADC(12, 5, 12), (12, 5, 12), 3)),
        refined_rows=((ADC(), (20, 10, 30), 0, 15, 150.0), (ADC(10, 17, 45), (10, 17, 45), 3, 7, 60.0)),
        launches_match=3, launches_refined=6, first_refused_window=37, even_window_above_top=None,
        status_input=_REGION_STATUS,
        bad_algs=(_AOK & ~(0x1F << 24), _AOK & ~(0xFF << 16), ADC(20, 32, 30), ADC(256, 10, 30), _AOK - (1 << 32) + (1 << 31),
                  _AOK | 0x40000000),
        unsupported_algs=((_AOK & ~0xFF) | 11, (_AOK & ~0xFF) | 13),
        bad_wrapper_params=(20, 32, 30),
        sweep_seed=20263, sweep_count=100,
        shim_input=lambda: cr.region_pair(37, 130, 17, 3, (9, 13), 0.12)[:2],
        shim_good=((0, (20, 10, 30), 15, 0, 1), (1, (20, 10, 30), 7, 3, 1), (0, (5, 17, 45), 15, 0, 0)),
        shim_throwing=(((20, 0, 30), 15), ((300, 10, 30), 15), ((20, 32, 30), 15), ((20, 10, 30), 37)),
    ),
    SimpleNamespace(
        name="twopass", ref=tp, encode=TPA, default=(30, 20), equivalents=(_TOK,),
        call=lambda ctx, L, R, dt, p, win, minD, numD, **kw: ctx.computeAdaptiveWeight_twopass(L, R, *p, dt, win, minD, numD, **kw),
        binding=asw.computeAdaptiveWeight_twopass,
        want=_twopass_want, planes=lambda numD: numD + 1, other_plain=None,
        forms_input=lambda: tp.textured_pair(37, 130, 3, 4, 41) + (15, 17),
        subpixel_input=lambda: tp.textured_pair(30, 130, 3, 5, 45) + (7, 12),
        refined_input=lambda: make_pair(60, 160, 16, seed=5, block=16)[:2] + (7, 16), forms_alt=(7, 36),
        batch_input=lambda: ([tp.textured_pair(24, 150, 3, 3, 200 + i) for i in range(5)], 15, 12),
        batch_algs=((_TOK, (30, 20)), (TPA(3, 9), (3, 9))),
        subpixel_rows=((_TOK, (30, 20), 0), (TPA(12, 40), (12, 40), 3)),
        refined_rows=((_TOK, (30, 20), 0, 15, 150.0), (TPA(10, 30), (10, 30), 2, 7, 150.0)),
        launches_match=1, launches_refined=2,
        first_refused_window=TOP + 2, even_window_above_top=TOP + 1,  # the even-window check comes before the launcher's limit
        status_input=lambda: tp.textured_pair(20, 70, 3, 3, 8),
        bad_algs=(TPA(0, 20), TPA(30, 0), TPA(256, 20), TPA(30, -1), _TOK | 0x01000000, _TOK | 0x08000000, _TOK - (1 << 32) + (1 << 31)),
        unsupported_algs=((_TOK & ~0xFF) | 3, (_TOK & ~0xFF) | 12, (_TOK & ~0xFF) | 13, _TOK & ~0xFF),
        bad_wrapper_params=(30, 256),
        sweep_seed=20261, sweep_count=300,
        # every two-pass row compares with the selector at its own gammas: selector_same is 1 throughout
        shim_input=lambda: tp.textured_pair(37, 130, 3, 5, 3),
        shim_good=((0, (30, 20), 15, 0, 1), (1, (7, 36), 7, 3, 1), (0, (255, 1), 35, 0, 1)),
        shim_throwing=(((0, 20), 15), ((30, 256), 15), ((30, 20), 97)),
    ),
]
for _m in METHODS:  # the seeded cases of the method's restatement module: the sweep of the suite and the fuzz leg draw from them
    _m.random_case, _m.build_case, _m.gpu_result = _m.ref.random_case, _m.ref.build_case, _m.ref.gpu_result
