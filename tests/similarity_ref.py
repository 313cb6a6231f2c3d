"""The literal second restatement of computeSimilarity ("TAD C+G", M.cpp:415-487, the only branch that can execute), line by line
over tests/cvlite.py's OpenCV primitives.  TEST INFRASTRUCTURE ONLY: tests/test_oracle_second.py pins the oracle to it, and
tests/test_geometry_cases_cpu.py does so again over the parameter grid of the launch-geometry tests."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvlite as cv  # noqa: E402

F32 = np.float32

SCHARR_X = ((-3, 0, 3), (-10, 0, 10), (-3, 0, 3))    # M.cpp:446-448


def similarity_literal(leftImg, rightImg, regularity, thresC, thresG, minD, numD):
    H, W = leftImg.shape[:2]
    max_offset = minD + numD - 1                                                   # :422-423
    regularityR = 1 - regularity                                                   # :435
    right_border = cv.copyMakeBorder(rightImg, 0, 0, max_offset, 0, cv.BORDER_REFLECT)   # :442
    sobel_x_left = cv.filter2D_f32(leftImg, SCHARR_X)                              # :449
    sobel_x_right = cv.filter2D_f32(right_border, SCHARR_X)                        # :450 (gradient of the PADDED image)
    out = []
    for offset in range(minD, max_offset + 1):                                     # :452
        x0 = max_offset - offset
        color_temp = cv.absdiff(leftImg, right_border[:, x0:x0 + W])               # :455
        c = [color_temp[..., k] for k in range(3)]                                 # :457-458
        color_ = cv.addWeighted_u8(cv.add_u8(c[0], c[1]), 1.0 / 3.0, c[2], 1.0 / 3.0)   # :459 (App. A-4)
        compare_thresC = cv.compare_gt(color_, thresC)                             # :461-462
        m1 = cv.mul_u8(color_, compare_thresC, 1.0 / 255.0)                        # color_.mul(compare/255)
        curCost_color = cv.addWeighted_u8(m1, 1.0, compare_thresC, thresC * (1.0 / 255.0)).astype(F32)   # :464-465
        g = cv.absdiff(sobel_x_left, sobel_x_right[:, x0:x0 + W])                  # :470
        curGridient_ = cv.addWeighted_f32(g[..., 0] + g[..., 1], 1.0 / 3.0, g[..., 2], 1.0 / 3.0)   # :473
        compare_thresG = cv.compare_gt(curGridient_, thresG)                       # :474-475
        bitImg = cv.scale_u8(compare_thresG, 1.0 / 255.0)                          # :477
        bit_not_img = np.bitwise_not(bitImg)                                       # :479  (255 / 254, App. B-6)
        curCost_grident = bit_not_img.astype(F32) * F32(thresG) + curGridient_ * bitImg.astype(F32)   # :482
        out.append(curCost_color * F32(regularityR) + curCost_grident * F32(regularity))            # :484
    return np.stack(out)
