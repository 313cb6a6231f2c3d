"""The scaled domain of k_asw_bilateral_xq (csrc/k_bilateral_xq.hip), restated on the CPU: weights staged x 2^60, the cost
sample |gL - gR| as the f64 denormal c * 2^-1074, E = ldexp(num', 954) / ldexp(den', -120).  Every sum must be bit-equal to
the reference's unscaled one whenever the nonzero weight products are >= 2^-68 (the host's guard, bilateral_xq_lut_ok).

numpy has no fma; `num + ab * c` is the same operation here because every product is exact (a 24-bit by 8-bit significand,
and in the scaled domain a nonzero product is >= 2^-1022 with no bit below 2^-1045), so only the addition rounds."""
import numpy as np

SCALE = 60          # XQ_LUT_SCALE_LOG2
GUARD = 2.0 ** -68  # smallest nonzero weight product the scaled domain admits


def lut_classic(gamma_c, gamma_g, win=15):
    """The host's weight LUT (asw_methods.hip, M.cpp:1065): float32 k * exp(-(dc / gamma_c + dist / gamma_g)), one row per
    distance class of the window, plus the all-zero class."""
    h = win // 2
    r2s = sorted({i * i + j * j for i in range(-h, h + 1) for j in range(-h, h + 1) if (i, j) != (0, 0)})
    rows = [np.float32(3.0 * np.exp(-(np.arange(256) / gamma_c + np.sqrt(r2) / gamma_g))) for r2 in r2s]
    return np.concatenate(rows + [np.zeros(256, np.float32)]).astype(np.float32)


def lut_ok(lut):
    """Restatement of bilateral_xq_lut_ok."""
    lut = lut.astype(np.float64)
    nz = lut[lut > 0]
    return nz.min() ** 2 >= GUARD and lut.max() ** 2 < 2.0 ** (128 - 2 * SCALE - 1)


def sums_unscaled(wl, wr, c):
    num = den = 0.0
    for a, b, ci in zip(wl, wr, c):
        ab = np.float64(np.float32(a) * np.float32(b))
        num = num + ab * np.float64(ci)
        den = den + ab
    with np.errstate(invalid="ignore"):  # 0 / 0 when every ab is 0, as in the reference
        return np.float64(num), np.float64(den), np.float64(num) / np.float64(den)


def sums_scaled(wl, wr, c):
    wls = np.ldexp(np.asarray(wl, np.float32), SCALE).astype(np.float32)
    wrs = np.ldexp(np.asarray(wr, np.float32), SCALE).astype(np.float32)
    cs = np.asarray(c, np.uint64).view(np.float64)  # low word |gL - gR|, high word 0: c * 2^-1074
    num = den = np.float64(0.0)
    for a, b, ci in zip(wls, wrs, cs):
        ab = np.float64(a * b)  # float32 product
        num = num + ab * ci
        den = den + ab
    with np.errstate(invalid="ignore"):
        return num, den, np.ldexp(num, 954) / np.ldexp(den, -120)


def check_equal(wl, wr, c):
    n0, d0, e0 = sums_unscaled(wl, wr, c)
    n1, d1, e1 = sums_scaled(wl, wr, c)
    assert np.ldexp(n1, 954).tobytes() == n0.tobytes(), (n0, np.ldexp(n1, 954))
    assert np.ldexp(d1, -120).tobytes() == d0.tobytes(), (d0, np.ldexp(d1, -120))
    assert e1.tobytes() == e0.tobytes(), (e0, e1)


def test_reference_gammas_pass_the_guard_and_low_gamma_c_does_not():
    assert lut_ok(lut_classic(30, 20))   # the benchmark's gammas: smallest product about 2^-23
    assert lut_ok(lut_classic(20, 30))
    assert lut_ok(lut_classic(10.6, 20))  # just above the bound (tests/test_gpu_bilateral_xq_guard.py)
    assert not lut_ok(lut_classic(10.5, 20))
    assert not lut_ok(lut_classic(7.5, 11.25))


def test_random_window_sums_bit_equal():
    rng = np.random.default_rng(20261016)
    for gc, gg in ((30, 20), (20, 30), (10.6, 20), (255, 1), (30, 2)):
        lut = lut_classic(gc, gg)
        assert lut_ok(lut)
        for _ in range(150):
            n = 224
            wl = lut[rng.integers(0, lut.size, n)]
            wr = lut[rng.integers(0, lut.size, n)]
            c = rng.integers(0, 256, n)
            check_equal(wl, wr, c)


def test_adversarial_sums_bit_equal():
    g = np.float32(2.0 ** -34)  # both weights at the guard: ab = 2^-68, ab * c * 2^-954 = c * 2^-1022
    g1 = np.nextafter(g, np.float32(1))
    rng = np.random.default_rng(7)
    cases = [
        ([g] * 224, [g] * 224, [1] * 224),                        # the smallest products, the smallest nonzero cost
        ([g1] * 224, [g1] * 224, [255] * 224),                    # a full 24-bit product at the bound
        ([g] * 112 + [np.float32(3)] * 112, [g] * 112 + [np.float32(3)] * 112, list(range(224))),  # tiny then the largest
        ([np.float32(3)] * 112 + [g] * 112, [np.float32(3)] * 112 + [g] * 112, [255] * 224),           # largest then tiny
        ([0] * 224, [g] * 224, rng.integers(0, 256, 224)),        # ab = 0 everywhere: 0 / 0
        ([g] * 224, [g] * 224, [0] * 224),                        # c = 0 everywhere
        ([0, g, 0, g1] * 56, [g1, g, np.float32(3), g] * 56, [0, 255, 17, 0] * 56),
    ]
    for wl, wr, c in cases:
        wl, wr = np.asarray(wl, np.float32), np.asarray(wr, np.float32)
        ab = wl.astype(np.float64) * wr.astype(np.float64)
        assert np.all((ab == 0) | (ab >= GUARD))
        n0, d0, e0 = sums_unscaled(wl, wr, c)
        n1, d1, e1 = sums_scaled(wl, wr, c)
        assert np.ldexp(n1, 954).tobytes() == n0.tobytes() and np.ldexp(d1, -120).tobytes() == d0.tobytes()
        assert e1.tobytes() == e0.tobytes() or (np.isnan(e0) and np.isnan(e1))


def test_below_the_guard_the_domains_can_differ():
    # a 24-bit product of 2^-100: its scaled form needs bits below 2^-1074, so the denormal product rounds -- the reason the
    # host sends such LUTs to the one-kernel form
    wl, wr = [np.float32((1 + 2.0 ** -23) * 2.0 ** -50)], [np.float32(2.0 ** -50)]
    n0, _, _ = sums_unscaled(wl, wr, [1])
    n1, _, _ = sums_scaled(wl, wr, [1])
    assert np.ldexp(n1, 954) != n0
