// Sub-pixel disparity (the rule is this library's own): after a method's winner-take-all, every pixel
// whose winner has two finite, not smaller neighbours in the aggregated volume moves by the vertex of the parabola / of the
// equiangular V through the three costs.  One thread per pixel: the integer map is read coalesced and overwritten in place,
// the three costs are gathers from the d-major volume (one 64-byte sector each where neighbouring pixels share a winner).
// Every operation is one IEEE f64 operation (the library is built with -ffp-contract=off; f64 division is correctly rounded),
// so tests/subpixel_ref.py restates it to the bit.
#include "asw_internal.h"

namespace {

template <int MODE>
__global__ __launch_bounds__(256) void k_subpixel(const float* __restrict__ vol, int n, size_t plane, int minD,
                                                  float* __restrict__ disp)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= plane) return;
    const float d = disp[i];
    // 0 < k < n - 1, tested on the float: NaN, inf and the literal 0 of a pixel without a winner (minD > 0) never index the volume
    if (!(d > (float)minD && d < (float)(minD + n - 1))) return;
    const int k = (int)d - minD;
    if (k < 1 || k > n - 2) return;
    const double c0 = (double)vol[(size_t)k * plane + i];
    const double cm = (double)vol[(size_t)(k - 1) * plane + i];
    const double cp = (double)vol[(size_t)(k + 1) * plane + i];
    const double big = 1.7976931348623157e308;
    if (!(fabs(c0) <= big && fabs(cm) <= big && fabs(cp) <= big)) return;  // NaN compares false
    if (!(cm >= c0 && cp >= c0)) return;
    const double den = MODE == ASW_DISPARITY_SUBPIXEL_PARABOLA ? (cm - c0) + (cp - c0) : fmax(cm, cp) - c0;
    if (!(den > 0.0)) return;
    double off = (cm - cp) / (2.0 * den);
    off = off < -0.5 ? -0.5 : (off > 0.5 ? 0.5 : off);
    disp[i] = (float)((double)d + off);
}

}  // namespace

int launch_subpixel(hipStream_t s, int mode, const float* vol, int n, int H, int W, int minD, float* disp)
{
    if (!vol || !disp || n < 1) return ASW_ERR_BAD_ARGUMENT;
    const size_t plane = (size_t)H * W;
    const dim3 grid((unsigned)((plane + 255) / 256));
    if (mode == ASW_DISPARITY_SUBPIXEL_PARABOLA)
        ASW_TRY(ASW_LAUNCH(k_subpixel<ASW_DISPARITY_SUBPIXEL_PARABOLA>, grid, dim3(256), 0, s, vol, n, plane, minD, disp));
    else if (mode == ASW_DISPARITY_SUBPIXEL_EQUIANGULAR)
        ASW_TRY(ASW_LAUNCH(k_subpixel<ASW_DISPARITY_SUBPIXEL_EQUIANGULAR>, grid, dim3(256), 0, s, vol, n, plane, minD, disp));
    else
        return ASW_ERR_BAD_ARGUMENT;
    return ASW_OK;
}
