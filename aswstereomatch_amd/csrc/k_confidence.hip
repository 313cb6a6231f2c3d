// Per-pixel confidence of a disparity map (the rule is this library's own, stated in asw_mi355x.h): the
// winner's margin over the best candidate that is not one of its two neighbours, divided by the column's range.  A function of
// the volume alone: the map is only carried along into the interleaved {disparity, confidence} output.
// Every lane owns VEC consecutive pixels and walks the n planes of the d-major volume once, so neighbouring lanes read neighbouring
// addresses of each plane (VEC = 4: one dwordx4 per lane and plane).  It carries the four smallest finite (value, k) pairs of each
// pixel, ordered by value, then by k, and the largest finite value, in registers: at most two of the four are the winner's
// neighbours, so the runner-up is among them.  CONF_UNROLL planes are loaded before the first of them is ranked, which keeps that
// many loads in flight per lane.  The only inexact operation is the one f64 division (correctly rounded; -ffp-contract=off), so
// tests/confidence_ref.py restates the kernel to the bit.
#include "asw_internal.h"

namespace {

constexpr int CONF_UNROLL = 4;
constexpr float CONF_FLT_MAX = 3.402823466e+38f;

struct Ranked {
    float v[4];  // ascending; +inf = empty
    int k[4];    // the plane of v[i]; -1 = empty
    float vmax;  // largest finite value; -inf = none
};

__device__ __forceinline__ void ranked_init(Ranked& r)
{
#pragma unroll
    for (int i = 0; i < 4; i++) { r.v[i] = __builtin_inff(); r.k[i] = -1; }
    r.vmax = -__builtin_inff();
}

// planes arrive in ascending k: strict '<' puts a tie behind the entries it ties with.  NaN and +-inf never enter.
__device__ __forceinline__ void ranked_insert(Ranked& r, float c, int k)
{
    const bool finite = fabsf(c) <= CONF_FLT_MAX;
    const float lo = finite ? c : __builtin_inff();  // +inf < anything is false
    r.vmax = fmaxf(r.vmax, finite ? c : -__builtin_inff());
    const bool l0 = lo < r.v[0], l1 = lo < r.v[1], l2 = lo < r.v[2], l3 = lo < r.v[3];  // l0 => l1 => l2 => l3
    r.v[3] = l2 ? r.v[2] : (l3 ? lo : r.v[3]); r.k[3] = l2 ? r.k[2] : (l3 ? k : r.k[3]);
    r.v[2] = l1 ? r.v[1] : (l2 ? lo : r.v[2]); r.k[2] = l1 ? r.k[1] : (l2 ? k : r.k[2]);
    r.v[1] = l0 ? r.v[0] : (l1 ? lo : r.v[1]); r.k[1] = l0 ? r.k[0] : (l1 ? k : r.k[1]);
    r.v[0] = l0 ? lo : r.v[0];                 r.k[0] = l0 ? k : r.k[0];
}

__device__ __forceinline__ float ranked_confidence(const Ranked& r)
{
    if (r.k[0] < 0) return 0.0f;  // F empty
    const float c1 = r.v[0];
    float c2 = 0.0f;
    bool has = false;
#pragma unroll
    for (int i = 3; i >= 1; i--) {  // the first entry in order that is in G
        const int dk = r.k[i] - r.k[0];
        const bool in_g = r.k[i] >= 0 && (dk >= 2 || dk <= -2);
        c2 = in_g ? r.v[i] : c2;
        has = has || in_g;
    }
    if (!has || r.vmax == c1 || c2 == c1) return 0.0f;  // G empty, a flat column, a non-adjacent tie: +0
    return (float)(((double)c2 - (double)c1) / ((double)r.vmax - (double)c1));
}

template <int VEC>
__device__ __forceinline__ void load_pixels(const float* __restrict__ p, float (&c)[VEC])
{
    if constexpr (VEC == 4) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
    } else {
        c[0] = p[0];
    }
}

// VEC = 4 needs plane % 4 == 0 and 16-byte aligned vol / disp / out (launch_confidence decides); then a lane's four pixels are
// all inside the plane
template <int VEC>
__global__ __launch_bounds__(256) void k_confidence(const float* __restrict__ vol, int n, size_t plane, const float* __restrict__ disp,
                                                    float2* __restrict__ out)
{
    const size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
    if (i0 >= plane) return;
    Ranked r[VEC];
#pragma unroll
    for (int j = 0; j < VEC; j++) ranked_init(r[j]);
    const float* p = vol + i0;
    int k = 0;
    for (; k + CONF_UNROLL <= n; k += CONF_UNROLL) {
        float c[CONF_UNROLL][VEC];
#pragma unroll
        for (int u = 0; u < CONF_UNROLL; u++) load_pixels<VEC>(p + (size_t)(k + u) * plane, c[u]);
#pragma unroll
        for (int u = 0; u < CONF_UNROLL; u++)
#pragma unroll
            for (int j = 0; j < VEC; j++) ranked_insert(r[j], c[u][j], k + u);
    }
    for (; k < n; k++) {
        float c[VEC];
        load_pixels<VEC>(p + (size_t)k * plane, c);
#pragma unroll
        for (int j = 0; j < VEC; j++) ranked_insert(r[j], c[j], k);
    }
    float d[VEC];
    load_pixels<VEC>(disp + i0, d);
    if constexpr (VEC == 4) {
        float4* o = reinterpret_cast<float4*>(out + i0);
        o[0] = make_float4(d[0], ranked_confidence(r[0]), d[1], ranked_confidence(r[1]));
        o[1] = make_float4(d[2], ranked_confidence(r[2]), d[3], ranked_confidence(r[3]));
    } else {
        out[i0] = make_float2(d[0], ranked_confidence(r[0]));
    }
}

}  // namespace

int launch_confidence(hipStream_t s, const float* vol, int n, int H, int W, const float* disp, float2* out)
{
    if (!vol || !disp || !out || n < 1 || H < 1 || W < 1) return ASW_ERR_BAD_ARGUMENT;
    const size_t plane = (size_t)H * W;
    const bool aligned = (((uintptr_t)vol | (uintptr_t)disp | (uintptr_t)out) & 15) == 0;
    if (aligned && (plane & 3) == 0)
        return ASW_LAUNCH(k_confidence<4>, dim3((unsigned)((plane / 4 + 255) / 256)), dim3(256), 0, s, vol, n, plane, disp, out);
    return ASW_LAUNCH(k_confidence<1>, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, s, vol, n, plane, disp, out);
}
