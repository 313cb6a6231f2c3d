// Cross-scale cost aggregation (Zhang, Fang, Dai, Shang, Zhang, Ren, CVPR 2014): DESIGN.md section 4.18; not in the reference.
// A 2x2-mean pyramid step, the closed-form inter-scale weights, and the one pass over the finest volume that combines the levels'
// aggregated volumes and picks the winner.
#include "asw_internal.h"
#include "asw_host.h"

namespace {

// one thread per output byte: (a + b + c + d + 2) >> 2 of the 2x2 block, the last row / column repeated where the block leaves the
// image (h or w odd, h or w = 1)
__global__ __launch_bounds__(256) void k_pyramid_down(const uint8_t* __restrict__ src, int H, int W, int C, int Ho, int Wo,
                                                      uint8_t* __restrict__ dst)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, rowb = (size_t)Wo * C;
    if (i >= (size_t)Ho * rowb) return;
    const int Y = (int)(i / rowb), r = (int)(i - (size_t)Y * rowb), X = r / C, c = r - X * C;
    const int y0 = 2 * Y, y1 = min(2 * Y + 1, H - 1), x0 = 2 * X, x1 = min(2 * X + 1, W - 1);
    const uint8_t* p0 = src + (size_t)y0 * W * C + c;
    const uint8_t* p1 = src + (size_t)y1 * W * C + c;
    const int sum = (int)p0[(size_t)x0 * C] + (int)p0[(size_t)x1 * C] + (int)p1[(size_t)x0 * C] + (int)p1[(size_t)x1 * C];
    dst[i] = (uint8_t)((sum + 2) >> 2);
}

struct CombineArgs {
    float* vol;
    float* disp;
    int H, W, n, minD, nc, store;  // nc = S - 1 coarse levels
    float w[CROSS_SCALE_MAX];
    const float* cv[CROSS_SCALE_MAX - 1];
    int cW[CROSS_SCALE_MAX - 1], cminD[CROSS_SCALE_MAX - 1];
    size_t cplane[CROSS_SCALE_MAX - 1];
};

constexpr int KU = 4;  // fine planes whose loads are issued together

// VEC consecutive x of one row per lane (4: one 16-byte access per plane, rows of a multiple of 4 columns; 1: every other row).
// A lane walks k upward with its running minimum in registers (k_wta's rule) and keeps the coarse values of level s for the 2^s
// consecutive k that share the coarse plane (minD + k) >> s: a level is loaded again only when that plane changes, so an odd minD
// just makes the first group short.  Four x aligned to 4 share one coarse pixel from level 2 up and two at level 1.
template <int VEC>
__global__ __launch_bounds__(256) void k_cross_scale_combine(const CombineArgs a)
{
    constexpr int NCV = VEC == 4 ? 2 : 1;  // distinct coarse pixels a lane can meet in a level
    const int groups = a.W / VEC;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)a.H * groups) return;
    const int y = (int)(t / groups), x = (int)(t - (size_t)y * groups) * VEC;
    const size_t plane = (size_t)a.H * a.W, pix = (size_t)y * a.W + x;
    size_t cpix[CROSS_SCALE_MAX - 1];
    int cplane_at[CROSS_SCALE_MAX - 1];
    float c[CROSS_SCALE_MAX - 1][NCV];
#pragma unroll
    for (int s = 0; s < CROSS_SCALE_MAX - 1; s++) {
        cpix[s] = s < a.nc ? (size_t)(y >> (s + 1)) * a.cW[s] + (x >> (s + 1)) : 0;
        cplane_at[s] = -1;
#pragma unroll
        for (int j = 0; j < NCV; j++) c[s][j] = 0.0f;
    }
    float best[VEC], bd[VEC];
    bool any[VEC];
#pragma unroll
    for (int j = 0; j < VEC; j++) { best[j] = 3.402823466e+38f; bd[j] = 0.0f; any[j] = false; }

    for (int k0 = 0; k0 < a.n; k0 += KU) {
        float v[KU][VEC];
#pragma unroll
        for (int u = 0; u < KU; u++) {
            if (k0 + u < a.n) {
                const float* p = a.vol + (size_t)(k0 + u) * plane + pix;
                if (VEC == 4) {
                    const float4 q = *reinterpret_cast<const float4*>(p);
                    v[u][0] = q.x; v[u][1 % VEC] = q.y; v[u][2 % VEC] = q.z; v[u][3 % VEC] = q.w;
                } else
                    v[u][0] = *p;
            }
        }
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int k = k0 + u;
            if (k < a.n) {
                const int d = a.minD + k;
#pragma unroll
                for (int s = 0; s < CROSS_SCALE_MAX - 1; s++)
                    if (s < a.nc) {
                        const int pl = (d >> (s + 1)) - a.cminD[s];
                        if (pl != cplane_at[s]) {
                            const float* p = a.cv[s] + (size_t)pl * a.cplane[s] + cpix[s];
                            c[s][0] = p[0];
                            if (NCV == 2) c[s][NCV - 1] = s == 0 ? p[1] : c[s][0];  // x + 2 is the next pixel of level 1 only
                            cplane_at[s] = pl;
                        }
                    }
                float o[VEC];
#pragma unroll
                for (int j = 0; j < VEC; j++) {
                    double acc = 0.0;
                    acc += (double)a.w[0] * (double)v[u][j];
#pragma unroll
                    for (int s = 0; s < CROSS_SCALE_MAX - 1; s++)
                        if (s < a.nc) acc += (double)a.w[s + 1] * (double)c[s][VEC == 4 ? j / 2 : 0];
                    o[j] = (float)acc;
                    const bool better = any[j] ? (o[j] < best[j]) : (o[j] <= 3.402823466e+38f);  // k_wta: the first must be < DBL_MAX
                    if (better) { best[j] = o[j]; bd[j] = (float)d; any[j] = true; }
                }
                if (a.store) {
                    float* p = a.vol + (size_t)k * plane + pix;
                    if (VEC == 4)
                        *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1 % VEC], o[2 % VEC], o[3 % VEC]);
                    else
                        *p = o[0];
                }
            }
        }
    }
    if (VEC == 4)
        *reinterpret_cast<float4*>(a.disp + pix) = make_float4(bd[0], bd[1 % VEC], bd[2 % VEC], bd[3 % VEC]);
    else
        a.disp[pix] = bd[0];
}

}  // namespace

int launch_pyramid_down(hipStream_t s, const uint8_t* src, int H, int W, int C, uint8_t* dst)
{
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const size_t n = (size_t)Ho * Wo * C;
    return ASW_LAUNCH(k_pyramid_down, dim3(blocks(n, 256)), dim3(256), 0, s, src, H, W, C, Ho, Wo, dst);
}

// A w = e_0, A the S x S tridiagonal matrix of the paper (diagonal 1 + lambda at both ends and 1 + 2 lambda between,
// off-diagonals -lambda), by the Thomas algorithm: forward sweep, back substitution.  One IEEE operation per statement: a fused
// b - a * c would give other bits than the restatement's
#pragma clang fp contract(off)
void cross_scale_weights(int S, int q, float* w)
{
    const double lam = (double)q / 64.0;
    const double off = -lam;
    double cp[CROSS_SCALE_MAX], dp[CROSS_SCALE_MAX], x[CROSS_SCALE_MAX];
    for (int i = 0; i < S; i++) {
        const double b = (i == 0 || i == S - 1) ? 1.0 + lam : 1.0 + 2.0 * lam;
        const double rhs = i == 0 ? 1.0 : 0.0;
        if (i == 0) {
            cp[0] = off / b;
            dp[0] = rhs / b;
        } else {
            const double t = off * cp[i - 1];
            const double den = b - t;
            const double u = off * dp[i - 1];
            cp[i] = off / den;
            dp[i] = (rhs - u) / den;
        }
    }
    x[S - 1] = dp[S - 1];
    for (int i = S - 2; i >= 0; i--) {
        const double t = cp[i] * x[i + 1];
        x[i] = dp[i] - t;
    }
    for (int i = 0; i < S; i++) w[i] = (float)x[i];
}

int launch_cross_scale_combine(hipStream_t s, const CrossScaleLaunch& l)
{
    CombineArgs a;
    a.vol = l.vol; a.disp = l.disp; a.H = l.H; a.W = l.W; a.n = l.n; a.minD = l.minD; a.nc = l.S - 1; a.store = l.store;
    for (int i = 0; i < CROSS_SCALE_MAX; i++) a.w[i] = i < l.S ? l.w[i] : 0.0f;
    for (int i = 0; i < CROSS_SCALE_MAX - 1; i++) {
        const bool on = i < a.nc;
        a.cv[i] = on ? l.cv[i] : nullptr; a.cW[i] = on ? l.cW[i] : 0; a.cminD[i] = on ? l.cminD[i] : 0;
        a.cplane[i] = on ? (size_t)l.cH[i] * l.cW[i] : 0;
    }
    // 16-byte accesses where every row starts on one and is wide enough to fill a wavefront's worth of them
    const bool vec = l.W % 4 == 0 && l.W >= 64;
    const size_t lanes = (size_t)l.H * (vec ? l.W / 4 : l.W);
    if (vec)
        ASW_TRY(ASW_LAUNCH(k_cross_scale_combine<4>, dim3(blocks(lanes, 256)), dim3(256), 0, s, a));
    else
        ASW_TRY(ASW_LAUNCH(k_cross_scale_combine<1>, dim3(blocks(lanes, 256)), dim3(256), 0, s, a));
    return ASW_OK;
}
