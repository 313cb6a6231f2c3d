// Two-pass (separable) adaptive-support-weight aggregation + fused WTA (Wang et al. 2006; not in the reference; DESIGN.md
// section 4.16), hand-written for gfx950.
//
// The support weight w(p, q) of the classic method is replaced by w(p, p') w(p', q), p' the pixel in p's row and q's column: a
// vertical 1-D weighted pass, then a horizontal one over its sums -- 2 win taps per (pixel, candidate) instead of win^2 - 1.
// With T[r][dc] = (float)exp(-(dc / gamma_c + r / gamma_g)) (host, double, libm), xr = max(0, x - d) and clamp to the image:
//     vertical,   j = -h..h, yy = clamp(y + j):  ab = T[|j|][|gL(yy,x) - gL(y,x)|] * T[|j|][|gR(yy,xr) - gR(y,xr)|]     f32
//                                                vn += (double)ab * |gL(yy,x) - gR(yy,xr)|,  vd += (double)ab            f64
//     horizontal, i = -h..h, xx = clamp(x + i), xri = clamp(xr + i):
//                                                ab = T[|i|][|gL(y,xx) - gL(y,x)|] * T[|i|][|gR(y,xri) - gR(y,xr)|]     f32
//                                                num = num + (double)ab * vn(xx,y,d),  den = den + (double)ab * vd(xx,y,d)
// and E = num / den feeds a strict-< running minimum over d in ascending order; the volume plane is (float)E.
//
// Design:
//  * one launch: a 256-thread workgroup owns a 64x4 pixel tile and walks the candidates in chunks of DC = 8 (remainder chunks of
//    4 / 2 / 1, so no lane computes a candidate that is thrown away).  Per chunk the vertical sums of the tile and its h halo
//    columns on each side are written to LDS as {vn, vd} f64 pairs and consumed by the horizontal pass of the same workgroup:
//    they never travel through HBM;
//  * the sums lie [row][candidate][column]: the lanes of a wavefront (one tile row) read and write consecutive 16-byte words;
//  * the table T sits in LDS; the left-image weight of a tap is looked up once and shared by the DC candidates of the chunk,
//    the right-image weight once per candidate, the product is the one f32 multiply of the definition;
//  * ab * |gL - gR| is exact in f64 (24 x 8 bits), so the vertical pass may fuse it; the horizontal products are not exact and are
//    rounded before they are added (__dmul_rn / __dadd_rn: never contracted);
//  * clamp borders are reproduced by building the tiles with clamped coordinates, as k_bilateral.hip does; the right tile holds
//    the image columns clamp(sRx0 + c) and is addressed with true image columns, because the horizontal neighbours of a right
//    pixel are clamped from max(0, x - d) itself;
//  * DISPARITY_RIGHT is DISPARITY_LEFT of the x-mirrored, swapped pair: the tiles are read and the results stored mirrored.
#include <algorithm>

#include "asw_device.h"
#include "asw_internal.h"

namespace {

constexpr int TW = 64;    // tile width  = one wavefront
constexpr int TH = 4;     // tile height = waves per workgroup
constexpr int DCMAX = 8;  // widest candidate chunk

struct TwoPassParams {
    int H, W, h, minD, nD;
    int flip;  // 1: the problem is mirrored in x (DISPARITY_RIGHT)
};

constexpr __host__ __device__ int round_up16(int v) { return (v + 15) / 16 * 16; }

// LDS layout as a function of the half window h
struct Layout {
    int h, TR, LW, LWp, RWp, offV, offT, offL, offR, total;
    __host__ __device__ constexpr Layout(int h_)
        : h(h_), TR(TH + 2 * h_), LW(TW + 2 * h_), LWp(round_up16(TW + 2 * h_)), RWp(round_up16(TW + 2 * h_ + DCMAX - 1)), offV(0),
          offT(TH * DCMAX * (TW + 2 * h_) * 16), offL(TH * DCMAX * (TW + 2 * h_) * 16 + (h_ + 1) * 256 * 4),
          offR(TH * DCMAX * (TW + 2 * h_) * 16 + (h_ + 1) * 256 * 4 + (TH + 2 * h_) * round_up16(TW + 2 * h_)),
          total(TH * DCMAX * (TW + 2 * h_) * 16 + (h_ + 1) * 256 * 4 + (TH + 2 * h_) * round_up16(TW + 2 * h_) +
                (TH + 2 * h_) * round_up16(TW + 2 * h_ + DCMAX - 1))
    {
    }
};

// One chunk of DC consecutive candidates starting at candidate index c0 for the whole tile.
template <int DC>
__device__ __forceinline__ void process_chunk(const TwoPassParams& p, const uint8_t* __restrict__ gR, float* __restrict__ vol,
                                              const Layout& lay, unsigned char* smem, int c0, double& bestE, float& bestD)
{
    double2* sV = reinterpret_cast<double2*>(smem + lay.offV);
    const float* sT = reinterpret_cast<const float*>(smem + lay.offT);
    const uint8_t* sL = smem + lay.offL;
    uint8_t* sR = smem + lay.offR;
    const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int H = p.H, W = p.W, h = lay.h, LW = lay.LW, LWp = lay.LWp, RWp = lay.RWp, TR = lay.TR;
    const int RW = TW + 2 * h + DC - 1;
    const int d0 = p.minD + c0;
    // first image column of the right tile.  Never left of -h: once max(0, x - d) clamps to column 0 the tile must still hold
    // columns 0..h (the clamped pixel's horizontal neighbours).  Column c holds image column clamp(sRx0 + c); every right pixel
    // the two passes touch, X in [0, W), sits at c = X - sRx0 in [0, RW).
    const int sRx0 = max(x0 - h - (d0 + DC - 1), -h);

    __syncthreads();  // the previous chunk finished reading sR / sV
    for (int i = tid; i < TR * RW; i += 256) {
        const int r = i / RW, c = i - r * RW;
        const int yy = min(max(y0 - h + r, 0), H - 1), xx = min(max(sRx0 + c, 0), W - 1);
        sR[r * RWp + c] = gR[(size_t)yy * W + (p.flip ? W - 1 - xx : xx)];
    }
    __syncthreads();

    // vertical pass: one item per (tile row r, tile column cx incl. halo); the image column of cx is clamp(x0 - h + cx)
    for (int it = tid; it < TH * LW; it += 256) {
        const int r = it / LW, cx = it - r * LW;
        if (y0 + r >= H) continue;
        const int ximg = min(max(x0 - h + cx, 0), W - 1);
        const uint8_t* colL = sL + (r + h) * LWp + cx;
        const uint8_t* rowR = sR + (r + h) * RWp;
        const uint32_t ctrL = colL[0];
        int oR[DC];
        uint32_t ctrR[DC];
        double vn[DC], vd[DC];
#pragma unroll
        for (int dd = 0; dd < DC; dd++) {
            oR[dd] = max(0, ximg - (d0 + dd)) - sRx0;
            ctrR[dd] = rowR[oR[dd]];
            vn[dd] = 0.0; vd[dd] = 0.0;
        }
        for (int j = -h; j <= h; j++) {
            const uint32_t tj = abs(j) * 256;  // row |j| of the table; v_sad_u16 adds the gray distance to it
            const uint32_t gl = colL[j * LWp];
            const float a = sT[__builtin_amdgcn_sad_u16(gl, ctrL, tj)];
#pragma unroll
            for (int dd = 0; dd < DC; dd++) {
                const uint32_t gr = rowR[j * RWp + oR[dd]];
                const float ab = a * sT[__builtin_amdgcn_sad_u16(gr, ctrR[dd], tj)];
                const double abd = (double)ab;
                vn[dd] = __builtin_fma(abd, (double)__builtin_amdgcn_sad_u8(gl, gr, 0u), vn[dd]);  // exact product -> == vn + ab * c
                vd[dd] = vd[dd] + abd;
            }
        }
#pragma unroll
        for (int dd = 0; dd < DC; dd++) sV[(r * DC + dd) * LW + cx] = make_double2(vn[dd], vd[dd]);
    }
    __syncthreads();

    // horizontal pass: one thread per pixel of the tile
    const int x = x0 + tx, y = y0 + ty;
    if (x < W && y < H) {
        const uint8_t* rowL = sL + (ty + h) * LWp + tx + h;
        const uint8_t* rowR = sR + (ty + h) * RWp - sRx0;  // addressed with image columns
        const double2* rowV = sV + ty * DC * LW + tx + h;
        const uint32_t ctrL = rowL[0];
        int xr[DC];
        uint32_t ctrR[DC];
        double num[DC], den[DC];
#pragma unroll
        for (int dd = 0; dd < DC; dd++) {
            xr[dd] = max(0, x - (d0 + dd));
            ctrR[dd] = rowR[xr[dd]];
            num[dd] = 0.0; den[dd] = 0.0;
        }
        for (int i = -h; i <= h; i++) {
            const uint32_t ti = abs(i) * 256;
            const float a = sT[__builtin_amdgcn_sad_u16((uint32_t)rowL[i], ctrL, ti)];
#pragma unroll
            for (int dd = 0; dd < DC; dd++) {
                const uint32_t gr = rowR[min(max(xr[dd] + i, 0), W - 1)];
                const float ab = a * sT[__builtin_amdgcn_sad_u16(gr, ctrR[dd], ti)];
                const double abd = (double)ab;
                const double2 v = rowV[dd * LW + i];
                num[dd] = __dadd_rn(num[dd], __dmul_rn(abd, v.x));  // the product is rounded, then added: no FMA
                den[dd] = __dadd_rn(den[dd], __dmul_rn(abd, v.y));
            }
        }
#pragma unroll
        for (int dd = 0; dd < DC; dd++) {
            const double E = num[dd] / den[dd];
            if (vol) vol[((size_t)(c0 + dd) * H + y) * W + (p.flip ? W - 1 - x : x)] = (float)E;
            if (E < bestE) {  // ascending d, strict <
                bestE = E;
                bestD = (float)(d0 + dd);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_asw_twopass(TwoPassParams p, const uint8_t* __restrict__ gL, const uint8_t* __restrict__ gR,
                                                     const float* __restrict__ table, float* __restrict__ vol,
                                                     float* __restrict__ disp)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const Layout lay(p.h);
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int H = p.H, W = p.W, h = lay.h;

    // the weight table and the left gray tile with replicate-clamped coordinates, staged once
    float* sT = reinterpret_cast<float*>(smem + lay.offT);
    for (int i = tid; i < (h + 1) * 256; i += 256) sT[i] = table[i];
    uint8_t* sL = smem + lay.offL;
    for (int i = tid; i < lay.TR * lay.LW; i += 256) {
        const int r = i / lay.LW, c = i - r * lay.LW;
        const int yy = min(max(y0 - h + r, 0), H - 1), xx = min(max(x0 - h + c, 0), W - 1);
        sL[r * lay.LWp + c] = gL[(size_t)yy * W + (p.flip ? W - 1 - xx : xx)];
    }

    double bestE = 1.7976931348623157e308;
    float bestD = 0.0f;
    int c0 = 0;
    for (; c0 + 8 <= p.nD; c0 += 8) process_chunk<8>(p, gR, vol, lay, smem, c0, bestE, bestD);
    if (p.nD - c0 >= 4) { process_chunk<4>(p, gR, vol, lay, smem, c0, bestE, bestD); c0 += 4; }
    if (p.nD - c0 >= 2) { process_chunk<2>(p, gR, vol, lay, smem, c0, bestE, bestD); c0 += 2; }
    if (p.nD - c0 >= 1) { process_chunk<1>(p, gR, vol, lay, smem, c0, bestE, bestD); c0 += 1; }

    const int x = x0 + (tid & 63), y = y0 + (tid >> 6);
    if (x < W && y < H) disp[(size_t)y * W + (p.flip ? W - 1 - x : x)] = bestD;
}

constexpr bool lds_fits(int win) { return Layout(win / 2).total <= 160 * 1024; }

}  // namespace

int twopass_max_window()
{
    static const int last = [] {  // asked on every call of a host entry: worked out once
        int win = 1;
        while (lds_fits(win + 2)) win += 2;
        return win;
    }();
    return last;
}

int launch_twopass(hipStream_t s, const TwoPassLaunch& a)
{
    if (a.win < 1 || a.win % 2 == 0 || !lds_fits(a.win) || a.nD < 1 || a.minD < 0) return ASW_ERR_BAD_ARGUMENT;
    if (a.H < 1 || a.W < 1 || a.H > TH * 65535 || (size_t)a.H * a.W >= ((size_t)1 << 31)) return ASW_ERR_BAD_ARGUMENT;  // grid.y, int columns
    if ((long long)a.minD + a.nD > (1 << 30)) return ASW_ERR_BAD_ARGUMENT;  // x - d stays an int
    TwoPassParams p;
    p.H = a.H; p.W = a.W; p.h = a.win / 2; p.minD = a.minD; p.nD = a.nD; p.flip = a.flip;
    const Layout lay(p.h);
    const dim3 grid((a.W + TW - 1) / TW, (a.H + TH - 1) / TH);
    return ASW_LAUNCH(k_asw_twopass, grid, dim3(256), lay.total, s, p, a.gL, a.gR, a.table, a.vol, a.disp);
}
