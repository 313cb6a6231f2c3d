// Cross-based support-region aggregation (Zhang, Lu, Lafruit 2009; the aggregation step of AD-Census), selector entry 12.
// Not in the reference; the definition is DESIGN.md section 4.12.  All integer until the one final division:
//   arms   a_u(p), u = left / right / up / down: the largest r <= L = win / 2 whose pixels p + k u, k = 1..r, lie inside the image and
//          differ from the ANCHOR p by at most tau in every channel
//   count  N(p) = sum over the rows y' of p's vertical arm of (left(x, y') + right(x, y') + 1)
//   sums   S(p, d) = the same sum of the truncated AD cost e = min(trunc, AD), by the two orthogonal integral steps
//   volume E = (float)S / (float)N, one correctly rounded f32 division (S <= 255 * 35^2 < 2^24: both operands are exact)
// k_cross_arms and k_cross_count run once per call on the view image; k_cross_aggregate runs over all candidates.
#include <algorithm>

#include "asw_device.h"
#include "asw_internal.h"

namespace {

constexpr int TW = 64, TH = 32;        // pixels a workgroup owns: TW columns x TH rows, 8 pixels per thread
constexpr int MAX_L = 17;              // win <= 35
constexpr int HROWS = (TH + 2 * MAX_L + 3) / 4;  // band rows per thread in the horizontal step (a thread row every 4 rows)

template <int C>
__device__ __forceinline__ bool cross_similar(const uint8_t* __restrict__ img, size_t q, const int* a, int tau)
{
    int m = 0;
#pragma unroll
    for (int c = 0; c < C; c++) m = max(m, abs((int)img[q * C + c] - a[c]));
    return m <= tau;
}

// four arm lengths of every pixel, packed left | right << 8 | up << 16 | down << 24
template <int C>
__global__ __launch_bounds__(256) void k_cross_arms(const uint8_t* __restrict__ img, int H, int W, int L, int tau,
                                                    uint32_t* __restrict__ arms)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    int a[C];
#pragma unroll
    for (int c = 0; c < C; c++) a[c] = img[p * C + c];
    int l = 0, r = 0, u = 0, d = 0;
    while (l < L && x - l - 1 >= 0 && cross_similar<C>(img, p - l - 1, a, tau)) l++;
    while (r < L && x + r + 1 < W && cross_similar<C>(img, p + r + 1, a, tau)) r++;
    while (u < L && y - u - 1 >= 0 && cross_similar<C>(img, p - (size_t)(u + 1) * W, a, tau)) u++;
    while (d < L && y + d + 1 < H && cross_similar<C>(img, p + (size_t)(d + 1) * W, a, tau)) d++;
    arms[p] = (uint32_t)l | (uint32_t)r << 8 | (uint32_t)u << 16 | (uint32_t)d << 24;
}

// N(p) <= 35 * 35 = 1225
__global__ __launch_bounds__(256) void k_cross_count(const uint32_t* __restrict__ arms, int H, int W, uint16_t* __restrict__ cnt)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const uint32_t a = arms[p];
    const int u = (a >> 16) & 255, d = a >> 24;
    int n = 0;
    for (int k = -u; k <= d; k++) {  // rows y - u .. y + d lie inside the image by the arm rule
        const uint32_t h = arms[(size_t)(y + k) * W + x];
        n += (int)(h & 255) + (int)((h >> 8) & 255) + 1;
    }
    cnt[p] = (uint16_t)n;
}

// One workgroup: a TW x TH tile of pixels, every candidate, DC candidates per pass.  Per pass, in LDS (int32 throughout: a row
// prefix stays below 255 * 99, a column prefix below 255 * 35 * 66):
//   A [DC][RH][SA]      e, then its inclusive row prefix P in place; column j <-> image column x0 - L - 1 + j (j = 0: the P[-1] of the
//                       leftmost pixel's longest arm), row i <-> image row y0 - L + i; 0 outside the image; SA odd: the scan walks one
//                       row per lane, lane stride SA dwords, every lane on its own bank
//   B [DC][RH + 1][TW]  E_H(q) = P[x + right(q)] - P[x - left(q) - 1] for the tile's columns on every band row, then its inclusive
//                       column prefix V in place; row 0 stays 0 (V[-1]), row i + 1 <-> band row i
// then S = V[y + down] - V[y - up - 1] and the division.  The running minimum of a pixel lives in its thread's registers across the
// passes (strict '<' in ascending d, k_wta's rule), so nothing depends on DC or on the grid.
__global__ __launch_bounds__(256) void k_cross_aggregate(const uint8_t* __restrict__ cost, const uint32_t* __restrict__ arms,
                                                         const uint16_t* __restrict__ cnt, int H, int W, int L, int trunc, int minD,
                                                         int numD, int DC, int SA, float* __restrict__ vol, float* __restrict__ disp)
{
    extern __shared__ int lds[];
    const int RH = TH + 2 * L, RW = TW + 2 * L + 1;
    int* A = lds;
    int* B = lds + (size_t)DC * RH * SA;
    const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
    // every XCD takes a contiguous run of tiles: neighbouring tiles share their halo lines of the cost volume in one L2
    const int vid = xcd_contiguous(gridDim.x * gridDim.y, blockIdx.x + gridDim.x * blockIdx.y);
    const int x0 = (vid % (int)gridDim.x) * TW, y0 = (vid / (int)gridDim.x) * TH;
    const int x = x0 + tx;
    const size_t plane = (size_t)H * W;

    // horizontal arms of this thread's column on the band rows ty, ty + 4, ...: left | right << 8, 0 outside the image
    uint32_t harm[HROWS];
#pragma unroll
    for (int m = 0; m < HROWS; m++) {
        const int yy = y0 - L + ty + 4 * m;
        harm[m] = (ty + 4 * m < RH && x < W && yy >= 0 && yy < H) ? (arms[(size_t)yy * W + x] & 0xFFFFu) : 0u;
    }
    // this thread's pixels: rows y0 + ty + 4 j
    int varm[TH / 4];
    float fn[TH / 4], best[TH / 4], bestd[TH / 4];
#pragma unroll
    for (int j = 0; j < TH / 4; j++) {
        const int y = y0 + ty + 4 * j;
        const bool in = x < W && y < H;
        varm[j] = in ? (int)(arms[(size_t)y * W + x] >> 16) : -1;  // up | down << 8; -1: no pixel
        fn[j] = in ? (float)cnt[(size_t)y * W + x] : 1.0f;
        best[j] = 3.402823466e+38f;
        bestd[j] = 0.0f;
    }
    for (int i = tid; i < DC * TW; i += 256) B[(size_t)(i >> 6) * (RH + 1) * TW + (i & 63)] = 0;  // V[-1]

    for (int k0 = 0; k0 < numD; k0 += DC) {
        const int nc = min(DC, numD - k0);
        // e rows: a wavefront per row, lanes along it
        for (int r = ty; r < nc * RH; r += 4) {
            const int c = r / RH, i = r - c * RH, yy = y0 - L + i;
            const bool row_in = yy >= 0 && yy < H;
            const uint8_t* src = cost + ((size_t)(k0 + c) * H + (row_in ? yy : 0)) * W;
            for (int j = tx; j < RW; j += 64) {
                const int xx = x0 - L - 1 + j;
                A[(size_t)r * SA + j] = (row_in && xx >= 0 && xx < W) ? min(trunc, (int)src[xx]) : 0;
            }
        }
        __syncthreads();
        // row prefix: a lane per row
        for (int r = tid; r < nc * RH; r += 256) {
            int* p = A + (size_t)r * SA;
            int acc = 0;
            for (int j = 0; j < RW; j++) {
                acc += p[j];
                p[j] = acc;
            }
        }
        __syncthreads();
        for (int c = 0; c < nc; c++) {
#pragma unroll
            for (int m = 0; m < HROWS; m++) {
                const int i = ty + 4 * m;
                if (i < RH) {
                    const int* p = A + ((size_t)c * RH + i) * SA + tx + L + 1;  // P of this thread's column
                    const int l = harm[m] & 255, r = harm[m] >> 8;
                    B[((size_t)c * (RH + 1) + i + 1) * TW + tx] = p[r] - p[-l - 1];
                }
            }
        }
        __syncthreads();
        // column prefix: a lane per column
        for (int it = tid; it < nc * TW; it += 256) {
            int* p = B + (size_t)(it >> 6) * (RH + 1) * TW + (it & 63);
            int acc = 0;
            for (int i = 1; i <= RH; i++) {
                acc += p[i * TW];
                p[i * TW] = acc;
            }
        }
        __syncthreads();
        for (int c = 0; c < nc; c++) {
            const int* p = B + (size_t)c * (RH + 1) * TW + tx;
#pragma unroll
            for (int j = 0; j < TH / 4; j++) {
                if (varm[j] >= 0) {
                    const int i = L + ty + 4 * j, u = varm[j] & 255, d = varm[j] >> 8;
                    const int S = p[(i + d + 1) * TW] - p[(i - u) * TW];
                    const float E = (float)S / fn[j];
                    if (vol) __builtin_nontemporal_store(E, vol + (size_t)(k0 + c) * plane + (size_t)(y0 + ty + 4 * j) * W + x);  // written once
                    if (E < best[j]) { best[j] = E; bestd[j] = (float)(minD + k0 + c); }
                }
            }
        }
        // the next pass writes A only after this pass's last read of it (two barriers back) and B only after two more barriers
    }
#pragma unroll
    for (int j = 0; j < TH / 4; j++)
        if (varm[j] >= 0) disp[(size_t)(y0 + ty + 4 * j) * W + x] = bestd[j];
}

}  // namespace

int launch_cross_arms(hipStream_t s, const uint8_t* img, int H, int W, int C, int win, int tau, uint32_t* arms, uint16_t* cnt)
{
    if (win < 1 || win / 2 > MAX_L || (C != 1 && C != 3)) return ASW_ERR_BAD_ARGUMENT;
    const dim3 grid((W + 63) / 64, (H + 3) / 4);
    if (C == 3)
        ASW_TRY(ASW_LAUNCH(k_cross_arms<3>, grid, dim3(256), 0, s, img, H, W, win / 2, tau, arms));
    else
        ASW_TRY(ASW_LAUNCH(k_cross_arms<1>, grid, dim3(256), 0, s, img, H, W, win / 2, tau, arms));
    return ASW_LAUNCH(k_cross_count, grid, dim3(256), 0, s, arms, H, W, cnt);
}

int launch_cross_aggregate(hipStream_t s, const uint8_t* cost, const uint32_t* arms, const uint16_t* cnt, int H, int W, int win,
                           int trunc, int minD, int numD, float* vol, float* disp)
{
    if (win < 1 || win / 2 > MAX_L || numD < 1) return ASW_ERR_BAD_ARGUMENT;
    const int L = win / 2, RH = TH + 2 * L, RW = TW + 2 * L + 1, SA = RW | 1;
    const size_t per_candidate = ((size_t)RH * SA + (size_t)(RH + 1) * TW) * sizeof(int);  // 18 KB (win 3) .. 43 KB (win 35)
    // candidates per pass: what fits 64 KB of LDS, at most 4 (256 lanes = 4 x 64 columns in the column prefix)
    const int DC = (int)std::max<size_t>(1, std::min<size_t>(std::min(4, numD), ((size_t)64 * 1024) / per_candidate));
    const dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH);
    return ASW_LAUNCH(k_cross_aggregate, grid, dim3(256), DC * per_candidate, s, cost, arms, cnt, H, W, L, trunc, minD, numD, DC, SA, vol,
                      disp);
}
