// Left-right disparity refinement (the rule is this library's own, like asw_lr_check's): cross-check of a
// left-view map against a right-view map, scan-line fill of the rejected pixels with the lower of the two neighbouring valid
// disparities, bilateral-weighted median over the filled pixels.  Integer weights throughout: every sum is exact in 32 bits
// and independent of the order it is taken in.
#include "asw_internal.h"

namespace {

constexpr unsigned short RF_NONE = 0xFFFF;  // F of an unfillable pixel / a tap outside the image: casts no vote
constexpr int RF_TW = 64, RF_TH = 16;       // pixel tile of one median workgroup
constexpr int RF_CHECK_CHUNKS = 8;          // 64-column chunks per wavefront of the cross-check

// Step 0 + 1: domain of dl (an integer in [minD, minD + n)) and asw_lr_check's rule.  mask: 0 valid, 1 rejected.
// counters: [0] rejected pixels, [2] != 0 when some dl leaves the domain.
__global__ __launch_bounds__(256) void k_refine_check(const float* __restrict__ dl, const float* __restrict__ dr, int H, int W,
                                                      int minD, int n, float max_diff, uint8_t* __restrict__ mask,
                                                      unsigned* __restrict__ counters)
{
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    unsigned nbad = 0;
    bool alien = false;
    for (int c = 0; c < RF_CHECK_CHUNKS; c++) {  // one counter update per wavefront and RF_CHECK_CHUNKS * 64 pixels
        const int x = (blockIdx.x * RF_CHECK_CHUNKS + c) * 64 + (threadIdx.x & 63);
        bool bad = false;
        if (x < W && y < H) {
            const float d = dl[(size_t)y * W + x];
            const bool dom = d >= (float)minD && d < (float)(minD + n) && d == floorf(d);  // NaN and inf compare false
            alien |= !dom;
            const int xr = x - (dom ? (int)d : 0);
            bad = !(dom && xr >= 0 && xr < W && fabsf(d - dr[(size_t)y * W + min(max(xr, 0), W - 1)]) <= max_diff);
            mask[(size_t)y * W + x] = bad ? 1 : 0;
        }
        nbad += (unsigned)__popcll(__ballot(bad));
    }
    const unsigned long long ma = __ballot(alien);
    if ((threadIdx.x & 63) == 0) {
        if (nbad) atomicAdd(counters, nbad);
        if (ma) atomicOr(counters + 2, 1u);
    }
}

// Step 2: one wavefront per row.  Forwards over 64-column chunks: a "last valid lane" max-scan gives every pixel the value of
// the nearest valid pixel to its left (carried from chunk to chunk), parked in F; backwards the same with a min-scan for the
// right neighbour, then F = min of the two (or the one that exists).  F holds disparity - minD; a row without a valid pixel
// becomes RF_NONE / mask 2.  out: dl where valid, minD + F where filled (the median kernel overwrites these), minD - 1 where
// unfillable.  counters[1]: unfillable pixels.
__global__ __launch_bounds__(256) void k_refine_fill(const float* __restrict__ dl, uint8_t* __restrict__ mask, int H, int W, int minD,
                                                     unsigned short* F, float* __restrict__ out, unsigned* __restrict__ counters)
{
    const int lane = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (y >= H) return;  // the whole wavefront
    const size_t row = (size_t)y * W;
    const int nchunk = (W + 63) / 64;
    int carry = -1;  // value of the nearest valid pixel before this chunk, -1: none
    for (int c = 0; c < nchunk; c++) {
        const int x = c * 64 + lane;
        const bool valid = x < W && mask[row + x] == 0;
        const int v = valid ? (int)dl[row + x] - minD : -1;
        int idx = valid ? lane : -1;
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(idx, off);
            if (lane >= off) idx = max(idx, t);
        }
        int a = __shfl(v, idx & 63);
        a = idx < 0 ? carry : a;
        if (x < W) F[row + x] = (unsigned short)a;  // valid: its own value; -1 -> RF_NONE
        carry = __shfl(a, 63);
    }
    if (carry < 0) {  // no valid pixel in the row
        for (int x = lane; x < W; x += 64) {
            mask[row + x] = 2;
            out[row + x] = (float)(minD - 1);
        }
        if (lane == 0) atomicAdd(counters + 1, (unsigned)W);
        return;
    }
    carry = -1;
    for (int c = nchunk - 1; c >= 0; c--) {
        const int x = c * 64 + lane;
        const bool valid = x < W && mask[row + x] == 0;
        const int a = x < W ? (int)F[row + x] : (int)RF_NONE;  // this lane's own store of the forward pass
        const int v = valid ? a : -1;
        int idx = valid ? lane : 64;
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_down(idx, off);
            if (lane + off < 64) idx = min(idx, t);
        }
        int b = __shfl(v, idx & 63);
        b = idx > 63 ? carry : b;
        if (x < W) {
            if (valid) {
                out[row + x] = dl[row + x];
            } else {
                const int f = a == (int)RF_NONE ? b : (b < 0 ? a : min(a, b));
                F[row + x] = (unsigned short)f;
                out[row + x] = (float)(minD + f);
            }
        }
        carry = __shfl(b, 0);
    }
}

// Step 3: weighted median of the filled pixels of one RF_TW x RF_TH tile.  The tile's filled pixels are compacted into an LDS
// list, so a lane never idles on a valid pixel; the guide (one packed word per pixel) and F are staged once with their k-pixel
// halo.  The median itself is a bisection on the value: the first pass over the window gives the total weight and the range of
// the votes, every further pass sums the weights of the votes <= mid.  No histogram, no LDS atomics beyond the list counter.
// Ts is read with a wavefront-uniform index (scalar loads); Tc, indexed by the colour distance, lives in LDS.
template <int C>
__global__ __launch_bounds__(256) void k_refine_median(const uint8_t* __restrict__ G, const unsigned short* __restrict__ F,
                                                       const uint8_t* __restrict__ mask, int H, int W, int k, int minD,
                                                       const unsigned* __restrict__ tc, int ntc, const unsigned* __restrict__ ts,
                                                       float* __restrict__ out)
{
    extern __shared__ unsigned rf_lds[];
    __shared__ int s_count;
    const int LW = RF_TW + 2 * k, LH = RF_TH + 2 * k, cells = LW * LH;
    unsigned* sG = rf_lds;
    unsigned* sTc = sG + cells;
    unsigned short* sF = reinterpret_cast<unsigned short*>(sTc + ntc);
    unsigned short* sList = sF + ((cells + 1) & ~1);
    const int t = threadIdx.x, lane = t & 63;
    const int x0 = blockIdx.x * RF_TW, y0 = blockIdx.y * RF_TH;

    if (t == 0) s_count = 0;
    __syncthreads();
    for (int r = 0; r < RF_TW * RF_TH / 256; r++) {
        const int p = r * 256 + t, x = x0 + (p & 63), y = y0 + (p >> 6);
        const bool filled = x < W && y < H && mask[(size_t)y * W + x] == 1;
        const unsigned long long m = __ballot(filled);
        int base = 0;
        if (lane == 0 && m) base = atomicAdd(&s_count, __popcll(m));
        base = __shfl(base, 0);
        if (filled) sList[base + __popcll(m & ((1ull << lane) - 1))] = (unsigned short)p;
    }
    __syncthreads();
    const int nlist = s_count;
    if (nlist == 0) return;  // nothing was rejected in this tile

    for (int i = t; i < cells; i += 256) {
        const int x = x0 - k + i % LW, y = y0 - k + i / LW;
        unsigned g = 0;
        unsigned short f = RF_NONE;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const size_t q = (size_t)y * W + x;
            f = F[q];
            if (C == 3)
                g = (unsigned)G[q * 3] | ((unsigned)G[q * 3 + 1] << 8) | ((unsigned)G[q * 3 + 2] << 16);
            else
                g = G[q];
        }
        sG[i] = g;
        sF[i] = f;
    }
    for (int i = t; i < ntc; i += 256) sTc[i] = tc[i];
    __syncthreads();

    const int tw = k + 1;  // row length of Ts
    for (int e = t; e < nlist; e += 256) {
        const int p = sList[e];
        const int ci = ((p >> 6) + k) * LW + (p & 63) + k;
        const unsigned g0 = sG[ci];
        unsigned T = 0;
        int lo = RF_NONE, hi = 0;
        for (int j = -k; j <= k; j++) {
            const unsigned* tsr = ts + abs(j) * tw;
            const int qr = ci + j * LW;
            for (int i = -k; i <= k; i++) {
                const int f = sF[qr + i];
                if (f != RF_NONE) {
                    T += sTc[__builtin_amdgcn_sad_u8(g0, sG[qr + i], 0u)] * tsr[abs(i)];
                    lo = min(lo, f);
                    hi = max(hi, f);
                }
            }
        }
        while (lo < hi) {  // smallest v with 2 * (weight of the votes <= v) >= T
            const int mid = (lo + hi) >> 1;
            unsigned below = 0;
            for (int j = -k; j <= k; j++) {
                const unsigned* tsr = ts + abs(j) * tw;
                const int qr = ci + j * LW;
                for (int i = -k; i <= k; i++)
                    if ((int)sF[qr + i] <= mid) below += sTc[__builtin_amdgcn_sad_u8(g0, sG[qr + i], 0u)] * tsr[abs(i)];
            }
            if (2u * below >= T)
                hi = mid;
            else
                lo = mid + 1;
        }
        out[(size_t)(y0 + (p >> 6)) * W + x0 + (p & 63)] = (float)(minD + lo);
    }
}

// dynamic LDS of k_refine_median: guide words, Tc, F, the list of filled pixels (33.7 KB at win 35, 3 channels)
size_t refine_median_lds_bytes(int win, int ntc)
{
    const int k = win / 2, cells = (RF_TW + 2 * k) * (RF_TH + 2 * k);
    return (size_t)cells * 4 + (size_t)ntc * 4 + (size_t)((cells + 1) & ~1) * 2 + (size_t)RF_TW * RF_TH * 2;
}

}  // namespace

int launch_refine(hipStream_t s, const RefineLaunch& a)
{
    const int H = a.H, W = a.W;
    if (a.C != 1 && a.C != 3) return ASW_ERR_UNSUPPORTED_LAYOUT;
    if (a.win < 1 || a.win > 35) return ASW_ERR_BAD_ARGUMENT;  // 32-bit sums; also keeps the dynamic LDS under 64 KB
    const size_t lds = refine_median_lds_bytes(a.win, a.ntc);
    ASW_HIP_TRY(hipMemsetAsync(a.counters, 0, 3 * sizeof(unsigned), s));
    ASW_TRY(ASW_LAUNCH(k_refine_check, dim3((W + 64 * RF_CHECK_CHUNKS - 1) / (64 * RF_CHECK_CHUNKS), (H + 3) / 4), dim3(256), 0, s, a.dl, a.dr, H, W, a.minD, a.n, a.max_diff,
                       a.mask, a.counters));
    ASW_TRY(ASW_LAUNCH(k_refine_fill, dim3((H + 3) / 4), dim3(256), 0, s, a.dl, a.mask, H, W, a.minD, a.F, a.out, a.counters));
    if (a.win > 1) {  // win = 1: the centre tap alone, the median is the fill
        const dim3 grid((W + RF_TW - 1) / RF_TW, (H + RF_TH - 1) / RF_TH);
        if (a.C == 3)
            ASW_TRY(ASW_LAUNCH(k_refine_median<3>, grid, dim3(256), lds, s, a.guide, a.F, a.mask, H, W, a.win / 2, a.minD, a.tc, a.ntc,
                               a.ts, a.out));
        else
            ASW_TRY(ASW_LAUNCH(k_refine_median<1>, grid, dim3(256), lds, s, a.guide, a.F, a.mask, H, W, a.win / 2, a.minD, a.tc, a.ntc,
                               a.ts, a.out));
    }
    return ASW_OK;
}
