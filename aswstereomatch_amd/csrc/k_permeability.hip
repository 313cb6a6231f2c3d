// Recursive (information-permeability) cost aggregation over the whole image + WTA (Cigla & Alatan 2013; not in the reference;
// DESIGN.md section 4.17), hand-written for gfx950.
//
// I = the view image, e(x,y,d) = min(trunc, AD(x,y,d)) from the u8 volume of launch_cost_ad, P[k] = (double)(float)exp(-k / sigma):
//     ph(x,y) = P[max_c |I_c(x,y) - I_c(x-1,y)|], x >= 1;    pv(x,y) = P[max_c |I_c(x,y) - I_c(x,y-1)|], y >= 1
//     horizontal, per row and plane, f64, every product rounded before it is added:
//         LR(0) = e(0),      LR(x) = e(x) + ph(x) LR(x-1)    ascending x
//         RL(W-1) = e(W-1),  RL(x) = e(x) + ph(x+1) RL(x+1)  descending x
//         Hs(x) = (LR(x) + RL(x)) - e(x)
//     vertical: the same three statements along every column with Hs for e and pv for ph -> S(x,y,d)
//     N = the same two passes over e == 1;  E = S / N;  volume plane (float)E;  map: strict '<' of the f64 E in ascending d.
//
// Design:
//  * one lane per scan, the lanes of a wavefront over 64 consecutive candidates of one row (horizontal) or one column (vertical):
//    a permeability is one wave-uniform value per step.  ph lies [y][x], pv transposed [x][y], both padded with zeros in front of the
//    first and behind the last position, so the border statements are the general ones (e + 0 * 0 == e exactly) and the steps of
//    the last, partial segment past the image are harmless;
//  * LR never travels through HBM: the forward scan keeps the value that enters every SEG-th position (a checkpoint, 1/SEG of the
//    volume), the backward scan recomputes LR inside a segment from its checkpoint into registers -- the same operations in the same
//    order, hence the same bits -- and runs RL and the combination back through the segment;
//  * the u8 costs [d][y][x] reach the lanes through an LDS tile of 64 candidates x 64 columns (coalesced byte rows in, one dword per
//    lane and four steps out, row stride 68 bytes: no bank conflict);
//  * Hs lies [y][x][candidate of the chunk]: the horizontal pass writes and the vertical pass reads 512 contiguous bytes per step;
//  * the vertical workgroup is XW wavefronts = XW neighbouring columns.  Per segment every wavefront leaves (float)E of its column
//    in an LDS tile [row][candidate][column] and its winner (wave minimum, lowest candidate among equals) beside it; the workgroup
//    then stores the tile as [d][y][x] rows and merges the winners into the running f64 best-E plane with strict '<'.  Candidate
//    groups of a chunk run in ascending order inside the workgroup, chunks in ascending order on the stream;
//  * no load stands under a condition: hipcc branches around such a load and waits for it before the next, which turns the 64 loads
//    of a cost tile or the 16 of a vertical segment into dependent round trips.  Addresses are clamped and a select follows; the
//    next vertical segment and the next checkpoint are issued ahead of the current segment's stores;
//  * N is the same two kernels over a one-plane volume of ones (trunc >= 1 leaves them 1), stored transposed and padded like pv;
//    the host runs them on a side stream beside the first chunk's horizontal pass.
#include <algorithm>

#include "asw_device.h"
#include "asw_internal.h"

namespace {

constexpr int SEG = 16;    // steps per register segment = checkpoint spacing
constexpr int TILE = 64;   // columns of the cost tile
constexpr int TROW = 68;   // its row stride in bytes
constexpr int XW = 8;      // columns (wavefronts) per workgroup of the vertical pass

struct PermParams {
    int H, W;
    int Wp, Hp;  // row strides of ph / pvT
    int nc;      // candidates of this chunk
    int trunc;
};

// ph [H][Wp], pvT [W][Hp]: zero at position 0 and from the image's end on
__global__ __launch_bounds__(256) void k_perm_weights_h(const uint8_t* __restrict__ img, int H, int W, int C, int Wp,
                                                        const double* __restrict__ P, double* __restrict__ ph)
{
    const int nbx = (Wp + 255) / 256;  // a flat grid: rows are not held to grid.y's 65535
    const int x = (blockIdx.x % nbx) * 256 + threadIdx.x, y = blockIdx.x / nbx;
    if (x >= Wp) return;
    double v = 0.0;
    if (x >= 1 && x < W) {
        const uint8_t* a = img + ((size_t)y * W + x) * C;
        int m = 0;
        for (int c = 0; c < C; c++) m = max(m, abs((int)a[c] - (int)a[c - C]));
        v = P[m];
    }
    ph[(size_t)y * Wp + x] = v;
}

__global__ __launch_bounds__(256) void k_perm_weights_v(const uint8_t* __restrict__ img, int H, int W, int C, int Hp,
                                                        const double* __restrict__ P, double* __restrict__ pvT)
{
    const int nby = (Hp + 63) / 64;
    const int y = (blockIdx.x % nby) * 64 + (threadIdx.x & 63), x = (blockIdx.x / nby) * 4 + (threadIdx.x >> 6);
    if (y >= Hp || x >= W) return;
    double v = 0.0;
    if (y >= 1 && y < H) {
        const uint8_t* a = img + ((size_t)y * W + x) * C;
        const uint8_t* b = a - (size_t)W * C;
        int m = 0;
        for (int c = 0; c < C; c++) m = max(m, abs((int)a[c] - (int)b[c]));
        v = P[m];
    }
    pvT[(size_t)x * Hp + y] = v;
}

// one statement of a scan: c + p * prev, the product rounded before it is added
__device__ __forceinline__ double scan_step(double c, double p, double prev) { return __dadd_rn(c, __dmul_rn(p, prev)); }

// Horizontal pass of one row (blockIdx.x) and 64 candidates (blockIdx.y) of the chunk whose first cost plane is `cost`.
__global__ __launch_bounds__(64) void k_perm_scan_h(PermParams p, const uint8_t* __restrict__ cost, const double* __restrict__ ph,
                                                    double* __restrict__ ck, double* __restrict__ hs)
{
    __shared__ uint32_t sC[64 * TROW / 4];
    const int lane = threadIdx.x, y = blockIdx.x, c0 = blockIdx.y * 64, cand = c0 + lane;
    const int W = p.W, nc = p.nc, nseg = (W + SEG - 1) / SEG, ncw = min(64, nc - c0);
    const bool active = cand < nc;
    const size_t plane = (size_t)p.H * W;
    const uint8_t* crow = cost + (size_t)c0 * plane + (size_t)y * W;
    const double* prow = ph + (size_t)y * p.Wp;
    double* ckrow = ck + (size_t)y * nseg * nc + cand;
    const double* ckload = ck + (size_t)y * nseg * nc + min(cand, nc - 1);  // loads are unconditional (clamped), stores guarded
    double* hrow = hs + (size_t)y * W * nc + cand;
    const uint32_t trunc = (uint32_t)p.trunc;

    // columns xt .. xt + 63 of the wavefront's candidates; zeros past the row.  Every load is unconditional on a clamped address
    // (a branch around a load would make the 64 of them dependent round trips), all 64 in flight at once
    auto stage = [&](int xt) {
        __syncthreads();
        const int x = xt + lane, xl = min(x, W - 1);
        uint8_t* sB = reinterpret_cast<uint8_t*>(sC);
        uint8_t v[64];
#pragma unroll
        for (int i = 0; i < 64; i++) v[i] = crow[(size_t)min(i, ncw - 1) * plane + xl];
#pragma unroll
        for (int i = 0; i < 64; i++) sB[i * TROW + lane] = x < W ? v[i] : (uint8_t)0;
        __syncthreads();
    };
    // e of the 16 steps from column xs on
    auto costs = [&](int xs, double* e) {
        const uint32_t* w = sC + lane * (TROW / 4) + (xs & (TILE - 1)) / 4;
#pragma unroll
        for (int q = 0; q < SEG / 4; q++) {
            const uint32_t v = w[q];
#pragma unroll
            for (int b = 0; b < 4; b++) e[q * 4 + b] = (double)min((v >> (8 * b)) & 0xFFu, trunc);
        }
    };

    // forward: the checkpoints
    double lr = 0.0;
    for (int s = 0; s < nseg; s++) {
        const int xs = s * SEG;
        if ((xs & (TILE - 1)) == 0) stage(xs);
        if (active) ckrow[(size_t)s * nc] = lr;
        double e[SEG];
        costs(xs, e);
#pragma unroll
        for (int j = 0; j < SEG; j++) lr = scan_step(e[j], prow[xs + j], lr);
    }
    // backward, segment by segment: LR again from the checkpoint, then RL and the combination
    double rl = 0.0, tnext = ckload[(size_t)(nseg - 1) * nc];
    for (int s = nseg - 1; s >= 0; s--) {
        const int xs = s * SEG;
        if (s == nseg - 1 || (xs & (TILE - 1)) == TILE - SEG) stage(xs & ~(TILE - 1));
        double e[SEG], l[SEG];
        costs(xs, e);
        double t = tnext;
        tnext = ckload[(size_t)max(s - 1, 0) * nc];  // the next segment's checkpoint, ahead of this segment's stores
#pragma unroll
        for (int j = 0; j < SEG; j++) l[j] = t = scan_step(e[j], prow[xs + j], t);
#pragma unroll
        for (int j = SEG - 1; j >= 0; j--) {
            rl = scan_step(e[j], prow[xs + j + 1], rl);
            const double h = __dsub_rn(__dadd_rn(l[j], rl), e[j]);
            if (active && xs + j < W) hrow[(size_t)(xs + j) * nc] = h;
        }
    }
}

// Vertical pass of XW columns and every candidate of the chunk.  Nin == nullptr: the frame's N (nc = 1) -> Nout, transposed and padded
// like pvT ([W][Hp]: a column's values are one contiguous, wave-uniform read); else
// E = S / Nin -> vol (optional) planes cbeg .., and the winners merged into bestE / disp (first: nothing to merge with yet).
__global__ __launch_bounds__(XW * 64) void k_perm_scan_v(PermParams p, int cbeg, int minD, int first, const double* __restrict__ hs,
                                                         const double* __restrict__ pvT, double* __restrict__ ck,
                                                         const double* __restrict__ Nin, double* __restrict__ Nout,
                                                         float* __restrict__ vol, double* __restrict__ bestE, float* __restrict__ disp)
{
    __shared__ float sE[SEG * 64 * (XW + 1)];
    __shared__ double sBE[SEG * XW];
    __shared__ int sBD[SEG * XW];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = p.H, W = p.W, nc = p.nc, nseg = (H + SEG - 1) / SEG;
    const int x0 = blockIdx.x * XW, x = x0 + w, xc = min(x, W - 1);
    const double* pcol = pvT + (size_t)xc * p.Hp;
    const size_t ystride = (size_t)W * nc;

    for (int g = 0; g * 64 < nc; g++) {
        const int cand = g * 64 + lane;
        const bool active = x < W && cand < nc;
        const int candc = min(cand, nc - 1);  // loads are unconditional on clamped addresses (a branch around a load would make the
                                              // 16 of a segment dependent round trips); what an idle lane computes is never stored
        const double* hcol = hs + (size_t)xc * nc + candc;
        double* ckcol = ck + (size_t)xc * nseg * nc + cand;
        const double* ckload = ck + (size_t)xc * nseg * nc + candc;
        // the 16 sums of segment s, rows past the image as 0; issued a segment ahead of their use
        auto load_segment = [&](int s, double* e) {
#pragma unroll
            for (int j = 0; j < SEG; j++) e[j] = hcol[(size_t)min(s * SEG + j, H - 1) * ystride];
        };
        auto mask_rows = [&](int s, double* e) {
#pragma unroll
            for (int j = 0; j < SEG; j++) e[j] = s * SEG + j < H ? e[j] : 0.0;
        };

        double lr = 0.0, en[SEG];
        load_segment(0, en);
        for (int s = 0; s < nseg; s++) {
            const int ys = s * SEG;
            if (active) ckcol[(size_t)s * nc] = lr;
            double e[SEG];
#pragma unroll
            for (int j = 0; j < SEG; j++) e[j] = en[j];
            load_segment(min(s + 1, nseg - 1), en);
            mask_rows(s, e);
#pragma unroll
            for (int j = 0; j < SEG; j++) lr = scan_step(e[j], pcol[ys + j], lr);
        }

        double rl = 0.0, tnext = ckload[(size_t)(nseg - 1) * nc];  // en holds segment nseg - 1
        for (int s = nseg - 1; s >= 0; s--) {
            const int ys = s * SEG;
            double e[SEG], l[SEG];
#pragma unroll
            for (int j = 0; j < SEG; j++) e[j] = en[j];
            double t = tnext;
            load_segment(max(s - 1, 0), en);  // ahead of this segment's stores
            tnext = ckload[(size_t)max(s - 1, 0) * nc];
            mask_rows(s, e);
            double nn[SEG];  // wave-uniform
#pragma unroll
            for (int j = 0; j < SEG; j++) nn[j] = Nin ? Nin[(size_t)xc * p.Hp + ys + j] : 1.0;  // rows past the image: never used
#pragma unroll
            for (int j = 0; j < SEG; j++) l[j] = t = scan_step(e[j], pcol[ys + j], t);
#pragma unroll
            for (int j = SEG - 1; j >= 0; j--) {
                const int y = ys + j;
                rl = scan_step(e[j], pcol[y + 1], rl);
                const double S = __dsub_rn(__dadd_rn(l[j], rl), e[j]);
                if (!Nin) {
                    if (active && y < H) Nout[(size_t)x * p.Hp + y] = S;
                    continue;
                }
                const bool live = active && y < H;
                const double q = S / nn[j];
                const double E = live ? q : 1.7976931348623157e308;
                if (vol) sE[(j * 64 + lane) * (XW + 1) + w] = (float)E;
                double m = E;
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) m = fmin(m, __shfl_xor(m, o));
                const unsigned long long eq = __ballot(live && E == m);
                if (lane == 0) {
                    sBE[j * XW + w] = m;
                    sBD[j * XW + w] = g * 64 + (eq ? __ffsll((long long)eq) - 1 : 0);
                }
            }
            if (!Nin) continue;
            __syncthreads();
            if (vol)
                for (int i = tid; i < SEG * 64 * XW; i += XW * 64) {
                    const int xx = i % XW, d = (i / XW) & 63, yy = i / (XW * 64);
                    const int y = ys + yy, xo = x0 + xx, c = g * 64 + d;
                    if (y < H && xo < W && c < nc) vol[((size_t)(cbeg + c) * H + y) * W + xo] = sE[(yy * 64 + d) * (XW + 1) + xx];
                }
            if (tid < SEG * XW) {
                const int yy = tid / XW, xx = tid % XW, y = ys + yy, xo = x0 + xx;
                if (y < H && xo < W) {
                    const size_t i = (size_t)y * W + xo;
                    const double old = (first && g == 0) ? 1.7976931348623157e308 : bestE[i];
                    const double m = sBE[tid];
                    if (m < old) {  // ascending d, strict <
                        bestE[i] = m;
                        disp[i] = (float)(minD + cbeg + sBD[tid]);
                    }
                }
            }
            __syncthreads();
        }
    }
}

int check(const PermLaunch& a)
{
    if (a.H < 1 || a.W < 1 || (size_t)a.H * a.W >= ((size_t)1 << 31)) return ASW_ERR_BAD_ARGUMENT;
    if (a.nc < 1 || a.nc > 64 * 65535 || a.trunc < 1 || a.trunc > 255) return ASW_ERR_BAD_ARGUMENT;  // grid.y of the horizontal pass
    return ASW_OK;
}

PermParams params(const PermLaunch& a)
{
    PermParams p;
    p.H = a.H; p.W = a.W; p.Wp = perm_padded(a.W); p.Hp = perm_padded(a.H); p.nc = a.nc; p.trunc = a.trunc;
    return p;
}

}  // namespace

int perm_segments(int n) { return (n + SEG - 1) / SEG; }
int perm_padded(int n) { return perm_segments(n) * SEG + SEG; }

int launch_perm_weights(hipStream_t s, const uint8_t* img, int H, int W, int C, const double* P, double* ph, double* pvT)
{
    if (H < 1 || W < 1 || (C != 1 && C != 3) || (size_t)H * W >= ((size_t)1 << 31)) return ASW_ERR_BAD_ARGUMENT;
    const int Wp = perm_padded(W), Hp = perm_padded(H);
    ASW_TRY(ASW_LAUNCH(k_perm_weights_h, dim3((unsigned)((size_t)((Wp + 255) / 256) * H)), dim3(256), 0, s, img, H, W, C, Wp, P, ph));
    return ASW_LAUNCH(k_perm_weights_v, dim3((unsigned)((size_t)((Hp + 63) / 64) * ((W + 3) / 4))), dim3(256), 0, s, img, H, W, C, Hp, P, pvT);
}

int launch_perm_scan_h(hipStream_t s, const PermLaunch& a)
{
    if (check(a) != ASW_OK) return ASW_ERR_BAD_ARGUMENT;
    return ASW_LAUNCH(k_perm_scan_h, dim3(a.H, (a.nc + 63) / 64), dim3(64), 0, s, params(a), a.cost, a.ph, a.ck, a.hs);
}

int launch_perm_scan_v(hipStream_t s, const PermLaunch& a)
{
    if (check(a) != ASW_OK) return ASW_ERR_BAD_ARGUMENT;
    if (!a.N && (a.nc != 1 || !a.Nout)) return ASW_ERR_BAD_ARGUMENT;
    return ASW_LAUNCH(k_perm_scan_v, dim3((a.W + XW - 1) / XW), dim3(XW * 64), 0, s, params(a), a.cbeg, a.minD, a.first, a.hs, a.pvT,
                      a.ck, a.N, a.Nout, a.vol, a.bestE, a.disp);
}
