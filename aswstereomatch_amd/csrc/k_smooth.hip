// Confidence-weighted edge-aware smoothing of a disparity map (the rule is stated in asw_mi355x.h under
// "Smoothing"): the fast global smoother of Min et al. (TIP 2014), T iterations of a row pass and a column pass, each pass one
// tridiagonal solve per line for the two right-hand sides N = confidence * disparity and D = confidence; the result is N / D.
// Every operation is one IEEE f64 operation in the written order (__dmul_rn / __dsub_rn: never contracted; the f64 division is
// correctly rounded), so tests/smooth_ref.py restates the kernels to the bit.
//
// One lane solves one line, a wavefront SM_LINES = 64 neighbouring lines.  Everything a sweep touches per step is laid out
// [step][line], so the 64 lanes of a step read and write 64 neighbouring values:
//   link    u16 [n][lines]  index into Wt of the link between steps i - 1 and i (entry 0 unused): the vertical links as the
//                           image lies, the horizontal links transposed by the prep kernel through LDS
//   cp, fN, fD  f64 [n][lines]  what the forward sweep leaves for the backward sweep
// N and D are [rows][cols].  The column pass (lines = columns) meets them in that order; the row pass (lines = rows) would read one
// cache line per lane and step, so it stages tiles of SM_LINES lines x SM_TILE steps through LDS: loaded and stored with 16
// neighbouring lanes on the 128 bytes of a line, walked with one lane per line (row stride SM_TILE + 1 doubles: the 32 lanes of
// a ds_read_b64 group fall on 32 different bank pairs).  Both forms take a step's inputs SM_TILE steps at a time, so the loads
// of a chunk are in flight together and the next tile of the row pass is on its way while the current one is walked.
#include "asw_internal.h"

namespace {

constexpr int SM_LINES = 64;  // lines per workgroup: one wavefront
constexpr int SM_TILE = 16;   // steps per chunk, and per staged tile of the row pass
constexpr int SM_PREP = 32;   // the prep kernel's tile side (transpose of the horizontal link indices)

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e+38f; }

// steps 1-2 and the link indices of step 4.  d / c are read with an element stride (1: two planes, 2: the interleaved
// {disparity, confidence} pairs of k_confidence).  Block (SM_PREP, 8), one SM_PREP x SM_PREP tile per workgroup.
__global__ __launch_bounds__(SM_PREP * 8) void k_smooth_prep(const uint8_t* __restrict__ G, int C, const float* __restrict__ d,
                                                             const float* __restrict__ c, int stride, int H, int W,
                                                             double* __restrict__ N, double* __restrict__ D,
                                                             uint16_t* __restrict__ linkV, uint16_t* __restrict__ linkHT)
{
    __shared__ uint16_t t[SM_PREP][SM_PREP + 1];
    const int x0 = blockIdx.x * SM_PREP, y0 = blockIdx.y * SM_PREP;
    const int tx = threadIdx.x;
    for (int ty = threadIdx.y; ty < SM_PREP; ty += 8) {
        const int x = x0 + tx, y = y0 + ty;
        int kh = 0;
        if (x < W && y < H) {
            const size_t i = (size_t)y * W + x;
            const float dv = d[i * stride], cv = c[i * stride];
            const double ce = (finite_f(dv) && finite_f(cv) && cv > 0.0f) ? (double)cv : 0.0;
            N[i] = ce > 0.0 ? __dmul_rn(ce, (double)dv) : 0.0;
            D[i] = ce;
            const uint8_t* g = G + i * C;
            int kv = 0;
            for (int ch = 0; ch < C; ch++) {
                const int v = g[ch];
                if (x >= 1) kh += abs(v - (int)g[ch - C]);
                if (y >= 1) kv += abs(v - (int)g[ch - (ptrdiff_t)W * C]);
            }
            linkV[i] = (uint16_t)kv;
        }
        t[ty][tx] = (uint16_t)kh;
    }
    __syncthreads();
    for (int ty = threadIdx.y; ty < SM_PREP; ty += 8) {  // tile column ty -> row x0 + ty of the transposed plane
        const int x = x0 + ty, y = y0 + tx;
        if (x < W && y < H) linkHT[(size_t)x * H + y] = t[tx][ty];
    }
}

// One pass: the lines of a frame, n steps each.  STAGED: N / D are [lines][n] (the row pass), else [n][lines] (the column pass).
template <bool STAGED>
__global__ __launch_bounds__(SM_LINES) void k_smooth_pass(double* __restrict__ N, double* __restrict__ D,
                                                          const uint16_t* __restrict__ link, const double* __restrict__ Wt,
                                                          double lam, int n, int lines, double* __restrict__ cp,
                                                          double* __restrict__ fN, double* __restrict__ fD)
{
    __shared__ double tN[STAGED ? SM_LINES : 1][SM_TILE + 1];
    __shared__ double tD[STAGED ? SM_LINES : 1][SM_TILE + 1];
    const int lane = threadIdx.x;
    const int line0 = blockIdx.x * SM_LINES;
    const bool active = line0 + lane < lines;
    const int line = active ? line0 + lane : lines - 1;  // a lane past the last line repeats it and stores nothing
    // the staged tile: register k of a lane holds line sl + 4 k, step sj of the tile
    const int sl = lane / SM_TILE, sj = lane % SM_TILE;
    constexpr int SREG = SM_TILE * SM_LINES / 64;  // tile values per lane
    constexpr int SROWS = 64 / SM_TILE;            // lines per load instruction
    double rN[STAGED ? SREG : 1], rD[STAGED ? SREG : 1];
    auto tile_load = [&](int i0) {
        if constexpr (STAGED) {
#pragma unroll
            for (int k = 0; k < SREG; k++) {
                const int l = line0 + sl + SROWS * k, i = i0 + sj;
                const bool in = l < lines && i < n;
                const size_t at = in ? (size_t)l * n + i : 0;
                rN[k] = N[at]; rD[k] = D[at];
            }
        }
    };

    // ---- forward sweep ----
    double a = 0.0, cpp = 0.0, fnp = 0.0, fdp = 0.0;  // a_0 = 0 and zeros in front of the line: step 0 is the general step
    tile_load(0);
    for (int i0 = 0; i0 < n; i0 += SM_TILE) {
        double f_n[SM_TILE], f_d[SM_TILE], w[SM_TILE];
#pragma unroll
        for (int j = 0; j < SM_TILE; j++) {  // w[j]: the weight of the link behind step i0 + j
            const int i = i0 + j + 1;
            const int k = i < n ? link[(size_t)i * lines + line] : 0;
            w[j] = Wt[k];
        }
        if constexpr (STAGED) {
            __syncthreads();  // the tile's readers of the last round are done
#pragma unroll
            for (int k = 0; k < SREG; k++) { tN[sl + SROWS * k][sj] = rN[k]; tD[sl + SROWS * k][sj] = rD[k]; }
            __syncthreads();
            if (i0 + SM_TILE < n) tile_load(i0 + SM_TILE);
#pragma unroll
            for (int j = 0; j < SM_TILE; j++) { f_n[j] = tN[lane][j]; f_d[j] = tD[lane][j]; }
        } else {
#pragma unroll
            for (int j = 0; j < SM_TILE; j++) {
                const size_t at = i0 + j < n ? (size_t)(i0 + j) * lines + line : 0;
                f_n[j] = N[at]; f_d[j] = D[at];
            }
        }
#pragma unroll
        for (int j = 0; j < SM_TILE; j++) {
            const int i = i0 + j;
            if (i < n) {
                const double c = i + 1 < n ? -__dmul_rn(lam, w[j]) : 0.0;
                const double b = __dsub_rn(__dsub_rn(1.0, a), c);
                const double m = __dsub_rn(b, __dmul_rn(a, cpp));
                const double r = 1.0 / m;
                cpp = __dmul_rn(c, r);
                fnp = __dmul_rn(__dsub_rn(f_n[j], __dmul_rn(a, fnp)), r);
                fdp = __dmul_rn(__dsub_rn(f_d[j], __dmul_rn(a, fdp)), r);
                a = c;  // a_{i+1} = -(lam * w_{i+1}) = c_i
                if (active) {
                    const size_t at = (size_t)i * lines + line;
                    cp[at] = cpp; fN[at] = fnp; fD[at] = fdp;
                }
            }
        }
    }

    // ---- backward sweep: chunks from the last one down, steps of a chunk from its last one down ----
    double un = 0.0, ud = 0.0;  // zeros behind the line: cp_{n-1} = 0, so step n - 1 is the general step
    for (int i0 = (n - 1) / SM_TILE * SM_TILE; i0 >= 0; i0 -= SM_TILE) {
        double q[SM_TILE], g_n[SM_TILE], g_d[SM_TILE];
#pragma unroll
        for (int j = 0; j < SM_TILE; j++) {
            const size_t at = i0 + j < n ? (size_t)(i0 + j) * lines + line : 0;
            q[j] = cp[at]; g_n[j] = fN[at]; g_d[j] = fD[at];
        }
        if constexpr (STAGED) __syncthreads();  // the tile's readers of the last round are done
#pragma unroll
        for (int j = SM_TILE - 1; j >= 0; j--) {
            const int i = i0 + j;
            if (i < n) {
                un = __dsub_rn(g_n[j], __dmul_rn(q[j], un));
                ud = __dsub_rn(g_d[j], __dmul_rn(q[j], ud));
                if constexpr (STAGED) {
                    tN[lane][j] = un; tD[lane][j] = ud;
                } else if (active) {
                    const size_t at = (size_t)i * lines + line;
                    N[at] = un; D[at] = ud;
                }
            }
        }
        if constexpr (STAGED) {
            __syncthreads();
#pragma unroll
            for (int k = 0; k < SREG; k++) {
                const int l = line0 + sl + SROWS * k, i = i0 + sj;
                if (l < lines && i < n) {
                    const size_t at = (size_t)l * n + i;
                    N[at] = tN[sl + SROWS * k][sj]; D[at] = tD[sl + SROWS * k][sj];
                }
            }
        }
    }
}

// step 6
__global__ __launch_bounds__(256) void k_smooth_final(const double* __restrict__ N, const double* __restrict__ D,
                                                      const float* __restrict__ d, int stride, size_t plane, float* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= plane) return;
    const double dn = D[i];
    const float keep = d[i * stride];
    out[i] = dn > 0.0 ? (float)(N[i] / dn) : keep;
}

}  // namespace

int launch_smooth(hipStream_t s, const SmoothLaunch& a)
{
    if (!a.guide || !a.d || !a.c || !a.out || !a.N || !a.D || !a.linkV || !a.linkHT || !a.cp || !a.fN || !a.fD || !a.Wt)
        return ASW_ERR_BAD_ARGUMENT;
    if (a.H < 1 || a.W < 1 || (a.C != 1 && a.C != 3) || a.T < 1 || a.T > 8 || (a.stride != 1 && a.stride != 2)) return ASW_ERR_BAD_ARGUMENT;
    const int H = a.H, W = a.W;
    const size_t plane = (size_t)H * W;
    if (plane >= ((size_t)1 << 31)) return ASW_ERR_BAD_ARGUMENT;
    const unsigned gy = (unsigned)((H + SM_PREP - 1) / SM_PREP);
    if (gy > 65535) return ASW_ERR_BAD_ARGUMENT;
    ASW_TRY(ASW_LAUNCH(k_smooth_prep, dim3((unsigned)((W + SM_PREP - 1) / SM_PREP), gy), dim3(SM_PREP, 8), 0, s, a.guide, a.C, a.d, a.c,
                       a.stride, H, W, a.N, a.D, a.linkV, a.linkHT));
    for (int t = 1; t <= a.T; t++) {
        const double lam = (1.5 * a.lambda * (double)(1 << 2 * (a.T - t))) / (double)((1 << 2 * a.T) - 1);
        // rows: H lines of W steps, N / D staged; columns: W lines of H steps
        ASW_TRY(ASW_LAUNCH(k_smooth_pass<true>, dim3((unsigned)((H + SM_LINES - 1) / SM_LINES)), dim3(SM_LINES), 0, s, a.N, a.D,
                           a.linkHT, a.Wt, lam, W, H, a.cp, a.fN, a.fD));
        ASW_TRY(ASW_LAUNCH(k_smooth_pass<false>, dim3((unsigned)((W + SM_LINES - 1) / SM_LINES)), dim3(SM_LINES), 0, s, a.N, a.D,
                           a.linkV, a.Wt, lam, H, W, a.cp, a.fN, a.fD));
    }
    return ASW_LAUNCH(k_smooth_final, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, s, (const double*)a.N, (const double*)a.D,
                      a.d, a.stride, plane, a.out);
}
