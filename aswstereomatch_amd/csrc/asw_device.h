// Device-side helpers shared by the kernels: OpenCV border index maps, the wavefront idioms (LDS fence, XCD remap, min / max,
// prefix sums, f64 lane moves) and the small per-sample functions more than one kernel file uses.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

// BORDER_REFLECT: fedcba|abcdefgh|hgfedcb -- copyMakeBorder(..., BORDER_REFLECT) of the reference
__device__ __forceinline__ int reflect_idx(int p, int len)
{
    if (len == 1) return 0;
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p - 1 : 2 * len - 1 - p;
    return p;
}

// BORDER_REFLECT_101 (App. A-3): gfedcb|abcdefgh|gfedcba -- the default border of boxFilter / filter2D
__device__ __forceinline__ int reflect101_idx(int p, int len)
{
    if (len == 1) return 0;
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

// Between a wavefront's LDS stores and the loads of OTHER lanes of the same wavefront (and again before the next round of stores
// overwrites what those loads read).  Same-wavefront LDS traffic is ordered in hardware: the reads see the writes without a
// workgroup barrier.  The COMPILER must be told that other lanes read these words: to a single thread its own store and its
// loads of the neighbours' slots never alias, and LLVM promotes the stored value to a register and sinks the store out of the
// row loop (seen in k_box_walk's straight-line walk: every row after the first was wrong).  Wavefront-scope fences cost no
// instruction.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Workgroups are dealt round-robin over the 8 XCDs in launch order: workgroup `lin` of `nwg` runs on XCD lin & 7.  The index
// returned here gives every XCD a CONTIGUOUS run of work items instead, so that the workgroups an XCD has in flight are
// neighbours and the lines they share (overlapping tiles, halos, one block's lists) come from HBM once and hit in that XCD's
// L2 afterwards.  A bijection of [0, nwg) for any nwg; every site says what its neighbours share.
__device__ __forceinline__ int xcd_contiguous(int nwg, int lin)
{
    const int xcd = lin & 7;
    return xcd * (nwg >> 3) + min(xcd, nwg & 7) + (lin >> 3);
}

// minimum over the 64 lanes of a wavefront, in every lane
__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

// The same for f32, for a dependent chain that cannot wait for six LDS-crossbar round trips: a running minimum by DPP moves (a lane
// without a source keeps its own value, which min() ignores) leaves the total in lane 63, read from there.  No lane may hold a NaN;
// the sign of a zero result is whichever lane's the reduction meets.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ float dpp_min_f32(float v)
{
    const int b = __float_as_int(v);
    return fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(b, b, CTRL, ROWMASK, 0xf, false)));
}
__device__ __forceinline__ float wave_min(float v)
{
    v = dpp_min_f32<0x111, 0xf>(v);  // row_shr:1
    v = dpp_min_f32<0x112, 0xf>(v);  // row_shr:2
    v = dpp_min_f32<0x114, 0xf>(v);  // row_shr:4
    v = dpp_min_f32<0x118, 0xf>(v);  // row_shr:8   -> lane 15 of each row of 16 holds the row's minimum
    v = dpp_min_f32<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
    v = dpp_min_f32<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// minimum of lo and maximum of hi over the 64 lanes, in every lane (int or uint32_t).  By value: through references the
// accumulators of the caller's loop come out in other registers.
template <class T>
struct MinMax { T lo, hi; };
template <class T>
__device__ __forceinline__ MinMax<T> wave_minmax(T lo, T hi)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, (T)__shfl_xor((int)lo, o));
        hi = max(hi, (T)__shfl_xor((int)hi, o));
    }
    return {lo, hi};
}

// f64 through a DPP control, one 32-bit half at a time; lanes without a source (row edge, masked rows) read 0
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_f64(double v)
{
    const long long b = __double_as_longlong(v);
    int lo, hi;
    if constexpr (ROWMASK == 0xf) {  // shifts inside a row: bound_ctrl supplies the zeros, no 'old' operand to initialise
        lo = __builtin_amdgcn_mov_dpp((int)(uint32_t)b, CTRL, 0xf, 0xf, true);
        hi = __builtin_amdgcn_mov_dpp((int)(uint32_t)((unsigned long long)b >> 32), CTRL, 0xf, 0xf, true);
    } else {                         // row broadcasts into some rows only: the other rows keep old = 0
        lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, ROWMASK, 0xf, false);
        hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)((unsigned long long)b >> 32), CTRL, ROWMASK, 0xf, false);
    }
    return __longlong_as_double((long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo));
}

// inclusive prefix sum over the 64 lanes
__device__ __forceinline__ double wave_inclusive_scan(double v)
{
    v += dpp_f64<0x111, 0xf>(v);  // row_shr:1
    v += dpp_f64<0x112, 0xf>(v);  // row_shr:2
    v += dpp_f64<0x114, 0xf>(v);  // row_shr:4
    v += dpp_f64<0x118, 0xf>(v);  // row_shr:8   -> inclusive inside each row of 16
    v += dpp_f64<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
    v += dpp_f64<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3
    return v;
}

__device__ __forceinline__ int wave_inclusive_scan(int v)
{
    v += __builtin_amdgcn_mov_dpp(v, 0x111, 0xf, 0xf, true);
    v += __builtin_amdgcn_mov_dpp(v, 0x112, 0xf, 0xf, true);
    v += __builtin_amdgcn_mov_dpp(v, 0x114, 0xf, 0xf, true);
    v += __builtin_amdgcn_mov_dpp(v, 0x118, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
    return v;
}

// v of lane l (wave-uniform l), in every lane
__device__ __forceinline__ double readlane_f64(double v, int l)
{
    const long long b = __double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// lut[idx] as a 32-bit byte offset from a uniform base: global_load with an SGPR base, no 64-bit address arithmetic per lane
__device__ __forceinline__ float lut_at(const float* __restrict__ lut, unsigned idx)
{
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(lut) + (idx << 2));
}

// u8 MatExpr (c0+c1+c2)/3 == round((min(255,c0+c1)+c2)/3): no exact .5 can occur, so the
// integer form floor((s+1)/3) is identical to OpenCV's float addWeighted + cvRound (App. A-4;
// tests/test_oracle_kat.py::test_ad_float_formula_equals_integer_rule).  The AD value of k_cost_ad and k_cost_census.
__device__ __forceinline__ uint32_t mean3_u8(int c0, int c1, int c2)
{
    int t = min(255, c0 + c1);
    return (uint32_t)((t + c2 + 1) / 3);
}

// colour distance of two packed BGRX pixels: |db| + |dg| + |dr| in one v_sad_u8
__device__ __forceinline__ uint32_t cdist(uint32_t a, uint32_t b) { return __builtin_amdgcn_sad_u8(a, b, 0u); }
