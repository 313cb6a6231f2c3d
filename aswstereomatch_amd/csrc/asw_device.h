// Device-side helpers shared by the kernels: OpenCV border index maps, the wavefront minimum.
#pragma once
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

// minimum over the 64 lanes of a wavefront, in every lane
__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
