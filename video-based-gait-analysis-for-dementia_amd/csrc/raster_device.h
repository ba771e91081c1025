// Device-side pieces shared by the two rasterisers, and by them alone (render_kernels.hip, skeleton_kernels.hip): snapped window coordinates, the
// depth key, the pixel tiles of the clear / resolve / winner kernels.
#pragma once
#include "kernels.h"

namespace grk {

constexpr int kSub = 1 << kRasterSnapBits;
constexpr int kHalf = kSub / 2;
constexpr unsigned long long kDepthClear = ~0ull;
constexpr int kTileW = 64, kTileH = 4;                        // pixels per 256-thread workgroup of the clear / resolve / winner kernels

__device__ __forceinline__ int snap(float win) {
    float v = floorf(win * (float)kSub + 0.5f);
    v = fminf(fmaxf(v, -(float)kRasterCoordLimit), (float)kRasterCoordLimit);      // fmaxf(NaN, a) = a
    return (int)v;
}

__device__ __forceinline__ int wave_max64(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// The pixels whose squares [256 i, 256 i + 256) meet [lo, hi]: where a line between lo and hi can put a fragment
__device__ __forceinline__ void pixel_range_squares(int lo, int hi, int n, int& first, int& last) {
    first = max(0, lo >> kRasterSnapBits);
    last = min(n - 1, hi >> kRasterSnapBits);
}

// float -> unsigned with the same order; -0 and +0 differ, so a depth is brought to +0 first (z + 0.f)
__device__ __forceinline__ unsigned ordered_bits(float z) {
    const unsigned u = __float_as_uint(z);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float line_t(const LineRec& r, int m) { return (float)(m * kSub + kHalf - r.P0) / (float)(r.P1 - r.P0); }

}  // namespace grk
