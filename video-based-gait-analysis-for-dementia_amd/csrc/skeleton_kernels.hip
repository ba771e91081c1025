// The 3D skeleton view of demo.py --skeleton_view on the device (demo.py:303-361 without --mesh_render, lib/utils/vis.py:571-587: matplotlib's 3D
// axes with the joints of every tracked person as coloured bones).  What is drawn is a stated rule, NOT matplotlib's Agg renderer:
// wide, non-antialiased lines without caps and without joins, one colour per segment, no shading.  All float arithmetic is fp32; after the points
// are snapped, coverage is the integer arithmetic of raster_lines.h, so it depends neither on the order in which threads run nor on what the
// compiler contracts.
//
// A launch group is up to kRasterSlots IMAGES, slot s with its own depth image and bounding box in the render workspace.  ALL skeletons aimed at
// an image share its depth image -- the reference draws every person of a frame into one axes -- and go through in batches of up to
// kSegBatchSkeletons skeletons, whose records (SegSkeleton: row of the call's points, slot, rank) are a kernel argument (SegBatch).
//
// segments_setup_kernel -- one thread per (skeleton, point): p' = R p; hw = Wh . (p', 1); x_win = cx + X . (p', 1) / hw, y_win likewise (the host
//   folds matplotlib's projection P and the window onto the centred S x S square, S = min(H, W), into X, Y, Wh, cx, cy in double: GL window
//   coordinates, origin bottom-left); snapped to 8 sub-pixel bits; depth d = Wh[0..2] . p' = hw minus the eye distance, so |d| stays near 1.  A
//   point is INVALID -- both coordinates INT_MIN -- if p' is not finite, hw <= 0, or a window coordinate exceeds 2^20 pixels in magnitude (so
//   |X|, |Y| <= 2^28 = kRasterCoordLimit and raster_lines.h's bounds hold).  The slot's bounding box is the wave's maximum of
//   (-X, -Y, X, Y) + pad, pad = (w_max - 1) 128: the column of a wide line reaches (w - 1) / 2 pixels beside the line; one atomicMax per wave.
// raster_clear_kernel<true> (render_kernels.hip) -- depth = all ones over the pixels whose squares meet a slot's box.
// segments_cover_kernel -- one WAVE per (skeleton, segment); a segment with an invalid end, or of length 0, draws nothing.  Ends ordered and
//   major axis chosen by line_order; major index m covered iff P0 <= 256 m + 128 < P1; lanes take m0 + lane, + 64, ...: one division
//   (line_minor_wide, the width's offset in the numerator) at a lane's first m, then line_stride(64) / line_advance.  The column n0 .. n0 + w - 1
//   inside the viewport gets ONE depth, d = fma(t, d1 - d0, d0) + 0 with the wireframe's t at m, as w 64-bit atomicMins on
//   (ordered(d) << 32) | (rank S + segment): GL_LESS, the lower id winning at equal depth, whatever the order of execution.
// segments_resolve_kernel -- one thread per pixel of a slot's box: the segment from the key's low word modulo S, its three colour bytes stored;
//   every other byte of the image is left as it is.
#include "raster_device.h"

namespace grk {
namespace {

__global__ __launch_bounds__(256) void segments_setup_kernel(const float* __restrict__ points, SegView v, SegTables t, SegBatch b, int pad, RasterWork w) {
    const int k = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const SegSkeleton sk = b.rec[k];
    int b0 = INT_MIN, b1 = INT_MIN, b2 = INT_MIN, b3 = INT_MIN;
    if (p < t.P) {
        const float* src = points + ((size_t)sk.index * t.P + p) * 3;
        const float x = src[0], y = src[1], z = src[2];
        const float px = v.R[0] * x + v.R[1] * y + v.R[2] * z;
        const float py = v.R[3] * x + v.R[4] * y + v.R[5] * z;
        const float pz = v.R[6] * x + v.R[7] * y + v.R[8] * z;
        const float d = v.Wh[0] * px + v.Wh[1] * py + v.Wh[2] * pz;
        const float hw = d + v.Wh[3];
        int X = INT_MIN, Y = INT_MIN;
        if (isfinite(px) && isfinite(py) && isfinite(pz) && hw > 0.f) {
            const float xw = v.cx + (v.X[0] * px + v.X[1] * py + v.X[2] * pz + v.X[3]) / hw;
            const float yw = v.cy + (v.Y[0] * px + v.Y[1] * py + v.Y[2] * pz + v.Y[3]) / hw;
            if (fabsf(xw) <= (float)kSegWindowLimit && fabsf(yw) <= (float)kSegWindowLimit) {      // false for a NaN
                X = snap(xw), Y = snap(yw);
                b0 = pad - X, b1 = pad - Y, b2 = pad + X, b3 = pad + Y;
            }
        }
        const size_t o = (size_t)(b.base + k) * t.P + p;
        w.xy[o * 2 + 0] = X;
        w.xy[o * 2 + 1] = Y;
        w.z[o] = X == INT_MIN ? 0.f : d;
    }
    b0 = wave_max64(b0), b1 = wave_max64(b1), b2 = wave_max64(b2), b3 = wave_max64(b3);
    if ((threadIdx.x & 63) == 0 && b2 != INT_MIN) {
        int* bb = w.bbox + sk.slot * 4;
        atomicMax(bb + 0, b0);
        atomicMax(bb + 1, b1);
        atomicMax(bb + 2, b2);
        atomicMax(bb + 3, b3);
    }
}

__device__ __forceinline__ bool snapped_ok(int c) { return c >= -kRasterCoordLimit && c <= kRasterCoordLimit; }      // false for the sentinel

__global__ __launch_bounds__(256) void segments_cover_kernel(SegView v, SegTables t, SegBatch b, RasterWork w) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= (long long)b.n * t.S) return;                      // wave-uniform, as everything up to the lane's first m
    const int k = (int)(g / t.S), s = (int)(g - (long long)k * t.S);
    const SegSkeleton sk = b.rec[k];
    const SegSegment sg = t.seg[s];
    const int* xy = w.xy + (size_t)(b.base + k) * t.P * 2;
    const float* dv = w.z + (size_t)(b.base + k) * t.P;
    const int ax = xy[2 * sg.a], ay = xy[2 * sg.a + 1], bx = xy[2 * sg.b], by = xy[2 * sg.b + 1];
    if (!snapped_ok(ax) || !snapped_ok(ay) || !snapped_ok(bx) || !snapped_ok(by)) return;
    LineRec r{};
    bool flip = false;
    if (!line_order(ax, ay, bx, by, r, flip)) return;
    r.z0 = flip ? dv[sg.b] : dv[sg.a], r.z1 = flip ? dv[sg.a] : dv[sg.b];
    line_range(r, r.xmajor ? v.W : v.H);
    if (r.m0 + lane > r.m1) return;
    const int n_minor = r.xmajor ? v.H : v.W;
    unsigned long long* depth = w.depth + (size_t)sk.slot * v.H * v.W;
    const unsigned id = (unsigned)sk.rank * (unsigned)t.S + (unsigned)s;
    const LineStride st = line_stride(r, 64);
    long long n, rem;
    line_minor_wide(r, r.m0 + lane, sg.width, n, rem);       // m0 + lane <= 4095 + 63: the numerator stays far inside int64
    for (int m = r.m0 + lane; m <= r.m1; m += 64, line_advance(st, n, rem)) {
        const float d = fmaf(line_t(r, m), r.z1 - r.z0, r.z0) + 0.f;                  // + 0: -0 and +0 are one depth
        const unsigned long long key = ((unsigned long long)ordered_bits(d) << 32) | id;
        const int lo = (int)(n > 0 ? n : 0), hi = (int)(n + sg.width - 1 < n_minor - 1 ? n + sg.width - 1 : n_minor - 1);      // the column cut by the viewport
        for (int q = lo; q <= hi; ++q) {
            const int i = r.xmajor ? m : q, j = r.xmajor ? q : m;
            atomicMin(depth + (size_t)j * v.W + i, key);
        }
    }
}

__global__ __launch_bounds__(256) void segments_resolve_kernel(SegView v, SegGroup g, SegTables t, RasterWork w, unsigned char* __restrict__ images) {
    const int slot = blockIdx.z;
    const int* bbox = w.bbox + slot * 4;
    int i0, i1, j0, j1;
    pixel_range_squares(-bbox[0], bbox[2], v.W, i0, i1);
    pixel_range_squares(-bbox[1], bbox[3], v.H, j0, j1);
    const int i = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1)), j = blockIdx.y * kTileH + threadIdx.x / kTileW;
    if (i < i0 || i > i1 || j < j0 || j > j1) return;
    const unsigned long long key = w.depth[(size_t)slot * v.H * v.W + (size_t)j * v.W + i];
    if (key == kDepthClear) return;
    const unsigned c = (unsigned)t.seg[(unsigned)key % (unsigned)t.S].colour;
    unsigned char* out = images + (((size_t)g.image[slot] * v.H + (v.H - 1 - j)) * v.W + i) * 3;
    out[0] = (unsigned char)(c & 255u);
    out[1] = (unsigned char)((c >> 8) & 255u);
    out[2] = (unsigned char)((c >> 16) & 255u);
}

}  // namespace

hipError_t launch_segments_setup(const float* points, const SegView& v, SegTables t, const SegBatch& b, int pad, RasterWork w, hipStream_t s) {
    hipLaunchKernelGGL(segments_setup_kernel, dim3((t.P + 255) / 256, b.n), dim3(256), 0, s, points, v, t, b, pad, w);
    return hipGetLastError();
}

hipError_t launch_segments_cover(const SegView& v, SegTables t, const SegBatch& b, RasterWork w, hipStream_t s) {
    const long long waves = (long long)b.n * t.S;
    if (!waves) return hipSuccess;
    hipLaunchKernelGGL(segments_cover_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, v, t, b, w);
    return hipGetLastError();
}

hipError_t launch_segments_resolve(const SegView& v, const SegGroup& g, SegTables t, RasterWork w, unsigned char* images, hipStream_t s) {
    hipLaunchKernelGGL(segments_resolve_kernel, dim3((v.W + kTileW - 1) / kTileW, (v.H + kTileH - 1) / kTileH, g.n), dim3(256), 0, s, v, g, t, w, images);
    return hipGetLastError();
}

}  // namespace grk
