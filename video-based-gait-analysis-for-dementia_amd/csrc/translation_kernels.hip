// The camera-space trajectory on the device: per frame the translation that makes the predicted 3D joints project onto the 2D detections (SPIN's
// weighted least squares, the reference's estimate_translation_np, lib/utils/geometry.py:296-337), its reprojection error and a status; per
// sequence the fill of the unfitted frames and a summary (definitions, bars and stated differences: DESIGN 4.9; the arithmetic: translation3.h).
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  Every float32 input is widened to float64 and every operation rounds once.
//
// translation_fit_kernel -- ONE LANE PER FRAME, 64 frames a workgroup, grid (frame tiles, sequence of the batch).  Why not a wave per frame: a
// frame is 13 to 64 pairs and seven sums, then a 3x3 solve and a second walk over the pairs that needs the solved t.  A wave per frame would keep
// 13 of its 64 lanes busy at 13 pairs, pay seven cross-lane reductions of float64 (no packed path: two 32-bit moves a step, six steps each), run
// the solve 64 times over, and broadcast t before the second walk; a 10 000-frame job would be 10 000 such waves.  A lane per frame has no
// cross-lane traffic, no LDS and no barrier, every lane does useful float64 work, the sums run in pair-table order exactly as translation3.h
// states them (so the host check runs the very same function), and 10 000 frames are 157 single-wave workgroups (175 in 25 sequences) that spread
// over as many CUs.
// The price is the load pattern: a lane walks its own frame's row (K x 12 bytes, contiguous), so one load instruction touches 64 rows.  Each
// row's cache lines are fetched once and then hit in L1 over the lane's following pairs (64 rows of 25 joints are 19 KB per input), the whole
// input is read from memory once, and at 6 MB for 10 000 frames it is latency, not bandwidth, that the call waits for; a pair-major copy would
// cost a transposing pass over the same bytes first.  The pair table, the offsets and the intrinsics travel as kernel arguments and are read
// with wave-uniform indices.  A frame's row depends on that frame's values and its sequence's (f, cx, cy) alone: the same bits in every call.
//
// translation_seq_kernel -- one workgroup per sequence, behind the fit on the same stream.  Thread t owns frames [t c, (t + 1) c), c =
// ceil(T / 256).  It notes the first and last fitted frame of its block in LDS; after a barrier every thread knows the last fitted frame before
// its block and the first after it, walks its block run by run and writes the filled rows (translation3_fill between two fitted frames, the
// nearest fitted t before the first and after the last; status 3, a NaN error).  Only statuses of the thread's own block are read while others
// write, and only fitted rows -- which nobody writes -- supply t.  After a second barrier the summary: each thread adds its block in frame order
// (fitted and filled counts, the reprojection errors of the fitted frames, the steps |(J_root + t)[i+1] - (J_root + t)[i]| between frames whose t
// are both finite), thread 0 adds the 256 partial sums in block order.  For T <= 256 that is the plain frame-order sum.  No atomics; a sequence's
// rows and summary depend on its own frames alone.
#include "kernels.h"
#include "device.h"
#include "translation3.h"

namespace grk {
namespace {

__global__ __launch_bounds__(64) void translation_fit_kernel(const float* __restrict__ joints3d, const float* __restrict__ joints2d, int K3, int K2,
                                                             TransPairs pairs, TransBatch b, double threshold, int min_joints,
                                                             double* __restrict__ per_frame) {
    const int q = blockIdx.y, f0 = b.off[q], T = b.off[q + 1] - f0;
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= T) return;
    const size_t f = (size_t)f0 + t;
    const Translation3 r = translation3_fit(joints3d + f * (size_t)K3 * 3, joints2d + f * (size_t)K2 * 3, pairs.p3, pairs.p2, pairs.n, b.cam[q][0], b.cam[q][1],
                                            b.cam[q][2], threshold, min_joints);
    double* row = per_frame + f * 6;
    row[0] = r.t[0];
    row[1] = r.t[1];
    row[2] = r.t[2];
    row[3] = r.reproj;
    row[4] = (double)r.n_used;
    row[5] = (double)r.status;
}

__device__ __forceinline__ bool finite3(const double* t) { return translation_detail::finite(t[0]) && translation_detail::finite(t[1]) && translation_detail::finite(t[2]); }

// per_frame is read and written by the threads of one workgroup across barriers: no __restrict__
__global__ __launch_bounds__(256) void translation_seq_kernel(const float* __restrict__ joints3d, int K3, int root, TransBatch b, int seq0, int fill,
                                                              double* per_frame, double* __restrict__ per_seq) {
    __shared__ int first_fit[256], last_fit[256], n_fit[256], n_fill[256];
    __shared__ double sum_reproj[256], sum_path[256];
    const int tid = threadIdx.x, f0 = b.off[blockIdx.x], T = b.off[blockIdx.x + 1] - f0;
    const int c = (T + 255) / 256, lo = min(tid * c, T), hi = min(lo + c, T);
    double* rows = per_frame + (size_t)f0 * 6;
    if (fill) {
        int first = T, last = -1;
        for (int i = lo; i < hi; ++i)
            if (rows[(size_t)i * 6 + 5] == 0.) { if (first == T) first = i; last = i; }
        first_fit[tid] = first;
        last_fit[tid] = last;
        __syncthreads();
        int prev = -1, after = T;
        for (int k = 0; k < tid; ++k) prev = last_fit[k] >= 0 ? last_fit[k] : prev;
        for (int k = 255; k > tid; --k) after = first_fit[k] < T ? first_fit[k] : after;
        const double nan = __builtin_nan("");
        int i = lo;
        while (i < hi) {
            if (rows[(size_t)i * 6 + 5] == 0.) { prev = i++; continue; }
            int e = i;                                         // the run of unfitted frames [i, e) inside this block
            while (e < hi && rows[(size_t)e * 6 + 5] != 0.) ++e;
            const int next = e < hi ? e : after;
            if (prev >= 0 || next < T) {                       // a sequence without a fitted frame keeps its rows
                for (int k = i; k < e; ++k) {
                    double t[3];
                    if (prev >= 0 && next < T) {
                        translation3_fill(rows + (size_t)prev * 6, rows + (size_t)next * 6, next - prev - 1, k - prev, t);
                    } else {
                        const double* src = rows + (size_t)(prev >= 0 ? prev : next) * 6;
                        t[0] = src[0]; t[1] = src[1]; t[2] = src[2];
                    }
                    double* row = rows + (size_t)k * 6;
                    row[0] = t[0]; row[1] = t[1]; row[2] = t[2];
                    row[3] = nan;
                    row[5] = (double)kTransFilled;
                }
            }
            i = e;
        }
        __syncthreads();
    }
    int fitted = 0, filled = 0;
    double reproj = 0., path = 0.;
    const float* jr = joints3d + ((size_t)f0 * K3 + root) * 3;
    for (int i = lo; i < hi; ++i) {
        const double* row = rows + (size_t)i * 6;
        if (row[5] == 0.) { ++fitted; reproj = reproj + row[3]; }
        if (row[5] == (double)kTransFilled) ++filled;
        if (i + 1 < T && finite3(row) && finite3(row + 6)) {
            const float* a = jr + (size_t)i * K3 * 3;
            const float* n = a + (size_t)K3 * 3;
            const double dx = ((double)n[0] + row[6]) - ((double)a[0] + row[0]), dy = ((double)n[1] + row[7]) - ((double)a[1] + row[1]),
                         dz = ((double)n[2] + row[8]) - ((double)a[2] + row[2]);
            path = path + sqrt((dx * dx + dy * dy) + dz * dz);
        }
    }
    n_fit[tid] = fitted; n_fill[tid] = filled; sum_reproj[tid] = reproj; sum_path[tid] = path;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < 256; ++k) { fitted += n_fit[k]; filled += n_fill[k]; reproj = reproj + sum_reproj[k]; path = path + sum_path[k]; }
        double* out = per_seq + ((size_t)seq0 + blockIdx.x) * 4;
        out[0] = (double)fitted;
        out[1] = (double)filled;
        out[2] = fitted > 0 ? reproj / (double)fitted : __builtin_nan("");
        out[3] = path;
    }
}

}  // namespace

hipError_t launch_translation_fit(const float* joints3d, const float* joints2d, int K3, int K2, const TransPairs& pairs, const TransBatch& b, double threshold,
                                  int min_joints, double* per_frame, hipStream_t s) {
    int most = 0;
    for (int q = 0; q < b.n; ++q) most = std::max(most, b.off[q + 1] - b.off[q]);
    return launch_k(translation_fit_kernel, dim3((most + 63) / 64, b.n), dim3(64), 0, s, joints3d, joints2d, K3, K2, pairs, b, threshold, min_joints, per_frame);
}

hipError_t launch_translation_seq(const float* joints3d, int K3, int root, const TransBatch& b, int seq0, int fill, double* per_frame, double* per_seq,
                                  hipStream_t s) {
    return launch_k(translation_seq_kernel, dim3(b.n), dim3(256), 0, s, joints3d, K3, root, b, seq0, fill, per_frame, per_seq);
}

}  // namespace grk
