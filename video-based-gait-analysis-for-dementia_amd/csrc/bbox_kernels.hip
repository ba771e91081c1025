// One box per sequence from 2D joints (batch_generation.py:39-93, get_bbox_from_joints2d; rules and bound: DESIGN 4.7).  The reference clusters all
// joints of a sequence with K-medoids, k = 1: its fixed point is the exact 1-medoid, argmin_i sum_j |p_i - p_j| over the n = T K points (x, y, score).
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  The prepare and assemble steps are the reference's float64 numpy expressions in the
// reference's order, one rounding per operation, so the box is the reference's bit for bit.  The two fmaf of the row-sum kernel are written out.
//
// bbox_prepare_kernel -- one WAVE per frame, lane j < K owns joint j.  np.argmax of the scores is a wave maximum and the lowest lane that holds it;
// joints whose score is below the threshold take that joint's three components; min / max of x and y are wave reductions (exact, order-free);
// lane 0 forms h = lr_y - (ul_y - (lr_y - ul_y) 0.10).  The points leave as float32 (x, y, s, 0), 16 bytes each.  (The reference also forms w and
// its median, :62,76, and overwrites both at :87; neither is computed here.)
//
// medoid_rowsum_kernel -- the hot path.  Grid (row tile, column split, sequence), 256 threads: thread r keeps row point i = 256 tile + r in registers
// and walks the split's columns, staged through LDS 1024 points (16 KiB) at a time.  Every lane reads the SAME column, so the LDS read is a broadcast
// of one ds_read_b128 per pair, conflict-free.  Per pair: three differences, d2 = fma(ds, ds, fma(dy, dy, dx dx)), ONE v_sqrt_f32 (<= 1 ulp), widened
// and added in float64.  Columns go eight at a time into four float64 accumulators, so the adds and square roots of neighbouring pairs overlap; the
// accumulators are added in a fixed order.  The split's sum goes to partial[split][i]: no atomics, the result does not depend on scheduling.
//
// medoid_argmin_kernel -- one workgroup per sequence: cost_i = the splits' partial sums added in split order; the smallest cost, lowest index on ties.
// bbox_assemble_kernel -- one workgroup per sequence: the median of h by exact rank counting in LDS (T <= 4096; (a + b) / 2 of the two middle
// elements, which is np.median for odd T too), then :87-90.
#include "kernels.h"
#include "device.h"

namespace grk {
namespace {

__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(256) void bbox_prepare_kernel(const double* __restrict__ joints, int K, int frames, double threshold,
                                                           f32x4* __restrict__ points, double* __restrict__ hgt) {
    const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= frames) return;                                   // wave-uniform
    const bool on = lane < K;
    const double* p = joints + ((size_t)f * K + (on ? lane : 0)) * 3;
    double x = p[0], y = p[1], s = p[2];
    const double inf = __builtin_huge_val();
    const double smax = wave_max_f64(on ? s : -inf);
    const int best = __ffsll((long long)__ballot(on && s == smax)) - 1;      // np.argmax: the first index of the maximum
    const double bx = __shfl(x, best, 64), by = __shfl(y, best, 64), bs = __shfl(s, best, 64);
    if (s < threshold) { x = bx; y = by; s = bs; }
    const double ul_x = wave_min_f64(on ? x : inf), lr_x = wave_max_f64(on ? x : -inf);
    double ul_y = wave_min_f64(on ? y : inf);
    const double lr_y = wave_max_f64(on ? y : -inf);
    (void)ul_x; (void)lr_x;                                    // w = lr_x - ul_x only feeds the median the reference drops
    if (on) points[(size_t)f * K + lane] = f32x4{(float)x, (float)y, (float)s, 0.f};
    if (lane == 0) {
        const double head = (lr_y - ul_y) * 0.10;              // :61, prevent cutting the head
        ul_y = ul_y - head;
        hgt[f] = lr_y - ul_y;
    }
}

__device__ __forceinline__ double pair_distance(const f32x4 p, const f32x4 q) {
    const float dx = p[0] - q[0], dy = p[1] - q[1], ds = p[2] - q[2];
    return (double)__builtin_amdgcn_sqrtf(fmaf(ds, ds, fmaf(dy, dy, dx * dx)));
}

__global__ __launch_bounds__(256) void medoid_rowsum_kernel(const f32x4* __restrict__ points, MedoidBatch b, int splits, double* __restrict__ partial) {
    __shared__ f32x4 tile[kMedoidTile];
    const int tid = threadIdx.x, p0 = b.off[blockIdx.z], n = b.off[blockIdx.z + 1] - p0;
    if ((int)blockIdx.x * kMedoidRows >= n) return;            // a shorter sequence of the batch: uniform for the workgroup
    const int row = blockIdx.x * kMedoidRows + tid;
    const f32x4* pts = points + p0;
    const f32x4 p = pts[min(row, n - 1)];
    const int chunk = medoid_split_columns(n, splits);
    const int c0 = min(n, (int)blockIdx.y * chunk), c1 = min(n, c0 + chunk);
    double acc[4] = {0., 0., 0., 0.};
    for (int t0 = c0; t0 < c1; t0 += kMedoidTile) {
        const int m = min(kMedoidTile, c1 - t0);
        if (t0 > c0) __syncthreads();                          // the previous tile has been read
        for (int j = tid; j < m; j += 256) tile[j] = pts[t0 + j];
        __syncthreads();
        int j = 0;
        for (; j + 8 <= m; j += 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u & 3] += pair_distance(p, tile[j + u]);
        }
        for (; j < m; ++j) acc[0] += pair_distance(p, tile[j]);
    }
    if (row < n) partial[(size_t)splits * p0 + (size_t)blockIdx.y * n + row] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

__global__ __launch_bounds__(256) void medoid_argmin_kernel(const f32x4* __restrict__ points, MedoidBatch b, int seq0, int splits,
                                                            const double* __restrict__ partial, int* __restrict__ index, double* __restrict__ cost,
                                                            float* __restrict__ centre) {
    __shared__ double sc[256];
    __shared__ int si[256];
    const int tid = threadIdx.x, p0 = b.off[blockIdx.x], n = b.off[blockIdx.x + 1] - p0;
    const double* part = partial + (size_t)splits * p0;
    double best = __builtin_huge_val();
    int at = 0x7fffffff;
    for (int i = tid; i < n; i += 256) {
        double c = 0.;
        for (int s = 0; s < splits; ++s) c += part[(size_t)s * n + i];
        if (c < best) { best = c; at = i; }                    // ascending i: the first of equal costs stays
    }
    sc[tid] = best, si[tid] = at;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            const double c = sc[tid + o];
            const int i = si[tid + o];
            if (c < sc[tid] || (c == sc[tid] && i < si[tid])) { sc[tid] = c; si[tid] = i; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int q = seq0 + blockIdx.x, i = si[0] < n ? si[0] : 0;      // no finite cost (non-finite points): stay inside the sequence
        if (index) index[q] = i;
        if (cost) cost[q] = sc[0];
        if (centre) { const f32x4 m = points[p0 + i]; centre[2 * q] = m[0]; centre[2 * q + 1] = m[1]; }
    }
}

__global__ __launch_bounds__(256) void bbox_assemble_kernel(const double* __restrict__ hgt, MedoidBatch b, int seq0, int K, const float* __restrict__ centre,
                                                            double* __restrict__ bbox) {
    __shared__ double sh[kBboxMaxFrames];
    __shared__ double mid[2];
    const int tid = threadIdx.x, f0 = b.off[blockIdx.x] / K, T = (b.off[blockIdx.x + 1] - b.off[blockIdx.x]) / K;
    for (int t = tid; t < T; t += 256) sh[t] = hgt[f0 + t];
    if (tid < 2) mid[tid] = __builtin_nan("");                 // stays if a non-finite height leaves a rank unclaimed
    __syncthreads();
    const int lo = (T - 1) / 2, hi = T / 2;                    // the two middle ranks (equal for odd T)
    for (int t = tid; t < T; t += 256) {
        const double v = sh[t];
        int rank = 0;                                          // position of element t in a stable sort
        for (int u = 0; u < T; ++u) rank += (sh[u] < v || (sh[u] == v && u < t)) ? 1 : 0;
        if (rank == lo) mid[0] = v;
        if (rank == hi) mid[1] = v;
    }
    __syncthreads();
    if (tid == 0) {
        const int q = seq0 + blockIdx.x;
        const double med = (mid[0] + mid[1]) / 2.;
        double nh = med * 1.1;                                 // :87 nw = nh = nh * 1.1: the width is the height's, to keep the aspect ratio
        if (nh < kBboxMinPixel) nh = nh * kBboxSmallScale;     // :88-89
        bbox[4 * q] = (double)centre[2 * q];
        bbox[4 * q + 1] = (double)centre[2 * q + 1];
        bbox[4 * q + 2] = nh;
        bbox[4 * q + 3] = nh;
    }
}

}  // namespace

hipError_t launch_bbox_prepare(const double* joints, int K, int frames, double threshold, float* points, double* hgt, hipStream_t s) {
    return launch_k(bbox_prepare_kernel, dim3((frames + 3) / 4), dim3(256), 0, s, joints, K, frames, threshold, reinterpret_cast<f32x4*>(points), hgt);
}

hipError_t launch_medoid_rowsum(const float* points, const MedoidBatch& b, int splits, double* partial, hipStream_t s) {
    int most = 0;
    for (int q = 0; q < b.n; ++q) most = std::max(most, b.off[q + 1] - b.off[q]);
    return launch_k(medoid_rowsum_kernel, dim3((most + kMedoidRows - 1) / kMedoidRows, splits, b.n), dim3(256), 0, s,
                    reinterpret_cast<const f32x4*>(points), b, splits, partial);
}

hipError_t launch_medoid_argmin(const float* points, const MedoidBatch& b, int seq0, int splits, const double* partial, int* index, double* cost,
                                float* centre, hipStream_t s) {
    return launch_k(medoid_argmin_kernel, dim3(b.n), dim3(256), 0, s, reinterpret_cast<const f32x4*>(points), b, seq0, splits, partial, index, cost, centre);
}

hipError_t launch_bbox_assemble(const double* hgt, const MedoidBatch& b, int seq0, int K, const float* centre, double* bbox, hipStream_t s) {
    return launch_k(bbox_assemble_kernel, dim3(b.n), dim3(256), 0, s, hgt, b, seq0, K, centre, bbox);
}

}  // namespace grk
