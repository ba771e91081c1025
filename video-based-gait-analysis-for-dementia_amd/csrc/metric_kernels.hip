// Pose metrics of the VIBE / PARE / SPIN family on the device: MPJPE, PA-MPJPE, PVE, acceleration and acceleration error (definitions, loop
// structure and error bound: DESIGN 4.8).  The reference has no evaluation code; DESIGN 4.8 is the specification.
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  Every float32 input is widened to float64 and every operation below rounds once,
// so the bound of DESIGN 4.8 counts the roundings that the text below shows, and no others.
//
// metric_joints_kernel -- one WAVE per frame, lane j < m owns selected joint j.  aligned_joint() subtracts the mean of the root joints (a wave sum
// over the r root lanes); the joint means, var1, the nine entries of K = X1 X2^T and the error sums are wave sums: an xor butterfly over all 64
// lanes, lanes >= m adding +0, so every lane ends with the same bits and the order never depends on the call.  Every lane then runs procrustes3()
// (procrustes3.h) on the same K -- no divergence, no broadcast -- and lane 0 writes mpjpe, pa_mpjpe and the structural NaNs of the row.
// metric_accel_kernel -- one wave per INTERIOR frame of a sequence, grid (frame tiles, sequence of the batch): the same aligned_joint() for
// f - 1, f, f + 1, second differences (P[f-1] - 2 P[f]) + P[f+1] of P and of P - G, two wave sums.
// metric_verts_kernel -- the stage that moves bytes (165 KB per frame at V = 6890).  One workgroup per frame; thread t owns the vertex pairs
// t, t + 256, ... (pair p = vertices 2p, 2p + 1: 24 contiguous bytes, three 8-byte loads where the frame starts 8-byte aligned -- 3 V even, as at
// 6890 -- else six 4-byte loads of the same floats); four pairs are in flight per thread, each with its own accumulator, added ((0+1)+(2+3)), then
// the wave butterfly, then the four waves in wave order.  Both load forms feed the same sequence of additions.
// metric_seq_means_kernel -- one workgroup per sequence: thread t adds the rows t, t + 256, ... in frame order, a fixed LDS tree adds the threads.
// Which entries count is structural (every frame for mpjpe and pa_mpjpe, every frame or none for pve, the interior frames for the two
// accelerations), never a test of the value.  The sums and counts stay in the scratch; metric_total_kernel adds them the same way in sequence order.
// No atomics; a frame's row depends on that frame's (and its neighbours') values alone, a sequence's means on its rows alone.
#include "kernels.h"
#include "device.h"
#include "procrustes3.h"

namespace grk {
namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

struct Joint3 { double x, y, z; };

// joint `sel` of frame f after root alignment: widened, minus the mean of the frame's root joints (lane k < n_root loads root joint k)
__device__ __forceinline__ Joint3 aligned_joint(const float* __restrict__ joints, size_t f, int J, int sel, bool on, const MetricJoints& mj, int lane) {
    const float* base = joints + f * (size_t)J * 3;
    Joint3 p{0., 0., 0.};
    if (on) { p.x = (double)base[3 * sel]; p.y = (double)base[3 * sel + 1]; p.z = (double)base[3 * sel + 2]; }
    if (mj.n_root > 0) {
        double rx = 0., ry = 0., rz = 0.;
        if (lane < mj.n_root) { const int k = mj.root[lane]; rx = (double)base[3 * k]; ry = (double)base[3 * k + 1]; rz = (double)base[3 * k + 2]; }
        const double inv = (double)mj.n_root;
        rx = wave_sum_f64(rx) / inv; ry = wave_sum_f64(ry) / inv; rz = wave_sum_f64(rz) / inv;
        if (on) { p.x = p.x - rx; p.y = p.y - ry; p.z = p.z - rz; }
    }
    return p;
}

__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

__global__ __launch_bounds__(256) void metric_joints_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int J, int frames, MetricJoints mj,
                                                            double unit, int has_verts, double* __restrict__ per_frame, double* __restrict__ transform) {
    const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= frames) return;                                   // wave-uniform
    const int m = mj.n_select;
    const bool on = lane < m;
    const int sel = on ? mj.select[lane] : 0;
    const Joint3 P = aligned_joint(pred, f, J, sel, on, mj, lane), G = aligned_joint(gt, f, J, sel, on, mj, lane);
    const double dm = (double)m;
    const double mpjpe = wave_sum_f64(on ? norm3(P.x - G.x, P.y - G.y, P.z - G.z) : 0.) / dm;
    const double m1x = wave_sum_f64(P.x) / dm, m1y = wave_sum_f64(P.y) / dm, m1z = wave_sum_f64(P.z) / dm;      // lanes >= m hold 0
    const double m2x = wave_sum_f64(G.x) / dm, m2y = wave_sum_f64(G.y) / dm, m2z = wave_sum_f64(G.z) / dm;
    double x1[3] = {0., 0., 0.}, x2[3] = {0., 0., 0.};
    if (on) { x1[0] = P.x - m1x; x1[1] = P.y - m1y; x1[2] = P.z - m1z; x2[0] = G.x - m2x; x2[1] = G.y - m2y; x2[2] = G.z - m2z; }
    const double var1 = wave_sum_f64((x1[0] * x1[0] + x1[1] * x1[1]) + x1[2] * x1[2]);
    double K[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) K[3 * a + b] = wave_sum_f64(x1[a] * x2[b]);
    double s = 0., R[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.};
    if (var1 > 0.) {                                           // var1 == 0: all selected pred joints equal -- s = 0, R = I is the least-squares minimiser
        const Procrustes3 pr = procrustes3(K);
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = pr.R[i];
        double tr = 0.;
#pragma unroll
        for (int i = 0; i < 3; ++i) tr = tr + ((R[3 * i] * K[i] + R[3 * i + 1] * K[3 + i]) + R[3 * i + 2] * K[6 + i]);
        s = tr / var1;
    }
    const double m1[3] = {m1x, m1y, m1z}, m2[3] = {m2x, m2y, m2z}, p[3] = {P.x, P.y, P.z}, g[3] = {G.x, G.y, G.z};
    double t[3], e[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        t[i] = m2[i] - s * ((R[3 * i] * m1[0] + R[3 * i + 1] * m1[1]) + R[3 * i + 2] * m1[2]);
        e[i] = (s * ((R[3 * i] * p[0] + R[3 * i + 1] * p[1]) + R[3 * i + 2] * p[2]) + t[i]) - g[i];
    }
    const double pa = wave_sum_f64(on ? norm3(e[0], e[1], e[2]) : 0.) / dm;
    if (lane == 0) {
        const double nan = __builtin_nan("");
        double* row = per_frame + (size_t)f * 5;
        row[0] = mpjpe * unit;
        row[1] = pa * unit;
        if (!has_verts) row[2] = nan;                          // the vertices kernel writes it otherwise
        row[3] = nan;                                          // the acceleration kernel, launched behind this one, overwrites the interior frames
        row[4] = nan;
        if (transform) {
            double* tf = transform + (size_t)f * 13;
            tf[0] = s;
#pragma unroll
            for (int i = 0; i < 9; ++i) tf[1 + i] = R[i];
            tf[10] = t[0]; tf[11] = t[1]; tf[12] = t[2];
        }
    }
}

__global__ __launch_bounds__(256) void metric_accel_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int J, MetricBatch b, MetricJoints mj,
                                                           double unit, double* __restrict__ per_frame) {
    const int lane = threadIdx.x & 63, f0 = b.off[blockIdx.y], T = b.off[blockIdx.y + 1] - f0;
    const int tf = 1 + blockIdx.x * 4 + (threadIdx.x >> 6);    // interior frames 1 .. T - 2
    if (tf > T - 2) return;                                    // wave-uniform
    const size_t f = (size_t)f0 + tf;
    const int m = mj.n_select;
    const bool on = lane < m;
    const int sel = on ? mj.select[lane] : 0;
    const Joint3 Pa = aligned_joint(pred, f - 1, J, sel, on, mj, lane), Ga = aligned_joint(gt, f - 1, J, sel, on, mj, lane);
    const Joint3 Pb = aligned_joint(pred, f, J, sel, on, mj, lane), Gb = aligned_joint(gt, f, J, sel, on, mj, lane);
    const Joint3 Pc = aligned_joint(pred, f + 1, J, sel, on, mj, lane), Gc = aligned_joint(gt, f + 1, J, sel, on, mj, lane);
    const double ax = (Pa.x - 2. * Pb.x) + Pc.x, ay = (Pa.y - 2. * Pb.y) + Pc.y, az = (Pa.z - 2. * Pb.z) + Pc.z;
    const double ex = ((Pa.x - Ga.x) - 2. * (Pb.x - Gb.x)) + (Pc.x - Gc.x), ey = ((Pa.y - Ga.y) - 2. * (Pb.y - Gb.y)) + (Pc.y - Gc.y),
                 ez = ((Pa.z - Ga.z) - 2. * (Pb.z - Gb.z)) + (Pc.z - Gc.z);
    const double dm = (double)m;
    const double accel = wave_sum_f64(on ? norm3(ax, ay, az) : 0.) / dm, err = wave_sum_f64(on ? norm3(ex, ey, ez) : 0.) / dm;
    if (lane == 0) {
        per_frame[f * 5 + 3] = accel * unit;
        per_frame[f * 5 + 4] = err * unit;
    }
}

struct PairFloats { float v[6]; };      // two vertices

template <bool kWide>
__device__ __forceinline__ PairFloats load_pair(const float* __restrict__ frame, int pair, int V) {
    PairFloats r;
    if (2 * pair + 1 < V) {
        const float* p = frame + (size_t)pair * 6;
        if (kWide) {
#pragma unroll
            for (int i = 0; i < 3; ++i) { const f32x2 w = *reinterpret_cast<const f32x2*>(p + 2 * i); r.v[2 * i] = w[0]; r.v[2 * i + 1] = w[1]; }
        } else {
#pragma unroll
            for (int i = 0; i < 6; ++i) r.v[i] = p[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) r.v[i] = 0.f;
        if (2 * pair < V) {                                    // the last vertex of an odd V
            const float* p = frame + (size_t)pair * 6;
            r.v[0] = p[0]; r.v[1] = p[1]; r.v[2] = p[2];
        }
    }
    return r;
}

template <bool kWide>
__global__ __launch_bounds__(256) void metric_verts_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int V, double unit,
                                                           double* __restrict__ per_frame) {
    __shared__ double wave_sums[4];
    const int tid = threadIdx.x;
    const size_t f = blockIdx.x;
    const float* pf = pred + f * (size_t)V * 3;
    const float* gf = gt + f * (size_t)V * 3;
    const int pairs = (V + 1) / 2;
    double acc[4] = {0., 0., 0., 0.};
    for (int p0 = tid; p0 < pairs; p0 += 4 * 256) {
        PairFloats a[4], c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {                          // a pair past the end loads nothing and adds +0: the sums keep their bits
            a[u] = load_pair<kWide>(pf, p0 + 256 * u, V);
            c[u] = load_pair<kWide>(gf, p0 + 256 * u, V);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double d0 = norm3((double)a[u].v[0] - (double)c[u].v[0], (double)a[u].v[1] - (double)c[u].v[1], (double)a[u].v[2] - (double)c[u].v[2]);
            const double d1 = norm3((double)a[u].v[3] - (double)c[u].v[3], (double)a[u].v[4] - (double)c[u].v[4], (double)a[u].v[5] - (double)c[u].v[5]);
            acc[u] = (acc[u] + d0) + d1;
        }
    }
    const double w = wave_sum_f64((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if ((tid & 63) == 0) wave_sums[tid >> 6] = w;
    __syncthreads();
    if (tid == 0) per_frame[f * 5 + 2] = ((((wave_sums[0] + wave_sums[1]) + wave_sums[2]) + wave_sums[3]) / (double)V) * unit;
}

// the five sums of 256 threads, added by a fixed tree; the result in sh[0 .. 4]
__device__ __forceinline__ void block_sum5(double (&v)[5], double* sh, int tid) {
#pragma unroll
    for (int c = 0; c < 5; ++c) sh[c * 256 + tid] = v[c];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int c = 0; c < 5; ++c) sh[c * 256 + tid] = sh[c * 256 + tid] + sh[c * 256 + tid + o];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void metric_seq_means_kernel(const double* __restrict__ per_frame, MetricBatch b, int seq0, int has_verts,
                                                               double* __restrict__ seq_sum, long long* __restrict__ seq_cnt, double* __restrict__ per_seq) {
    __shared__ double sh[5 * 256];
    const int tid = threadIdx.x, f0 = b.off[blockIdx.x], T = b.off[blockIdx.x + 1] - f0;
    double v[5] = {0., 0., 0., 0., 0.};
    for (int t = tid; t < T; t += 256) {
        const double* row = per_frame + ((size_t)f0 + t) * 5;
        v[0] = v[0] + row[0];
        v[1] = v[1] + row[1];
        if (has_verts) v[2] = v[2] + row[2];
        if (t > 0 && t < T - 1) { v[3] = v[3] + row[3]; v[4] = v[4] + row[4]; }
    }
    block_sum5(v, sh, tid);
    if (tid < 5) {
        const long long cnt = tid < 2 ? T : (tid == 2 ? (has_verts ? T : 0) : (T > 2 ? T - 2 : 0));
        const size_t q = (size_t)seq0 + blockIdx.x;
        const double sum = sh[tid * 256];
        seq_sum[q * 5 + tid] = sum;
        seq_cnt[q * 5 + tid] = cnt;
        if (per_seq) per_seq[q * 5 + tid] = cnt > 0 ? sum / (double)cnt : __builtin_nan("");
    }
}

__global__ __launch_bounds__(256) void metric_total_kernel(const double* __restrict__ seq_sum, const long long* __restrict__ seq_cnt, int n_seq,
                                                           double* __restrict__ total) {
    __shared__ double sh[5 * 256];
    __shared__ long long cnt_sh[5 * 256];
    const int tid = threadIdx.x;
    double v[5] = {0., 0., 0., 0., 0.};
    long long n[5] = {0, 0, 0, 0, 0};
    for (int q = tid; q < n_seq; q += 256)
#pragma unroll
        for (int c = 0; c < 5; ++c) { v[c] = v[c] + seq_sum[(size_t)q * 5 + c]; n[c] += seq_cnt[(size_t)q * 5 + c]; }
#pragma unroll
    for (int c = 0; c < 5; ++c) cnt_sh[c * 256 + tid] = n[c];
    block_sum5(v, sh, tid);                                    // its barriers also order cnt_sh
    if (tid < 5) {
        long long cnt = 0;
        for (int i = 0; i < 256; ++i) cnt += cnt_sh[tid * 256 + i];
        total[tid] = cnt > 0 ? sh[tid * 256] / (double)cnt : __builtin_nan("");
    }
}

__global__ __launch_bounds__(64) void procrustes_kernel(const double* __restrict__ K, int k, double* __restrict__ R, double* __restrict__ sigma) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= k) return;
    double Kl[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) Kl[e] = K[(size_t)i * 9 + e];
    const Procrustes3 pr = procrustes3(Kl);
#pragma unroll
    for (int e = 0; e < 9; ++e) R[(size_t)i * 9 + e] = pr.R[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) sigma[(size_t)i * 3 + e] = pr.sigma[e];
}

}  // namespace

hipError_t launch_metric_joints(const float* pred, const float* gt, int J, int frames, const MetricJoints& mj, double unit, int has_verts, double* per_frame,
                                double* transform, hipStream_t s) {
    return launch_k(metric_joints_kernel, dim3((frames + 3) / 4), dim3(256), 0, s, pred, gt, J, frames, mj, unit, has_verts, per_frame, transform);
}

hipError_t launch_metric_accel(const float* pred, const float* gt, int J, const MetricBatch& b, const MetricJoints& mj, double unit, double* per_frame,
                               hipStream_t s) {
    int most = 0;
    for (int q = 0; q < b.n; ++q) most = std::max(most, b.off[q + 1] - b.off[q]);
    if (most < 3) return hipSuccess;                           // no interior frame in the batch
    return launch_k(metric_accel_kernel, dim3((most - 2 + 3) / 4, b.n), dim3(256), 0, s, pred, gt, J, b, mj, unit, per_frame);
}

hipError_t launch_metric_verts(const float* pred, const float* gt, int V, int frames, double unit, double* per_frame, hipStream_t s) {
    const bool wide = (3 * (long long)V) % 2 == 0 && !((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(gt)) & 7);
    if (wide) return launch_k(metric_verts_kernel<true>, dim3(frames), dim3(256), 0, s, pred, gt, V, unit, per_frame);
    return launch_k(metric_verts_kernel<false>, dim3(frames), dim3(256), 0, s, pred, gt, V, unit, per_frame);
}

hipError_t launch_metric_seq_means(const double* per_frame, const MetricBatch& b, int seq0, int has_verts, double* seq_sum, long long* seq_cnt,
                                   double* per_seq, hipStream_t s) {
    return launch_k(metric_seq_means_kernel, dim3(b.n), dim3(256), 0, s, per_frame, b, seq0, has_verts, seq_sum, seq_cnt, per_seq);
}

hipError_t launch_metric_total(const double* seq_sum, const long long* seq_cnt, int n_seq, double* total, hipStream_t s) {
    return launch_k(metric_total_kernel, dim3(1), dim3(256), 0, s, seq_sum, seq_cnt, n_seq, total);
}

hipError_t launch_procrustes(const double* K, int k, double* R, double* sigma, hipStream_t s) {
    return launch_k(procrustes_kernel, dim3((k + 63) / 64), dim3(64), 0, s, K, k, R, sigma);
}

}  // namespace grk
