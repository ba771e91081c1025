// The --smooth step on the device (lib/utils/smooth_pose.py:28-116): One-Euro filter over the axis-angle pose, smplx's batch_rodrigues,
// and the 54 = 24 + 21 + 9 joints from which lib/models/smpl.py:119-121 selects the 49 SPIN joints.
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  The reference filter is numpy in float32: one rounding per operation.
// The recurrence below is written operation by operation in the reference's order, divisions are IEEE (hipcc's default for `/`), and
// no product may be fused into the sum that follows it: a build that contracts them differs from the reference in a third of the
// elements (<= 1.2e-7 after 40 frames, 2.4e-6 after 10 000), a build that does not reproduces it bit for bit
// (tests/test_gpu_smooth.py compares with array_equal).  No fast-math, no __fdividef, no __sinf / __cosf anywhere in this file.
//
// one_euro_kernel -- ONE workgroup filters one sequence of T frames x 72 channels.  The recurrence is nonlinear in its state, so time is
// serial: lane c < 72 owns channel c for the whole sequence and the step's dependent chain (13 operations, one of them a division) is
// the kernel's time.  Memory stays off that chain: the sequence is walked in blocks of kOneEuroBlock = 32 frames (32 x 72 floats,
// contiguous in memory when ld == 72); all 256 threads issue the coalesced loads of block k+1 into registers BEFORE block k is filtered
// and put them into the other LDS input buffer after it; the block's results are collected in LDS and leave as coalesced stores by
// all threads after the block's only barrier.  Input and output buffers alternate (4 x 9 KiB of LDS), so one barrier per block orders
// everything: what iteration k writes was last read before barrier k-1.
// x has a row stride ld >= 72 (theta rows: ld 85, pointer advanced by 3); xhat is exactly (T,72).  Frame 0 is copied (x^[0] = x[0],
// dx^[0] = 0); a one-frame sequence is that copy and nothing else.
//
// aa_to_rotmat_kernel -- pipeline.rodrigues / smplx batch_rodrigues, one thread per joint: angle = |aa + 1e-8|, d = aa / angle,
// R = I + sin K + (1 - cos) K^2 with sinf / cosf.  Inside grnet_smooth_pose the same launch copies row 0 of betas to every frame of the
// chunk (smooth_pose.py:97).
//
// smpl_joints54_kernel -- one workgroup per frame: the 24 posed joints the chain kernel wrote, the 21 vertex picks of smplx's
// VertexJointSelector and the rows of J_regressor_extra (9,6890) as (vertex, weight) lists built at load, then the selection
// (49 SPIN joints, the 29 spin2 joints, or the 25 kinectv2 joints of those) written directly.  A row is summed by ONE wave: lane l takes
// entries l, l+64, ... in order, then the xor butterfly -- a fixed order per frame, whatever the call size; no atomics.
#include "kernels.h"
#include "device.h"

namespace grk {
namespace {

constexpr int kCh = 72;                                        // 24 joints x 3 axis-angle components
constexpr int kBlockFloats = kOneEuroBlock * kCh;              // 2304
constexpr int kUnits = kBlockFloats / 256;                     // floats per thread per block (9)
static_assert(kBlockFloats % 256 == 0, "a block must be a whole number of floats per thread");


// one_euro_filter.py:27-46 with t_e = 1: every line one float32 operation of the reference
__device__ __forceinline__ float one_euro_step(float x, float& x_prev, float& dx_prev, const OneEuroCoef& c) {
    const float dx = x - x_prev;
    const float p0 = c.a_d * dx;
    const float p1 = c.one_minus_a_d * dx_prev;
    const float dx_hat = p0 + p1;
    const float slope = c.beta * fabsf(dx_hat);
    const float cutoff = c.min_cutoff + slope;
    const float r = c.two_pi * cutoff;
    const float r1 = r + 1.f;
    const float a = r / r1;
    const float q0 = a * x;
    const float na = 1.f - a;
    const float q1 = na * x_prev;
    const float x_hat = q0 + q1;
    x_prev = x_hat;
    dx_prev = dx_hat;
    return x_hat;
}

__global__ __launch_bounds__(256) void one_euro_kernel(const float* __restrict__ x, int ld, int T, OneEuroCoef c, float* __restrict__ xhat) {
    __shared__ float in[2][kBlockFloats];
    __shared__ float out[2][kBlockFloats];
    const int tid = threadIdx.x;
    const int nblk = (T + kOneEuroBlock - 1) / kOneEuroBlock;
    float stage[kUnits];
    auto load = [&](int k) {
        const int f0 = k * kOneEuroBlock, nf = min(kOneEuroBlock, T - f0);
#pragma unroll
        for (int i = 0; i < kUnits; ++i) {
            const int e = tid + 256 * i, f = e / kCh, ch = e - f * kCh;
            stage[i] = f < nf ? x[(size_t)(f0 + f) * ld + ch] : 0.f;
        }
    };
    auto put = [&](int buf) {
#pragma unroll
        for (int i = 0; i < kUnits; ++i) in[buf][tid + 256 * i] = stage[i];
    };
    load(0);
    put(0);
    __syncthreads();
    float x_prev = 0.f, dx_prev = 0.f;
    for (int k = 0; k < nblk; ++k) {
        const int cur = k & 1, f0 = k * kOneEuroBlock, nf = min(kOneEuroBlock, T - f0);
        const bool more = k + 1 < nblk;
        if (more) load(k + 1);                                 // in flight while this block is filtered
        if (tid < kCh) {
            const float* xi = in[cur] + tid;
            float* xo = out[cur] + tid;
            if (k > 0 && nf == kOneEuroBlock) {                // whole block: the lane's 32 inputs are read from LDS BEFORE the chain starts
                float xs[kOneEuroBlock];
#pragma unroll
                for (int f = 0; f < kOneEuroBlock; ++f) xs[f] = xi[f * kCh];
                __builtin_amdgcn_sched_barrier(0);             // or the scheduler sinks each read next to its use, one exposed LDS latency per two steps
#pragma unroll
                for (int f = 0; f < kOneEuroBlock; ++f) xo[f * kCh] = one_euro_step(xs[f], x_prev, dx_prev, c);
            } else {
                int f = 0;
                if (k == 0) { x_prev = xi[0]; xo[0] = x_prev; f = 1; }
                for (; f < nf; ++f) xo[f * kCh] = one_euro_step(xi[f * kCh], x_prev, dx_prev, c);
            }
        }
        if (more) put(cur ^ 1);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kUnits; ++i) {
            const int e = tid + 256 * i;
            if (e < nf * kCh) xhat[(size_t)f0 * kCh + e] = out[cur][e];
        }
    }
}

__global__ __launch_bounds__(256) void aa_to_rotmat_kernel(const float* __restrict__ aa, float* __restrict__ R, int m,
                                                           const float* __restrict__ betas0, float* __restrict__ betas_out, int nb) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (betas_out != nullptr && i < nb * 10) betas_out[i] = betas0[i % 10];
    if (i >= m) return;
    const float x = aa[(size_t)i * 3], y = aa[(size_t)i * 3 + 1], z = aa[(size_t)i * 3 + 2];
    const float ex = x + 1e-8f, ey = y + 1e-8f, ez = z + 1e-8f;
    const float angle = sqrtf(ex * ex + ey * ey + ez * ez);
    const float dx = x / angle, dy = y / angle, dz = z / angle;
    const float s = sinf(angle), oc = 1.f - cosf(angle);
    const float K[9] = {0.f, -dz, dy, dz, 0.f, -dx, -dy, dx, 0.f};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int col = 0; col < 3; ++col) {
            const float kk = K[r * 3] * K[col] + K[r * 3 + 1] * K[3 + col] + K[r * 3 + 2] * K[6 + col];
            R[(size_t)i * 9 + r * 3 + col] = ((r == col ? 1.f : 0.f) + s * K[r * 3 + col]) + oc * kk;
        }
}

// smplx VertexJointSelector ids behind the 24 joints (netspec.SMPL_EXTRA_VERT_IDS): joints 24..44 of the 54
__constant__ int kExtraVertIds[21] = {332, 6260, 2800, 4071, 583, 3216, 3226, 3387, 6617, 6624, 6787,
                                      2746, 2319, 2445, 2556, 2673, 6191, 5782, 5905, 6016, 6133};

struct JointSelection {
    int count;
    unsigned rows;                 // bit r: row r of J_regressor_extra is selected somewhere
    unsigned char src[49];         // index into the 54 joints per output joint
};

__global__ __launch_bounds__(256) void smpl_joints54_kernel(const float* __restrict__ kp29, const float* __restrict__ verts, SmplTables t,
                                                            JointSelection sel, float* __restrict__ joints) {
    __shared__ float sj[54][3];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* vn = verts + (size_t)n * 6890 * 3;
    if (tid < 72) sj[tid / 3][tid % 3] = kp29[(size_t)n * 87 + tid];          // the 24 posed joints (smpl_chain_kernel)
    if (tid >= 128 && tid < 128 + 63) {
        const int e = tid - 128, j = e / 3, d = e - j * 3;
        sj[24 + j][d] = vn[kExtraVertIds[j] * 3 + d];
    }
    for (int r = wave; r < 9; r += 4) {
        if (!(sel.rows >> r & 1u)) continue;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int k = t.extra_ptr[r] + lane; k < t.extra_ptr[r + 1]; k += 64) {
            const int v = t.extra_idx[k];
            const float w = t.extra_w[k];
            a0 += w * vn[v * 3]; a1 += w * vn[v * 3 + 1]; a2 += w * vn[v * 3 + 2];
        }
        a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
        if (lane == 0) { sj[45 + r][0] = a0; sj[45 + r][1] = a1; sj[45 + r][2] = a2; }
    }
    __syncthreads();
    for (int e = tid; e < sel.count * 3; e += 256) {
        const int j = e / 3;
        joints[(size_t)n * sel.count * 3 + e] = sj[sel.src[j]][e - j * 3];
    }
}

// [JOINT_MAP[n] for n in JOINT_NAMES] (smpl.py:16-87,102; netspec.SPIN49_FROM_54)
constexpr unsigned char kSpin49[49] = {24, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 8, 5, 45, 46, 4, 7,
                                       21, 19, 17, 16, 18, 20, 47, 48, 49, 50, 51, 52, 53, 24, 35, 40, 10, 11};
// the 29 spin2 joints of smpl.py:113-118 as smpl_joints_kernel writes them: 24 joints, vertices 2746 / 2445 / 6191 / 5905, 'Thorax (MPII)'
constexpr unsigned char kSpin2[29] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 35, 37, 40, 42, 50};
// kp_utils.py:211-242,904-931 (netspec.SPIN2_TO_KINECTV2)
constexpr unsigned char kKinectFromSpin2[25] = {0, 6, 12, 15, 16, 18, 20, 22, 17, 19, 21, 23, 1, 4, 7, 10, 2, 5, 8, 11, 28, 25, 24, 27, 26};

}  // namespace

int smooth_joint_count(int kind) { return kind == 0 ? 49 : kind == 1 ? 29 : kind == 2 ? 25 : 0; }

hipError_t launch_one_euro(const float* x, int ld, int T, OneEuroCoef c, float* xhat, hipStream_t s) {
    return launch_k(one_euro_kernel, dim3(1), dim3(256), 0, s, x, ld, T, c, xhat);
}

hipError_t launch_aa_to_rotmat(const float* aa, float* R, int m, const float* betas0, float* betas_out, int nb, hipStream_t s) {
    return launch_k(aa_to_rotmat_kernel, dim3((m + 255) / 256), dim3(256), 0, s, aa, R, m, betas0, betas_out, nb);
}

hipError_t launch_smpl_joints54(const float* kp29, const float* verts, SmplTables t, int kind, float* joints, int n, hipStream_t s) {
    JointSelection sel{};
    sel.count = smooth_joint_count(kind);
    if (!sel.count) return hipErrorInvalidValue;
    for (int j = 0; j < sel.count; ++j) {
        sel.src[j] = kind == 0 ? kSpin49[j] : kind == 1 ? kSpin2[j] : kSpin2[kKinectFromSpin2[j]];
        if (sel.src[j] >= 45) sel.rows |= 1u << (sel.src[j] - 45);
    }
    return launch_k(smpl_joints54_kernel, dim3(n), dim3(256), 0, s, kp29, verts, t, sel, joints);
}

}  // namespace grk
