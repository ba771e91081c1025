// Joints regressed from vertices -- VPRegressor.forward's J_regressor override (lib/models/pare.py:70-76):
//     joints[n][j][k] = sum_v W[j][v] * verts[n][v][k],   W (Jout,6890) fp32, any content (dense or sparse, signed, rows of any sum).
//
// GEMM on the fp32 matrix cores with M = joints (padded to MT*16), K = vertices, N = the (frame, xyz) columns of 16 frames (48 = 3 tiles).
// The 6890 vertices are split, always the same way, into 27 slices of 256; a workgroup owns one slice and each of its 4 waves 64 vertices
// of it, whose table columns it keeps in registers as MFMA A fragments (the host packs the table in fragment order, zero-padded, so the
// loads are coalesced and need no bounds).  The workgroup then walks passes of 16 frames: every wave stages the 768 contiguous bytes per
// frame of its vertices in LDS (8-byte loads: a frame's 20670 floats start 8-byte aligned on odd frames), the next pass's loads are issued
// before the current pass's MFMA chain, the 4 waves' tiles are added in wave order in LDS, and the slice's partial sums go to the
// workspace.  A second launch adds the 27 partials in slice order.  Every output element is one fixed sequence of fp32 fma's and adds,
// whatever the number of frames in the call and wherever the frame sits in it: bit-identical across call sizes, no atomics.
// The table is read once per frame chunk (blockIdx.y, at most kJregChunks per call), not once per frame.
#include "kernels.h"
#include "device.h"

namespace grk {
namespace {


constexpr int kVerts = 6890, kFrameFloats = kVerts * 3;
constexpr int kPassFrames = 16, kPassCols = kPassFrames * 3;     // 48 columns = 3 MFMA column tiles
constexpr int kWaveVerts = 64, kWaveFloats = kWaveVerts * 3;     // 192 floats of a frame per wave
constexpr int kLd = kWaveFloats + 12;                            // LDS row stride of a staged frame (even: 8-byte stores stay aligned)
constexpr int kUnits = kPassFrames * kWaveFloats / 2 / 64;       // 8-byte units per lane per pass (24)

__device__ __forceinline__ void stage_load(f32x2 (&v)[kUnits], const float* __restrict__ verts, int f0, int n, int float0, int lane) {
#pragma unroll
    for (int i = 0; i < kUnits; ++i) {
        const int u = lane + 64 * i, f = u / (kWaveFloats / 2), e = float0 + 2 * (u - f * (kWaveFloats / 2));
        v[i] = (f0 + f < n && e < kFrameFloats) ? *reinterpret_cast<const f32x2*>(verts + (size_t)(f0 + f) * kFrameFloats + e) : f32x2{0.f, 0.f};
    }
}

template <int MT>
__global__ __launch_bounds__(256) void joint_regress_kernel(const float* __restrict__ verts, const float* __restrict__ wpack, float* __restrict__ partial,
                                                           int n, int jout) {
    // the staged frames of the 4 waves; re-used for the 4 waves' result tiles (4 x MT*16 x 48 floats <= 4 x 16 x kLd) once the chains are done
    __shared__ __align__(16) float smem[4 * kPassFrames * kLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lq = lane >> 4;
    const int slice = blockIdx.x, wslice = slice * 4 + wave;
    float wreg[MT][kWaveVerts / 4];
#pragma unroll
    for (int ks = 0; ks < kWaveVerts / 4; ++ks)
#pragma unroll
        for (int m = 0; m < MT; ++m) wreg[m][ks] = wpack[(((size_t)wslice * (kWaveVerts / 4) + ks) * MT + m) * 64 + lane];
    float* vs = smem + wave * kPassFrames * kLd;
    int boff[3];                                                 // B fragment: column c = t*16 + l15 -> (frame c/3, xyz c%3), k = vertex 4*ks + lq
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int c = t * 16 + l15;
        boff[t] = (c / 3) * kLd + lq * 3 + c % 3;
    }
    const int npass = (n + kPassFrames - 1) / kPassFrames;
    f32x2 stage[kUnits];
    int pass = blockIdx.y;
    if (pass < npass) stage_load(stage, verts, pass * kPassFrames, n, wslice * kWaveFloats, lane);
    for (; pass < npass; pass += gridDim.y) {
        const int f0 = pass * kPassFrames;
        __syncthreads();                                         // the previous pass is done with smem
#pragma unroll
        for (int i = 0; i < kUnits; ++i) {
            const int u = lane + 64 * i, f = u / (kWaveFloats / 2);
            *reinterpret_cast<f32x2*>(vs + f * kLd + 2 * (u - f * (kWaveFloats / 2))) = stage[i];
        }
        __syncthreads();
        if (pass + (int)gridDim.y < npass) stage_load(stage, verts, (pass + gridDim.y) * kPassFrames, n, wslice * kWaveFloats, lane);
        f32x4 acc[MT][3];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int t = 0; t < 3; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < kWaveVerts / 4; ++ks) {
            float b[3];
#pragma unroll
            for (int t = 0; t < 3; ++t) b[t] = vs[boff[t] + 12 * ks];
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int t = 0; t < 3; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[m][ks], b[t], acc[m][t], 0, 0, 0);
        }
        __syncthreads();                                         // every wave is done reading its staged frames
        float* ps = smem + wave * (MT * 16 * kPassCols);         // D: row = 4*lq + r, column = l15
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) ps[(m * 16 + lq * 4 + r) * kPassCols + t * 16 + l15] = acc[m][t][r];
        __syncthreads();
        // partial[slice][frame][j][k]: the pass's frames are contiguous there; waves added in wave order
        const int nf = min(kPassFrames, n - f0), per = jout * 3;
        float* dst = partial + ((size_t)slice * n + f0) * per;
        for (int e = tid; e < nf * per; e += 256) {
            const int f = e / per, jk = e - f * per, j = jk / 3, k = jk - j * 3;
            const float* p = smem + j * kPassCols + f * 3 + k;
            float s = p[0];
#pragma unroll
            for (int w = 1; w < 4; ++w) s += p[w * (MT * 16 * kPassCols)];
            dst[e] = s;
        }
    }
}

__global__ __launch_bounds__(256) void joint_regress_sum_kernel(const float* __restrict__ partial, float* __restrict__ joints, int total) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    float s = partial[e];
    for (int sl = 1; sl < kJregSlices; ++sl) s += partial[(size_t)sl * total + e];     // slice order
    joints[e] = s;
}

}  // namespace

size_t joint_regress_pack_floats(int jout) { return (size_t)kJregSlices * 4 * (kWaveVerts / 4) * ((jout + 15) / 16) * 64; }

size_t joint_regress_workspace_floats(int jout, int max_frames) { return (size_t)kJregSlices * max_frames * jout * 3; }

// W (jout,6890) row-major -> MFMA A fragments: [wave slice][k step][row tile][lane] = W[tile*16 + (lane & 15)][wslice*64 + 4*ks + (lane >> 4)], zero outside
void joint_regress_pack(const float* W, int jout, float* out) {
    const int mt = (jout + 15) / 16;
    size_t o = 0;
    for (int ws = 0; ws < kJregSlices * 4; ++ws)
        for (int ks = 0; ks < kWaveVerts / 4; ++ks)
            for (int m = 0; m < mt; ++m)
                for (int lane = 0; lane < 64; ++lane, ++o) {
                    const int j = m * 16 + (lane & 15), v = ws * kWaveVerts + 4 * ks + (lane >> 4);
                    out[o] = (j < jout && v < kVerts) ? W[(size_t)j * kVerts + v] : 0.f;
                }
}

hipError_t launch_joint_regress(const float* verts, const float* wpack, int jout, float* partial, float* joints, int n, hipStream_t s) {
    const int npass = (n + kPassFrames - 1) / kPassFrames;
    const dim3 grid(kJregSlices, npass < kJregChunks ? npass : kJregChunks);
    switch ((jout + 15) / 16) {
        case 1: joint_regress_kernel<1><<<grid, 256, 0, s>>>(verts, wpack, partial, n, jout); break;
        case 2: joint_regress_kernel<2><<<grid, 256, 0, s>>>(verts, wpack, partial, n, jout); break;
        case 3: joint_regress_kernel<3><<<grid, 256, 0, s>>>(verts, wpack, partial, n, jout); break;
        case 4: joint_regress_kernel<4><<<grid, 256, 0, s>>>(verts, wpack, partial, n, jout); break;
        default: return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int total = n * jout * 3;
    joint_regress_sum_kernel<<<(total + 255) / 256, 256, 0, s>>>(partial, joints, total);
    return hipGetLastError();
}

}  // namespace grk
