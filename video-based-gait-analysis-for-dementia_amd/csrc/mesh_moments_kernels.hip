// Volume, centre of mass, central second moments and area of the closed SMPL mesh of every frame on the device (rules and columns: DESIGN 4.25;
// the arithmetic: mesh_moments.h, which the host checker runs too).
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  Everything is float64 and every operation rounds once.
//
// ONE launch, whatever the number of frames: mesh_moments_kernel, a workgroup of kMeshCols lanes (16 waves) per frame.  Lane l IS column l of rule
// 3: it adds the eleven terms of faces l, l + 1024, ... in rising order from +0.0 in registers (mesh_column: 22 VGPRs of accumulators).  The tree
// col[l] += col[l + h] then runs in the stated order: h = 512, 256, 128, 64 across the waves through LDS (the upper half of the live columns stores
// its eleven values, a barrier, the lower half adds them), h = 32 .. 1 inside wave 0 by x + __shfl_xor(x, h) -- the lower lane of every pair makes
// exactly col[l] + col[l + h], and + is commutative, so lane 0 ends with S.  Lane 0 writes the sums (where the caller takes them) and the row
// (mesh_row).  No atomics; no sum depends on the launch, so a frame has the same bits alone or among others.  Every value is written with a plain
// vector store.
//
// TWO forms of the gather, both kept so that tools/mesh_moments_time.py can time them side by side (profiles/mesh_moments_times.txt):
//   kMeshFormDirect -- the three corners of a face are read straight from global memory: a vertex is named by about six faces that lie near each
//                      other in the table, so most reads hit lines the workgroup has fetched already.  45 056 bytes of LDS (the tree's).
//   kMeshFormStaged -- the frame's 82 680 bytes of vertices are first copied into LDS by 16-byte loads (the image is shifted by the frame's
//                      misalignment of 0 to 3 floats, so that an aligned global quad is an aligned LDS quad; the partial quads at either end go
//                      float by float, inside the frame) and gathered from there.  127 760 bytes of dynamic LDS: one workgroup per CU.
// The face table (165 KB for SMPL) is the same for every frame and is served by the L2.
#include "kernels.h"
#include "device.h"
#include "mesh_moments.h"

#include <cstdint>

namespace grk {
namespace {

constexpr size_t kMeshPartBytes = (size_t)(kMeshCols / 2) * kMeshTerms * sizeof(double);      // 45 056: a multiple of 16
static_assert(kMeshPartBytes % 16 == 0, "the staged image behind the tree's block starts 16-byte aligned");
constexpr size_t mesh_stage_bytes(int V) { return (((size_t)V * 3 + 3 + 3) / 4) * 16; }         // the frame's floats, up to 3 in front, whole quads

template <bool kStaged>
__global__ __launch_bounds__(kMeshCols) void mesh_moments_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                                 double* __restrict__ rows, double* __restrict__ sums) {
    extern __shared__ __attribute__((aligned(16))) char mesh_lds[];
    double* part = reinterpret_cast<double*>(mesh_lds);      // (kMeshCols / 2, kMeshTerms)
    const int frame = blockIdx.x, l = threadIdx.x;
    const float* v = verts + (size_t)frame * V * 3;
    double o[3], acc[kMeshTerms];
    if (kStaged) {
        float* stage = reinterpret_cast<float*>(mesh_lds + kMeshPartBytes);
        const int mis = (int)((reinterpret_cast<uintptr_t>(v) >> 2) & 3), total = mis + 3 * V, quads = (total + 3) >> 2;
        const float* vb = v - mis;                           // 16-byte aligned; floats [mis, total) of it are the frame's
        for (int q = l; q < quads; q += kMeshCols) {
            const int i0 = 4 * q;
            if (i0 >= mis && i0 + 4 <= total) {
                *reinterpret_cast<float4*>(stage + i0) = *reinterpret_cast<const float4*>(vb + i0);
            } else {
                for (int k = 0; k < 4; ++k)
                    if (i0 + k >= mis && i0 + k < total) stage[i0 + k] = vb[i0 + k];
            }
        }
        __syncthreads();
        mesh_origin(stage + mis, faces, o);
        mesh_column(stage + mis, faces, F, l, o, acc);
    } else {
        mesh_origin(v, faces, o);
        mesh_column(v, faces, F, l, o, acc);
    }
    // the tree across the waves: columns [h, 2h) hand their sums to columns [0, h)
    for (int h = kMeshCols / 2; h >= 64; h >>= 1) {
        if (l >= h && l < 2 * h)
            for (int k = 0; k < kMeshTerms; ++k) part[(l - h) * kMeshTerms + k] = acc[k];
        __syncthreads();
        if (l < h)
            for (int k = 0; k < kMeshTerms; ++k) acc[k] = acc[k] + part[l * kMeshTerms + k];
        __syncthreads();
    }
    if (l >= 64) return;
    // ... and inside wave 0
    for (int h = 32; h >= 1; h >>= 1)
        for (int k = 0; k < kMeshTerms; ++k) acc[k] = acc[k] + __shfl_xor(acc[k], h, 64);
    if (l != 0) return;
    if (sums)
        for (int k = 0; k < kMeshTerms; ++k) sums[(size_t)frame * kMeshTerms + k] = acc[k];
    double row[kMeshRowCols];
    mesh_row(acc, o, row);
    for (int k = 0; k < kMeshRowCols; ++k) rows[(size_t)frame * kMeshRowCols + k] = row[k];
}

}  // namespace

hipError_t launch_mesh_moments(const float* verts, int n, const RasterMesh& m, int form, double* rows, double* sums, hipStream_t s) {
    if (form == kMeshFormStaged) {
        const size_t lds = kMeshPartBytes + mesh_stage_bytes(m.n_verts);
        // more than the 64 KB a launch may ask for unannounced
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(mesh_moments_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        return launch_k(mesh_moments_kernel<true>, dim3(n), dim3(kMeshCols), lds, s, verts, m.n_verts, m.faces, m.n_faces, rows, sums);
    }
    return launch_k(mesh_moments_kernel<false>, dim3(n), dim3(kMeshCols), kMeshPartBytes, s, verts, m.n_verts, m.faces, m.n_faces, rows, sums);
}

}  // namespace grk
