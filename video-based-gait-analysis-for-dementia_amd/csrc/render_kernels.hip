// The mesh overlay of demo.py --mesh_render on the device (lib/utils/renderer.py:78-126: one opaque triangle mesh, a weak-perspective camera,
// a z-buffer, a mask composite over the frame).  Geometry follows OpenGL's rules; the shading is a stated Lambert model, NOT pyrender's
// metallic-roughness shader.  All float arithmetic is fp32; after the vertices are snapped, coverage is integer arithmetic, so it
// depends neither on the order in which threads run nor on what the compiler contracts.
//
// A launch group draws up to kRasterSlots meshes, each into its OWN image (the host never puts two meshes of one image into a group), slot s
// on blockIdx.y / .z with its own vertex records and depth image in the workspace:
//
// raster_setup_kernel -- one thread per vertex: q = M (x, -y, -z); x_ndc = sx (q.x + tx), y_ndc = sy (q.y - ty), z_ndc = -q.z; window
//   coordinates with GL's origin at the bottom-left, snapped to 8 sub-pixel bits, X = floor(256 x_win + 0.5), and clamped to +-2^28 (a NaN
//   lands on the lower clamp), so every edge function below fits int64.  The mesh's bounding box is the wave's maximum of (-X, -Y, X, Y)
//   followed by one integer atomicMax per wave and component.
// raster_normals_kernel -- one thread per vertex: the sum, in table order, of the un-normalised face normals cross(q1 - q0, q2 - q0) of the
//   faces at the vertex (the vertex -> face table grnet_load_faces built), normalised; a vertex without faces, or with a zero sum, gets 0.
// raster_clear_kernel -- depth = all ones inside the mesh's bounding box clamped to the viewport; workgroups outside it leave at once.
// raster_cover_kernel -- a wave takes 64 faces, one per lane, for the per-face work: twice the signed area A2 in GL window space (A2 <= 0: back
//   face or degenerate, culled) and the face's pixel box clamped to the viewport (empty: dropped before any loop over pixels).  The
//   surviving faces are then walked one at a time by the WHOLE wave, their records broadcast with __shfl, the 64 lanes laid as an 8 x 8 pixel
//   tile stepped over the box: an SMPL triangle at 1080p (20-40 pixels) takes one or two steps, a triangle larger than the image is spread
//   over 64 lanes instead of being one lane's loop.  The sample is the pixel centre (256 i + 128, 256 j + 128); a centre exactly on an edge
//   belongs to the triangle only if that edge is a top or a left edge in IMAGE space (y down), which for a counter-clockwise triangle in GL
//   window space is: dy < 0, or dy == 0 and dx < 0.  z from the barycentrics of the edge values; outside [-1, 1] the fragment is discarded
//   (near / far clipping for w = 1); GL_LESS with the lower face index winning at equal depth, as ONE 64-bit atomicMin per fragment on
//   (ordered(z) << 32) | face -- the result does not depend on execution order.
// raster_resolve_kernel -- one thread per pixel of the bounding box: the winning face's barycentrics again from the integer edge values, the
//   interpolated unit normal and position, three point lights at (0,-1,1), (0,1,1), (1,1,2) in q space:
//   shade = 0.3 + sum_l max(0, n.l) / (pi d_l^2), byte k of the pixel = floor(255 min(1, colour_k shade) + 0.5).  Only covered pixels are stored
//   (three byte stores each: a person covers a few percent of a frame); the depth reads are 512 contiguous bytes per wave.
// raster_winner_kernel -- the test hook's read-out: the low word of the key per pixel in image rows, -1 where uncovered.
//
// The wireframe (--wireframe: GL_LINE polygon mode) replaces the cover and the resolve; setup, normals, clear and winner are shared:
// raster_lines_cover_kernel -- the same 64 faces per wave and the same A2 cull, then the three edges k = 0: v0 -> v1, 1: v1 -> v2,
//   2: v2 -> v0 of every front face.  An edge is x-major if |dx| >= |dy|, else y-major; P is the major coordinate, Q the minor one; the end
//   points are ordered P_lo < P_hi and EVERYTHING after that is computed from (lo, hi), so the two draws of a shared edge are the same
//   fragments with the same depths.  Major index m is covered iff P_lo <= 256 m + 128 < P_hi; there the minor index is
//   n = floor((Q_lo dP + (256 m + 128 - P_lo) dQ) / (256 dP)) in int64: one division for the first m of a lane, then the remainder is stepped
//   (add 256 dQ, carry against 256 dP), which gives the same integers.  An edge of at most kRasterLineWaveSteps major steps is its lane's own
//   loop; a longer one is collected with __ballot and walked by the whole wave, 64 major steps an iteration.  t = (256 m + 128 - P_lo) / dP,
//   z = fma(t, z_hi - z_lo, z_lo) + 0; outside [-1, 1] discarded; one atomicMin on (ordered(z) << 32) | (3 face + k).
// raster_resolve_kernel<true> -- face and k from the key, the major axis, (lo, hi) and t again from the pixel, normal and position
//   interpolated between the two end points with t, then the same shade and store.  A line's pixel is the one whose SQUARE holds the line, so
//   its centre may lie up to half a pixel outside the mesh's bounding box: the clear and the resolve of a wireframe take the pixels whose
//   squares meet the box (pixel_range_squares), a superset of the fill's.
#include "raster_device.h"

namespace grk {
namespace {

// The pixels whose centres lie inside [lo, hi] (snapped units) on an axis of n pixels: first and last index, first > last if there is none
__device__ __forceinline__ void pixel_range(int lo, int hi, int n, int& first, int& last) {
    first = max(0, (lo - kHalf + kSub - 1) >> kRasterSnapBits);
    last = min(n - 1, (hi - kHalf) >> kRasterSnapBits);
}

template <bool kLines>
__device__ __forceinline__ bool slot_box(const int* bbox, const RasterView& v, int& i0, int& i1, int& j0, int& j1) {
    if constexpr (kLines) {
        pixel_range_squares(-bbox[0], bbox[2], v.W, i0, i1);
        pixel_range_squares(-bbox[1], bbox[3], v.H, j0, j1);
    } else {
        pixel_range(-bbox[0], bbox[2], v.W, i0, i1);
        pixel_range(-bbox[1], bbox[3], v.H, j0, j1);
    }
    return i0 <= i1 && j0 <= j1;
}

__device__ __forceinline__ long long edge(int ax, int ay, int bx, int by, int px, int py) {
    return (long long)(bx - ax) * (long long)(py - ay) - (long long)(by - ay) * (long long)(px - ax);
}

// a top or a left edge in image space, for the edge a -> b of a triangle that is counter-clockwise in GL window space
__device__ __forceinline__ bool top_left(int ax, int ay, int bx, int by) { return by < ay || (by == ay && bx < ax); }

__global__ __launch_bounds__(256) void raster_setup_kernel(const float* __restrict__ verts, const float* __restrict__ cams, RasterChunk c, RasterView view,
                                                           int n_verts, RasterWork w) {
    const int slot = blockIdx.y;
    const int v = blockIdx.x * 256 + threadIdx.x;
    int b0 = INT_MIN, b1 = INT_MIN, b2 = INT_MIN, b3 = INT_MIN;
    if (v < n_verts) {
        const int mesh = c.mesh[slot];
        const float* p = verts + ((size_t)mesh * n_verts + v) * 3;
        const float* cam = cams + (size_t)mesh * 4;
        const float x = p[0], y = -p[1], z = -p[2];
        const float qx = view.M[0] * x + view.M[1] * y + view.M[2] * z;
        const float qy = view.M[3] * x + view.M[4] * y + view.M[5] * z;
        const float qz = view.M[6] * x + view.M[7] * y + view.M[8] * z;
        const float x_ndc = cam[0] * (qx + cam[2]);
        const float y_ndc = cam[1] * (qy - cam[3]);
        const int X = snap((x_ndc + 1.f) * (0.5f * (float)view.W));
        const int Y = snap((y_ndc + 1.f) * (0.5f * (float)view.H));
        const size_t o = (size_t)slot * n_verts + v;
        w.q[o * 3 + 0] = qx;
        w.q[o * 3 + 1] = qy;
        w.q[o * 3 + 2] = qz;
        w.xy[o * 2 + 0] = X;
        w.xy[o * 2 + 1] = Y;
        w.z[o] = -qz;
        b0 = -X, b1 = -Y, b2 = X, b3 = Y;
    }
    b0 = wave_max64(b0), b1 = wave_max64(b1), b2 = wave_max64(b2), b3 = wave_max64(b3);
    if ((threadIdx.x & 63) == 0 && b2 != INT_MIN) {
        int* bb = w.bbox + slot * 4;
        atomicMax(bb + 0, b0);
        atomicMax(bb + 1, b1);
        atomicMax(bb + 2, b2);
        atomicMax(bb + 3, b3);
    }
}

__global__ __launch_bounds__(256) void raster_normals_kernel(RasterMesh m, RasterWork w) {
    const int slot = blockIdx.y;
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= m.n_verts) return;
    const float* q = w.q + (size_t)slot * m.n_verts * 3;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int k = m.vf_off[v]; k < m.vf_off[v + 1]; ++k) {
        const int* f = m.faces + (size_t)m.vf_idx[k] * 3;
        const float* a = q + (size_t)f[0] * 3;
        const float* b = q + (size_t)f[1] * 3;
        const float* cc = q + (size_t)f[2] * 3;
        const float ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
        const float vx = cc[0] - a[0], vy = cc[1] - a[1], vz = cc[2] - a[2];
        nx += uy * vz - uz * vy;
        ny += uz * vx - ux * vz;
        nz += ux * vy - uy * vx;
    }
    const float l2 = nx * nx + ny * ny + nz * nz;
    const float inv = l2 > 0.f ? 1.f / sqrtf(l2) : 0.f;
    float* o = w.nrm + ((size_t)slot * m.n_verts + v) * 3;
    o[0] = nx * inv;
    o[1] = ny * inv;
    o[2] = nz * inv;
}

template <bool kLines>
__global__ __launch_bounds__(256) void raster_clear_kernel(RasterView view, RasterWork w) {
    const int slot = blockIdx.z;
    int i0, i1, j0, j1;
    if (!slot_box<kLines>(w.bbox + slot * 4, view, i0, i1, j0, j1)) return;
    const int i = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1)), j = blockIdx.y * kTileH + threadIdx.x / kTileW;
    if (i < i0 || i > i1 || j < j0 || j > j1) return;
    w.depth[(size_t)slot * view.H * view.W + (size_t)j * view.W + i] = kDepthClear;
}

__global__ __launch_bounds__(256) void raster_cover_kernel(RasterView view, RasterMesh m, RasterWork w) {
    const int slot = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * 256 + threadIdx.x;
    const int* xy = w.xy + (size_t)slot * m.n_verts * 2;
    const float* zv = w.z + (size_t)slot * m.n_verts;
    unsigned long long* depth = w.depth + (size_t)slot * view.H * view.W;
    int X0 = 0, Y0 = 0, X1 = 0, Y1 = 0, X2 = 0, Y2 = 0, i0 = 0, i1 = -1, j0 = 0, j1 = -1;
    float z0 = 0.f, z1 = 0.f, z2 = 0.f;
    bool live = false;
    if (f < m.n_faces) {
        const int a = m.faces[(size_t)f * 3], b = m.faces[(size_t)f * 3 + 1], cc = m.faces[(size_t)f * 3 + 2];
        X0 = xy[2 * a], Y0 = xy[2 * a + 1], X1 = xy[2 * b], Y1 = xy[2 * b + 1], X2 = xy[2 * cc], Y2 = xy[2 * cc + 1];
        z0 = zv[a], z1 = zv[b], z2 = zv[cc];
        const long long A2 = edge(X0, Y0, X1, Y1, X2, Y2);
        if (A2 > 0) {
            pixel_range(min(X0, min(X1, X2)), max(X0, max(X1, X2)), view.W, i0, i1);
            pixel_range(min(Y0, min(Y1, Y2)), max(Y0, max(Y1, Y2)), view.H, j0, j1);
            live = i0 <= i1 && j0 <= j1;
        }
    }
    unsigned long long todo = __ballot(live);
    while (todo) {                                             // wave-uniform
        const int t = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int ax = __shfl(X0, t, 64), ay = __shfl(Y0, t, 64), bx = __shfl(X1, t, 64), by = __shfl(Y1, t, 64), cx = __shfl(X2, t, 64), cy = __shfl(Y2, t, 64);
        const float za = __shfl(z0, t, 64), zb = __shfl(z1, t, 64), zc = __shfl(z2, t, 64);
        const int ti0 = __shfl(i0, t, 64), ti1 = __shfl(i1, t, 64), tj0 = __shfl(j0, t, 64), tj1 = __shfl(j1, t, 64);
        const unsigned face = (unsigned)(f - lane + t);
        const float inv_area = 1.f / (float)edge(ax, ay, bx, by, cx, cy);
        // a centre on an edge that is neither top nor left is outside: such an edge asks for a value >= 1
        const long long m0 = top_left(bx, by, cx, cy) ? 0 : 1, m1 = top_left(cx, cy, ax, ay) ? 0 : 1, m2 = top_left(ax, ay, bx, by) ? 0 : 1;
        for (int j = tj0 + (lane >> 3); j <= tj1; j += 8) {
            const int py = j * kSub + kHalf;
            for (int i = ti0 + (lane & 7); i <= ti1; i += 8) {
                const int px = i * kSub + kHalf;
                const long long w0 = edge(bx, by, cx, cy, px, py), w1 = edge(cx, cy, ax, ay, px, py), w2 = edge(ax, ay, bx, by, px, py);
                if (w0 < m0 || w1 < m1 || w2 < m2) continue;
                const float b1 = (float)w1 * inv_area, b2 = (float)w2 * inv_area;
                const float z = (za + b1 * (zb - za) + b2 * (zc - za)) + 0.f;      // + 0: -0 and +0 are one depth
                if (!(z >= -1.f && z <= 1.f)) continue;
                atomicMin(depth + (size_t)j * view.W + i, ((unsigned long long)ordered_bits(z) << 32) | face);
            }
        }
    }
}

// The edge records and their integer arithmetic: raster_lines.h; line_t: raster_device.h

__device__ __forceinline__ void line_fragment(const LineRec& r, int m, long long n, unsigned id, const RasterView& view, unsigned long long* depth) {
    if (n < 0 || n >= (r.xmajor ? view.H : view.W)) return;
    const float z = fmaf(line_t(r, m), r.z1 - r.z0, r.z0) + 0.f;                   // + 0: -0 and +0 are one depth
    if (!(z >= -1.f && z <= 1.f)) return;
    const int i = r.xmajor ? m : (int)n, j = r.xmajor ? (int)n : m;
    atomicMin(depth + (size_t)j * view.W + i, ((unsigned long long)ordered_bits(z) << 32) | id);
}

__global__ __launch_bounds__(256) void raster_lines_cover_kernel(RasterView view, RasterMesh m, RasterWork w) {
    const int slot = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * 256 + threadIdx.x;
    const int* xy = w.xy + (size_t)slot * m.n_verts * 2;
    const float* zv = w.z + (size_t)slot * m.n_verts;
    unsigned long long* depth = w.depth + (size_t)slot * view.H * view.W;
    int X[3] = {0, 0, 0}, Y[3] = {0, 0, 0};
    float Z[3] = {0.f, 0.f, 0.f};
    bool front = false;
    if (f < m.n_faces) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int v = m.faces[(size_t)f * 3 + k];
            X[k] = xy[2 * v], Y[k] = xy[2 * v + 1], Z[k] = zv[v];
        }
        front = edge(X[0], Y[0], X[1], Y[1], X[2], Y[2]) > 0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = k, b = (k + 1) % 3;
        LineRec r{};
        r.m1 = -1;
        bool flip = false;
        if (front && line_order(X[a], Y[a], X[b], Y[b], r, flip)) {
            r.z0 = flip ? Z[b] : Z[a], r.z1 = flip ? Z[a] : Z[b];
            line_range(r, r.xmajor ? view.W : view.H);
        }
        const int steps = r.m1 - r.m0 + 1;
        const bool wide = steps > kRasterLineWaveSteps;
        if (steps > 0 && !wide) {                                                  // a short edge: this lane's own loop
            const LineStride st = line_stride(r, 1);
            long long n, rem;
            line_minor(r, r.m0, n, rem);
            for (int mm = r.m0; mm <= r.m1; ++mm, line_advance(st, n, rem)) line_fragment(r, mm, n, 3u * (unsigned)f + k, view, depth);
        }
        unsigned long long todo = __ballot(wide);
        while (todo) {                                         // wave-uniform: a long edge is 64 lanes' work
            const int t = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            LineRec e;
            e.P0 = __shfl(r.P0, t, 64), e.Q0 = __shfl(r.Q0, t, 64), e.P1 = __shfl(r.P1, t, 64), e.Q1 = __shfl(r.Q1, t, 64);
            e.z0 = __shfl(r.z0, t, 64), e.z1 = __shfl(r.z1, t, 64);
            e.m0 = __shfl(r.m0, t, 64), e.m1 = __shfl(r.m1, t, 64), e.xmajor = __shfl(r.xmajor, t, 64);
            const unsigned id = 3u * (unsigned)(f - lane + t) + k;
            const LineStride st = line_stride(e, 64);          // wave-uniform
            long long n, rem;
            line_minor(e, e.m0 + lane, n, rem);               // m0 + lane <= 4095 + 63: the numerator stays far inside int64
            for (int mm = e.m0 + lane; mm <= e.m1; mm += 64, line_advance(st, n, rem)) line_fragment(e, mm, n, id, view, depth);
        }
    }
}

// bytes of a covered pixel from the interpolated normal n (any length) and position p, in q space
__device__ __forceinline__ void shade_store(const float n[3], const float p[3], const float colour[3], unsigned char* out) {
    const float n2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    const float ninv = n2 > 0.f ? 1.f / sqrtf(n2) : 0.f;
    const float lights[3][3] = {{0.f, -1.f, 1.f}, {0.f, 1.f, 1.f}, {1.f, 1.f, 2.f}};
    float shade = 0.3f;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        const float dx = lights[l][0] - p[0], dy = lights[l][1] - p[1], dz = lights[l][2] - p[2];
        const float d2 = dx * dx + dy * dy + dz * dz;
        const float cosine = (n[0] * dx + n[1] * dy + n[2] * dz) * ninv / sqrtf(d2);
        shade += fmaxf(0.f, cosine) / (3.14159265358979323846f * d2);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
        out[k] = (unsigned char)floorf(255.f * fmaxf(0.f, fminf(1.f, colour[k] * shade)) + 0.5f);
}

template <bool kLines>
__global__ __launch_bounds__(256) void raster_resolve_kernel(RasterChunk c, RasterView view, RasterMesh m, RasterWork w, unsigned char* __restrict__ images) {
    const int slot = blockIdx.z;
    int i0, i1, j0, j1;
    if (!slot_box<kLines>(w.bbox + slot * 4, view, i0, i1, j0, j1)) return;
    const int i = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1)), j = blockIdx.y * kTileH + threadIdx.x / kTileW;
    if (i < i0 || i > i1 || j < j0 || j > j1) return;
    const unsigned long long key = w.depth[(size_t)slot * view.H * view.W + (size_t)j * view.W + i];
    if (key == kDepthClear) return;
    const size_t vo = (size_t)slot * m.n_verts;
    float n[3], p[3];
    if constexpr (kLines) {
        const unsigned id = (unsigned)key;
        const int* f = m.faces + (size_t)(id / 3) * 3;
        int va = f[id % 3], vb = f[(id % 3 + 1) % 3];
        const int* xa = w.xy + (vo + va) * 2;
        const int* xb = w.xy + (vo + vb) * 2;
        LineRec r{};
        bool flip = false;
        if (!line_order(xa[0], xa[1], xb[0], xb[1], r, flip)) return;             // never: a point draws no fragment
        if (flip) { const int s = va; va = vb, vb = s; }
        const float t = line_t(r, r.xmajor ? i : j);
        const float *na = w.nrm + (vo + va) * 3, *nb = w.nrm + (vo + vb) * 3, *qa = w.q + (vo + va) * 3, *qb = w.q + (vo + vb) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            n[k] = na[k] + t * (nb[k] - na[k]);
            p[k] = qa[k] + t * (qb[k] - qa[k]);
        }
    } else {
        const int* f = m.faces + (size_t)(unsigned)key * 3;
        const int* xa = w.xy + (vo + f[0]) * 2;
        const int* xb = w.xy + (vo + f[1]) * 2;
        const int* xc = w.xy + (vo + f[2]) * 2;
        const int px = i * kSub + kHalf, py = j * kSub + kHalf;
        const float inv_area = 1.f / (float)edge(xa[0], xa[1], xb[0], xb[1], xc[0], xc[1]);
        const float b0 = (float)edge(xb[0], xb[1], xc[0], xc[1], px, py) * inv_area;
        const float b1 = (float)edge(xc[0], xc[1], xa[0], xa[1], px, py) * inv_area;
        const float b2 = (float)edge(xa[0], xa[1], xb[0], xb[1], px, py) * inv_area;
        const float *na = w.nrm + (vo + f[0]) * 3, *nb = w.nrm + (vo + f[1]) * 3, *nc = w.nrm + (vo + f[2]) * 3;
        const float *qa = w.q + (vo + f[0]) * 3, *qb = w.q + (vo + f[1]) * 3, *qc = w.q + (vo + f[2]) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            n[k] = b0 * na[k] + b1 * nb[k] + b2 * nc[k];
            p[k] = b0 * qa[k] + b1 * qb[k] + b2 * qc[k];
        }
    }
    shade_store(n, p, c.colour[slot], images + (((size_t)c.image[slot] * view.H + (view.H - 1 - j)) * view.W + i) * 3);
}

__global__ __launch_bounds__(256) void raster_winner_kernel(RasterView view, RasterWork w, int* __restrict__ winner) {
    const int i = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1)), r = blockIdx.y * kTileH + threadIdx.x / kTileW;
    if (i >= view.W || r >= view.H) return;
    const unsigned long long key = w.depth[(size_t)(view.H - 1 - r) * view.W + i];
    winner[(size_t)r * view.W + i] = key == kDepthClear ? -1 : (int)(unsigned)key;
}

dim3 pixel_grid(const RasterView& v, int slots) { return dim3((v.W + kTileW - 1) / kTileW, (v.H + kTileH - 1) / kTileH, slots); }

}  // namespace

size_t raster_depth_words(int H, int W) { return (size_t)H * W; }

hipError_t launch_raster_setup(const float* verts, const float* cams, const RasterChunk& c, const RasterView& v, const RasterMesh& m, RasterWork w,
                               hipStream_t s) {
    // every byte 0x80: below -(2^28) in all four components, the start of the atomicMax
    hipError_t e = hipMemsetAsync(w.bbox, 0x80, (size_t)c.n * 4 * sizeof(int), s);
    if (e != hipSuccess || !m.n_verts) return e;
    const dim3 grid((m.n_verts + 255) / 256, c.n);
    hipLaunchKernelGGL(raster_setup_kernel, grid, dim3(256), 0, s, verts, cams, c, v, m.n_verts, w);
    hipLaunchKernelGGL(raster_normals_kernel, grid, dim3(256), 0, s, m, w);
    return hipGetLastError();
}

hipError_t launch_raster_cover(const RasterChunk& c, const RasterView& v, const RasterMesh& m, RasterWork w, hipStream_t s) {
    hipLaunchKernelGGL(raster_clear_kernel<false>, pixel_grid(v, c.n), dim3(256), 0, s, v, w);
    if (m.n_faces) hipLaunchKernelGGL(raster_cover_kernel, dim3((m.n_faces + 255) / 256, c.n), dim3(256), 0, s, v, m, w);
    return hipGetLastError();
}

hipError_t launch_raster_resolve(const RasterChunk& c, const RasterView& v, const RasterMesh& m, RasterWork w, unsigned char* images, hipStream_t s) {
    hipLaunchKernelGGL(raster_resolve_kernel<false>, pixel_grid(v, c.n), dim3(256), 0, s, c, v, m, w, images);
    return hipGetLastError();
}

hipError_t launch_raster_lines_cover(const RasterChunk& c, const RasterView& v, const RasterMesh& m, RasterWork w, hipStream_t s) {
    hipLaunchKernelGGL(raster_clear_kernel<true>, pixel_grid(v, c.n), dim3(256), 0, s, v, w);
    if (m.n_faces) hipLaunchKernelGGL(raster_lines_cover_kernel, dim3((m.n_faces + 255) / 256, c.n), dim3(256), 0, s, v, m, w);
    return hipGetLastError();
}

hipError_t launch_raster_lines_resolve(const RasterChunk& c, const RasterView& v, const RasterMesh& m, RasterWork w, unsigned char* images, hipStream_t s) {
    hipLaunchKernelGGL(raster_resolve_kernel<true>, pixel_grid(v, c.n), dim3(256), 0, s, c, v, m, w, images);
    return hipGetLastError();
}

hipError_t launch_raster_lines_clear(const RasterView& v, RasterWork w, int slots, hipStream_t s) {
    hipLaunchKernelGGL(raster_clear_kernel<true>, pixel_grid(v, slots), dim3(256), 0, s, v, w);
    return hipGetLastError();
}

hipError_t launch_raster_winner(const RasterView& v, RasterWork w, int* winner, hipStream_t s) {
    hipLaunchKernelGGL(raster_winner_kernel, pixel_grid(v, 1), dim3(256), 0, s, v, w, winner);
    return hipGetLastError();
}

}  // namespace grk
