// Volume, centre of mass, central second moments and area of a closed triangle mesh in float64: no HIP, no libm and nothing of the
// library, so mesh_moments_kernels.hip uses it on the device and the stand-alone checker tests/helpers/gait_body_check.cpp on the host.  Whoever
// includes it compiles WITHOUT fma contraction (-ffp-contract=off): every operation below rounds once, in the order the parentheses show.  Every
// test is a comparison that is false for NaN.
//
// mesh_face_terms  -- rule 2 of ONE face: the eleven terms of its corners a, b, c, each already relative to the frame's origin (rule 1).
// mesh_face        -- rules 1 and 2 of face i of a frame: the three corners gathered from float32 vertices, widened, the origin subtracted.
// mesh_column      -- rule 3's first half: column l of kMeshCols adds the terms of faces l, l + kMeshCols, ... in rising order from +0.0.
// mesh_tree        -- rule 3's second half on the host: col[l] += col[l + h] for l < h, h = kMeshCols / 2 .. 1 (the device does the same additions
//                     through LDS across waves and by x + shuffle_xor(x, h) inside a wave: + is commutative, lane 0 holds the same bits).
// mesh_row         -- rule 4: the eleven columns of a frame's row from its sums and its origin.
// mesh_unmatched_edges / mesh_table_text -- rule 5 and what a call refuses (host only), so that the stand-alone checker runs them too.
#pragma once

#include <cstdio>

#if defined(__HIPCC__)
#define GRK_MESH_HD __host__ __device__ inline
#else
#define GRK_MESH_HD inline
#endif

namespace grk {

constexpr int kMeshCols = 1024;           // NCOL: the columns of the fixed summation order
constexpr int kMeshTerms = 11;            // d, d s (3), d (aa + bb + cc + ss) (xx, yy, zz, xy, xz, yz), |n|
constexpr int kMeshRowCols = 11;          // volume, com (3), C (xx, yy, zz, xy, xz, yz), area
// the six second moments in the order xx, yy, zz, xy, xz, yz: the two axes of moment q
GRK_MESH_HD int mesh_axis_k(int q) { return q < 3 ? q : (q == 5 ? 1 : 0); }
GRK_MESH_HD int mesh_axis_l(int q) { return q < 3 ? q : (q == 3 ? 1 : 2); }

// rule 2.  a, b, c: the corners relative to the origin
GRK_MESH_HD void mesh_face_terms(const double* a, const double* b, const double* c, double* t) {
    const double d = (a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2])) + a[2] * (b[0] * c[1] - b[1] * c[0]);
    double s[3];
    for (int k = 0; k < 3; ++k) s[k] = (a[k] + b[k]) + c[k];
    t[0] = d;
    for (int k = 0; k < 3; ++k) t[1 + k] = d * s[k];
    for (int m = 0; m < 6; ++m) {
        const int k = mesh_axis_k(m), l = mesh_axis_l(m);
        t[4 + m] = d * (((a[k] * a[l] + b[k] * b[l]) + c[k] * c[l]) + s[k] * s[l]);
    }
    double u[3], w[3];
    for (int k = 0; k < 3; ++k) { u[k] = b[k] - a[k]; w[k] = c[k] - a[k]; }
    const double nx = u[1] * w[2] - u[2] * w[1], ny = u[2] * w[0] - u[0] * w[2], nz = u[0] * w[1] - u[1] * w[0];
    t[10] = __builtin_sqrt((nx * nx + ny * ny) + nz * nz);
}

// rules 1 and 2 of face i.  verts: the frame's (V,3) float32 vertices; faces: the (F,3) table; o: the frame's origin, widened
GRK_MESH_HD void mesh_face(const float* verts, const int* faces, int i, const double* o, double* t) {
    double p[3][3];
    for (int k = 0; k < 3; ++k) {
        const float* v = verts + 3 * (long long)faces[3 * i + k];
        for (int x = 0; x < 3; ++x) p[k][x] = (double)v[x] - o[x];
    }
    mesh_face_terms(p[0], p[1], p[2], t);
}

// rule 1: the first index of the table names the origin
GRK_MESH_HD void mesh_origin(const float* verts, const int* faces, double* o) {
    const float* v = verts + 3 * (long long)faces[0];
    for (int x = 0; x < 3; ++x) o[x] = (double)v[x];
}

// rule 3, column l of one frame: acc[kMeshTerms]
GRK_MESH_HD void mesh_column(const float* verts, const int* faces, int F, int l, const double* o, double* acc) {
    for (int k = 0; k < kMeshTerms; ++k) acc[k] = 0.;
    for (int i = l; i < F; i += kMeshCols) {
        double t[kMeshTerms];
        mesh_face(verts, faces, i, o, t);
        for (int k = 0; k < kMeshTerms; ++k) acc[k] = acc[k] + t[k];
    }
}

// rule 3, the tree over col (kMeshCols, kMeshTerms) in place: row 0 becomes S (host only; the device: mesh_moments_kernels.hip)
inline void mesh_tree(double* col) {
    for (int h = kMeshCols / 2; h >= 1; h >>= 1)
        for (int l = 0; l < h; ++l)
            for (int k = 0; k < kMeshTerms; ++k) col[l * kMeshTerms + k] = col[l * kMeshTerms + k] + col[(l + h) * kMeshTerms + k];
}

// rule 4.  S: the eleven sums; o: the origin; row: kMeshRowCols
GRK_MESH_HD void mesh_row(const double* S, const double* o, double* row) {
    const double none = __builtin_nan("");
    const bool has = S[0] > 0.;
    const double four = 4. * S[0], twenty = 20. * S[0];
    double m[3];
    row[0] = S[0] / 6.;
    for (int k = 0; k < 3; ++k) {
        m[k] = S[1 + k] / four;
        row[1 + k] = has ? o[k] + m[k] : none;
    }
    for (int q = 0; q < 6; ++q) {
        const double E = S[4 + q] / twenty;
        row[4 + q] = has ? E - m[mesh_axis_k(q)] * m[mesh_axis_l(q)] : none;
    }
    row[10] = S[10] / 2.;
}

// ---------------------------------------------------------------------------------------------------------------- rule 5 and the refusals (host only)
namespace mesh_detail {
inline void sift(unsigned long long* a, long long start, long long end) {      // heap sort's sift-down over a[start .. end)
    long long root = start;
    while (2 * root + 1 < end) {
        long long child = 2 * root + 1;
        if (child + 1 < end && a[child] < a[child + 1]) ++child;
        if (!(a[root] < a[child])) return;
        const unsigned long long t = a[root]; a[root] = a[child]; a[child] = t;
        root = child;
    }
}
inline void sort(unsigned long long* a, long long n) {
    for (long long s = n / 2 - 1; s >= 0; --s) sift(a, s, n);
    for (long long e = n - 1; e > 0; --e) {
        const unsigned long long t = a[0]; a[0] = a[e]; a[e] = t;
        sift(a, 0, e);
    }
}
inline long long lower(const unsigned long long* a, long long n, unsigned long long key) {      // the first place whose key is not below `key`
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
}  // namespace mesh_detail

// what is wrong with a face table: nothing, too few faces, an index outside [0, V), or directed edges without a partner
enum MeshTableKind { kMeshTableFine = 0, kMeshTableEmpty = 1, kMeshTableIndex = 2, kMeshTableOpen = 3 };
struct MeshTableFault { int kind; long long face, value; };      // kMeshTableEmpty: value = F; kMeshTableIndex: face names vertex value; kMeshTableOpen: value edges

// the first index outside [0, V) of a table of F >= 1 faces
inline MeshTableFault mesh_table_indices(const int* faces, int F, int V) {
    if (F < 1) return {kMeshTableEmpty, 0, F};
    for (long long k = 0; k < 3LL * F; ++k)
        if (faces[k] < 0 || faces[k] >= V) return {kMeshTableIndex, k / 3, faces[k]};
    return {kMeshTableFine, 0, 0};
}

// rule 5: of the 3 F directed edges (i, j) of a table whose indices lie in [0, V), those whose key i V + j is held by another edge too, that have no
// reverse edge (j, i), or that join a vertex to itself.  keys: 3 F words of the caller's, sorted here.  0: closed and consistently oriented
inline long long mesh_unmatched_edges(const int* faces, int F, int V, unsigned long long* keys) {
    const long long E = 3LL * F;
    for (long long f = 0; f < F; ++f)
        for (int k = 0; k < 3; ++k)
            keys[3 * f + k] = (unsigned long long)faces[3 * f + k] * (unsigned long long)V + (unsigned long long)faces[3 * f + (k + 1) % 3];
    mesh_detail::sort(keys, E);
    long long bad = 0;
    for (long long e = 0; e < E; ++e) {
        const unsigned long long i = keys[e] / (unsigned long long)V, j = keys[e] % (unsigned long long)V, back = j * (unsigned long long)V + i;
        const bool twice = (e > 0 && keys[e - 1] == keys[e]) || (e + 1 < E && keys[e + 1] == keys[e]);
        const long long at = mesh_detail::lower(keys, E, back);
        const bool answered = i != j && at < E && keys[at] == back;
        if (twice || !answered) ++bad;
    }
    return bad;
}

// the sentence of a fault, as the library says it behind its entry's name; `V` as the call knows it
inline void mesh_table_text(const MeshTableFault& w, int V, char* out, size_t cap) {
    if (w.kind == kMeshTableEmpty) std::snprintf(out, cap, "n_faces %lld < 1", w.value);
    else if (w.kind == kMeshTableIndex) std::snprintf(out, cap, "face %lld names vertex %lld, outside [0, %d)", w.face, w.value, V);
    else if (w.kind == kMeshTableOpen)
        std::snprintf(out, cap, "the face table is not a closed, consistently oriented surface: %lld directed edges are duplicated or lack their reverse edge", w.value);
    else if (cap) out[0] = 0;
}

}  // namespace grk
