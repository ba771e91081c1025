// The integer part of the wireframe's line rule ("Lines"): no HIP and nothing of the library, so render_kernels.hip uses it on the
// device and the stand-alone checker tests/helpers/raster_lines_check.cpp on the host, against the formula in 128-bit arithmetic.
//
// An edge between two snapped vertices is x-major if |dx| >= |dy|, else y-major; P is the major coordinate, Q the minor one; the end points
// are ordered P0 < P1 (lo, hi) and everything after that reads (lo, hi) only.  Major index m is covered iff P0 <= 256 m + 128 < P1.  There the
// minor index is n = floor((Q0 dP + (256 m + 128 - P0) dQ) / (256 dP)): the pixel whose square holds the line at the centre of m.  With
// |X|, |Y| <= 2^28: dP < 2^29 + 1, |Q0 dP| < 2^58, |(.) dQ| < 2^59, D = 256 dP < 2^38; everything fits int64.
// One division gives n and the remainder at a lane's first m (line_minor); a stride of s major steps adds s * 256 dQ = sq D + sr to the
// numerator, 0 <= sr < D (line_stride: s = 1 needs no division), so line_advance is an add and one carry and gives the same integers.
//
// Wide lines (the skeleton view; skeleton_kernels.hip): a line of width w pixels, 1 <= w <= 16, covers at major index m the w
// minor indices n0 .. n0 + w - 1, n0 = floor((Q0 dP + (256 m + 128 - P0) dQ - (w - 1) 128 dP) / (256 dP)) -- OpenGL's rule for non-antialiased wide
// lines: the column of w pixels starts (w - 1) / 2 pixels below the line.  The offset is constant along the line, so it goes into the numerator
// once (line_minor_wide; |(w - 1) 128 dP| < 2^41) and the stepping above is unchanged.  w = 1 is line_minor.
#pragma once

#if defined(__HIPCC__)
#define GRK_LINES_HD __host__ __device__ __forceinline__
#else
#define GRK_LINES_HD inline
#endif

namespace grk {

constexpr int kRasterSnapBits = 8;           // sub-pixel bits of the snapped window coordinates

struct LineRec {
    int P0, Q0, P1, Q1;    // lo, hi
    float z0, z1;
    int m0, m1;            // the covered major indices inside the viewport; m0 > m1: none
    int xmajor;
};

struct LineStride { long long D, sq, sr; };

// The record of a -> b but for z and the range; flip: lo is b.  false: a point, which draws nothing.  b -> a gives the same P, Q and !flip
GRK_LINES_HD bool line_order(int ax, int ay, int bx, int by, LineRec& r, bool& flip) {
    const int dx = bx - ax, dy = by - ay;
    if (dx == 0 && dy == 0) return false;
    r.xmajor = (dx < 0 ? -dx : dx) >= (dy < 0 ? -dy : dy);
    const int pa = r.xmajor ? ax : ay, qa = r.xmajor ? ay : ax, pb = r.xmajor ? bx : by, qb = r.xmajor ? by : bx;
    flip = pb < pa;
    r.P0 = flip ? pb : pa, r.Q0 = flip ? qb : qa, r.P1 = flip ? pa : pb, r.Q1 = flip ? qa : qb;
    return true;
}

// 256 m + 128 in [P0, P1): m from ceil((P0 - 128) / 256) to ceil((P1 - 128) / 256) - 1, clamped to [0, n_major)
GRK_LINES_HD void line_range(LineRec& r, int n_major) {
    constexpr int sub = 1 << kRasterSnapBits, half = sub / 2;
    const int first = (r.P0 - half + sub - 1) >> kRasterSnapBits, last = ((r.P1 - half + sub - 1) >> kRasterSnapBits) - 1;
    r.m0 = first > 0 ? first : 0;
    r.m1 = last < n_major - 1 ? last : n_major - 1;
}

GRK_LINES_HD void line_minor(const LineRec& r, int m, long long& n, long long& rem) {
    constexpr int sub = 1 << kRasterSnapBits, half = sub / 2;
    const long long dP = (long long)r.P1 - r.P0, dQ = (long long)r.Q1 - r.Q0, D = sub * dP;
    const long long num = (long long)r.Q0 * dP + ((long long)m * sub + half - r.P0) * dQ;
    n = num / D;
    rem = num - n * D;
    if (rem < 0) rem += D, --n;
}

// n0 of a line of width w at major index m (w = 1: line_minor)
GRK_LINES_HD void line_minor_wide(const LineRec& r, int m, int w, long long& n, long long& rem) {
    constexpr int sub = 1 << kRasterSnapBits, half = sub / 2;
    const long long dP = (long long)r.P1 - r.P0, dQ = (long long)r.Q1 - r.Q0, D = sub * dP;
    const long long num = (long long)r.Q0 * dP + ((long long)m * sub + half - r.P0) * dQ - (long long)(w - 1) * half * dP;
    n = num / D;
    rem = num - n * D;
    if (rem < 0) rem += D, --n;
}

GRK_LINES_HD LineStride line_stride(const LineRec& r, int s) {
    constexpr int sub = 1 << kRasterSnapBits;
    LineStride st;
    st.D = sub * ((long long)r.P1 - r.P0);
    const long long step = (long long)s * sub * ((long long)r.Q1 - r.Q0);
    if (s == 1) st.sq = step == st.D ? 1 : (step >= 0 ? 0 : -1);          // |dQ| <= dP
    else st.sq = step / st.D;
    st.sr = step - st.sq * st.D;
    if (st.sr < 0) st.sr += st.D, --st.sq;
    return st;
}

GRK_LINES_HD void line_advance(const LineStride& st, long long& n, long long& rem) {
    n += st.sq, rem += st.sr;
    if (rem >= st.D) rem -= st.D, ++n;
}

}  // namespace grk
