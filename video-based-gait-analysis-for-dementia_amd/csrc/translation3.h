// The camera-space translation of one frame in float64: no HIP and nothing of the library, so translation_kernels.hip uses it on the
// device and the stand-alone checker tests/helpers/translation3_check.cpp on the host.  Whoever includes it compiles WITHOUT fma contraction
// (-ffp-contract=off): every operation below rounds once, in the order the parentheses show.
//
// translation3_fit -- SPIN's weighted least squares (the reference's estimate_translation_np, lib/utils/geometry.py:296-337) for the t that makes
// the 3D joints (X, Y, Z) + t project onto the 2D detections (x, y) through a pinhole camera (f, cx, cy).  Pair j of the table joins 3D joint
// p3[j] with 2D joint p2[j]; its weight is w = conf where conf > threshold and conf is finite, else the pair is not used at all (its other values
// are loaded and dropped: they never enter the arithmetic, so a NaN beside a dead confidence does no harm).  With u = x - cx, v = y - cy, ex = u Z - f X, ey = v Z - f Y:
//     A = [[f^2 Sw, 0, -f Swu], [0, f^2 Sw, -f Swv], [-f Swu, -f Swv, Sw(u^2 + v^2)]],   b = [f Sw ex, f Sw ey, -Sw(u ex + v ey)]
// which is Q^T W^2 Q and Q^T W^2 c of the reference with W^2 = conf (the reference squares float64 sqrt(conf): one rounding per weight apart).
// The seven sums run over the used pairs in table order.  A t = b is solved by elimination with partial pivoting (the first of equal pivots).
// The pairs are LOADED kTransGroup at a time, before the first of them is looked at: a lane of the kernel walks its own frame's rows, every load is
// a trip to memory of its own, and a load behind a test of the confidence would wait for that test -- two dependent trips a pair.  The arithmetic
// still takes the pairs one by one in table order, so the grouping changes no bit.
// The reprojection error is the weighted mean over the used pairs of |f (X + tx, Y + ty) / (Z + tz) + (cx, cy) - (x, y)|, in pixels.
// status: kFitted; kTooFew: fewer than min_joints used pairs; kDegenerate: a zero pivot, a non-finite t or error, or a used joint with
// Z + tz <= 0 (a body behind the camera).  t and the error are NaN unless kFitted; n_used is always the count.
//
// translation3_fill -- frame i (1 <= i <= gap) of a run of `gap` unfitted frames between the fitted translations prev and next, by the arithmetic
// of numpy.linspace(prev, next, gap + 2)[i] on (3,) arrays: step = (next - prev) / (gap + 1) per component, out = i * step + prev (a multiply, then
// an add) -- unless a component's step is zero (equal ends, or an underflow), where numpy switches ALL three to (i / (gap + 1)) * (next - prev) + prev.
#pragma once

#if defined(__HIPCC__)
#define GRK_TRANS_HD __host__ __device__ inline
#else
#define GRK_TRANS_HD inline
#endif

namespace grk {

constexpr int kTransFitted = 0, kTransTooFew = 1, kTransDegenerate = 2, kTransFilled = 3;

struct Translation3 {
    double t[3];     // NaN unless status == kTransFitted
    double reproj;   // pixels; NaN unless status == kTransFitted
    int n_used;      // pairs whose confidence passed
    int status;
};

constexpr int kTransGroup = 4;

namespace translation_detail {

struct PairGroup { double w[kTransGroup], X[kTransGroup], Y[kTransGroup], Z[kTransGroup], x[kTransGroup], y[kTransGroup]; };

// pairs j0 .. j0 + kTransGroup - 1 of the table, widened; past the end of the table w = 0, which no threshold >= 0 lets through
GRK_TRANS_HD PairGroup load_group(const float* joints3d, const float* joints2d, const int* p3, const int* p2, int P, int j0) {
    PairGroup g;
    for (int k = 0; k < kTransGroup; ++k) {
        const bool in = j0 + k < P;
        const float* s = joints3d + 3 * (in ? p3[j0 + k] : p3[j0]);
        const float* d = joints2d + 3 * (in ? p2[j0 + k] : p2[j0]);
        g.X[k] = (double)s[0]; g.Y[k] = (double)s[1]; g.Z[k] = (double)s[2];
        const double x = (double)d[0], y = (double)d[1], w = (double)d[2];      // all three loaded, whatever `in` says: no load waits for a branch
        g.x[k] = x; g.y[k] = y;
        g.w[k] = in ? w : 0.;
    }
    return g;
}

GRK_TRANS_HD bool finite(double v) { return v - v == 0.; }     // false for NaN and for either infinity

// x of A x = b (A row-major, both overwritten) by elimination with partial pivoting; false at a zero (or NaN) pivot
GRK_TRANS_HD bool solve3(double (&A)[9], double (&b)[3], double (&x)[3]) {
    for (int k = 0; k < 3; ++k) {
        int p = k;
        double best = __builtin_fabs(A[3 * k + k]);
        for (int r = k + 1; r < 3; ++r) {
            const double a = __builtin_fabs(A[3 * r + k]);
            if (a > best) { best = a; p = r; }
        }
        if (!(best > 0.)) return false;
        if (p != k) {
            for (int c = 0; c < 3; ++c) { const double s = A[3 * k + c]; A[3 * k + c] = A[3 * p + c]; A[3 * p + c] = s; }
            const double s = b[k]; b[k] = b[p]; b[p] = s;
        }
        for (int r = k + 1; r < 3; ++r) {
            const double m = A[3 * r + k] / A[3 * k + k];
            for (int c = k + 1; c < 3; ++c) A[3 * r + c] = A[3 * r + c] - m * A[3 * k + c];
            b[r] = b[r] - m * b[k];
        }
    }
    x[2] = b[2] / A[8];
    x[1] = (b[1] - A[5] * x[2]) / A[4];
    x[0] = ((b[0] - A[1] * x[1]) - A[2] * x[2]) / A[0];
    return true;
}

}  // namespace translation_detail

// joints3d: the frame's (K3,3) float32 joints, joints2d: its (K2,3) float32 rows (x, y, conf); p3, p2: the P pairs (indices inside K3 and K2)
GRK_TRANS_HD Translation3 translation3_fit(const float* joints3d, const float* joints2d, const int* p3, const int* p2, int P, double f, double cx, double cy,
                                           double threshold, int min_joints) {
    using translation_detail::finite;
    const double nan = __builtin_nan("");
    Translation3 out{{nan, nan, nan}, nan, 0, kTransTooFew};
    double sw = 0., swu = 0., swv = 0., swr = 0., sbx = 0., sby = 0., sbz = 0.;
    int used = 0;
    for (int j0 = 0; j0 < P; j0 += kTransGroup) {
        const translation_detail::PairGroup g = translation_detail::load_group(joints3d, joints2d, p3, p2, P, j0);
        for (int k = 0; k < kTransGroup; ++k) {
            const double w = g.w[k];
            if (!(w > threshold) || !finite(w)) continue;
            const double u = g.x[k] - cx, v = g.y[k] - cy;
            const double ex = u * g.Z[k] - f * g.X[k], ey = v * g.Z[k] - f * g.Y[k];
            sw = sw + w;
            swu = swu + w * u;
            swv = swv + w * v;
            swr = swr + w * (u * u + v * v);
            sbx = sbx + w * ex;
            sby = sby + w * ey;
            sbz = sbz + w * (u * ex + v * ey);
            ++used;
        }
    }
    out.n_used = used;
    if (used < min_joints) return out;
    out.status = kTransDegenerate;
    const double d0 = (f * f) * sw, ax = -(f * swu), ay = -(f * swv);
    double A[9] = {d0, 0., ax, 0., d0, ay, ax, ay, swr}, b[3] = {f * sbx, f * sby, -sbz}, t[3];
    if (!translation_detail::solve3(A, b, t)) return out;
    if (!finite(t[0]) || !finite(t[1]) || !finite(t[2])) return out;
    double acc = 0.;
    for (int j0 = 0; j0 < P; j0 += kTransGroup) {
        const translation_detail::PairGroup g = translation_detail::load_group(joints3d, joints2d, p3, p2, P, j0);
        for (int k = 0; k < kTransGroup; ++k) {
            const double w = g.w[k];
            if (!(w > threshold) || !finite(w)) continue;
            const double depth = g.Z[k] + t[2];
            if (!(depth > 0.)) return out;
            const double px = ((f * (g.X[k] + t[0])) / depth + cx) - g.x[k];
            const double py = ((f * (g.Y[k] + t[1])) / depth + cy) - g.y[k];
            acc = acc + w * __builtin_sqrt(px * px + py * py);
        }
    }
    const double reproj = acc / sw;
    if (!finite(reproj)) return out;
    out.t[0] = t[0]; out.t[1] = t[1]; out.t[2] = t[2];
    out.reproj = reproj;
    out.status = kTransFitted;
    return out;
}

GRK_TRANS_HD void translation3_fill(const double* prev, const double* next, int gap, int i, double* out) {
    const double div = (double)(gap + 1), y = (double)i;
    double delta[3], step[3];
    bool any_zero = false;
    for (int c = 0; c < 3; ++c) {
        delta[c] = next[c] - prev[c];
        step[c] = delta[c] / div;
        any_zero = any_zero || step[c] == 0.;
    }
    for (int c = 0; c < 3; ++c) out[c] = (any_zero ? (y / div) * delta[c] : y * step[c]) + prev[c];
}

}  // namespace grk
