// The rotation of the 3x3 orthogonal Procrustes problem in float64: no HIP and nothing of the library, so metric_kernels.hip uses it on
// the device and the stand-alone checker tests/helpers/procrustes_check.cpp on the host.
//
// Given K (row-major), procrustes3 returns the proper rotation R that maximises trace(R K), the singular values s1 >= s2 >= s3 >= 0 of K and
// sign = sign det(U V^T) of its SVD K = U S V^T, so that trace(R K) = s1 + s2 + sign s3 and R = V diag(1, 1, sign) U^T.
//
// One-sided (Hestenes) Jacobi on K itself: plane rotations from the right make the columns of A = K V orthogonal, A = U S.  Nothing is squared
// and divided by s3 (an eigen-decomposition of K^T K would lose (s1 / s3)^2), and the sweep count is FIXED: kProcrustesSweeps sweeps of the three
// column pairs, no data-dependent exit.  A 3x3 matrix is orthogonal to rounding after 5 or 6 sweeps (quadratic convergence); 10 are run.
// K is first divided by its largest |entry|, so 1e-30 K and 1e+30 K take the same path (the singular values are scaled back).
//
// The columns are then sorted by norm, V is made proper (negating the third column of both V and A keeps K V = A), and U' = [u1 u2 u1 x u2] is
// built by Gram-Schmidt from the two LARGEST columns only: u3' = +-u3 wherever s3 > 0 decides it, and sign = sign(a3 . u3').  R = V U'^T is then a
// product of two proper rotations for every rank:
//   rank 2 (s3 = 0): u3' completes the frame, trace = s1 + s2;
//   rank 1 (the second column's part orthogonal to u1 is rounding noise, <= 4e-16 s1): u2 = the unit vector orthogonal to u1 nearest the axis
//           on which u1 is smallest -- any choice costs at most that noise;
//   rank 0 (K = 0): R = I, the rule DESIGN 4.8 states for var1 == 0.
// Which of several maximisers comes back for repeated singular values is whatever the sweeps leave (for a diagonal K: V = I).
#pragma once

#if defined(__HIPCC__)
#define GRK_PROC_HD __host__ __device__ inline
#else
#define GRK_PROC_HD inline
#endif

namespace grk {

constexpr int kProcrustesSweeps = 10;

struct Procrustes3 {
    double R[9];       // row-major proper rotation maximising trace(R K)
    double sigma[3];   // s1 >= s2 >= s3 >= 0
    double sign;       // +1 or -1: trace(R K) = s1 + s2 + sign s3
};

namespace procrustes_detail {

// rotate columns p and q of A and V (3x3 row-major) so that the two columns of A become orthogonal
GRK_PROC_HD void rotate_pair(double* A, double* V, int p, int q) {
    const double alpha = A[p] * A[p] + A[3 + p] * A[3 + p] + A[6 + p] * A[6 + p];
    const double beta = A[q] * A[q] + A[3 + q] * A[3 + q] + A[6 + q] * A[6 + q];
    const double gamma = A[p] * A[q] + A[3 + p] * A[3 + q] + A[6 + p] * A[6 + q];
    if (gamma == 0.) return;
    const double zeta = (beta - alpha) / (2. * gamma);                         // may be +-inf for a tiny gamma: t = 0, no rotation
    const double t = (zeta >= 0. ? 1. : -1.) / (__builtin_fabs(zeta) + __builtin_sqrt(1. + zeta * zeta));
    const double c = 1. / __builtin_sqrt(1. + t * t), s = c * t;
    for (int i = 0; i < 3; ++i) {
        const double ap = A[3 * i + p], aq = A[3 * i + q];
        A[3 * i + p] = c * ap - s * aq;
        A[3 * i + q] = s * ap + c * aq;
        const double vp = V[3 * i + p], vq = V[3 * i + q];
        V[3 * i + p] = c * vp - s * vq;
        V[3 * i + q] = s * vp + c * vq;
    }
}

GRK_PROC_HD void swap_columns(double* A, double* V, double* n2, int p, int q) {
    for (int i = 0; i < 3; ++i) {
        double x = A[3 * i + p]; A[3 * i + p] = A[3 * i + q]; A[3 * i + q] = x;
        x = V[3 * i + p]; V[3 * i + p] = V[3 * i + q]; V[3 * i + q] = x;
    }
    const double x = n2[p]; n2[p] = n2[q]; n2[q] = x;
}

}  // namespace procrustes_detail

GRK_PROC_HD Procrustes3 procrustes3(const double* K) {
    using namespace procrustes_detail;
    Procrustes3 out;
    for (int i = 0; i < 9; ++i) out.R[i] = (i % 4 == 0) ? 1. : 0.;
    out.sigma[0] = out.sigma[1] = out.sigma[2] = 0.;
    out.sign = 1.;
    double scale = 0.;
    for (int i = 0; i < 9; ++i) scale = __builtin_fabs(K[i]) > scale ? __builtin_fabs(K[i]) : scale;
    if (!(scale > 0.)) return out;                                              // rank 0: R = I
    double A[9], V[9];
    for (int i = 0; i < 9; ++i) { A[i] = K[i] / scale; V[i] = (i % 4 == 0) ? 1. : 0.; }
    for (int sweep = 0; sweep < kProcrustesSweeps; ++sweep) {
        rotate_pair(A, V, 0, 1);
        rotate_pair(A, V, 0, 2);
        rotate_pair(A, V, 1, 2);
    }
    double n2[3];
    for (int c = 0; c < 3; ++c) n2[c] = A[c] * A[c] + A[3 + c] * A[3 + c] + A[6 + c] * A[6 + c];
    if (n2[0] < n2[1]) swap_columns(A, V, n2, 0, 1);
    if (n2[1] < n2[2]) swap_columns(A, V, n2, 1, 2);
    if (n2[0] < n2[1]) swap_columns(A, V, n2, 0, 1);
    const double detV = V[0] * (V[4] * V[8] - V[5] * V[7]) - V[1] * (V[3] * V[8] - V[5] * V[6]) + V[2] * (V[3] * V[7] - V[4] * V[6]);
    if (detV < 0.)
        for (int i = 0; i < 3; ++i) { V[3 * i + 2] = -V[3 * i + 2]; A[3 * i + 2] = -A[3 * i + 2]; }
    const double s1 = __builtin_sqrt(n2[0]), s2 = __builtin_sqrt(n2[1]), s3 = __builtin_sqrt(n2[2]);     // s1 >= 1 / sqrt(3): the largest |entry| is 1
    double u1[3], u2[3], u3[3];
    for (int i = 0; i < 3; ++i) u1[i] = A[3 * i] / s1;
    for (int i = 0; i < 3; ++i) u2[i] = A[3 * i + 1];
    double w2 = 0.;
    for (int pass = 0; pass < 2; ++pass) {                                      // Gram-Schmidt, twice
        const double d = u2[0] * u1[0] + u2[1] * u1[1] + u2[2] * u1[2];
        for (int i = 0; i < 3; ++i) u2[i] -= d * u1[i];
        w2 = u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2];
    }
    if (!(w2 > 1.6e-31 * n2[0])) {                                              // rank 1: |w| <= 4e-16 s1 is noise; any unit vector orthogonal to u1 serves
        const double a0 = __builtin_fabs(u1[0]), a1 = __builtin_fabs(u1[1]), a2 = __builtin_fabs(u1[2]);
        const int axis = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
        for (int pass = 0; pass < 2; ++pass) {
            if (pass == 0) for (int i = 0; i < 3; ++i) u2[i] = (i == axis) ? 1. : 0.;
            const double d = u2[0] * u1[0] + u2[1] * u1[1] + u2[2] * u1[2];
            for (int i = 0; i < 3; ++i) u2[i] -= d * u1[i];
        }
        w2 = u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2];                     // >= 2/3: u1's smallest component is at most 1 / sqrt(3)
    }
    const double w = __builtin_sqrt(w2);
    for (int i = 0; i < 3; ++i) u2[i] /= w;
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
    u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
    u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    const double d3 = A[2] * u3[0] + A[5] * u3[1] + A[8] * u3[2];
    out.sign = d3 < 0. ? -1. : 1.;
    out.sigma[0] = s1 * scale; out.sigma[1] = s2 * scale; out.sigma[2] = s3 * scale;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out.R[3 * i + j] = V[3 * i] * u1[j] + V[3 * i + 1] * u2[j] + V[3 * i + 2] * u3[j];
    return out;
}

}  // namespace grk
