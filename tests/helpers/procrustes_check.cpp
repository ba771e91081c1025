// Stand-alone check of csrc/procrustes3.h on the host: its own main, no HIP, nothing of the library but that header.  Built with AddressSanitizer
// and UBSan and run directly (tests/test_procrustes_host_cpu.py).
//
// For every matrix K the returned R must pass a certificate that trusts no SVD: R^T R = I to 1e-12 (largest absolute row sum of the difference),
// det R > 0, M = R K symmetric to 1e-12 |K|_F, and the eigenvalues l1 >= l2 >= l3 of M (cyclic two-sided Jacobi in long double, written here)
// satisfy l2 >= |l3| and l2 + l3 >= 0 to 1e-12 |K|_F.  A proper rotation maximises trace(R K) exactly when R K is symmetric with such a spectrum.
// The returned singular values must be ordered and non-negative, carry |K|_F^2 = s1^2 + s2^2 + s3^2, and give trace(M) = s1 + s2 + sign s3.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "procrustes3.h"

namespace {

uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint64_t next_u64() {                                          // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
double uniform(double lo, double hi) { return lo + (hi - lo) * (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }

void random_rotation(double* Q) {
    double q[4], n = 0;
    do {
        n = 0;
        for (double& v : q) { v = uniform(-1, 1); n += v * v; }
    } while (n < 1e-3 || n > 1.0);
    n = std::sqrt(n);
    const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                         2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    for (int i = 0; i < 9; ++i) Q[i] = R[i];
}

void matmul(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

// eigenvalues of a symmetric matrix, descending
void sym_eigenvalues(const double* M, long double* l) {
    long double a[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) a[i][j] = 0.5L * ((long double)M[3 * i + j] + (long double)M[3 * j + i]);
    for (int sweep = 0; sweep < 30; ++sweep)
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (a[p][q] == 0) continue;
                const long double theta = (a[q][q] - a[p][p]) / (2 * a[p][q]);
                const long double t = (theta >= 0 ? 1 : -1) / (std::fabs(theta) + std::sqrt(1 + theta * theta));
                const long double c = 1 / std::sqrt(1 + t * t), s = c * t;
                for (int k = 0; k < 3; ++k) { const long double x = a[k][p], y = a[k][q]; a[k][p] = c * x - s * y; a[k][q] = s * x + c * y; }
                for (int k = 0; k < 3; ++k) { const long double x = a[p][k], y = a[q][k]; a[p][k] = c * x - s * y; a[q][k] = s * x + c * y; }
            }
    l[0] = a[0][0]; l[1] = a[1][1]; l[2] = a[2][2];
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2 - i; ++j)
            if (l[j] < l[j + 1]) { const long double x = l[j]; l[j] = l[j + 1]; l[j + 1] = x; }
}

int g_failures = 0, g_count = 0;
double g_worst_orth = 0, g_worst_sym = 0, g_worst_trace = 0;

void check(const double* K, const char* what, bool want_identity = false) {
    ++g_count;
    const grk::Procrustes3 pr = grk::procrustes3(K);
    const double* R = pr.R;
    double normK = 0;
    for (int i = 0; i < 9; ++i) normK += K[i] * K[i];
    normK = std::sqrt(normK);
    const double tol = 1e-12 * normK;
    bool ok = true;
    double orth = 0;
    for (int i = 0; i < 3; ++i) {
        double row = 0;
        for (int j = 0; j < 3; ++j) row += std::fabs(R[i] * R[j] + R[3 + i] * R[3 + j] + R[6 + i] * R[6 + j] - (i == j ? 1.0 : 0.0));
        orth = std::fmax(orth, row);
    }
    ok = ok && orth <= 1e-12;
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    ok = ok && det > 0;
    double M[9];
    matmul(R, K, M);
    double sym = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) sym = std::fmax(sym, std::fabs(M[3 * i + j] - M[3 * j + i]));
    ok = ok && sym <= tol;
    long double l[3];
    sym_eigenvalues(M, l);
    ok = ok && (double)(l[1] - std::fabs(l[2])) >= -tol && (double)(l[1] + l[2]) >= -tol;
    const double* s = pr.sigma;
    ok = ok && s[0] >= s[1] && s[1] >= s[2] && s[2] >= 0 && (pr.sign == 1.0 || pr.sign == -1.0);
    ok = ok && std::fabs(std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]) - normK) <= 1e-12 * normK;
    const double trace_err = std::fabs((M[0] + M[4] + M[8]) - (s[0] + s[1] + pr.sign * s[2]));
    ok = ok && trace_err <= tol;
    if (want_identity)
        for (int i = 0; i < 9; ++i) ok = ok && R[i] == (i % 4 == 0 ? 1.0 : 0.0);
    if (normK > 0) {
        g_worst_orth = std::fmax(g_worst_orth, orth);
        g_worst_sym = std::fmax(g_worst_sym, sym / normK);
        g_worst_trace = std::fmax(g_worst_trace, trace_err / normK);
    }
    if (!ok) {
        if (++g_failures <= 10) {
            std::printf("FAIL %s #%d: orth %.3e det %.3f sym %.3e (tol %.3e) eig %.6Le %.6Le %.6Le sigma %.6e %.6e %.6e sign %.0f trace_err %.3e\n  K =", what, g_count, orth,
                        det, sym, tol, l[0], l[1], l[2], s[0], s[1], s[2], pr.sign, trace_err);
            for (int i = 0; i < 9; ++i) std::printf(" %.17g", K[i]);
            std::printf("\n");
        }
    }
}

void scaled(const double* K, double f, double* out) {
    for (int i = 0; i < 9; ++i) out[i] = K[i] * f;
}

}  // namespace

int main() {
    const double zero[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const double rank1[9] = {1, 2, 3, 2, 4, 6, 3, 6, 9};
    const double rank1b[9] = {0, 0, 0, 0, 0, -5, 0, 0, 0};
    const double rank2[9] = {3, 0, 0, 0, 2, 0, 0, 0, 0};
    const double rank2b[9] = {1, 1, 0, 1, -1, 0, 0, 0, 0};
    const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double refl[9] = {2, 0, 0, 0, 1, 0, 0, 0, -1};
    const double minus_eye[9] = {-1, 0, 0, 0, -1, 0, 0, 0, -1};
    const double repeated[9] = {0, 2, 0, -2, 0, 0, 0, 0, 1};
    const double dense[9] = {0.3, -1.2, 0.7, 2.1, 0.4, -0.9, -0.6, 1.5, 0.8};
    check(zero, "zero", true);
    check(rank1, "rank 1");
    check(rank1b, "rank 1, one entry");
    check(rank2, "rank 2");
    check(rank2b, "rank 2, reflection in the plane");
    check(eye, "diag(1,1,1)");
    check(refl, "diag(2,1,-1)");
    check(minus_eye, "-I");
    check(repeated, "repeated sigma");
    check(dense, "dense");
    double K[9];
    const double* const exact[] = {rank1, rank2, eye, refl, dense};
    for (const double* e : exact) {
        scaled(e, 1e-30, K); check(K, "1e-30 scaling");
        scaled(e, 1e+30, K); check(K, "1e+30 scaling");
    }
    const int kExact = g_count;
    for (int i = 0; i < 40000; ++i) {
        double A[9], B[9], Q1[9], Q2[9];
        switch (i % 8) {
            case 4: {                                          // rank 1
                double u[3], v[3];
                for (int k = 0; k < 3; ++k) { u[k] = uniform(-1, 1); v[k] = uniform(-1, 1); }
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c) K[3 * r + c] = u[r] * v[c];
                check(K, "random rank 1");
                break;
            }
            case 5: {                                          // rank 2 up to rounding
                random_rotation(Q1); random_rotation(Q2);
                const double d[3] = {uniform(0.1, 2), uniform(0.1, 2) * (i % 16 == 5 ? -1 : 1), 0};
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c) A[3 * r + c] = Q1[3 * r + c] * d[c];
                matmul(A, Q2, K);
                check(K, "random rank 2");
                break;
            }
            case 6: {                                          // two equal singular values, either sign of the determinant
                random_rotation(Q1); random_rotation(Q2);
                const double a = uniform(0.1, 2), b = uniform(0.0, 2) * (i % 16 == 6 ? -1 : 1);
                const double d[3] = {a, i % 32 < 16 ? a : b, i % 32 < 16 ? b : b};
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c) A[3 * r + c] = Q1[3 * r + c] * d[c];
                matmul(A, Q2, K);
                check(K, "random repeated sigma");
                break;
            }
            case 7: {                                          // any scale
                const double f = std::pow(10.0, uniform(-30, 30));
                for (int k = 0; k < 9; ++k) K[k] = uniform(-1, 1) * f;
                check(K, "random scaled");
                break;
            }
            case 3: {                                          // ill-conditioned: singular values 1, 10^-a, 10^-b
                random_rotation(Q1); random_rotation(Q2);
                const double d[3] = {1, std::pow(10.0, -uniform(0, 14)), std::pow(10.0, -uniform(0, 16)) * (i % 16 == 3 ? -1 : 1)};
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c) B[3 * r + c] = Q1[3 * r + c] * d[c];
                matmul(B, Q2, K);
                check(K, "random ill-conditioned");
                break;
            }
            default:
                for (int k = 0; k < 9; ++k) K[k] = uniform(-1, 1);
                check(K, "random dense");
        }
    }
    std::printf("matrices: %d, exact: %d, failures: %d\n", g_count, kExact, g_failures);
    std::printf("worst |R^T R - I| %.3e, asymmetry / |K| %.3e, trace error / |K| %.3e\n", g_worst_orth, g_worst_sym, g_worst_trace);
    if (g_failures) return 1;
    std::printf("ok\n");
    return 0;
}
