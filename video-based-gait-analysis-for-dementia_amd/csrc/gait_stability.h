// Local dynamic stability of four body signals in float64 and integers (Rosenstein, Collins and De Luca, Physica D 65, 1993; Dingwell
// and Cusumano, Chaos 10, 2000): the nearest neighbour of every state of the delay-embedded signal and the geometric mean of the distance to it k
// frames later, carried as a mantissa product with an integer exponent.  No HIP and nothing of the library, so gait_stability_kernels.hip uses it on
// the device and the stand-alone checker tests/helpers/gait_stability_check.cpp on the host.  Whoever includes it compiles WITHOUT fma contraction
// (-ffp-contract=off): every operation below rounds once, in the order the parentheses show.  The four signals, their validity and the differenced
// signal y are gait_regularity.h's and gait_entropy.h's (reg_frame, reg_valid, ent_diff): an invalid y is NaN and "valid" is "finite".
//
// stab_frexp       -- C's frexp of a positive finite double, BY THE BITS (no builtin: the device and the host checker have no common one whose
//                     result on subnormals is stated): the mantissa in [0.5, 1) and the exponent, exact, subnormals included.
// stab_points      -- span, M and E of a sequence of T frames.
// stab_dist2       -- D2 of two points: the terms (a - b)(a - b) added in the order k = 0, 1, .. from the first term.  No square root.
// stab_scan        -- the candidates j of one stretch, in increasing j, against reference i: keeps (best D2, best j) under a strict <, so that
//                     among equal D2 the smallest j wins.  On the device a lane owns i and the stretch is an LDS tile.
// stab_walk        -- the divergence at ONE k: over the references in increasing i, n, S and P of rule 6.  On the device a lane owns a k.
// stab_rule_error  -- what a call refuses about its scalars (host only).  A sequence too long is ent_long_sequence's.
#pragma once

#include "gait_entropy.h"

namespace grk {

constexpr int kStabMaxDim = 8;            // a lane keeps the dim values of its point in registers
constexpr int kStabMaxLag = 16;
constexpr int kStabMaxTheiler = 4096;
constexpr int kStabMaxHorizon = 63;       // horizon + 1 lanes walk the references: one wave
constexpr int kStabTile = 1024;           // candidates of one LDS tile of the search
constexpr int kStabMaxSpan = (kStabMaxDim - 1) * kStabMaxLag;
constexpr int kStabPairCols = 2;          // n, S

// the two long loops are unrolled four times where the compiler knows the pragma (the device's and clang on the host), so that the loads of the next
// candidates and references are issued ahead of the comparison and the product they do not depend on
#if defined(__clang__)
#define GRK_STAB_UNROLL4 _Pragma("unroll 4")
#else
#define GRK_STAB_UNROLL4
#endif

struct StabRule { int derivative, dim, lag, theiler, horizon; };

// null, or what is wrong with a call's scalars: the refusals of DESIGN 4.18 beyond those of every call over sequences (host only)
inline const char* stab_rule_error(const StabRule& r) {
    if (r.derivative < 0 || r.derivative > 2) return "derivative outside [0, 2]";
    if (r.dim < 2 || r.dim > kStabMaxDim) return "dim outside [2, 8]";
    if (r.lag < 1 || r.lag > kStabMaxLag) return "lag outside [1, 16]";
    if (r.theiler < 0 || r.theiler > kStabMaxTheiler) return "theiler outside [0, 4096]";
    if (r.horizon < 1 || r.horizon > kStabMaxHorizon) return "horizon outside [1, 63]";
    return nullptr;
}
static_assert(kStabMaxDim == 8 && kStabMaxLag == 16 && kStabMaxTheiler == 4096 && kStabMaxHorizon == 63, "stab_rule_error's messages name the limits");

// v: positive and finite (of anything else the result is not used, and nothing here is undefined on it) -> f in [0.5, 1) and *e with v = f 2^e
GRK_TRANS_HD double stab_frexp(double v, int* e) {
    unsigned long long u;
    __builtin_memcpy(&u, &v, sizeof u);
    const unsigned long long mask = (1ULL << 52) - 1;
    unsigned long long m = u & mask;
    int ex = (int)((u >> 52) & 0x7ff);
    if (ex == 0) {                                              // subnormal: m 2^-1074, shifted until its leading one is the hidden bit
        const int s = __builtin_clzll(m | 1) - 11;
        m = (m << s) & mask;
        ex = 1 - s;
    }
    *e = ex - 1022;
    u = (1022ULL << 52) | m;
    double f;
    __builtin_memcpy(&f, &u, sizeof f);
    return f;
}

struct StabPoints { int span, M, E; };

GRK_TRANS_HD StabPoints stab_points(int T, const StabRule& r) {
    StabPoints p;
    p.span = (r.dim - 1) * r.lag;
    p.M = T - p.span > 0 ? T - p.span : 0;
    p.E = p.M - r.horizon > 0 ? p.M - r.horizon : 0;
    return p;
}

// a: the DIM values of one point; y: the first value of the other, whose next lie `lag` apart
template <int DIM>
GRK_TRANS_HD double stab_dist2(const double* a, const double* y, int lag) {
    const double t0 = a[0] - y[0];
    double s = t0 * t0;
    for (int k = 1; k < DIM; ++k) {
        const double t = a[k] - y[(size_t)k * lag];
        s = s + t * t;
    }
    return s;
}

// a: the values of reference i; y: y(j0) and what follows it, as far as y(j0 + n - 1 + span).  A candidate with a NaN fails D2 > 0 by itself
template <int DIM>
GRK_TRANS_HD void stab_scan(const double* a, const double* y, int j0, int n, int i, int theiler, int lag, double* best, int* best_j) {
    double b = *best;
    int bj = *best_j;
    GRK_STAB_UNROLL4
    for (int jj = 0; jj < n; ++jj) {
        const int j = j0 + jj;
        const double d2 = stab_dist2<DIM>(a, y + jj, lag);
        // & and |, not && and ||: no branch parts one candidate from the next, so the loads of four of them are issued together
        const bool take = ((j - i > theiler) | (i - j > theiler)) & (d2 > 0.) & ((bj < 0) | (d2 < b));
        b = take ? d2 : b;
        bj = take ? j : bj;
    }
    *best = b;
    *best_j = bj;
}

// y: the sequence's T values; nn: its T neighbours, nn_stride apart; 0 <= k <= horizon.  Every index is bounded without the data: i < E and 0 <= nn(i) < E, so
// i + k + span < T.  The loads and the distance of a reference do not depend on the product of the one before: the product is chosen, not branched on
template <int DIM>
GRK_TRANS_HD void stab_walk(const double* y, const int* nn, int nn_stride, int T, const StabRule& r, int k, long long* pair, double* mant) {
    const StabPoints p = stab_points(T, r);
    double P = 1.;
    long long S = 0, n = 0;
    GRK_STAB_UNROLL4
    for (int i = 0; i < p.E; ++i) {
        const int j = nn[(size_t)i * nn_stride];
        const bool has = (j >= 0) & (j < p.E);
        const int at = has ? j : 0;                             // a reference without a neighbour loads in bounds all the same, and does not count
        double a[DIM];
        for (int c = 0; c < DIM; ++c) a[c] = y[i + k + c * r.lag];
        const double d2 = stab_dist2<DIM>(a, y + at + k, r.lag);
        const bool ok = has & (d2 > 0.) & translation_detail::finite(d2);
        int e;
        const double f = stab_frexp(d2, &e);
        // (P, e') = frexp(P f): both factors lie in [0.5, 1] and f below 1, so the product lies in [0.25, 1): e' is -1 or 0, and doubling is exact
        const double prod = P * (ok ? f : 0.5);
        const bool low = prod < 0.5;
        P = ok ? (low ? prod * 2. : prod) : P;
        S += ok ? e - (low ? 1 : 0) : 0;
        n += ok;
    }
    pair[0] = n;
    pair[1] = S;
    *mant = P;
}

// the same with dim a variable
GRK_TRANS_HD void stab_walk_dim(const double* y, const int* nn, int nn_stride, int T, const StabRule& r, int k, long long* pair, double* mant) {
    switch (r.dim) {
        case 2: stab_walk<2>(y, nn, nn_stride, T, r, k, pair, mant); break;
        case 3: stab_walk<3>(y, nn, nn_stride, T, r, k, pair, mant); break;
        case 4: stab_walk<4>(y, nn, nn_stride, T, r, k, pair, mant); break;
        case 5: stab_walk<5>(y, nn, nn_stride, T, r, k, pair, mant); break;
        case 6: stab_walk<6>(y, nn, nn_stride, T, r, k, pair, mant); break;
        case 7: stab_walk<7>(y, nn, nn_stride, T, r, k, pair, mant); break;
        default: stab_walk<8>(y, nn, nn_stride, T, r, k, pair, mant); break;
    }
}

}  // namespace grk
