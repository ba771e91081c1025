// Sample entropy of four body signals at several scales in float64 and 64-bit integers (Richman and Moorman, Am. J. Physiol. 278, 2000;
// the coarse-graining of Costa, Goldberger and Peng, Phys. Rev. Lett. 89, 2002): no HIP and nothing of the library, so gait_entropy_kernels.hip uses
// it on the device and the stand-alone checker tests/helpers/gait_entropy_check.cpp on the host.  Whoever includes it compiles WITHOUT fma contraction
// (-ffp-contract=off): every operation below rounds once, in the order the parentheses show.  The four signals and their validity are
// gait_regularity.h's (reg_frame, reg_valid).
//
// An invalid value of the differenced signal y and of a coarse-grained signal z is STORED AS NaN, and so is one that is not finite: from y on, "valid"
// is "finite", and no mask is kept.
//
// ent_diff            -- y(t) of one frame: the signal differenced `derivative` times, or NaN.  On the device a lane owns a frame.
// ent_spread          -- n, mu, SD and r = fraction SD over the valid frames of y in time order (one thread, as reg_mean walks a sequence).
// ent_coarse          -- z_tau(j), the mean of tau consecutive frames of y added in time order, or NaN.  On the device a lane owns a j.
// ent_template_valid  -- whether z[i .. i + m] are all valid.
// ent_pair            -- ONE pair of templates: whether the first m values match within r (B) and whether the next one does too (A).
// ent_partners        -- every partner of template i, by circular offsets, so that each pair of a sequence is met once and every template has
//                        the same number of partners, or one more.  On the device a lane owns a template.
// ent_rule_error      -- what a call refuses about its scalars; ent_long_sequence -- the first sequence too long for a call (host only).
#pragma once

#include "gait_regularity.h"

namespace grk {

constexpr int kEntMaxM = 4;               // the longest template: a lane keeps m + 1 values in registers
constexpr int kEntMaxScales = 8;
constexpr int kEntMaxFrames = 32768;      // of one sequence: the work is quadratic and one workgroup owns a (sequence, channel, scale)
constexpr int kEntSeqCols = 4;            // n, mu, SD, r
constexpr int kEntCountCols = 3;          // valid templates, B, A

struct EntRule { int m; double fraction; int derivative, scales; };

// null, or what is wrong with a call's scalars: the refusals of DESIGN 4.17 beyond those of every call over sequences (host only)
inline const char* ent_rule_error(const EntRule& r) {
    if (r.m < 1 || r.m > kEntMaxM) return "m outside [1, 4]";
    if (!translation_detail::finite(r.fraction) || !(r.fraction > 0.) || !(r.fraction <= 10.)) return "fraction must be finite and within (0, 10]";
    if (r.derivative < 0 || r.derivative > 2) return "derivative outside [0, 2]";
    if (r.scales < 1 || r.scales > kEntMaxScales) return "scales outside [1, 8]";
    return nullptr;
}
static_assert(kEntMaxM == 4 && kEntMaxScales == 8, "ent_rule_error's messages name the limits");

// the first of n_seq sequences (n_seq + 1 offsets that hold the rules of every sequence call) with more than kEntMaxFrames frames, or -1 (host only)
inline int ent_long_sequence(const int* off, int n_seq) {
    for (int q = 0; q < n_seq; ++q)
        if ((long long)off[q + 1] - off[q] > kEntMaxFrames) return q;
    return -1;
}

// x: the channel's column of the sequence's rows, kRegChannels values apart; exclude: the sequence's per-frame entries or null.  y_0 = x,
// y_(k+1)(t) = y_k(t + 1) - y_k(t): valid where the frames t .. t + d all are
GRK_TRANS_HD double ent_diff(const double* x, const int* exclude, int t, int T, int d) {
    if (t + d >= T) return gait_detail::nan();
    double v[3];
    for (int k = 0; k <= d; ++k) {
        v[k] = x[(size_t)(t + k) * kRegChannels];
        if (!reg_valid(v[k], exclude, t + k)) return gait_detail::nan();
    }
    const double y = d == 0 ? v[0] : d == 1 ? v[1] - v[0] : (v[2] - v[1]) - (v[1] - v[0]);
    return translation_detail::finite(y) ? y : gait_detail::nan();
}

// y: T values, one apart -> out[0 .. 3] = n, mu = S / n, SD = sqrt(Q / (n - 1)) with Q the sum of (y - mu)^2, r = fraction SD; both sums in time
// order from +0.0.  As in reg_mean every frame is loaded whether it counts or not and the addition is chosen, so no load waits for a branch
GRK_TRANS_HD void ent_spread(const double* y, int T, double fraction, double* out) {
    using translation_detail::finite;
    double S = 0.;
    long long n = 0;
    for (int t = 0; t < T; ++t) {
        const double v = y[t], with = S + v;
        const bool ok = finite(v);
        S = ok ? with : S;
        n += ok;
    }
    const double mu = n ? S / (double)n : gait_detail::nan();
    double Q = 0.;
    for (int t = 0; t < T; ++t) {
        const double v = y[t], e = v - mu, with = Q + e * e;
        Q = finite(v) ? with : Q;
    }
    const double sd = n >= 2 ? __builtin_sqrt(Q / (double)(n - 1)) : gait_detail::nan();
    out[0] = (double)n;
    out[1] = mu;
    out[2] = sd;
    out[3] = fraction * sd;
}

// y: the sequence's differenced signal; 0 <= j < T / tau
GRK_TRANS_HD double ent_coarse(const double* y, int j, int tau) {
    const double* p = y + (size_t)j * tau;
    double s = p[0];
    for (int k = 1; k < tau; ++k) s = s + p[k];
    const double z = s / (double)tau;
    return translation_detail::finite(z) ? z : gait_detail::nan();
}

GRK_TRANS_HD bool ent_template_valid(const double* z, int i, int m) {
    bool ok = true;
    for (int k = 0; k <= m; ++k) ok = ok && translation_detail::finite(z[i + k]);
    return ok;
}

// a: the M + 1 values of a VALID template; w: those of its partner, of which any may be NaN -- a comparison with NaN is false, and the partner is a
// template only where its last value is one too
template <int M>
GRK_TRANS_HD void ent_pair(const double* a, const double* w, double r, long long* B, long long* A) {
    bool match = true;
    for (int k = 0; k < M; ++k) match = match && __builtin_fabs(a[k] - w[k]) <= r;
    const double last = __builtin_fabs(a[M] - w[M]);
    match = match && last == last;
    *B += match;
    *A += match && last <= r;
}

// z: N values, Nt = N - M templates; i: a VALID template.  Its partners are j = (i + s) mod Nt for s = 1 .. (Nt - 1) / 2 and, where Nt is even, for
// s = Nt / 2 of the templates i < Nt / 2: every pair once.  The partner's values slide: one load a pair (on the device j is consecutive across the
// lanes), M more where j wraps
template <int M>
GRK_TRANS_HD void ent_partners(const double* z, int Nt, int i, double r, long long* B, long long* A) {
    double a[M + 1], w[M + 1];
    for (int k = 0; k <= M; ++k) a[k] = z[i + k];
    const int steps = (Nt - 1) / 2 + (Nt % 2 == 0 && i < Nt / 2 ? 1 : 0);
    int j = i;
    bool reload = true;
    for (int s = 1; s <= steps; ++s) {
        if (++j == Nt) { j = 0; reload = true; }
        if (reload) {
            for (int k = 0; k < M; ++k) w[k] = z[j + k];
            reload = false;
        }
        w[M] = z[j + M];
        ent_pair<M>(a, w, r, B, A);
        for (int k = 0; k < M; ++k) w[k] = w[k + 1];
    }
}

// the same with m a variable
GRK_TRANS_HD void ent_partners_m(int m, const double* z, int Nt, int i, double r, long long* B, long long* A) {
    switch (m) {
        case 1: ent_partners<1>(z, Nt, i, r, B, A); break;
        case 2: ent_partners<2>(z, Nt, i, r, B, A); break;
        case 3: ent_partners<3>(z, Nt, i, r, B, A); break;
        default: ent_partners<4>(z, Nt, i, r, B, A); break;
    }
}

}  // namespace grk
