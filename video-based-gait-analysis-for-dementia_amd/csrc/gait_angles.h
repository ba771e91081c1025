// Joint-angle kinematics per gait cycle in float64: no HIP and nothing of the library, so gait_kinematics_kernels.hip uses it on the
// device and the stand-alone checker tests/helpers/gait_angles_check.cpp on the host.  Whoever includes it compiles WITHOUT fma contraction
// (-ffp-contract=off): every operation below rounds once, in the order the parentheses show.  The frame's axes are gait_events.h's, the Gaussian and
// the searches by word in a 64-frames-a-word bitmask track_boxes.h's.
//
// gait_atan2      -- atan2 out of + - * / and sqrt alone, so that numpy, the host checker and the kernel give the same bits (no two libm do):
//                    t = min(|y|, |x|) / max(|y|, |x|) in [0, 1]; twice t <- t / (1 + sqrt(1 + t t)) (the tangent of half the angle), which leaves
//                    t <= tan(pi / 16) = 0.199; the 12 terms of atan's Taylor series t (1 - z / 3 + z^2 / 5 - ... - z^11 / 23), z = t t, by Horner
//                    (the first term left out is below 2^-61 of the result); times 4; then pi / 2 - a where |y| > |x|, pi - a where x < 0, -a where
//                    y < 0.  NaN where both arguments are zero or either is not finite.  A zero result is +0.
// kin_frame       -- the 13 channels of one frame in degrees.  tab = the indices of pelvis, spine-shoulder, left / right hip, knee, ankle, foot,
//                    shoulder, elbow, wrist.  l, u, f, n as gait_frame makes them, w = f x n (the body's up); a frame where |l x u| or |l| is not a
//                    positive finite number is invalid: the channels that use the axes -- hip, shoulder, trunk -- are NaN, the others are not.
// kin_cycle_point -- point p = 0 .. 100 of the cycle curve of the stride [t0, t0 + L]: q = (p L) div 100, r = (p L) mod 100, x[t0 + q] where r = 0,
//                    else x[t0 + q] + (x[t0 + q + 1] - x[t0 + q]) * (r / 100.0).
// kin_strides     -- the walk through ONE foot's heel-strike bitmask by word: every pair of consecutive strikes t0 < t1 with
//                    min_stride <= t1 - t0 <= max_stride is handed to `extent`, which says whether the channel is finite on all of [t0, t1] and gives
//                    its maximum and minimum there (+0.0 is added to both, so that a zero has one sign whatever the order of the comparisons), and the
//                    strides it accepts to `each`, in time order.  On the device `extent` is a reduction of the whole workgroup, on the host a loop.
// kin_channel     -- the row [0 .. 4] of a channel and point p of its curve: every sum begins at +0.0 and adds in time order, every mean is S / n,
//                    every standard deviation two-pass with ddof = 0.  kin_rom is the first pass of the range of motion alone (for the partner
//                    channel of the symmetry index), the same operations in the same order as kin_channel's.
#pragma once

#include "gait_events.h"

namespace grk {

constexpr int kKinTable = 16;             // joints the call names
constexpr int kKinChannels = 13;
constexpr int kKinPoints = 101;           // 0 .. 100 % of the cycle
constexpr int kKinSeqCols = 6;            // strides used, mean max, mean min, ROM mean, ROM SD, symmetry index
constexpr double kKinDegrees = 57.29577951308232, kKinPi = 3.141592653589793, kKinHalfPi = 1.5707963267948966;

GRK_TRANS_HD double gait_atan2(double y, double x) {
    using translation_detail::finite;
    if (!finite(y) || !finite(x) || (y == 0. && x == 0.)) return gait_detail::nan();
    const double ay = __builtin_fabs(y), ax = __builtin_fabs(x);
    const bool steep = ay > ax;
    double t = (steep ? ax : ay) / (steep ? ay : ax);
    t = t / (1. + __builtin_sqrt(1. + t * t));
    t = t / (1. + __builtin_sqrt(1. + t * t));
    const double z = t * t;
    double p = -1. / 23.;
    p = p * z + 1. / 21.;
    p = p * z - 1. / 19.;
    p = p * z + 1. / 17.;
    p = p * z - 1. / 15.;
    p = p * z + 1. / 13.;
    p = p * z - 1. / 11.;
    p = p * z + 1. / 9.;
    p = p * z - 1. / 7.;
    p = p * z + 1. / 5.;
    p = p * z - 1. / 3.;
    p = p * z + 1.;
    double a = 4. * (t * p);
    if (steep) a = kKinHalfPi - a;
    if (x < 0.) a = kKinPi - a;
    if (y < 0.) a = -a;
    return a + 0.;
}

namespace kin_detail {
GRK_TRANS_HD void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
// the angle between two vectors in degrees, 0 .. 180: atan2(|a x b|, a . b)
GRK_TRANS_HD double bend(const double* a, const double* b) {
    double c[3];
    cross3(a, b, c);
    return gait_atan2(__builtin_sqrt(gait_detail::dot3(c, c)), gait_detail::dot3(a, b)) * kKinDegrees;
}
}  // namespace kin_detail

// rows: the frame's (J,3) float32 joints; out: the 13 channels
GRK_TRANS_HD void kin_frame(const float* rows, const int* tab, double* out) {
    using translation_detail::finite;
    using gait_detail::dot3;
    double p[kKinTable][3];
    for (int k = 0; k < kKinTable; ++k)
        for (int a = 0; a < 3; ++a) p[k][a] = (double)rows[3 * tab[k] + a];
    double l[3], u[3], c[3], f[3], n[3], w[3];
    for (int a = 0; a < 3; ++a) { l[a] = p[2][a] - p[3][a]; u[a] = p[1][a] - p[0][a]; }
    kin_detail::cross3(l, u, c);
    const double nc = __builtin_sqrt(dot3(c, c)), nl = __builtin_sqrt(dot3(l, l));
    const bool valid = nc > 0. && finite(nc) && nl > 0. && finite(nl);
    for (int a = 0; a < 3; ++a) { f[a] = c[a] / (valid ? nc : 1.); n[a] = l[a] / (valid ? nl : 1.); }      // of an invalid frame they are not used
    kin_detail::cross3(f, n, w);
    const double none = gait_detail::nan();
    for (int side = 0; side < 2; ++side) {
        double d[3], s[3], g[3], a[3], b[3];
        for (int i = 0; i < 3; ++i) {
            d[i] = p[4 + side][i] - p[2 + side][i];            // hip -> knee
            s[i] = p[6 + side][i] - p[4 + side][i];            // knee -> ankle
            g[i] = p[8 + side][i] - p[6 + side][i];            // ankle -> foot
            a[i] = p[12 + side][i] - p[10 + side][i];          // shoulder -> elbow
            b[i] = p[14 + side][i] - p[12 + side][i];          // elbow -> wrist
        }
        const double down = -dot3(d, w), out_d = dot3(d, n);
        out[0 + side] = valid ? gait_atan2(dot3(d, f), down) * kKinDegrees : none;
        out[2 + side] = valid ? gait_atan2(side ? -out_d : out_d, down) * kKinDegrees : none;
        out[4 + side] = kin_detail::bend(d, s);
        out[6 + side] = kin_detail::bend(s, g) - 90.;
        out[8 + side] = valid ? gait_atan2(dot3(a, f), -dot3(a, w)) * kKinDegrees : none;
        out[10 + side] = kin_detail::bend(a, b);
    }
    const double e[3] = {0., -1., 0.};
    out[12] = valid ? kin_detail::bend(u, e) : none;
}

// the foot whose strides cut channel c, and the other channel of its left / right pair (-1: none)
GRK_TRANS_HD int kin_foot(int c) { return c == 12 ? 0 : c & 1; }
GRK_TRANS_HD int kin_partner(int c) { return c == 12 ? -1 : c ^ 1; }

GRK_TRANS_HD double kin_cycle_point(const double* x, long long stride, int t0, int L, int p) {
    const int q = (p * L) / 100, r = (p * L) % 100;
    const double v = x[(long long)(t0 + q) * stride];
    if (r == 0) return v;
    return v + (x[(long long)(t0 + q + 1) * stride] - v) * ((double)r / 100.0);
}

// the loop an `extent` of the host is: finite on all of [t0, t0 + L], its maximum and minimum
GRK_TRANS_HD bool kin_extent_serial(const double* x, long long stride, int t0, int L, double* mx, double* mn) {
    bool fin = true;
    double a = -__builtin_inf(), b = __builtin_inf();
    for (int i = 0; i <= L; ++i) {
        const double v = x[(long long)(t0 + i) * stride];
        fin = fin && translation_detail::finite(v);
        a = v > a ? v : a;
        b = v < b ? v : b;
    }
    *mx = a; *mn = b;
    return fin;
}

template <class Extent, class Each>
GRK_TRANS_HD void kin_strides(const unsigned long long* words, int T, int min_stride, int max_stride, Extent extent, Each each) {
    long long prev = -1;
    for (long long t = track_first(words, 0, T); t >= 0; t = track_first(words, t + 1, T)) {
        const long long L = t - prev;
        if (prev >= 0 && L >= min_stride && L <= max_stride) {
            double mx, mn;
            if (extent((int)prev, (int)L, &mx, &mn)) each((int)prev, (int)L, mx + 0., mn + 0.);
        }
        prev = t;
    }
}

// strides used and the mean of their range of motion (NaN of none)
template <class Extent>
GRK_TRANS_HD void kin_rom(const unsigned long long* words, int T, int min_stride, int max_stride, Extent extent, double* count, double* mean) {
    long long n = 0;
    double s = 0.;
    kin_strides(words, T, min_stride, max_stride, extent, [&](int, int, double mx, double mn) { s = s + (mx - mn); ++n; });
    *count = (double)n;
    *mean = n ? s / (double)n : gait_detail::nan();
}

// x: the channel's column of ONE sequence (frame i at x[i * stride]); row[0 .. 4]; point[0, 1] = mean and SD of cycle point p (p < 0: not made)
template <class Extent>
GRK_TRANS_HD void kin_channel(const unsigned long long* words, const double* x, long long stride, int T, int min_stride, int max_stride, Extent extent, int p,
                              double* row, double* point) {
    long long n = 0;
    double s_max = 0., s_min = 0., s_rom = 0., s_pt = 0.;
    kin_strides(words, T, min_stride, max_stride, extent, [&](int t0, int L, double mx, double mn) {
        s_max = s_max + mx;
        s_min = s_min + mn;
        s_rom = s_rom + (mx - mn);
        if (p >= 0) s_pt = s_pt + kin_cycle_point(x, stride, t0, L, p);
        ++n;
    });
    const double none = gait_detail::nan(), m_rom = n ? s_rom / (double)n : none, m_pt = n ? s_pt / (double)n : none;
    double q_rom = 0., q_pt = 0.;
    if (n)
        kin_strides(words, T, min_stride, max_stride, extent, [&](int t0, int L, double mx, double mn) {
            const double d = (mx - mn) - m_rom;
            q_rom = q_rom + d * d;
            if (p >= 0) { const double e = kin_cycle_point(x, stride, t0, L, p) - m_pt; q_pt = q_pt + e * e; }
        });
    row[0] = (double)n;
    row[1] = n ? s_max / (double)n : none;
    row[2] = n ? s_min / (double)n : none;
    row[3] = m_rom;
    row[4] = n ? __builtin_sqrt(q_rom / (double)n) : none;
    if (p >= 0) { point[0] = m_pt; point[1] = n ? __builtin_sqrt(q_pt / (double)n) : none; }
}

// 100 |ROM_L - ROM_R| / (0.5 (ROM_L + ROM_R)); NaN where a side has no stride or the denominator is not positive
GRK_TRANS_HD double kin_symmetry(double n_l, double rom_l, double n_r, double rom_r) {
    const double den = 0.5 * (rom_l + rom_r);
    if (!(n_l > 0.) || !(n_r > 0.) || !(den > 0.)) return gait_detail::nan();
    return (100. * __builtin_fabs(rom_l - rom_r)) / den;
}

}  // namespace grk
