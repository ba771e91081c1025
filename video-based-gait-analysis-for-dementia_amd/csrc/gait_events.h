// Gait events and parameters from 3D joints in float64 (the coordinate-based events of Zeni, Richards and Higginson, Gait & Posture 27,
// 2008): no HIP and nothing of the library, so gait_kernels.hip uses it on the device and the stand-alone checker tests/helpers/gait_events_check.cpp
// on the host.  Whoever includes it compiles WITHOUT fma contraction (-ffp-contract=off): every operation below rounds once, in the order the
// parentheses show.  The 1-D Gaussian and the searches by word in a 64-frames-a-word bitmask are those of track_boxes.h.
//
// gait_frame       -- the frame's axes and signals.  tab = the indices of pelvis, spine-shoulder, left hip, right hip, left ankle, right ankle, left
//                     foot, right foot.  l = lhip - rhip, u = spine_shoulder - pelvis, f = (l x u) / |l x u|, n = l / |l|; hL, hR = (ankle - pelvis) . f,
//                     tL, tR = (foot - pelvis) . f, wd = |(lankle - rankle) . n|; a dot product is ((x + y) + z), a norm sqrt((x^2 + y^2) + z^2).  A frame
//                     where |l x u| or |l| is not a positive finite number is invalid: all five are NaN.
// gait_heel_strike -- frame t of a signal h[0, T) (any stride): all of [t - w, t + w] inside, h(t) > 0, h(t) > h(t - i) and h(t) >= h(t + i) for
//                     i = 1 .. w (of a plateau the earliest frame), and h(t) - min over the window >= min_excursion.  Every test is a comparison that
//                     is false for NaN.  gait_toe_off is its mirror image: t(t) < 0, < before, <= after, max over the window - t(t) >= min_excursion.
// gait_next_strike -- the heel strikes of both feet in time order, the left foot first where both strike in one frame.
// gait_counts / gait_steps / gait_strides / gait_stance / gait_traj_speed -- the columns of the per-sequence row (below), each a walk through the
//                     event bitmasks of ONE sequence (bit i & 63 of word i >> 6 for its frame i) by word, every sum in time order, every mean S / n,
//                     every standard deviation two-pass with ddof = 0: sqrt(sum((x - mean)^2) / n).
#pragma once

#include "track_boxes.h"

namespace grk {

constexpr int kGaitHeelL = 1, kGaitHeelR = 2, kGaitToeL = 4, kGaitToeR = 8;       // the bits of an events entry
constexpr int kGaitTable = 8;             // joints the call names
constexpr int kGaitFrameCols = 7;         // hL, hR, tL, tR, wd, step_length, step_width
constexpr int kGaitSeqCols = 18;
// the per-sequence row
constexpr int kGaitColCounts = 0, kGaitColSteps = 4, kGaitColStepTime = 5, kGaitColStepTimeSd = 6, kGaitColCadence = 7, kGaitColStride = 8, kGaitColStrideSd = 9,
              kGaitColStrideCv = 10, kGaitColStepLen = 11, kGaitColStepLenSd = 12, kGaitColStepWidth = 13, kGaitColStepWidthSd = 14, kGaitColStance = 15,
              kGaitColSpeed = 16, kGaitColTrajSpeed = 17;

namespace gait_detail {
GRK_TRANS_HD double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
GRK_TRANS_HD double nan() { return __builtin_nan(""); }
GRK_TRANS_HD bool bit(const unsigned long long* words, long long i) { return (words[i >> 6] >> (i & 63)) & 1; }
}  // namespace gait_detail

// rows: the frame's (J,3) float32 joints; sig = [hL, hR, tL, tR, wd]
GRK_TRANS_HD void gait_frame(const float* rows, const int* tab, double* sig) {
    using translation_detail::finite;
    double p[kGaitTable][3];
    for (int k = 0; k < kGaitTable; ++k)
        for (int a = 0; a < 3; ++a) p[k][a] = (double)rows[3 * tab[k] + a];
    double l[3], u[3], c[3];
    for (int a = 0; a < 3; ++a) { l[a] = p[2][a] - p[3][a]; u[a] = p[1][a] - p[0][a]; }
    c[0] = l[1] * u[2] - l[2] * u[1];
    c[1] = l[2] * u[0] - l[0] * u[2];
    c[2] = l[0] * u[1] - l[1] * u[0];
    const double nc = __builtin_sqrt(gait_detail::dot3(c, c)), nl = __builtin_sqrt(gait_detail::dot3(l, l));
    if (!(nc > 0.) || !finite(nc) || !(nl > 0.) || !finite(nl)) {
        for (int k = 0; k < 5; ++k) sig[k] = gait_detail::nan();
        return;
    }
    double f[3], n[3], d[3];
    for (int a = 0; a < 3; ++a) { f[a] = c[a] / nc; n[a] = l[a] / nl; }
    for (int k = 0; k < 4; ++k) {                               // left ankle, right ankle, left foot, right foot
        for (int a = 0; a < 3; ++a) d[a] = p[4 + k][a] - p[0][a];
        sig[k] = gait_detail::dot3(d, f);
    }
    for (int a = 0; a < 3; ++a) d[a] = p[4][a] - p[5][a];
    sig[4] = __builtin_fabs(gait_detail::dot3(d, n));
}

GRK_TRANS_HD bool gait_heel_strike(const double* h, long long stride, int T, int t, int w, double min_excursion) {
    if (t < w || t + w >= T) return false;
    const double v = h[t * stride];
    bool ok = v > 0.;
    double m = v;
    for (int i = 1; i <= w; ++i) {
        const double a = h[(t - i) * stride], b = h[(t + i) * stride];
        ok = ok && v > a && v >= b;
        m = a < m ? a : m;
        m = b < m ? b : m;
    }
    return ok && v - m >= min_excursion;
}

GRK_TRANS_HD bool gait_toe_off(const double* s, long long stride, int T, int t, int w, double min_excursion) {
    if (t < w || t + w >= T) return false;
    const double v = s[t * stride];
    bool ok = v < 0.;
    double m = v;
    for (int i = 1; i <= w; ++i) {
        const double a = s[(t - i) * stride], b = s[(t + i) * stride];
        ok = ok && v < a && v <= b;
        m = a > m ? a : m;
        m = b > m ? b : m;
    }
    return ok && m - v >= min_excursion;
}

// frame t of a sequence whose smoothed signals lie in row[0 .. 3] of its per-frame rows: the events entry; row[5], row[6] of frame t are written
GRK_TRANS_HD int gait_frame_events(double* rows, int T, int t, int w, double min_excursion) {
    int ev = 0;
    for (int k = 0; k < 2; ++k) {
        if (gait_heel_strike(rows + k, kGaitFrameCols, T, t, w, min_excursion)) ev |= kGaitHeelL << k;
        if (gait_toe_off(rows + 2 + k, kGaitFrameCols, T, t, w, min_excursion)) ev |= kGaitToeL << k;
    }
    double* row = rows + (long long)t * kGaitFrameCols;
    const int foot = (ev & kGaitHeelL) ? 0 : 1;
    const bool strike = (ev & (kGaitHeelL | kGaitHeelR)) != 0;
    row[5] = strike ? row[foot] - row[1 - foot] : gait_detail::nan();
    row[6] = strike ? row[4] : gait_detail::nan();
    return ev;
}

// (t, foot) -> the next heel strike in time order; begin with t = -1, foot = 1
GRK_TRANS_HD bool gait_next_strike(const unsigned long long* hs_l, const unsigned long long* hs_r, int T, int* t, int* foot) {
    if (*t >= 0 && *foot == 0 && gait_detail::bit(hs_r, *t)) { *foot = 1; return true; }
    const long long a = track_first(hs_l, (long long)*t + 1, T), b = track_first(hs_r, (long long)*t + 1, T);
    if (a < 0 && b < 0) return false;
    if (a >= 0 && (b < 0 || a <= b)) { *t = (int)a; *foot = 0; } else { *t = (int)b; *foot = 1; }
    return true;
}

// column k = 0 .. 3 of the row: the events of one kind
GRK_TRANS_HD double gait_count(const unsigned long long* words, int T) {
    long long n = 0;
    for (int w = 0; w <= (T - 1) >> 6; ++w) n += __builtin_popcountll(words[w]);
    return (double)n;
}

// columns 4 .. 7, 11 .. 14 and 16
GRK_TRANS_HD void gait_steps(const unsigned long long* hs_l, const unsigned long long* hs_r, int T, const double* rows, double fps, double* out) {
    double mean[3] = {0., 0., 0.}, acc[3] = {0., 0., 0.};
    long long n = 0;
    for (int pass = 0; pass < 2; ++pass) {
        int t = -1, foot = 1, pt = -1, pf = -1;
        acc[0] = acc[1] = acc[2] = 0.;
        while (gait_next_strike(hs_l, hs_r, T, &t, &foot)) {
            if (pt >= 0 && pf != foot) {
                const double* row = rows + (long long)t * kGaitFrameCols;
                const double x[3] = {(double)(t - pt) / fps, row[foot] - row[1 - foot], row[4]};
                for (int k = 0; k < 3; ++k) {
                    if (pass == 0) { acc[k] = acc[k] + x[k]; }
                    else { const double d = x[k] - mean[k]; acc[k] = acc[k] + d * d; }
                }
                n += pass == 0;
            }
            pt = t; pf = foot;
        }
        if (n == 0) break;
        if (pass == 0) for (int k = 0; k < 3; ++k) mean[k] = acc[k] / (double)n;
    }
    out[kGaitColSteps] = (double)n;
    const double none = gait_detail::nan();
    out[kGaitColStepTime] = n ? mean[0] : none;
    out[kGaitColStepTimeSd] = n ? __builtin_sqrt(acc[0] / (double)n) : none;
    out[kGaitColCadence] = n ? 60. / mean[0] : none;
    out[kGaitColStepLen] = n ? mean[1] : none;
    out[kGaitColStepLenSd] = n ? __builtin_sqrt(acc[1] / (double)n) : none;
    out[kGaitColStepWidth] = n ? mean[2] : none;
    out[kGaitColStepWidthSd] = n ? __builtin_sqrt(acc[2] / (double)n) : none;
    out[kGaitColSpeed] = n ? (mean[1] * out[kGaitColCadence]) / 60. : none;
}

// columns 8 .. 10: the left foot's strides, then the right foot's
GRK_TRANS_HD void gait_strides(const unsigned long long* hs_l, const unsigned long long* hs_r, int T, double fps, double* out) {
    double mean = 0., acc = 0.;
    long long n = 0;
    for (int pass = 0; pass < 2; ++pass) {
        acc = 0.;
        for (int foot = 0; foot < 2; ++foot) {
            const unsigned long long* words = foot ? hs_r : hs_l;
            long long prev = -1;
            for (long long t = track_first(words, 0, T); t >= 0; t = track_first(words, t + 1, T)) {
                if (prev >= 0) {
                    const double x = (double)(t - prev) / fps;
                    if (pass == 0) { acc = acc + x; ++n; }
                    else { const double d = x - mean; acc = acc + d * d; }
                }
                prev = t;
            }
        }
        if (n == 0) break;
        if (pass == 0) mean = acc / (double)n;
    }
    const double none = gait_detail::nan(), sd = n ? __builtin_sqrt(acc / (double)n) : none;
    out[kGaitColStride] = n ? mean : none;
    out[kGaitColStrideSd] = sd;
    out[kGaitColStrideCv] = n ? (100. * sd) / mean : none;
}

// column 15: per stride of a foot whose first toe-off after the opening strike lies before the closing strike, 100 (t_TO - t_HS) / (t_HS' - t_HS)
GRK_TRANS_HD void gait_stance(const unsigned long long* hs_l, const unsigned long long* hs_r, const unsigned long long* to_l, const unsigned long long* to_r, int T,
                              double* out) {
    double acc = 0.;
    long long n = 0;
    for (int foot = 0; foot < 2; ++foot) {
        const unsigned long long *hs = foot ? hs_r : hs_l, *to = foot ? to_r : to_l;
        long long prev = -1;
        for (long long t = track_first(hs, 0, T); t >= 0; t = track_first(hs, t + 1, T)) {
            if (prev >= 0) {
                const long long off = track_first(to, prev + 1, t);
                if (off >= 0) { acc = acc + (100. * (double)(off - prev)) / (double)(t - prev); ++n; }
            }
            prev = t;
        }
    }
    out[kGaitColStance] = n ? acc / (double)n : gait_detail::nan();
}

// column 17: joints = the sequence's (T,J,3) float32 rows, trans its (T,3) float64 rows or null
GRK_TRANS_HD void gait_traj_speed(const unsigned long long* hs_l, const unsigned long long* hs_r, int T, const float* joints, int J, int pelvis, const double* trans,
                                  double fps, double* out) {
    using translation_detail::finite;
    out[kGaitColTrajSpeed] = gait_detail::nan();
    if (!trans) return;
    int t = -1, foot = 1, ta = -1, tb = -1;
    while (gait_next_strike(hs_l, hs_r, T, &t, &foot)) {
        const double* r = trans + 3 * (long long)t;
        if (!finite(r[0]) || !finite(r[1]) || !finite(r[2])) continue;
        if (ta < 0) ta = t;
        tb = t;
    }
    if (ta < 0 || ta == tb) return;
    double d[3];
    for (int a = 0; a < 3; ++a) {
        const double pb = (double)joints[((long long)tb * J + pelvis) * 3 + a] + trans[3 * (long long)tb + a];
        const double pa = (double)joints[((long long)ta * J + pelvis) * 3 + a] + trans[3 * (long long)ta + a];
        d[a] = pb - pa;
    }
    out[kGaitColTrajSpeed] = __builtin_sqrt(gait_detail::dot3(d, d)) / ((double)(tb - ta) / fps);
}

}  // namespace grk
