// Arm swing and inter-limb coordination in float64 (the magnitude-squared coherence by Welch's overlapped segments of Carter, Knapp and
// Nuttall, IEEE Trans. Audio Electroacoust. 21, 1973, as PAPERS.md cites it): no HIP and nothing of the library, so gait_coordination_kernels.hip uses
// it on the device and the stand-alone checker tests/helpers/gait_coordination_check.cpp on the host.  Whoever includes it compiles WITHOUT fma
// contraction (-ffp-contract=off): every operation below rounds once, in the order the parentheses show.  No libm and no device library: the segments,
// the window, the twiddles and the density are gait_spectrum.h's, the arctangent is gait_atan2 (gait_angles.h).  Every test is a comparison, so it is
// false for NaN.
//
// coord_frame      -- rule 1: the shoulder flexion left / right and the hip flexion left / right of ONE frame in degrees, kin_frame's operations for
//                     its channels 8, 9, 0 and 1 and nothing else of the frame, so that the bits are kin_frame's.
// coord_valid      -- rule 2: the four differenced values of a frame (ent_diff per channel) and whether all four are finite: ONE mask for the call.
// coord_bin        -- rule 4 of ONE bin k: the sixteen sums over the segments, in their order from +0.0: four auto sums C_c C_c + S_c S_c and, per
//                     pair (a, b) of kCoordPairs, Re += C_a C_b + S_a S_b and Im += S_a C_b - C_a S_b, the sign of conj(X_a) X_b.  On the device a
//                     lane owns a bin for all four channels: y, the means and the window are one address for the wave, the twiddles ONE gather at
//                     (k i) mod N for the four channels.  The operations on one channel are spec_bin's, so an auto sum has spec_bin's bits.
// coord_pair_row   -- rule 7's ten columns of one pair from the finished rows P_aa, P_bb, Re and Im, serially in rising k.
// coord_rule_error -- what a call refuses about its scalars (host only; null: nothing): spec_rule_error's sentences, and one segment is refused.
#pragma once

#include "gait_spectrum.h"
#include "gait_angles.h"

namespace grk {

constexpr int kCoordChannels = 4;         // arm_left, arm_right, leg_left, leg_right: kin_frame's channels 8, 9, 0, 1
constexpr int kCoordPairs = 6;
constexpr int kCoordSums = kCoordChannels + 2 * kCoordPairs;      // of one bin: four auto sums, then (Re, Im) of every pair
constexpr int kCoordPairCols = 10;        // used, peak_bin, peak_hz, cross_amplitude, coherence_peak, phase_peak, phase_deviation, lag_seconds, coherence_band,
                                          // coherence_bins
constexpr int kCoordMinMinSegments = 2;   // with one segment the coherence is 1 whatever the signals are
constexpr int kCoordColUsed = 0, kCoordColPeakBin = 1, kCoordColPeakHz = 2, kCoordColAmplitude = 3, kCoordColCoherence = 4, kCoordColPhase = 5,
              kCoordColDeviation = 6, kCoordColLag = 7, kCoordColBand = 8, kCoordColBins = 9;
static_assert(kCoordChannels == kRegChannels, "ent_diff reads a column of rows that are kRegChannels wide");

// the pairs in COORDINATION_PAIRS order: the arms, the legs, each arm with the other side's leg, each arm with its own side's leg
GRK_TRANS_HD int coord_pair_a(int p) { return p == 1 ? 2 : p == 3 ? 1 : p == 5 ? 1 : 0; }
GRK_TRANS_HD int coord_pair_b(int p) { return p == 0 ? 1 : p == 3 ? 2 : p == 4 ? 2 : 3; }
// whether the pair is expected in antiphase (180 degrees): all but an arm with the other side's leg
GRK_TRANS_HD bool coord_antiphase(int p) { return p != 2 && p != 3; }

// null, or what is wrong with a call's scalars: spec_rule_error's refusals in its order, min_segments' own last (host only)
inline const char* coord_rule_error(const SpecRule& r) {
    SpecRule q = r;
    q.min_segments = kCoordMinMinSegments;
    if (const char* why = spec_rule_error(q)) return why;
    if (r.min_segments < kCoordMinMinSegments || r.min_segments > kSpecMaxMinSegments) return "min_segments outside [2, 2^20]";
    return nullptr;
}
static_assert(kCoordMinMinSegments == 2 && kSpecMaxMinSegments == 1048576, "coord_rule_error's message names the limits");

// rows: the frame's (J,3) float32 joints; tab: the 16 indices kin_frame takes; out: arm_left, arm_right, leg_left, leg_right
GRK_TRANS_HD void coord_frame(const float* rows, const int* tab, double* out) {
    using translation_detail::finite;
    using gait_detail::dot3;
    double pelvis[3], spine[3], hip[2][3], knee[2][3], shoulder[2][3], elbow[2][3];
    for (int a = 0; a < 3; ++a) {
        pelvis[a] = (double)rows[3 * tab[0] + a];
        spine[a] = (double)rows[3 * tab[1] + a];
        for (int side = 0; side < 2; ++side) {
            hip[side][a] = (double)rows[3 * tab[2 + side] + a];
            knee[side][a] = (double)rows[3 * tab[4 + side] + a];
            shoulder[side][a] = (double)rows[3 * tab[10 + side] + a];
            elbow[side][a] = (double)rows[3 * tab[12 + side] + a];
        }
    }
    double l[3], u[3], c[3], f[3], n[3], w[3];
    for (int a = 0; a < 3; ++a) { l[a] = hip[0][a] - hip[1][a]; u[a] = spine[a] - pelvis[a]; }
    kin_detail::cross3(l, u, c);
    const double nc = __builtin_sqrt(dot3(c, c)), nl = __builtin_sqrt(dot3(l, l));
    const bool valid = nc > 0. && finite(nc) && nl > 0. && finite(nl);
    for (int a = 0; a < 3; ++a) { f[a] = c[a] / (valid ? nc : 1.); n[a] = l[a] / (valid ? nl : 1.); }
    kin_detail::cross3(f, n, w);
    const double none = gait_detail::nan();
    for (int side = 0; side < 2; ++side) {
        double d[3], a[3];
        for (int i = 0; i < 3; ++i) {
            d[i] = knee[side][i] - hip[side][i];               // hip -> knee
            a[i] = elbow[side][i] - shoulder[side][i];         // shoulder -> elbow
        }
        out[0 + side] = valid ? gait_atan2(dot3(a, f), -dot3(a, w)) * kKinDegrees : none;
        out[2 + side] = valid ? gait_atan2(dot3(d, f), -dot3(d, w)) * kKinDegrees : none;
    }
}

// x: the sequence's rows (T,4); y: the four differenced values of frame t; whether the frame counts
GRK_TRANS_HD bool coord_valid(const double* x, const int* exclude, int t, int T, int d, double* y) {
    bool all = true;
    for (int c = 0; c < kCoordChannels; ++c) {
        y[c] = ent_diff(x + c, exclude, t, T, d);
        all = all && translation_detail::finite(y[c]);
    }
    return all;
}

// y: the sequence's four differenced columns, channel c at y + c * stride; start: of the `used` segments; mu: their means, four a segment; w: L window
// values; sn, cs: har_twiddle(j, N) for j = 0 .. N - 1 -> acc: the kCoordSums sums of bin k
GRK_TRANS_HD void coord_bin(const double* y, size_t stride, const int* start, const double* mu, int used, const double* w, int L, const double* sn, const double* cs,
                            int N, int k, double* acc) {
    for (int e = 0; e < kCoordSums; ++e) acc[e] = 0.;
    for (int s = 0; s < used; ++s) {
        const double* ys = y + start[s];
        const double* m = mu + (size_t)s * kCoordChannels;
        double C[kCoordChannels] = {0., 0., 0., 0.}, S[kCoordChannels] = {0., 0., 0., 0.};
        for (int i = 0, j = 0; i < L; ++i) {
            const double wi = w[i], cj = cs[j], sj = sn[j];
            for (int c = 0; c < kCoordChannels; ++c) {
                const double v = (ys[c * stride + i] - m[c]) * wi;
                C[c] = C[c] + v * cj;
                S[c] = S[c] + v * sj;
            }
            j += k;
            if (j >= N) j -= N;                                // k <= N / 2: one subtraction is enough
        }
        for (int c = 0; c < kCoordChannels; ++c) acc[c] = acc[c] + (C[c] * C[c] + S[c] * S[c]);
        for (int p = 0; p < kCoordPairs; ++p) {
            const int a = coord_pair_a(p), b = coord_pair_b(p);
            acc[kCoordChannels + 2 * p] = acc[kCoordChannels + 2 * p] + (C[a] * C[b] + S[a] * S[b]);
            acc[kCoordChannels + 2 * p + 1] = acc[kCoordChannels + 2 * p + 1] + (S[a] * C[b] - C[a] * S[b]);
        }
    }
}

// Paa, Pbb, Re, Im: the N / 2 + 1 densities of the pair's two limbs and of its cross spectrum -> the row
GRK_TRANS_HD void coord_pair_row(const double* Paa, const double* Pbb, const double* Re, const double* Im, const SpecRule& r, bool antiphase, int used, double* out) {
    using translation_detail::finite;
    const double none = gait_detail::nan();
    for (int c = 0; c < kCoordPairCols; ++c) out[c] = none;
    out[kCoordColUsed] = (double)used;
    if (used < 1) return;
    int k_lo, k_hi;
    spec_band(r, &k_lo, &k_hi);
    int best = -1, bins = 0;
    double top = 0., sum = 0.;
    for (int k = k_lo; k <= k_hi; ++k) {
        const double m2 = Re[k] * Re[k] + Im[k] * Im[k], den = Paa[k] * Pbb[k];
        if (m2 > 0. && finite(m2) && (best < 0 || m2 > top)) { best = k; top = m2; }
        if (den > 0. && finite(den)) { sum = sum + m2 / den; ++bins; }
    }
    if (best < 0) return;
    const double hz = spec_freq((double)best, r), den = Paa[best] * Pbb[best];
    const double phase = gait_atan2(Im[best], Re[best]) * kKinDegrees, mag = __builtin_fabs(phase);
    out[kCoordColPeakBin] = (double)best;
    out[kCoordColPeakHz] = hz;
    out[kCoordColAmplitude] = __builtin_sqrt(top);
    if (den > 0. && finite(den)) out[kCoordColCoherence] = top / den;      // not clamped: a few ulps above 1 are reported as they are
    out[kCoordColPhase] = phase;
    out[kCoordColDeviation] = antiphase ? __builtin_fabs(180. - mag) : mag;
    out[kCoordColLag] = phase / (360. * hz);
    if (bins > 0) out[kCoordColBand] = sum / (double)bins;
    out[kCoordColBins] = (double)bins;
}

}  // namespace grk
