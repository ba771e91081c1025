// Gait regularity and symmetry from the autocorrelation of four body signals in float64 (the unbiased autocorrelation of Moe-Nilssen
// and Helbostad, J. Biomech. 37, 2004): no HIP and nothing of the library, so gait_regularity_kernels.hip uses it on the device and the stand-alone
// checker tests/helpers/gait_regularity_check.cpp on the host.  Whoever includes it compiles WITHOUT fma contraction (-ffp-contract=off): every
// operation below rounds once, in the order the parentheses show.  The searches by word in a 64-frames-a-word bitmask are track_boxes.h's and
// gait_turns.h's.
//
// reg_frame    -- the four signals of one frame: sep, lift, sway (NaN without valid axes, the validity of gait_frame) and bob (NaN without a finite
//                 translation row).
// reg_valid    -- whether a frame counts for a channel; reg_mean -- S / n over the valid frames in time order; reg_key -- a valid frame's run number
//                 (the invalid frames before it) from the validity mask and the words' running counts, -1 of an invalid frame.
// reg_lag      -- ONE lag m of one (sequence, channel): the sum of d(t) d(t + m) over the counting pairs in time order and their number.  On the
//                 device a lane owns a lag: d[t] and key[t] are one address for the whole wave, d[t + m] and key[t + m] consecutive across its lanes.
// reg_rho      -- A(m) / A(0), or NaN by rule 5.
// reg_is_max / reg_is_min / reg_first_peak -- rule 6's tests of one lag (a comparison with NaN is false, which is what "defined" asks).
// reg_row      -- the ten columns from rho and the three masks of the lags (first-peak candidates, local maxima, local minima).
// reg_rule_error -- what a call refuses about its scalars (host only; null: nothing).
#pragma once

#include "gait_turns.h"

namespace grk {

constexpr int kRegChannels = 4;           // sep, lift, sway (odd: a step is half a stride with the sign turned), bob (even: it repeats every step)
constexpr int kRegSeqCols = 10;           // n, A(0), d1, d1 refined, step regularity, d2, d2 refined, stride regularity, symmetry, cadence
constexpr int kRegMaxLag = 255;           // a lane of the sequence kernel's workgroup per lag 0 .. 255
constexpr int kRegMinLagLimit = 8;        // the least max_lag
constexpr int kRegLagWords = 4;           // words of a mask over the lags
constexpr int kRegMaxPairs = 1 << 20;
constexpr int kRegColN = 0, kRegColA0 = 1, kRegColStepLag = 2, kRegColStepLagFine = 3, kRegColStepReg = 4, kRegColStrideLag = 5, kRegColStrideLagFine = 6,
              kRegColStrideReg = 7, kRegColSymmetry = 8, kRegColCadence = 9;

struct RegRule { double fps; int max_lag, min_lag; double min_peak; int min_pairs; };

// null, or what is wrong with a call's scalars: the refusals of DESIGN 4.15 beyond those of every call over sequences (host only)
inline const char* reg_rule_error(const RegRule& r) {
    using translation_detail::finite;
    if (!finite(r.fps) || !(r.fps > 0.)) return "fps must be positive and finite";
    if (r.max_lag < kRegMinLagLimit || r.max_lag > kRegMaxLag) return "max_lag outside [8, 255]";
    if (r.min_lag < 2 || r.min_lag > r.max_lag - 2) return "min_lag outside [2, max_lag - 2]";
    if (!(r.min_peak > 0.) || !(r.min_peak <= 1.)) return "min_peak outside (0, 1]";
    if (r.min_pairs < 2 || r.min_pairs > kRegMaxPairs) return "min_pairs outside [2, 2^20]";
    return nullptr;
}
static_assert(kRegMinLagLimit == 8 && kRegMaxLag == 255 && kRegMaxPairs == 1048576, "reg_rule_error's messages name the limits");

GRK_TRANS_HD bool reg_odd(int channel) { return channel < 3; }

// rows: the frame's (J,3) float32 joints; tab: the gait call's table, whose foot entries are not read; trans: the frame's translation row or null
GRK_TRANS_HD void reg_frame(const float* rows, const int* tab, const double* trans, double* sig) {
    using translation_detail::finite;
    double p[6][3];
    for (int k = 0; k < 6; ++k)
        for (int a = 0; a < 3; ++a) p[k][a] = (double)rows[3 * tab[k] + a];
    sig[3] = trans && finite(trans[0]) && finite(trans[1]) && finite(trans[2]) ? -(p[0][1] + trans[1]) : gait_detail::nan();
    double l[3], u[3], c[3];
    for (int a = 0; a < 3; ++a) { l[a] = p[2][a] - p[3][a]; u[a] = p[1][a] - p[0][a]; }
    c[0] = l[1] * u[2] - l[2] * u[1];
    c[1] = l[2] * u[0] - l[0] * u[2];
    c[2] = l[0] * u[1] - l[1] * u[0];
    const double nc = __builtin_sqrt(gait_detail::dot3(c, c)), nl = __builtin_sqrt(gait_detail::dot3(l, l));
    if (!(nc > 0.) || !finite(nc) || !(nl > 0.) || !finite(nl)) {
        sig[0] = sig[1] = sig[2] = gait_detail::nan();
        return;
    }
    const double nu = __builtin_sqrt(gait_detail::dot3(u, u));      // positive wherever |l x u| is
    double f[3], n[3], up[3], d[3];
    for (int a = 0; a < 3; ++a) { f[a] = c[a] / nc; n[a] = l[a] / nl; up[a] = u[a] / nu; d[a] = p[4][a] - p[5][a]; }
    sig[0] = gait_detail::dot3(d, f);
    sig[1] = gait_detail::dot3(d, up);
    sig[2] = gait_detail::dot3(up, n);
}

// exclude: the sequence's per-frame entries or null
GRK_TRANS_HD bool reg_valid(double x, const int* exclude, long long t) { return translation_detail::finite(x) && (!exclude || exclude[t] == 0); }

// x: the sequence's signal, one value apart; valid: its mask -> mu = S / n (NaN of no valid frame); prefix[w]: the valid frames before word w
GRK_TRANS_HD double reg_mean(const double* x, const unsigned long long* valid, int T, long long* prefix, long long* n) {
    double S = 0.;
    long long count = 0;
    for (int w = 0; w <= (T - 1) >> 6; ++w) {
        prefix[w] = count;
        const unsigned long long v = valid[w];
        count += __builtin_popcountll(v);
        // every frame of the word is loaded, whether it counts or not (behind the sequence: its last frame again, whose bit there is clear), and the
        // addition is chosen, not branched to: the loads do not wait for one another, and the chain is one addition a frame
        for (int i = 0; i < 64; ++i) {
            const int t = w * 64 + i < T ? w * 64 + i : T - 1;
            const double with = S + x[t];
            S = ((v >> i) & 1) ? with : S;
        }
    }
    *n = count;
    return count ? S / (double)count : gait_detail::nan();
}

// run(t) = t - the valid frames before t, of a valid frame; -1 of an invalid one, which equals no run
GRK_TRANS_HD int reg_key(const unsigned long long* valid, const long long* prefix, int t) {
    const unsigned long long v = valid[t >> 6];
    if (!((v >> (t & 63)) & 1)) return -1;
    return t - (int)(prefix[t >> 6] + __builtin_popcountll(v & ~(~0ull << (t & 63))));
}

// d: the centred signal; key: reg_key of every frame -> the sum over the counting pairs (t, t + m) in time order, from +0.0; *N their number
GRK_TRANS_HD double reg_lag(const double* d, const int* key, int T, int m, long long* N) {
    double acc = 0.;
    long long count = 0;
    // as in reg_mean, both frames are loaded whether the pair counts or not (behind the sequence: its last frame) and the addition is chosen: a
    // value that is not chosen may be NaN
    for (int t = 0; t < T; ++t) {
        const int j = t + m < T ? t + m : T - 1;
        const int k = key[t];                                  // one address for the wave
        const bool counts = k >= 0 && t + m < T && key[j] == k;
        const double with = acc + d[t] * d[j];
        acc = counts ? with : acc;
        count += counts;
    }
    *N = count;
    return acc;
}

GRK_TRANS_HD double reg_rho(double sum_m, long long N_m, double sum_0, long long N_0, int min_pairs) {
    if (N_m < min_pairs || N_0 < min_pairs) return gait_detail::nan();
    const double A0 = sum_0 / (double)N_0;
    if (!(A0 > 0.)) return gait_detail::nan();
    return (sum_m / (double)N_m) / A0;
}

// rho: max_lag + 1 values.  A local maximum of rho (sign +1) or of -rho (sign -1) at lag m: both neighbours inside and all three defined
GRK_TRANS_HD bool reg_extremum(const double* rho, int max_lag, int m, double sign) {
    if (m < 1 || m >= max_lag) return false;
    const double a = sign * rho[m - 1], b = sign * rho[m], c = sign * rho[m + 1];
    return b > a && b >= c;
}
GRK_TRANS_HD bool reg_is_max(const double* rho, int max_lag, int m) { return reg_extremum(rho, max_lag, m, 1.); }
GRK_TRANS_HD bool reg_is_min(const double* rho, int max_lag, int m) { return reg_extremum(rho, max_lag, m, -1.); }
GRK_TRANS_HD bool reg_first_peak(const double* rho, const RegRule& r, int m) {
    return m >= r.min_lag && m <= r.max_lag - 1 && reg_is_max(rho, r.max_lag, m) && rho[m] >= r.min_peak;
}

// rule 7 at an extremum m, whose neighbours are defined
GRK_TRANS_HD double reg_refine(const double* rho, int m) {
    const double a = rho[m - 1], b = rho[m], c = rho[m + 1], den = (a - 2. * b) + c;
    return den == 0. ? (double)m : (double)m + (0.5 * (a - c)) / den;
}

// the extremum of `mask` in [lo, hi] with the largest sign * rho, of a tie the earliest; -1: none
GRK_TRANS_HD int reg_best(const double* rho, const unsigned long long* mask, long long lo, long long hi, double sign) {
    int best = -1;
    for (long long m = track_first(mask, lo, hi + 1); m >= 0; m = track_first(mask, m + 1, hi + 1))
        if (best < 0 || sign * rho[m] > sign * rho[best]) best = (int)m;
    return best;
}

// peak, maxima, minima: kRegLagWords words each, bit m for lag m; sum_0, n: reg_lag of lag 0 -> the row
GRK_TRANS_HD void reg_row(const double* rho, const unsigned long long* peak, const unsigned long long* maxima, const unsigned long long* minima, const RegRule& r,
                          bool odd, long long n, double sum_0, double* out) {
    const double none = gait_detail::nan();
    for (int c = 1; c < kRegSeqCols; ++c) out[c] = none;
    out[kRegColN] = (double)n;
    if (rho[0] != rho[0]) return;                              // rho(0) is not defined: nothing is
    out[kRegColA0] = sum_0 / (double)n;
    const int first = (int)track_first(peak, r.min_lag, r.max_lag);
    int d1 = -1, d2 = -1;
    if (odd) {
        d2 = first;
        if (d2 >= 0) d1 = reg_best(rho, minima, d2 - 3 * d2 / 4, d2 - d2 / 4, -1.);
    } else {
        d1 = first;
        if (d1 >= 0) {
            const long long lo = 2 * d1 - d1 / 2, hi = 2 * d1 + d1 / 2;
            d2 = reg_best(rho, maxima, lo < 1 ? 1 : lo, hi > r.max_lag - 1 ? r.max_lag - 1 : hi, 1.);
        }
    }
    out[kRegColStepLag] = (double)d1;
    out[kRegColStrideLag] = (double)d2;
    if (d1 >= 0) {
        out[kRegColStepLagFine] = reg_refine(rho, d1);
        out[kRegColStepReg] = odd ? -rho[d1] : rho[d1];
    }
    if (d2 >= 0) {
        out[kRegColStrideLagFine] = reg_refine(rho, d2);
        out[kRegColStrideReg] = rho[d2];
        out[kRegColCadence] = (120. * r.fps) / out[kRegColStrideLagFine];
        if (d1 >= 0 && out[kRegColStrideReg] > 0.) out[kRegColSymmetry] = out[kRegColStepReg] / out[kRegColStrideReg];
    }
}

}  // namespace grk
