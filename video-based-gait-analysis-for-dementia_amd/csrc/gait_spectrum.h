// Welch power spectral density of four body signals in float64 (Welch, IEEE Trans. Audio Electroacoust. 15, 1967; the band and the peak's
// width of Weiss et al., Neurorehabil. Neural Repair 25, 2011, as PAPERS.md cites it): no HIP and nothing of the library, so gait_spectrum_kernels.hip uses it on the device and the
// stand-alone checker tests/helpers/gait_spectrum_check.cpp on the host.  Whoever includes it compiles WITHOUT fma contraction (-ffp-contract=off):
// every operation below rounds once, in the order the parentheses show.  No libm and no device library: the sine and cosine are har_twiddle's
// (gait_harmonics.h), the differenced signal is ent_diff's (gait_entropy.h), whose NaN marks a frame that does not count.
//
// spec_runs       -- rule 2: f(s, t0) of every segment of a sequence in order, from the validity bitmask of y (64 frames a word, track_first's and
//                    turn_first_clear's searches): inside every run of valid frames, `hop` apart, while the whole segment fits.
// spec_used       -- rule 2's `used` from the number of segments laid.
// spec_hann       -- rule 3's window value w_i; spec_window_power -- W2.
// spec_mean       -- rule 3's mu of one segment.  On the device a lane owns a segment.
// spec_bin        -- rules 3 and 4 of ONE bin k: the sum over the segments, in their order, of C^2 + S^2.  On the device a lane owns a bin: y, mu and
//                    w are one address for the wave, the twiddles a gather at (k i) mod N.  The samples behind L are zeros, and a sum that began at
//                    +0.0 is not changed by adding a zero of either sign: the loop ends at L.
// spec_density    -- rule 4's P(k) from that sum.
// spec_freq / spec_band -- a bin's frequency and rule 5's band, ONE function for the device, the checker and (the same operations) the statement.
// spec_row        -- rule 5's thirteen columns from a finished row of P, serially in rising k.
// spec_rule_error -- what a call refuses about its scalars (host only; null: nothing).
#pragma once

#include "gait_harmonics.h"
#include "gait_entropy.h"

namespace grk {

constexpr int kSpecSeqCols = 13;          // n, candidates, used, band_power, total_power, peak_bin, peak_hz, peak_height, peak_width_hz, dominance,
                                          // centroid_hz, edge_hz, cadence
constexpr int kSpecMinSegment = 8;
constexpr int kSpecMaxSegment = 256;      // the Hann table of a workgroup
constexpr int kSpecMaxNfft = 1024;        // the twiddle table of a workgroup: 1024 sines and 1024 cosines
constexpr int kSpecMaxMinSegments = 1 << 20;
constexpr int kSpecColN = 0, kSpecColCandidates = 1, kSpecColUsed = 2, kSpecColBandPower = 3, kSpecColTotalPower = 4, kSpecColPeakBin = 5, kSpecColPeakHz = 6,
              kSpecColPeakHeight = 7, kSpecColPeakWidth = 8, kSpecColDominance = 9, kSpecColCentroid = 10, kSpecColEdge = 11, kSpecColCadence = 12;

struct SpecRule { double fps; int derivative, segment, hop, nfft; double f_lo, f_hi; int min_segments; };

// null, or what is wrong with a call's scalars: the refusals of DESIGN 4.19 beyond those of every call over sequences (host only)
inline const char* spec_rule_error(const SpecRule& r) {
    using translation_detail::finite;
    if (!finite(r.fps) || !(r.fps > 0.)) return "fps must be positive and finite";
    if (r.derivative < 0 || r.derivative > 2) return "derivative outside [0, 2]";
    if (r.segment < kSpecMinSegment || r.segment > kSpecMaxSegment || (r.segment & 1)) return "segment must be even and within [8, 256]";
    if (r.hop < r.segment / 8 || r.hop > r.segment) return "hop outside [segment / 8, segment]";
    if (r.nfft < r.segment || r.nfft > kSpecMaxNfft || (r.nfft & 1)) return "nfft must be even and within [segment, 1024]";
    if (!finite(r.f_lo) || !finite(r.f_hi) || !(r.f_lo > 0.) || !(r.f_lo < r.f_hi) || !(r.f_hi <= r.fps / 2.)) return "f_lo and f_hi must obey 0 < f_lo < f_hi <= fps / 2";
    if (r.min_segments < 1 || r.min_segments > kSpecMaxMinSegments) return "min_segments outside [1, 2^20]";
    return nullptr;
}
static_assert(kSpecMinSegment == 8 && kSpecMaxSegment == 256 && kSpecMaxNfft == 1024 && kSpecMaxMinSegments == 1048576, "spec_rule_error's messages name the limits");

// the segments a run of `run` valid frames holds, and the most a sequence of T frames can hold (one run: a split only loses some)
GRK_TRANS_HD int spec_run_segments(int run, int L, int hop) { return run >= L ? (run - L) / hop + 1 : 0; }

// valid: the bitmask of the finite frames of y, bits at and behind T clear -> f(s, t0) of segment s = 0, 1, ..; returns their number
template <class F>
GRK_TRANS_HD int spec_runs(const unsigned long long* valid, int T, int L, int hop, F&& f) {
    int s = 0;
    long long a = track_first(valid, 0, T);
    while (a >= 0) {
        const long long clear = turn_first_clear(valid, a, T), e = clear < 0 ? T : clear;
        for (long long t0 = a; t0 + L <= e; t0 += hop) f(s++, (int)t0);
        a = track_first(valid, e, T);
    }
    return s;
}

GRK_TRANS_HD int spec_used(int candidates, int min_segments) { return candidates >= min_segments ? candidates : 0; }

// the periodic Hann window: cs_i the cosine of har_twiddle(i, L)
GRK_TRANS_HD double spec_hann(double cs_i) { return 0.5 - 0.5 * cs_i; }

GRK_TRANS_HD double spec_window_power(const double* w, int L) {
    double W2 = 0.;
    for (int i = 0; i < L; ++i) W2 = W2 + w[i] * w[i];
    return W2;
}

// y: the segment's L values, all finite
GRK_TRANS_HD double spec_mean(const double* y, int L) {
    double S = 0.;
    for (int i = 0; i < L; ++i) S = S + y[i];
    return S / (double)L;
}

// y: the sequence's differenced signal; start, mu: of its `used` segments; w: L window values; sn, cs: har_twiddle(j, N) for j = 0 .. N - 1
GRK_TRANS_HD double spec_bin(const double* y, const int* start, const double* mu, int used, const double* w, int L, const double* sn, const double* cs, int N, int k) {
    double acc = 0.;
    for (int s = 0; s < used; ++s) {
        const double* ys = y + start[s];
        const double m = mu[s];
        double C = 0., S = 0.;
        for (int i = 0, j = 0; i < L; ++i) {
            const double v = (ys[i] - m) * w[i];
            C = C + v * cs[j];
            S = S + v * sn[j];
            j += k;
            if (j >= N) j -= N;                                // k <= N / 2: one subtraction is enough
        }
        acc = acc + (C * C + S * S);
    }
    return acc;
}

GRK_TRANS_HD double spec_density(double acc, int k, int used, const SpecRule& r, double W2) {
    if (used < 1) return gait_detail::nan();
    const double g = k > 0 && k < r.nfft / 2 ? 2. : 1.;
    return (g * acc) / (((double)used * r.fps) * W2);
}

GRK_TRANS_HD double spec_freq(double k, const SpecRule& r) { return (k * r.fps) / (double)r.nfft; }

// the bins 0 .. N / 2 whose frequency lies in [f_lo, f_hi]: k_lo .. k_hi, or k_lo > k_hi where there is none
GRK_TRANS_HD void spec_band(const SpecRule& r, int* k_lo, int* k_hi) {
    int lo = r.nfft / 2 + 1, hi = -1;
    for (int k = 0; k <= r.nfft / 2; ++k) {
        const double f = spec_freq((double)k, r);
        if (f >= r.f_lo && f <= r.f_hi) {
            if (k < lo) lo = k;
            hi = k;
        }
    }
    *k_lo = lo;
    *k_hi = hi;
}

// P: the N / 2 + 1 values of one (sequence, channel); n: the valid values of y -> the row
GRK_TRANS_HD void spec_row(const double* P, const SpecRule& r, bool odd, long long n, int candidates, int used, double* out) {
    using translation_detail::finite;
    const double none = gait_detail::nan();
    for (int c = 0; c < kSpecSeqCols; ++c) out[c] = none;
    out[kSpecColN] = (double)n;
    out[kSpecColCandidates] = (double)candidates;
    out[kSpecColUsed] = (double)used;
    if (used < 1) return;
    const int half = r.nfft / 2;
    const double df = r.fps / (double)r.nfft;
    int k_lo, k_hi;
    spec_band(r, &k_lo, &k_hi);
    double band = 0., total = 0., sum_p = 0., sum_fp = 0.;
    int best = -1;
    for (int k = 1; k <= half; ++k) total = total + P[k] * df;
    for (int k = k_lo; k <= k_hi; ++k) {
        band = band + P[k] * df;
        sum_p = sum_p + P[k];
        sum_fp = sum_fp + spec_freq((double)k, r) * P[k];
        if (P[k] > 0. && finite(P[k]) && (best < 0 || P[k] > P[best])) best = k;
    }
    out[kSpecColBandPower] = band;
    out[kSpecColTotalPower] = total;
    if (sum_p > 0. && finite(sum_p)) out[kSpecColCentroid] = sum_fp / sum_p;
    if (band > 0. && finite(band)) {
        const double bar = 0.95 * band;
        double running = 0.;
        for (int k = k_lo; k <= k_hi; ++k) {
            running = running + P[k] * df;
            if (running >= bar) { out[kSpecColEdge] = spec_freq((double)k, r); break; }
        }
    }
    if (best < 0) return;
    const double b = P[best];
    double at = (double)best;
    if (best > 0 && best < half) {
        const double a = P[best - 1], c = P[best + 1], den = (a - 2. * b) + c;
        if (den < 0. && b >= a && b >= c) at = (double)best + (0.5 * (a - c)) / den;      // else the peak's own bin: on a slope, or flat
    }
    out[kSpecColPeakBin] = (double)best;
    out[kSpecColPeakHz] = spec_freq(at, r);
    out[kSpecColPeakHeight] = b;
    out[kSpecColCadence] = (odd ? 120. : 60.) * out[kSpecColPeakHz];
    const double level = 0.5 * b;
    double left = none, right = none;
    for (int j = best - 1; j >= 0; --j)
        if (P[j] < level) { left = (double)j + (level - P[j]) / (P[j + 1] - P[j]); break; }
    for (int j = best + 1; j <= half; ++j)
        if (P[j] < level) { right = (double)(j - 1) + (P[j - 1] - level) / (P[j - 1] - P[j]); break; }
    out[kSpecColPeakWidth] = spec_freq(right - left, r);
    double three = 0.;
    for (int j = best - 1; j <= best + 1; ++j)
        if (j >= k_lo && j <= k_hi) three = three + P[j] * df;
    if (band > 0. && finite(band)) out[kSpecColDominance] = three / band;
}

}  // namespace grk
