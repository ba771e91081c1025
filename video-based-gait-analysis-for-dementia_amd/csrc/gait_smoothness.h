// Movement smoothness of four body signals in float64 (the spectral arc length and the dimensionless jerk of Balasubramanian,
// Melendez-Calderon, Roby-Brami and Burdet, J. NeuroEng. Rehabil. 12, 2015, as PAPERS.md cites it): no HIP and nothing of the library, so
// gait_smoothness_kernels.hip uses it on the device and the stand-alone checker tests/helpers/gait_smoothness_check.cpp on the host.  Whoever includes
// it compiles WITHOUT fma contraction (-ffp-contract=off): every operation below rounds once, in the order the parentheses show.  No libm and no
// device library: the sine and cosine are har_twiddle's, the differenced signal is ent_diff's, the segments are spec_runs', a bin's frequency is
// spec_freq's (all through gait_spectrum.h).  Every test on data is a comparison that is false for NaN.
//
// smo_rule_error   -- what a call refuses about its scalars (host only; null: nothing).
// smo_cut_bin      -- rule 3's k_c: the largest bin whose frequency is at most f_cut.
// smo_magnitude    -- rule 3 of ONE bin k of one segment: M_k.  On the device a lane owns a bin: y is one address for the wave, the twiddles a
//                     gather at (k i) mod N from a table of (sine, cosine) pairs.  No mean is taken off and no window applied.
// smo_peak_take    -- rule 3's M_max one bin at a time in rising k; smo_peak_merge joins two such results whatever their order, which is what
//                     the device's lanes do: the largest magnitude, at the smallest bin of a tie.
// smo_arc_term     -- rule 4's term of one k; smo_arc the serial sum over the band; smo_segment rules 3 (behind the magnitudes) and 4 serially.
// smo_jerk         -- rule 5 of one segment.
// smo_row_take / smo_row_spread / smo_row_write -- rule 7 one slot at a time, in time order; smo_row the serial walk.
#pragma once

#include "gait_spectrum.h"

namespace grk {

constexpr int kSmoSegCols = 8;            // start, sparc, k_first, k_last, peak_bin, peak_magnitude, dj, v_peak
constexpr int kSmoSeqCols = 10;           // n, candidates, used, defined, sparc_mean, sparc_sd, sparc_min, sparc_max, last_hz_mean, dj_defined
constexpr int kSmoMaxNfft = 4096;         // the twiddle table of a call: 4096 (sine, cosine) pairs
constexpr int kSmoMaxBins = kSmoMaxNfft / 2 + 1;
constexpr int kSmoColStart = 0, kSmoColSparc = 1, kSmoColFirst = 2, kSmoColLast = 3, kSmoColPeakBin = 4, kSmoColPeakMagnitude = 5, kSmoColDj = 6, kSmoColVPeak = 7;
constexpr int kSmoColN = 0, kSmoColCandidates = 1, kSmoColUsed = 2, kSmoColDefined = 3, kSmoColMean = 4, kSmoColSd = 5, kSmoColMin = 6, kSmoColMax = 7,
              kSmoColLastHz = 8, kSmoColDjDefined = 9;

struct SmoRule { double fps; int derivative, segment, hop, nfft; double f_cut, amplitude; int min_segments; };

// the rule as gait_spectrum.h's functions read it: spec_freq takes fps and nfft from it, nothing else is read
GRK_TRANS_HD SpecRule smo_spec(const SmoRule& r) { return SpecRule{r.fps, r.derivative, r.segment, r.hop, r.nfft, 0., 0., r.min_segments}; }

// null, or what is wrong with a call's scalars: the refusals of DESIGN 4.24 beyond those of every call over sequences (host only)
inline const char* smo_rule_error(const SmoRule& r) {
    using translation_detail::finite;
    // spec_rule_error's own sentences for fps, derivative, segment, hop and min_segments: its nfft and its band are given values it accepts
    if (const char* why = spec_rule_error(SpecRule{r.fps, r.derivative, r.segment, r.hop, r.segment, r.fps / 4., r.fps / 2., r.min_segments})) return why;
    if (r.nfft < r.segment || r.nfft > kSmoMaxNfft || (r.nfft & 1)) return "nfft must be even and within [segment, 4096]";
    if (!finite(r.f_cut) || !(r.f_cut > 0.) || !(r.f_cut <= r.fps / 2.)) return "f_cut must obey 0 < f_cut <= fps / 2";
    if (!(r.amplitude > 0.) || !(r.amplitude <= 1.)) return "amplitude must be within (0, 1]";
    return nullptr;
}
static_assert(kSmoMaxNfft == 4096, "smo_rule_error's messages name the limits");

// the largest k of 0 .. N / 2 with spec_freq(k) <= f_cut: bin 0 has frequency 0 < f_cut
GRK_TRANS_HD int smo_cut_bin(const SmoRule& r) {
    const SpecRule sr = smo_spec(r);
    int kc = 0;
    for (int k = 1; k <= r.nfft / 2; ++k)
        if (spec_freq((double)k, sr) <= r.f_cut) kc = k;
    return kc;
}

// y: the segment's L values, all finite; tw: har_twiddle(j, N) for j = 0 .. N - 1 as pairs (sine, cosine).  The samples behind L are zeros, and
// a sum that began at +0.0 is not changed by adding a zero of either sign: the loop ends at L
GRK_TRANS_HD double smo_magnitude(const double* y, int L, const double* tw, int N, int k) {
    double C = 0., S = 0.;
    for (int i = 0, j = 0; i < L; ++i) {
        const double v = y[i];
        C = C + v * tw[2 * j + 1];
        S = S + v * tw[2 * j];
        j += k;
        if (j >= N) j -= N;                                    // k <= N / 2: one subtraction is enough
    }
    return __builtin_sqrt(C * C + S * S);
}

// the largest magnitude so far and its bin; none yet: (+0.0, kSmoNoBin).  A NaN magnitude never becomes the peak: both comparisons are false for it
constexpr int kSmoNoBin = 0x7fffffff;
struct SmoPeak { double m; int k; };
GRK_TRANS_HD SmoPeak smo_peak_none() { return SmoPeak{0., kSmoNoBin}; }
GRK_TRANS_HD SmoPeak smo_peak_merge(SmoPeak a, SmoPeak b) { return b.m > a.m || (b.m == a.m && b.k < a.k) ? b : a; }
GRK_TRANS_HD SmoPeak smo_peak_take(SmoPeak a, double M, int k) { return smo_peak_merge(a, SmoPeak{M, k}); }
GRK_TRANS_HD bool smo_peak_holds(SmoPeak p) { return p.m > 0. && translation_detail::finite(p.m); }      // M_max positive and finite

GRK_TRANS_HD double smo_arc_term(double u, double m0, double m1) { return __builtin_sqrt(u * u + (m1 - m0) * (m1 - m0)); }

// term: k_b - k_a values, rule 4's terms in rising k
GRK_TRANS_HD double smo_arc(const double* term, int n) {
    double arc = 0.;
    for (int k = 0; k < n; ++k) arc = arc + term[k];
    return 0. - arc;
}

// M: the k_c + 1 magnitudes of one segment, turned into m_k = M_k / M_max in place; term: room for k_c values -> the columns sparc .. peak_magnitude
// of the slot's row (NaN where M_max is not positive and finite); returns whether they hold
GRK_TRANS_HD bool smo_segment(double* M, int bins, double amplitude, double* term, double* row) {
    SmoPeak p = smo_peak_none();
    for (int k = 0; k < bins; ++k) p = smo_peak_take(p, M[k], k);
    if (!smo_peak_holds(p)) {
        for (int c = kSmoColSparc; c <= kSmoColPeakMagnitude; ++c) row[c] = gait_detail::nan();
        return false;
    }
    int ka = bins, kb = -1;
    for (int k = 0; k < bins; ++k) {
        M[k] = M[k] / p.m;
        if (M[k] >= amplitude) {
            if (k < ka) ka = k;
            kb = k;
        }
    }
    double sparc = 0.;
    if (kb > ka) {
        const double u = 1.0 / (double)(kb - ka);
        for (int k = ka; k < kb; ++k) term[k - ka] = smo_arc_term(u, M[k], M[k + 1]);
        sparc = smo_arc(term, kb - ka);
    }
    row[kSmoColSparc] = sparc;
    row[kSmoColFirst] = (double)ka;
    row[kSmoColLast] = (double)kb;
    row[kSmoColPeakBin] = (double)p.k;
    row[kSmoColPeakMagnitude] = p.m;
    return true;
}

// x: the segment's L undifferenced values, all finite -> dj and v_peak (dj NaN where v_peak is not positive)
GRK_TRANS_HD void smo_jerk(const double* x, int L, double* dj, double* v_peak) {
    double top = 0., J = 0.;
    for (int i = 0; i + 1 < L; ++i) {
        const double a = __builtin_fabs(x[i + 1] - x[i]);
        if (a > top) top = a;
    }
    for (int i = 0; i + 3 < L; ++i) {
        const double j = ((x[i + 3] - 3. * x[i + 2]) + 3. * x[i + 1]) - x[i];
        J = J + j * j;
    }
    const double l1 = (double)(L - 1);
    *v_peak = top;
    *dj = top > 0. ? (J * ((l1 * l1) * l1)) / (top * top) : gait_detail::nan();      // (L - 1)^3 <= 255^3: exact in every order
}

// rule 7, one slot at a time in time order.  First every slot through smo_row_take, then, with the mean, every slot through smo_row_spread
struct SmoSums { long long defined, dj_defined; double S, H, lo, hi; };
GRK_TRANS_HD SmoSums smo_row_none() { return SmoSums{0, 0, 0., 0., 0., 0.}; }
GRK_TRANS_HD void smo_row_take(SmoSums& a, double sparc, double k_last, double dj, const SpecRule& sr) {
    using translation_detail::finite;
    if (finite(dj)) ++a.dj_defined;
    if (!finite(sparc)) return;
    if (a.defined == 0 || sparc < a.lo) a.lo = sparc;
    if (a.defined == 0 || sparc > a.hi) a.hi = sparc;
    a.S = a.S + sparc;
    a.H = a.H + spec_freq(k_last, sr);
    ++a.defined;
}
GRK_TRANS_HD double smo_row_mean(const SmoSums& a) { return a.S / (double)a.defined; }
GRK_TRANS_HD double smo_row_spread(double Q, double sparc, double mean) {
    if (!translation_detail::finite(sparc)) return Q;
    const double d = sparc - mean;
    return Q + d * d;
}
// out: the row, whose n, candidates and used are written already
GRK_TRANS_HD void smo_row_write(const SmoSums& a, double Q, int used, double* out) {
    for (int c = kSmoColDefined; c < kSmoSeqCols; ++c) out[c] = gait_detail::nan();
    if (used < 1) return;
    out[kSmoColDefined] = (double)a.defined;
    out[kSmoColDjDefined] = (double)a.dj_defined;
    if (a.defined < 1) return;
    out[kSmoColMean] = smo_row_mean(a);
    out[kSmoColSd] = __builtin_sqrt(Q / (double)a.defined);
    out[kSmoColMin] = a.lo;
    out[kSmoColMax] = a.hi;
    out[kSmoColLastHz] = a.H / (double)a.defined;
}

// seg: the slot rows of one (sequence, channel), `stride` values apart; candidates of them are written
GRK_TRANS_HD void smo_row(const double* seg, size_t stride, int candidates, int used, const SmoRule& r, double* out) {
    const SpecRule sr = smo_spec(r);
    SmoSums a = smo_row_none();
    double Q = 0.;
    if (used > 0) {
        for (int s = 0; s < candidates; ++s) smo_row_take(a, seg[s * stride + kSmoColSparc], seg[s * stride + kSmoColLast], seg[s * stride + kSmoColDj], sr);
        if (a.defined > 0) {
            const double mean = smo_row_mean(a);
            for (int s = 0; s < candidates; ++s) Q = smo_row_spread(Q, seg[s * stride + kSmoColSparc], mean);
        }
    }
    smo_row_write(a, Q, used, out);
}

// the slots of n_seq sequences lying back to back: slots[q] = the slots in front of sequence q, slots[n_seq] all of them (host only)
inline void smo_slot_offsets(const int* off, int n_seq, int L, int hop, long long* slots) {
    slots[0] = 0;
    for (int q = 0; q < n_seq; ++q) slots[q + 1] = slots[q] + spec_run_segments(off[q + 1] - off[q], L, hop);
}

}  // namespace grk
