// Harmonic ratios per stride of the four body signals of gait_regularity.h in float64 (Smidt et al. 1971, Menz et al. 2003, Bellanca et
// al. 2013, the bounded form of Pasciuto et al. 2017): no HIP and nothing of the library, so gait_harmonics_kernels.hip uses it on the device and the
// stand-alone checker tests/helpers/gait_harmonics_check.cpp on the host.  Whoever includes it compiles WITHOUT fma contraction (-ffp-contract=off):
// every operation below rounds once, in the order the parentheses show.  No libm and no device library: the sine and cosine are har_twiddle's, so
// that the device, the host checker and the numpy statement give the same bits.
//
// har_walk      -- rule 3's candidates of one sequence in order, from the two heel-strike bitmasks (64 frames a word, track_first's searches).
// har_twiddle   -- rule 5: (sin, cos) of 2 pi j / L by integer reduction to [0, pi/4] and two Horner polynomials.
// har_detrend   -- rule 4; har_harmonics -- rule 6's H; har_amplitude -- a_k from the two sums.
// har_add / har_ratio -- rule 7: the four sums over the harmonics in rising k, then HR and iHR, or "degenerate".
// har_stride    -- rules 3 to 7 of ONE candidate of one channel, serially: the host checker's; the device makes the same values with a lane per
//                  frame and per (harmonic, cosine | sine), out of the same pieces.
// har_summary / har_spectrum -- rule 8's per_seq row and one harmonic's spectrum entry from the strides' slots, serially on both sides.
// har_rule_error -- what a call refuses about its scalars (host only; null: nothing).
#pragma once

#include "gait_regularity.h"

namespace grk {

constexpr int kHarSeqCols = 12;            // candidates, used, HR mean, SD, HR left, right, left / right index, iHR mean, SD, mean L, strides a second, least H
constexpr int kHarStrideCols = 6;          // t0, t1, +1 left / -1 right, H if used else 0, HR, iHR
constexpr int kHarMaxHarmonics = 32;       // a lane per (harmonic, cosine | sine)
constexpr int kHarMinStrideLimit = 6;      // H >= 2 needs L >= 6; the slots of a sequence are counted by it (har_slots)
constexpr int kHarMaxStride = 255;         // y and the two tables of a stride are 256 entries each
constexpr int kHarMaxStrides = 512;
constexpr int kHarSlotTail = 4;            // behind a slot's n_harmonics amplitudes: HR, iHR, H if used else 0, +L left / -L right

struct HarRule { double fps; int n_harmonics, derivative, min_stride, max_stride, max_strides; };

// null, or what is wrong with a call's scalars: the refusals of DESIGN 4.16 beyond those of every call over sequences (host only)
inline const char* har_rule_error(const HarRule& r) {
    using translation_detail::finite;
    if (!finite(r.fps) || !(r.fps > 0.)) return "fps must be positive and finite";
    if (r.n_harmonics < 2 || r.n_harmonics > kHarMaxHarmonics || (r.n_harmonics & 1)) return "n_harmonics must be even and within [2, 32]";
    if (r.derivative < 0 || r.derivative > 2) return "derivative outside [0, 2]";
    if (r.max_stride > kHarMaxStride) return "max_stride above 255";
    if (r.min_stride < kHarMinStrideLimit || r.min_stride > r.max_stride) return "min_stride outside [6, max_stride]";
    if (r.max_strides < 1 || r.max_strides > kHarMaxStrides) return "max_strides outside [1, 512]";
    return nullptr;
}
static_assert(kHarMaxHarmonics == 32 && kHarMaxStride == 255 && kHarMinStrideLimit == 6 && kHarMaxStrides == 512, "har_rule_error's messages name the limits");

// The slots of a sequence of T frames: its candidates whose length lies within [min_stride, max_stride].  Those of one foot are disjoint stretches of
// at least kHarMinStrideLimit frames inside T - 1, so both feet have at most 2 ((T - 1) / 6) <= T / 3 of them.  Sequence q, frames f0 onwards, begins
// at f0 / 3 + q: floor(a / 3) + floor(b / 3) <= floor((a + b) / 3), so no two sequences overlap and all end inside har_slots of the call.
GRK_TRANS_HD size_t har_slots(int frames, int n_seq) { return (size_t)(frames / 3) + (size_t)n_seq; }
GRK_TRANS_HD size_t har_slot_at(int f0, int q) { return (size_t)(f0 / 3) + (size_t)q; }
GRK_TRANS_HD int har_slot_room(int T) { return T / 3 + 1; }

// f(c, foot, t0, t1) of every candidate in rule 3's order; returns their number
template <class F>
GRK_TRANS_HD long long har_walk(const unsigned long long* m_l, const unsigned long long* m_r, int T, F&& f) {
    long long c = 0;
    for (int foot = 0; foot < 2; ++foot) {
        const unsigned long long* m = foot ? m_r : m_l;
        long long t0 = track_first(m, 0, T);
        while (t0 >= 0) {
            const long long t1 = track_first(m, t0 + 1, T);
            if (t1 < 0) break;
            f(c, foot, (int)t0, (int)t1);
            ++c;
            t0 = t1;
        }
    }
    return c;
}

// rule 5: S_k the double nearest to (-1)^k / (2k + 1)!, C_k to (-1)^k / (2k)!  (every factorial here is a double, and the division rounds once)
GRK_TRANS_HD void har_twiddle(int j, int L, double* sn, double* cs) {
    const int r = 4 * j, q = r / L, m = r % L;
    const bool swap = 2 * m > L;
    const int mm = swap ? L - m : m;
    const double phi = (1.5707963267948966 * (double)mm) / (double)L, z = phi * phi;
    double p = 1. / 355687428096000.;
    p = p * z + -1. / 1307674368000.;
    p = p * z + 1. / 6227020800.;
    p = p * z + -1. / 39916800.;
    p = p * z + 1. / 362880.;
    p = p * z + -1. / 5040.;
    p = p * z + 1. / 120.;
    p = p * z + -1. / 6.;
    p = p * z + 1.;
    const double s = phi * p;
    double c = -1. / 6402373705728000.;
    c = c * z + 1. / 20922789888000.;
    c = c * z + -1. / 87178291200.;
    c = c * z + 1. / 479001600.;
    c = c * z + -1. / 3628800.;
    c = c * z + 1. / 40320.;
    c = c * z + -1. / 720.;
    c = c * z + 1. / 24.;
    c = c * z + -1. / 2.;
    c = c * z + 1.;
    const double a = swap ? c : s, b = swap ? s : c;           // (sin, cos) of the angle inside its quarter
    *sn = q == 0 ? a : q == 1 ? b : q == 2 ? -a : -b;
    *cs = q == 0 ? b : q == 1 ? -a : q == 2 ? -b : a;
}

// rule 4: x0 and x1 the signal at t0 and t1, xi at t0 + i
GRK_TRANS_HD double har_detrend(double xi, double x0, double x1, int i, int L) { return (xi - x0) - (x1 - x0) * ((double)i / (double)L); }

// rule 6: strictly below Nyquist, as many even as odd harmonics
GRK_TRANS_HD int har_harmonics(int n_harmonics, int L) {
    const int h = n_harmonics < (L - 1) / 2 ? n_harmonics : (L - 1) / 2;
    return h & ~1;
}

GRK_TRANS_HD double har_amplitude(double C, double S, int L) { return __builtin_sqrt(C * C + S * S) * (2.0 / (double)L); }

struct HarSums { double E = 0., O = 0., PE = 0., PO = 0.; };

// rule 7, called in rising k
GRK_TRANS_HD void har_add(HarSums& s, int k, double a_k, int derivative) {
    const double g = derivative == 0 ? 1. : derivative == 1 ? (double)k : (double)(k * k), w = a_k * g;
    if (k & 1) { s.O = s.O + w; s.PO = s.PO + w * w; }
    else { s.E = s.E + w; s.PE = s.PE + w * w; }
}

// false: the stride is degenerate
GRK_TRANS_HD bool har_ratio(const HarSums& s, bool odd, double* HR, double* iHR) {
    using translation_detail::finite;
    if (!(s.E > 0.) || !finite(s.E) || !(s.O > 0.) || !finite(s.O)) return false;
    *HR = odd ? s.O / s.E : s.E / s.O;
    *iHR = (100. * (odd ? s.PO : s.PE)) / (s.PE + s.PO);
    return true;
}

// One candidate [t0, t1] of one channel, serially.  x: the sequence's signal, `step` values apart; exclude: its entries or null; y, sn, cs: room for
// kHarMaxStride + 1 values each; amp: n_harmonics values, NaN where the stride is not used or k > H -> H if used, else 0
GRK_TRANS_HD int har_stride(const double* x, int step, const int* exclude, const HarRule& r, bool odd, int t0, int t1, double* y, double* sn, double* cs,
                            double* amp, double* HR, double* iHR) {
    const int L = t1 - t0;
    *HR = *iHR = gait_detail::nan();
    for (int k = 0; k < r.n_harmonics; ++k) amp[k] = gait_detail::nan();
    if (L < r.min_stride || L > r.max_stride) return 0;
    for (int t = t0; t <= t1; ++t)
        if (!reg_valid(x[(size_t)t * step], exclude, t)) return 0;
    const double x0 = x[(size_t)t0 * step], x1 = x[(size_t)t1 * step];
    for (int i = 0; i < L; ++i) {
        y[i] = har_detrend(x[(size_t)(t0 + i) * step], x0, x1, i, L);
        har_twiddle(i, L, sn + i, cs + i);
    }
    const int H = har_harmonics(r.n_harmonics, L);
    HarSums sums;
    for (int k = 1; k <= H; ++k) {
        double C = 0., S = 0.;
        for (int i = 0, j = 0; i < L; ++i) {
            C = C + y[i] * cs[j];
            S = S + y[i] * sn[j];
            j += k;
            if (j >= L) j -= L;
        }
        amp[k - 1] = har_amplitude(C, S, L);
        har_add(sums, k, amp[k - 1], r.derivative);
    }
    if (!har_ratio(sums, odd, HR, iHR)) {
        for (int k = 0; k < r.n_harmonics; ++k) amp[k] = gait_detail::nan();
        return 0;
    }
    return H;
}

// a slot: amp[n_harmonics], then HR, iHR, H if used else 0, +L left / -L right
GRK_TRANS_HD void har_slot_tail(double* slot, int n_harmonics, double HR, double iHR, int H, int foot, int L) {
    slot[n_harmonics] = HR;
    slot[n_harmonics + 1] = iHR;
    slot[n_harmonics + 2] = (double)H;
    slot[n_harmonics + 3] = foot ? -(double)L : (double)L;
}

// mean and two-pass SD (ddof 0) of column `col` of the used slots among n_slots, those with side * slot[.. + 3] > 0 alone where side != 0
GRK_TRANS_HD void har_moments(const double* slots, long long n_slots, int n_harmonics, int col, double side, double* mean, double* sd) {
    const int w = n_harmonics + kHarSlotTail;
    double S = 0.;
    long long n = 0;
    for (long long e = 0; e < n_slots; ++e) {
        const double* s = slots + e * w;
        if (!(s[n_harmonics + 2] > 0.) || (side != 0. && !(side * s[n_harmonics + 3] > 0.))) continue;
        S = S + (col < 0 ? __builtin_fabs(s[n_harmonics + 3]) : s[col]);
        ++n;
    }
    *mean = *sd = gait_detail::nan();
    if (!n) return;
    const double m = S / (double)n;
    double Q = 0.;
    for (long long e = 0; e < n_slots; ++e) {
        const double* s = slots + e * w;
        if (!(s[n_harmonics + 2] > 0.) || (side != 0. && !(side * s[n_harmonics + 3] > 0.))) continue;
        const double v = (col < 0 ? __builtin_fabs(s[n_harmonics + 3]) : s[col]) - m;
        Q = Q + v * v;
    }
    *mean = m;
    *sd = __builtin_sqrt(Q / (double)n);
}

// rule 8's row of one (sequence, channel)
GRK_TRANS_HD void har_summary(const double* slots, long long n_slots, int n_harmonics, long long candidates, double fps, double* out) {
    const int w = n_harmonics + kHarSlotTail;
    long long used = 0;
    double least = gait_detail::nan(), unused;
    for (long long e = 0; e < n_slots; ++e) {
        const double H = slots[e * w + n_harmonics + 2];
        if (!(H > 0.)) continue;
        ++used;
        if (!(least <= H)) least = H;
    }
    out[0] = (double)candidates;
    out[1] = (double)used;
    har_moments(slots, n_slots, n_harmonics, n_harmonics, 0., out + 2, out + 3);
    har_moments(slots, n_slots, n_harmonics, n_harmonics, 1., out + 4, &unused);
    har_moments(slots, n_slots, n_harmonics, n_harmonics, -1., out + 5, &unused);
    out[6] = (100. * __builtin_fabs(out[4] - out[5])) / (0.5 * (out[4] + out[5]));
    har_moments(slots, n_slots, n_harmonics, n_harmonics + 1, 0., out + 7, out + 8);
    har_moments(slots, n_slots, n_harmonics, -1, 0., out + 9, &unused);
    out[10] = fps / out[9];
    out[11] = least;
}

// rule 8's spectrum entry of harmonic k: mean and SD of a_k over the used strides whose H >= k
GRK_TRANS_HD void har_spectrum(const double* slots, long long n_slots, int n_harmonics, int k, double* out) {
    const int w = n_harmonics + kHarSlotTail;
    double S = 0.;
    long long n = 0;
    for (long long e = 0; e < n_slots; ++e)
        if (slots[e * w + n_harmonics + 2] >= (double)k) { S = S + slots[e * w + k - 1]; ++n; }
    out[0] = out[1] = gait_detail::nan();
    if (!n) return;
    const double m = S / (double)n;
    double Q = 0.;
    for (long long e = 0; e < n_slots; ++e)
        if (slots[e * w + n_harmonics + 2] >= (double)k) { const double v = slots[e * w + k - 1] - m; Q = Q + v * v; }
    out[0] = m;
    out[1] = __builtin_sqrt(Q / (double)n);
}

}  // namespace grk
