// Footprints, centre of mass and margin of stability in float64: no HIP and nothing of the library, so gait_balance_kernels.hip uses it
// on the device and the stand-alone checker tests/helpers/gait_balance_check.cpp on the host.  Whoever includes it compiles WITHOUT fma contraction
// (-ffp-contract=off): every operation below rounds once, in the order the parentheses show.  Every test is a comparison that is false for NaN.
//
// balance_com       -- rule 1 of ONE frame: c, rL = c - left ankle, rR = c - right ankle, the nine values of a row of `rel`.
// balance_rel_of    -- the same row from a centre of mass the caller brings (grnet_gait_balance_com).
// A MARK is a frame whose events carry a heel-strike bit; the sequence's marks in time order are a list of (frame << 2 | bits).  A frame with both
// bits is a mark that is a strike of neither foot: no pair with it is a step.
// balance_marks_before / balance_mark_count -- a mark's place in the list from the two heel-strike bitmasks and the marks in front of each word.
// balance_pair      -- rules 3 and 4 of ONE pair of consecutive marks: a row of kBalancePairCols values, whose first 15 are the step table's.
// balance_chain     -- rule 5, SERIAL over the pairs of one sequence in time order: chain numbers, footprints, each step's number and its place
//                      in its chain.
// balance_stride    -- rules 6 and 8 of ONE step.          balance_path -- rule 7 of ONE frame.
// balance_row       -- the per-sequence row, serial in time order.
// balance_rule_error / balance_segments_error -- what a call refuses (host only; null: nothing), so that the stand-alone checker runs them too.
#pragma once

#include "gait_turns.h"

namespace grk {

constexpr int kBalanceRelCols = 9;        // [c, rL, rR]
constexpr int kBalanceFrameCols = 8;      // c, W, stance side, chain
constexpr int kBalanceStepCols = 15;      // t1, t2, s_Y, chain, G (3), stride length, step length, step width, sp, MoS_AP, MoS_ML, vertical, lateral
constexpr int kBalanceSeqCols = 24;
constexpr int kBalancePairCols = 20;      // the step table's 15, then b (3), the step's number in its sequence (-1: no step), its place in its chain
constexpr int kBalanceColB = 15, kBalanceColNumber = 18, kBalanceColLink = 19;
constexpr int kBalanceMaxSegments = 16, kBalanceMaxWindow = 16, kBalanceMaxSettle = 4, kBalanceMaxSteps = 1024;
constexpr int kBalanceLeft = 1, kBalanceRight = 2;      // the bits of a mark: kGaitHeelL, kGaitHeelR
static_assert(kBalanceLeft == kGaitHeelL && kBalanceRight == kGaitHeelR, "a mark keeps the events' two heel-strike bits");

struct BalanceSegments { int n; int joint[kBalanceMaxSegments][2]; double mass[kBalanceMaxSegments], fraction[kBalanceMaxSegments]; };
struct BalanceRule { double fps, gravity; int window, settle, max_step, max_steps; };

// null, or what is wrong with a call's rule: the refusals of DESIGN 4.22 beyond those of every call over sequences (host only)
inline const char* balance_rule_error(const BalanceRule& r) {
    using translation_detail::finite;
    if (!finite(r.fps) || !(r.fps > 0.)) return "fps must be positive and finite";
    if (!finite(r.gravity) || !(r.gravity > 0.)) return "gravity must be positive and finite";
    if (r.window < 1 || r.window > kBalanceMaxWindow) return "window outside [1, 16]";
    if (r.settle < 0 || r.settle > kBalanceMaxSettle) return "settle outside [0, 4]";
    if (r.max_step < 1) return "max_step must be at least 1";
    if (r.max_steps < 1 || r.max_steps > kBalanceMaxSteps) return "max_steps outside [1, 1024]";
    return nullptr;
}
static_assert(kBalanceMaxWindow == 16 && kBalanceMaxSettle == 4 && kBalanceMaxSteps == 1024, "balance_rule_error's messages name the limits");

// segments (n_seg,2): proximal and distal joint; weights (n_seg,2): mass and the COM's fraction from the proximal joint -> *out, or what is wrong
inline const char* balance_segments_error(const int* segments, const double* weights, int n_seg, int J, BalanceSegments* out) {
    using translation_detail::finite;
    if (n_seg < 1 || n_seg > kBalanceMaxSegments) return "n_seg outside [1, 16]";
    out->n = n_seg;
    for (int i = 0; i < n_seg; ++i) {
        for (int k = 0; k < 2; ++k) {
            if (segments[2 * i + k] < 0 || segments[2 * i + k] >= J) return "segment joint outside [0, J)";
            out->joint[i][k] = segments[2 * i + k];
        }
        if (!finite(weights[2 * i]) || !(weights[2 * i] > 0.)) return "segment mass must be positive and finite";
        if (!finite(weights[2 * i + 1])) return "segment fraction must be finite";
        out->mass[i] = weights[2 * i];
        out->fraction[i] = weights[2 * i + 1];
    }
    return nullptr;
}
static_assert(kBalanceMaxSegments == 16, "balance_segments_error's message names the limit");

// rule 1.  rows: the frame's (J,3) float32 joints; rel: [c, c - left ankle, c - right ankle]
GRK_TRANS_HD void balance_com(const float* rows, const BalanceSegments& seg, int lankle, int rankle, double* rel) {
    double den = 0.;
    for (int i = 0; i < seg.n; ++i) den = den + seg.mass[i];
    for (int a = 0; a < 3; ++a) {
        double num = 0.;
        for (int i = 0; i < seg.n; ++i) {
            const double P = (double)rows[3 * seg.joint[i][0] + a], D = (double)rows[3 * seg.joint[i][1] + a];
            num = num + seg.mass[i] * (P + seg.fraction[i] * (D - P));
        }
        const double c = num / den;
        rel[a] = c;
        rel[3 + a] = c - (double)rows[3 * lankle + a];
        rel[6 + a] = c - (double)rows[3 * rankle + a];
    }
}

// rule 1 with a given c (3 values): [c, c - left ankle, c - right ankle]
GRK_TRANS_HD void balance_rel_of(const float* rows, const double* c, int lankle, int rankle, double* rel) {
    for (int a = 0; a < 3; ++a) {
        rel[a] = c[a];
        rel[3 + a] = c[a] - (double)rows[3 * lankle + a];
        rel[6 + a] = c[a] - (double)rows[3 * rankle + a];
    }
}

// the marks in front of frame t (t < 64 * words): left, right: the heel-strike bitmasks of the sequence; before[w]: the marks in front of word w
GRK_TRANS_HD long long balance_marks_before(const unsigned long long* left, const unsigned long long* right, const unsigned long long* before, long long t) {
    const unsigned long long v = (left[t >> 6] | right[t >> 6]) & ~(~0ull << (t & 63));
    return (long long)before[t >> 6] + __builtin_popcountll(v);
}
GRK_TRANS_HD long long balance_mark_count(const unsigned long long* left, const unsigned long long* right, const unsigned long long* before, int T) {
    const int w = (T - 1) >> 6;
    return (long long)before[w] + __builtin_popcountll(left[w] | right[w]);
}

// where r_X lies in a row of rel: the stance foot's bit -> 3 (left) or 6 (right)
GRK_TRANS_HD int balance_rel_col(int foot) { return foot == kBalanceLeft ? 3 : 6; }

// rules 3 and 4 of the pair of consecutive marks m1, m2 of a sequence of T frames, rel (T,9): the pair's row, NaN but for its number where it is no step
GRK_TRANS_HD bool balance_pair(const double* rel, int T, int m1, int m2, const BalanceRule& r, double* row) {
    using translation_detail::finite;
    for (int k = 0; k < kBalancePairCols; ++k) row[k] = gait_detail::nan();
    row[kBalanceColNumber] = -1.;
    const int t1 = m1 >> 2, X = m1 & 3, t2 = m2 >> 2, Y = m2 & 3, w = r.window;
    if (X == 3 || Y == 3 || X == Y) return false;
    if (t2 - t1 < w || t2 - t1 > r.max_step) return false;
    const int tb = t2 + r.settle;
    if (tb > T - 1) return false;
    const int cx = balance_rel_col(X), cy = balance_rel_col(Y);
    for (int t = t1; t <= t2; ++t)
        for (int a = 0; a < 3; ++a)
            if (!finite(rel[(long long)t * kBalanceRelCols + cx + a])) return false;
    double b[3];
    for (int a = 0; a < 3; ++a) {
        b[a] = rel[(long long)tb * kBalanceRelCols + cx + a] - rel[(long long)tb * kBalanceRelCols + cy + a];
        if (!finite(b[a])) return false;
    }
    const double half = (double)w / 2.0;
    double D = 0., Nx = 0., Nz = 0.;
    for (int i = 0; i <= w; ++i) {
        const double k = (double)i - half;
        const double* p = rel + (long long)(t2 - w + i) * kBalanceRelCols + cx;
        Nx = Nx + k * p[0];
        Nz = Nz + k * p[2];
        D = D + k * k;
    }
    const double vx = (Nx / D) * r.fps, vz = (Nz / D) * r.fps;
    const double sp = __builtin_sqrt(vx * vx + vz * vz);
    if (!(sp > 0.) || !finite(sp)) return false;
    const double ax = vx / sp, az = vz / sp, lx = -az, lz = ax;
    const double* p2 = rel + (long long)t2 * kBalanceRelCols + cx;
    const double l = -p2[1];
    if (!(l > 0.)) return false;
    const double w0 = __builtin_sqrt(r.gravity / l);
    const double dx = b[0] - (p2[0] + vx / w0), dz = b[2] - (p2[2] + vz / w0);
    const double sY = Y == kBalanceLeft ? 1. : -1.;
    row[0] = (double)t1;
    row[1] = (double)t2;
    row[2] = sY;
    row[10] = sp;
    row[11] = dx * ax + dz * az;
    row[12] = sY * (dx * lx + dz * lz);
    for (int a = 0; a < 3; ++a) row[kBalanceColB + a] = b[a];
    row[kBalanceColNumber] = 0.;
    return true;
}

// rule 5 over the n_pairs rows of one sequence in time order; counts = [steps, chains]
GRK_TRANS_HD void balance_chain(double* pairs, long long n_pairs, long long* counts) {
    long long steps = 0, chains = 0, link = 0;
    bool prev = false;
    double G[3] = {0., 0., 0.};
    for (long long i = 0; i < n_pairs; ++i) {
        double* row = pairs + i * kBalancePairCols;
        const bool step = row[kBalanceColNumber] >= 0.;
        if (step) {
            if (!prev) { G[0] = G[1] = G[2] = 0.; link = 0; ++chains; }
            for (int a = 0; a < 3; ++a) { G[a] = G[a] + row[kBalanceColB + a]; row[4 + a] = G[a]; }
            row[3] = (double)(chains - 1);
            row[kBalanceColNumber] = (double)steps++;
            row[kBalanceColLink] = (double)link++;
        }
        prev = step;
    }
    counts[0] = steps;
    counts[1] = chains;
}

// G_j of the step in `row`: where the step's stance foot stands
GRK_TRANS_HD void balance_stance_print(const double* row, double* G) {
    const bool first = !(row[kBalanceColLink] >= 1.);
    for (int a = 0; a < 3; ++a) G[a] = first ? 0. : (row - kBalancePairCols)[4 + a];
}

// rules 6 and 8 of the step in pair i (behind balance_chain): columns 7, 8, 9, 13, 14 of its row
GRK_TRANS_HD void balance_stride(const double* rel, double* pairs, long long i) {
    double* row = pairs + i * kBalancePairCols;
    if (!(row[kBalanceColLink] >= 1.)) return;
    const double* prev = row - kBalancePairCols;
    double Gm[3], Gj[3];
    balance_stance_print(prev, Gm);
    balance_stance_print(row, Gj);
    const double qx = row[4] - Gm[0], qz = row[6] - Gm[2];
    const double L = __builtin_sqrt(qx * qx + qz * qz);
    const bool has = L > 0.;
    double px = 0., pz = 0.;
    if (has) {
        px = qx / L;
        pz = qz / L;
        row[7] = L;
        row[8] = row[kBalanceColB] * px + row[kBalanceColB + 2] * pz;
        row[9] = __builtin_fabs(row[kBalanceColB] * (-pz) + row[kBalanceColB + 2] * px);
    }
    const int ta = (int)prev[0], t1 = (int)row[0], tb = (int)row[1];
    const int cp = balance_rel_col(prev[2] > 0. ? kBalanceRight : kBalanceLeft), cc = balance_rel_col(row[2] > 0. ? kBalanceRight : kBalanceLeft);
    double hy = 0., ly = 0., hl = 0., ll = 0.;
    for (int t = ta; t <= tb; ++t) {
        const double* G = t < t1 ? Gm : Gj;
        const double* p = rel + (long long)t * kBalanceRelCols + (t < t1 ? cp : cc);
        const double Wx = G[0] + p[0], Wy = G[1] + p[1], Wz = G[2] + p[2];
        const double lat = (Wx - Gm[0]) * (-pz) + (Wz - Gm[2]) * px;
        if (t == ta) { hy = ly = Wy; hl = ll = lat; }
        hy = Wy > hy ? Wy : hy;
        ly = Wy < ly ? Wy : ly;
        hl = lat > hl ? lat : hl;
        ll = lat < ll ? lat : ll;
    }
    row[13] = (hy - ly) + 0.;                                  // + 0.0: a spread of zeros of either sign is +0.0
    if (has) row[14] = (hl - ll) + 0.;
}

// rule 7 of frame t: before = the marks in front of it, at = it is a mark itself, n_marks = the sequence's; out: the frame's 8 columns
GRK_TRANS_HD void balance_path(const double* rel, const double* pairs, long long n_marks, long long before, bool at, int t, double* out) {
    const double* p = rel + (long long)t * kBalanceRelCols;
    const long long i = before + (at ? 1 : 0) - 1;             // the last mark at or before t: the pair it begins
    const double* row = nullptr;
    if (i >= 0 && i < n_marks - 1 && pairs[i * kBalancePairCols + kBalanceColNumber] >= 0.) row = pairs + i * kBalancePairCols;
    else if (at && i >= 1 && pairs[(i - 1) * kBalancePairCols + kBalanceColNumber] >= 0.) row = pairs + (i - 1) * kBalancePairCols;
    for (int a = 0; a < 3; ++a) { out[a] = p[a]; out[3 + a] = gait_detail::nan(); }
    out[6] = 0.;
    out[7] = gait_detail::nan();
    if (!row) return;
    double G[3];
    balance_stance_print(row, G);
    const int c = balance_rel_col(row[2] > 0. ? kBalanceRight : kBalanceLeft);
    for (int a = 0; a < 3; ++a) out[3 + a] = G[a] + p[c + a];
    out[6] = -row[2];
    out[7] = row[3];
}

// the per-sequence row from the pairs in time order; strikes: the marks with one bit
GRK_TRANS_HD void balance_row(const double* pairs, long long n_pairs, long long strikes, long long steps, long long chains, double fps, double* out) {
    constexpr int kStats = 8;
    const int src[kStats] = {7, 8, 9, 10, 11, 12, 13, 14}, dst[kStats] = {4, 6, 8, 11, 14, 16, 20, 22};
    const double none = gait_detail::nan();
    double S[kStats], mean[kStats], side[4] = {0., 0., 0., 0.}, dist = 0., time = 0.;      // side: step length left, right; MoS_ML left, right
    long long n[kStats], n_side[4] = {0, 0, 0, 0};
    for (int k = 0; k < kStats; ++k) { S[k] = 0.; n[k] = 0; }
    for (long long i = 0; i < n_pairs; ++i) {
        const double* row = pairs + i * kBalancePairCols;
        if (!(row[kBalanceColNumber] >= 0.)) continue;
        for (int k = 0; k < kStats; ++k) {
            const double x = row[src[k]];
            if (x == x) { S[k] = S[k] + x; ++n[k]; }
        }
        const int f = row[2] > 0. ? 0 : 1;
        if (row[8] == row[8]) { side[f] = side[f] + row[8]; ++n_side[f]; }
        if (row[12] == row[12]) { side[2 + f] = side[2 + f] + row[12]; ++n_side[2 + f]; }
        dist = dist + __builtin_sqrt(row[kBalanceColB] * row[kBalanceColB] + row[kBalanceColB + 2] * row[kBalanceColB + 2]);
        time = time + (row[1] - row[0]) / fps;
    }
    for (int k = 0; k < kStats; ++k) { mean[k] = n[k] ? S[k] / (double)n[k] : none; S[k] = 0.; }
    for (long long i = 0; i < n_pairs; ++i) {
        const double* row = pairs + i * kBalancePairCols;
        if (!(row[kBalanceColNumber] >= 0.)) continue;
        for (int k = 0; k < kStats; ++k) {
            const double x = row[src[k]];
            if (x == x) { const double d = x - mean[k]; S[k] = S[k] + d * d; }
        }
    }
    out[0] = (double)strikes;
    out[1] = (double)steps;
    out[2] = (double)chains;
    out[3] = (double)n[0];
    for (int k = 0; k < kStats; ++k) {
        out[dst[k]] = mean[k];
        out[dst[k] + 1] = n[k] ? __builtin_sqrt(S[k] / (double)n[k]) : none;
    }
    const double L = n_side[0] ? side[0] / (double)n_side[0] : none, R = n_side[1] ? side[1] / (double)n_side[1] : none;
    out[10] = n_side[0] && n_side[1] ? (100. * __builtin_fabs(L - R)) / (0.5 * (L + R)) : none;
    out[13] = steps ? dist / time : none;
    out[18] = n_side[2] ? side[2] / (double)n_side[2] : none;
    out[19] = n_side[3] ? side[3] / (double)n_side[3] : none;
}

}  // namespace grk
