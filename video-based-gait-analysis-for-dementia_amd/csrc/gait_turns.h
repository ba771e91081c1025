// Turns and straight-walking gait parameters in float64 (the thresholds after El-Gohary et al., Sensors 14, 2014): no HIP and nothing of
// the library, so gait_turns_kernels.hip uses it on the device and the stand-alone checker tests/helpers/gait_turns_check.cpp on the host.  Whoever
// includes it compiles WITHOUT fma contraction (-ffp-contract=off): every operation below rounds once, in the order the parentheses show.  The frame's
// axes are gait_events.h's, the arctangent gait_angles.h's, the Gaussian and the searches by word in a 64-frames-a-word bitmask track_boxes.h's.
//
// turn_heading      -- g = (f_x, f_z) of one frame, f made as gait_frame makes it (the same operations); NaN of an invalid frame.
// turn_step         -- the yaw step in degrees from g(t - 1) to g(t): gait_atan2(cross, dot) * kKinDegrees, positive towards the subject's left.
// turn_first_clear / turn_last_clear -- the searches track_first / track_last make for a set bit, for a CLEAR one: the end of a run of set bits.
// turn_run          -- the walk of ONE run of frames [a, e): max |w|, the sum of the raw steps in time order from +0.0, and the verdict of rule 4.
// turn_row          -- the turn table's row of an accepted run.
// turn_rule_error   -- what a call refuses about its rule (host only; null: nothing), so that the stand-alone checker runs every refusal too.
// turn_counts / turn_mean / turn_steps / turn_strides / turn_stance -- the columns of the per-sequence row, each a walk through the bitmasks of ONE
//                      sequence by word; the last three are gait_steps, gait_strides and gait_stance with one test more per link: the interval counts
//                      where no frame of it is set in the not-straight mask.  With that mask empty they are those functions in every operation.
#pragma once

#include "gait_angles.h"

namespace grk {

constexpr int kTurnFrameCols = 2;         // [yaw step, yaw rate as smoothed]
constexpr int kTurnCols = 7;              // first, last, direction, angle, duration, peak, steps in turn
constexpr int kTurnSeqCols = 24;
constexpr int kTurnMaxTurns = 64;         // rows of a sequence's turn table, at most
constexpr int kTurnGaitAt = 7;            // column k of the gait row's 4 .. 16 lies at k + 7
constexpr int kTurnStraight = 0, kTurnLeft = 1, kTurnRight = 2, kTurnUnknown = 3;      // a frame's phase
constexpr int kTurnColTurns = 0, kTurnColLeft = 1, kTurnColRight = 2, kTurnColTurnFrames = 3, kTurnColUnknown = 4, kTurnColBouts = 5, kTurnColStraight = 6,
              kTurnColDuration = 7, kTurnColAngle = 8, kTurnColPeak = 9, kTurnColTurnSteps = 10;

struct TurnRule { double fps, edge_rate, peak_rate, min_angle; int min_frames, max_frames, max_turns; };

// null, or what is wrong with a call's rule: the refusals of DESIGN 4.13 beyond those of every call over sequences (host only)
inline const char* turn_rule_error(const TurnRule& r) {
    using translation_detail::finite;
    if (!finite(r.fps) || !(r.fps > 0.)) return "fps must be positive and finite";
    if (!finite(r.edge_rate) || r.edge_rate < 0.) return "edge_rate must be finite and not negative";
    if (!finite(r.peak_rate) || r.peak_rate < r.edge_rate) return "peak_rate must be finite and not below edge_rate";
    if (!finite(r.min_angle) || r.min_angle < 0.) return "min_angle must be finite and not negative";
    if (r.min_frames < 1) return "min_frames must be at least 1";
    if (r.max_frames < r.min_frames) return "max_frames must not be below min_frames";
    if (r.max_turns < 1 || r.max_turns > kTurnMaxTurns) return "max_turns outside [1, 64]";
    return nullptr;
}
static_assert(kTurnMaxTurns == 64, "turn_rule_error's message names the limit");

// the bitmasks of one sequence, each ceil(T / 64) words: yaw rate above the edge, below minus the edge, NaN; a run's first frame where it is a turn;
// frames of left turns, of right turns, of either or unknown; the heel strikes and toe-offs of the events
struct TurnMasks { unsigned long long *left, *right, *unknown, *accept, *turn_l, *turn_r, *not_straight, *hs_l, *hs_r, *to_l, *to_r; };
constexpr int kTurnMaskSets = 11;

// rows: the frame's (J,3) float32 joints; tab: pelvis, spine-shoulder, left hip, right hip
GRK_TRANS_HD void turn_heading(const float* rows, const int* tab, double* g) {
    using translation_detail::finite;
    double p[4][3];
    for (int k = 0; k < 4; ++k)
        for (int a = 0; a < 3; ++a) p[k][a] = (double)rows[3 * tab[k] + a];
    double l[3], u[3], c[3];
    for (int a = 0; a < 3; ++a) { l[a] = p[2][a] - p[3][a]; u[a] = p[1][a] - p[0][a]; }
    c[0] = l[1] * u[2] - l[2] * u[1];
    c[1] = l[2] * u[0] - l[0] * u[2];
    c[2] = l[0] * u[1] - l[1] * u[0];
    const double nc = __builtin_sqrt(gait_detail::dot3(c, c)), nl = __builtin_sqrt(gait_detail::dot3(l, l));
    if (!(nc > 0.) || !finite(nc) || !(nl > 0.) || !finite(nl)) { g[0] = g[1] = gait_detail::nan(); return; }
    g[0] = c[0] / nc;
    g[1] = c[2] / nc;
}

GRK_TRANS_HD double turn_step(const double* g0, const double* g1) {
    return gait_atan2(g0[0] * g1[1] - g0[1] * g1[0], g0[0] * g1[0] + g0[1] * g1[1]) * kKinDegrees;
}

// the yaw step of frame t of a sequence whose joints begin at `joints`: +0 at t = 0
GRK_TRANS_HD double turn_frame_step(const float* joints, int J, const int* tab, int t) {
    if (t == 0) return 0.;
    double g0[2], g1[2];
    turn_heading(joints + (long long)(t - 1) * J * 3, tab, g0);
    turn_heading(joints + (long long)t * J * 3, tab, g1);
    return turn_step(g0, g1);
}

// the first / last frame of [lo, hi) whose bit is clear, or -1
GRK_TRANS_HD long long turn_first_clear(const unsigned long long* words, long long lo, long long hi) {
    for (long long w = lo >> 6; w <= (hi - 1) >> 6 && lo < hi; ++w) {
        unsigned long long v = ~words[w];
        if (w == lo >> 6) v &= ~0ull << (lo & 63);
        if (v) { const long long g = w * 64 + __builtin_ctzll(v); return g < hi ? g : -1; }
    }
    return -1;
}
GRK_TRANS_HD long long turn_last_clear(const unsigned long long* words, long long lo, long long hi) {
    for (long long w = (hi - 1) >> 6; lo < hi && w >= lo >> 6; --w) {
        unsigned long long v = ~words[w];
        if (w == (hi - 1) >> 6 && (hi & 63)) v &= ~(~0ull << (hi & 63));
        if (v) { const long long g = w * 64 + 63 - __builtin_clzll(v); return g >= lo ? g : -1; }
    }
    return -1;
}

// set bits of [lo, hi)
GRK_TRANS_HD long long turn_popcount(const unsigned long long* words, long long lo, long long hi) {
    long long n = 0;
    for (long long w = lo >> 6; w <= (hi - 1) >> 6 && lo < hi; ++w) {
        unsigned long long v = words[w];
        if (w == lo >> 6) v &= ~0ull << (lo & 63);
        if (w == (hi - 1) >> 6 && (hi & 63)) v &= ~(~0ull << (hi & 63));
        n += __builtin_popcountll(v);
    }
    return n;
}

// whether frame t begins a run of `words` (its bit is set and the frame before it is none of the run)
GRK_TRANS_HD bool turn_run_begins(const unsigned long long* words, int t) { return gait_detail::bit(words, t) && (t == 0 || !gait_detail::bit(words, t - 1)); }

// the frame behind the run of `words` that holds frame t
GRK_TRANS_HD int turn_run_end(const unsigned long long* words, int T, int t) {
    const long long e = turn_first_clear(words, t, T);
    return e < 0 ? T : (int)e;
}

// rows: the sequence's (T,2) [yaw step, yaw rate]; the run [a, e): peak = max |rate|, angle = the sum of the steps; true where it is a turn.  The
// frames are read eight at a time (of a short last batch the last frame again, which is not added): the loads of a batch do not wait for one
// another, the additions keep their order in time.
GRK_TRANS_HD bool turn_run(const double* rows, int a, int e, const TurnRule& r, double* peak, double* angle) {
    constexpr int kBatch = 8;
    double m = 0., s = 0.;
    for (int t = a; t < e; t += kBatch) {
        double d[kBatch], w[kBatch];
        for (int k = 0; k < kBatch; ++k) {
            const long long at = (long long)(t + k < e ? t + k : e - 1) * kTurnFrameCols;
            d[k] = rows[at];
            w[k] = __builtin_fabs(rows[at + 1]);
        }
        for (int k = 0; k < kBatch; ++k) {
            if (t + k >= e) break;
            m = w[k] > m ? w[k] : m;
            s = s + d[k];
        }
    }
    *peak = m; *angle = s;
    const int len = e - a;
    return m >= r.peak_rate && __builtin_fabs(s) >= r.min_angle && len >= r.min_frames && len <= r.max_frames;
}

// heel strikes of either foot inside [a, e)
GRK_TRANS_HD double turn_strikes(const TurnMasks& m, int a, int e) { return (double)(turn_popcount(m.hs_l, a, e) + turn_popcount(m.hs_r, a, e)); }

GRK_TRANS_HD void turn_row(const TurnMasks& m, int a, int e, bool left, double peak, double angle, double fps, double* row) {
    row[0] = (double)a;
    row[1] = (double)(e - 1);
    row[2] = left ? 1. : -1.;
    row[3] = angle;
    row[4] = (double)(e - a) / fps;
    row[5] = peak;
    row[6] = turn_strikes(m, a, e);
}

// columns 0 .. 6
GRK_TRANS_HD void turn_counts(const TurnMasks& m, int T, double* out) {
    long long turns = 0, left = 0, right = 0, frames = 0, unknown = 0, busy = 0, bouts = 0;
    unsigned long long carry = 1ull;                           // the frame before the sequence counts as not straight: frame 0 may open a bout
    for (int w = 0; w <= (T - 1) >> 6; ++w) {
        const unsigned long long in = (w == (T - 1) >> 6 && (T & 63)) ? ~(~0ull << (T & 63)) : ~0ull;
        const unsigned long long ns = m.not_straight[w] & in;
        turns += __builtin_popcountll(m.accept[w] & in);
        left += __builtin_popcountll(m.accept[w] & m.left[w] & in);
        right += __builtin_popcountll(m.accept[w] & m.right[w] & in);
        frames += __builtin_popcountll((m.turn_l[w] | m.turn_r[w]) & in);
        unknown += __builtin_popcountll(m.unknown[w] & in);
        busy += __builtin_popcountll(ns);
        bouts += __builtin_popcountll(~ns & in & ((ns << 1) | carry));
        carry = ns >> 63;
    }
    out[kTurnColTurns] = (double)turns;
    out[kTurnColLeft] = (double)left;
    out[kTurnColRight] = (double)right;
    out[kTurnColTurnFrames] = (double)frames;
    out[kTurnColUnknown] = (double)unknown;
    out[kTurnColBouts] = (double)bouts;
    out[kTurnColStraight] = (double)((long long)T - busy);
}

// one of the columns 7 .. 10 (which = 0 duration, 1 |angle|, 2 peak, 3 steps in turn): the mean over ALL turns of the sequence in time order.  Angle and
// peak of a stored turn are read from its row of the table `turns`; the run of a turn that is not stored is walked again as turn_run walks it, which
// gives the same bits.
GRK_TRANS_HD double turn_mean(const TurnMasks& m, const double* rows, int T, const TurnRule& r, int which, const double* turns) {
    double s = 0.;
    long long n = 0;
    for (long long a = track_first(m.accept, 0, T); a >= 0; a = track_first(m.accept, a + 1, T)) {
        const bool left = gait_detail::bit(m.left, a);
        const int e = turn_run_end(left ? m.left : m.right, T, (int)a);
        double x;
        if (which == 0) x = (double)(e - a) / r.fps;
        else if (which == 3) x = turn_strikes(m, (int)a, e);
        else if (n < r.max_turns) x = which == 1 ? __builtin_fabs(turns[n * kTurnCols + 3]) : turns[n * kTurnCols + 5];
        else {
            double peak, angle;
            turn_run(rows, (int)a, e, r, &peak, &angle);
            x = which == 1 ? __builtin_fabs(angle) : peak;
        }
        s = s + x;
        ++n;
    }
    return n ? s / (double)n : gait_detail::nan();
}

// no frame of [a, b] is set in the not-straight mask
GRK_TRANS_HD bool turn_straight(const unsigned long long* ns, long long a, long long b) { return track_first(ns, a, b + 1) < 0; }

// gait_steps with the mask test; out = the per-sequence row + kTurnGaitAt, so that the gait row's column constants name the places
GRK_TRANS_HD void turn_steps(const TurnMasks& m, int T, const double* rows, double fps, double* out) {
    double mean[3] = {0., 0., 0.}, acc[3] = {0., 0., 0.};
    long long n = 0;
    for (int pass = 0; pass < 2; ++pass) {
        int t = -1, foot = 1, pt = -1, pf = -1;
        acc[0] = acc[1] = acc[2] = 0.;
        while (gait_next_strike(m.hs_l, m.hs_r, T, &t, &foot)) {
            if (pt >= 0 && pf != foot && turn_straight(m.not_straight, pt, t)) {
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

// gait_strides with the mask test
GRK_TRANS_HD void turn_strides(const TurnMasks& m, int T, double fps, double* out) {
    double mean = 0., acc = 0.;
    long long n = 0;
    for (int pass = 0; pass < 2; ++pass) {
        acc = 0.;
        for (int foot = 0; foot < 2; ++foot) {
            const unsigned long long* words = foot ? m.hs_r : m.hs_l;
            long long prev = -1;
            for (long long t = track_first(words, 0, T); t >= 0; t = track_first(words, t + 1, T)) {
                if (prev >= 0 && turn_straight(m.not_straight, prev, t)) {
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

// gait_stance with the mask test on the stride
GRK_TRANS_HD void turn_stance(const TurnMasks& m, int T, double* out) {
    double acc = 0.;
    long long n = 0;
    for (int foot = 0; foot < 2; ++foot) {
        const unsigned long long *hs = foot ? m.hs_r : m.hs_l, *to = foot ? m.to_r : m.to_l;
        long long prev = -1;
        for (long long t = track_first(hs, 0, T); t >= 0; t = track_first(hs, t + 1, T)) {
            if (prev >= 0 && turn_straight(m.not_straight, prev, t)) {
                const long long off = track_first(to, prev + 1, t);
                if (off >= 0) { acc = acc + (100. * (double)(off - prev)) / (double)(t - prev); ++n; }
            }
            prev = t;
        }
    }
    out[kGaitColStance] = n ? acc / (double)n : gait_detail::nan();
}

}  // namespace grk
