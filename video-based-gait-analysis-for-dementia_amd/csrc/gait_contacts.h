// Foot contact phases and double support in float64: no HIP and nothing of the library, so gait_contacts_kernels.hip uses it on the
// device and the stand-alone checker tests/helpers/gait_contacts_check.cpp on the host.  Whoever includes it compiles WITHOUT fma contraction
// (-ffp-contract=off): every operation below rounds once, in the order the parentheses show.  The searches by word in a 64-frames-a-word bitmask are
// track_boxes.h's and gait_turns.h's.  An INTERVAL k of a sequence of T frames lies between its frames k and k + 1, 0 <= k <= T - 2; bit k of a mask
// speaks of interval k, and bit T - 1 of the interval masks is always clear, so that every run of set bits ends inside the sequence.
//
// contact_vector    -- d = left ankle - right ankle of one frame; contact_speed -- s of one interval from the d of its two frames.
// contact_block_sum -- the balanced tree over one block of 64 intervals, adjacent pairs first (on the device a cross-lane butterfly makes the same
//                      additions); contact_threshold -- the blocks added in time order, the mean S / n and the threshold.
// contact_run       -- everything of ONE static run [a, b]: closed or open, its two edges, who led it and by which heel strike, its least speed.
// contact_row       -- the run table's row; contact_phase -- the phase its intervals get.
// contact_rule_error -- what a call refuses about its rule (host only; null: nothing), so that the stand-alone checker runs every refusal too.
// contact_counts / contact_support / contact_strides -- the columns of the per-sequence row, each a walk in time order through the bitmasks of ONE
//                      sequence (contact_next).  Lead, edges and end of the sequence's first runs are kept (ContactKept: the kernel keeps them in
//                      LDS when it makes them) and read back; the others are found by word in the masks and their edges made again from s (the
//                      same operations, the same bits), so no column depends on how many runs the table stores or how many are kept.
#pragma once

#include "gait_turns.h"

namespace grk {

constexpr int kContactFrameCols = 4;      // [s, d_x, d_y, d_z as smoothed]
constexpr int kContactRunCols = 6;        // t_start, t_end, lead, heel-strike frame, duration, least s
constexpr int kContactSeqCols = 20;
constexpr int kContactMaxRuns = 512;      // rows of a sequence's run table, at most
constexpr int kContactMaxReach = 8;
constexpr int kContactBlock = 64;         // intervals of one block of the fixed-tree sum: a word of the masks, a wave of the kernel
constexpr int kContactMoving = 0, kContactLeft = 1, kContactRight = 2, kContactUnattributed = 3, kContactNan = 4;      // an interval's phase
constexpr int kContactColThr = 0, kContactColMean = 1, kContactColRuns = 2, kContactColLeft = 3, kContactColRight = 4, kContactColUnattributed = 5,
              kContactColSupport = 6, kContactColSupportSd = 7, kContactColSupportL = 8, kContactColSupportR = 9, kContactColAsymmetry = 10,
              kContactColStrides = 11, kContactColStride = 12, kContactColStrideSd = 13, kContactColStance = 14, kContactColSwing = 15,
              kContactColSingle = 16, kContactColStanceShare = 17, kContactColSupportShare = 18, kContactColStrideCv = 19;

struct ContactRule { double fps, fraction, speed; int reach, max_frames, max_runs; };

// null, or what is wrong with a call's rule: the refusals of DESIGN 4.14 beyond those of every call over sequences (host only)
inline const char* contact_rule_error(const ContactRule& r) {
    using translation_detail::finite;
    if (!finite(r.fps) || !(r.fps > 0.)) return "fps must be positive and finite";
    if (!finite(r.fraction) || r.fraction < 0.) return "fraction must be finite and not negative";
    if (!finite(r.speed) || r.speed < 0.) return "speed must be finite and not negative";
    if (r.fraction == 0. && r.speed == 0.) return "fraction and speed are both zero: no threshold";
    if (r.reach < 0 || r.reach > kContactMaxReach) return "reach outside [0, 8]";
    if (r.max_frames < 1) return "max_frames must be at least 1";
    if (r.max_runs < 1 || r.max_runs > kContactMaxRuns) return "max_runs outside [1, 512]";
    return nullptr;
}
static_assert(kContactMaxReach == 8 && kContactMaxRuns == 512, "contact_rule_error's messages name the limits");

// the bitmasks of one sequence, each ceil(T / 64) words: static intervals, intervals whose s is finite, the heel strikes of the events (by frame);
// at a run's FIRST interval: led by the left foot, led by the right foot
struct ContactMasks { unsigned long long *is_static, *finite, *hs_l, *hs_r, *lead_l, *lead_r; };
constexpr int kContactMaskSets = 6;

// rows: the frame's (J,3) float32 joints; tab: the gait call's table, of which entries 4 and 5 (the ankles) are read
GRK_TRANS_HD void contact_vector(const float* rows, const int* tab, double* d) {
    for (int a = 0; a < 3; ++a) d[a] = (double)rows[3 * tab[4] + a] - (double)rows[3 * tab[5] + a];
}

GRK_TRANS_HD double contact_speed(const double* d0, const double* d1, double fps) {
    const double x = d1[0] - d0[0], y = d1[1] - d0[1], z = d1[2] - d0[2];
    return __builtin_sqrt((x * x + y * y) + z * z) * fps;
}

// the sum of block `block` of the n intervals s[0], s[stride], ...: a non-finite or missing entry adds +0.0; 0+1, 2+3, ..., then pairs of those
GRK_TRANS_HD double contact_block_sum(const double* s, long long stride, int n, int block) {
    double v[kContactBlock];
    for (int i = 0; i < kContactBlock; ++i) {
        const long long k = (long long)block * kContactBlock + i;
        const double x = k < n ? s[k * stride] : 0.;
        v[i] = translation_detail::finite(x) ? x : 0.;
    }
    for (int width = kContactBlock / 2; width >= 1; width /= 2)
        for (int i = 0; i < width; ++i) v[i] = v[2 * i] + v[2 * i + 1];
    return v[0];
}

// blocks: the sums of the sequence's ceil(T / 64) blocks; finite: its mask -> the threshold; *mean = S / n (NaN where no s is finite)
GRK_TRANS_HD double contact_threshold(const double* blocks, const unsigned long long* finite, int T, const ContactRule& r, double* mean) {
    double S = 0.;
    for (int w = 0; w <= (T - 1) >> 6; ++w) S = S + blocks[w];
    const long long n = turn_popcount(finite, 0, T);
    *mean = n ? S / (double)n : gait_detail::nan();
    return r.speed > 0. ? r.speed : r.fraction * *mean;
}

// whether interval k begins a static run, the interval behind the run that holds interval k, and the runs that begin below interval k
GRK_TRANS_HD bool contact_run_begins(const unsigned long long* words, int k) { return turn_run_begins(words, k); }
GRK_TRANS_HD int contact_run_end(const unsigned long long* words, int T, long long k) {
    const long long e = turn_first_clear(words, k, T);
    return e < 0 ? T - 1 : (int)e;                              // bit T - 1 is clear: not reached
}
GRK_TRANS_HD long long contact_runs_before(const unsigned long long* words, long long k) {
    long long n = 0;
    unsigned long long carry = 0ull;
    for (long long w = 0; w <= (k - 1) >> 6 && k > 0; ++w) {
        const unsigned long long v = words[w];
        unsigned long long begins = v & ~((v << 1) | carry);
        if (w == (k - 1) >> 6 && (k & 63)) begins &= ~(~0ull << (k & 63));
        n += __builtin_popcountll(begins);
        carry = v >> 63;
    }
    return n;
}

struct ContactRun {
    bool closed;
    int lead;                              // +1 the left foot, -1 the right foot, 0 unattributed
    long long strike;                      // the leading foot's earliest heel strike in the window, -1 unattributed
    double t_start, t_end, least;          // the edges in frames (NaN of an open run), min s over the run
};

// the two edges of the closed run [a, b] in frames: s sits at k + 1/2, the threshold is crossed on the straight line to the neighbour outside
GRK_TRANS_HD void contact_edges(const double* s, long long stride, int a, int b, double thr, double* t_start, double* t_end) {
    const double before = s[(long long)(a - 1) * stride], first = s[(long long)a * stride], last = s[(long long)b * stride], after = s[(long long)(b + 1) * stride];
    *t_start = ((double)a - 0.5) + (before - thr) / (before - first);
    *t_end = ((double)b + 0.5) + (thr - last) / (after - last);
}

// what is kept of the sequence's runs 0 .. slots - 1 in time order, kContactKeptCols values a run: [t_start, t_end (NaN of an open run), lead, the
// interval behind the run]; runs: how many runs the sequence has
constexpr int kContactKeptCols = 4;
constexpr int kContactKeptRuns = 512;      // what the kernel keeps in LDS: 16 KB
struct ContactKept { const double* rows; int slots; long long runs; };

GRK_TRANS_HD void contact_keep(double* rows, long long index, int lead, double t_start, double t_end, int behind) {
    double* row = rows + index * kContactKeptCols;
    row[0] = t_start; row[1] = t_end; row[2] = (double)lead; row[3] = (double)behind;
}

GRK_TRANS_HD bool contact_closed(const unsigned long long* finite, int T, int a, int b) {
    return a >= 1 && b <= T - 3 && gait_detail::bit(finite, a - 1) && gait_detail::bit(finite, b + 1);
}

// who leads the closed run [a, b]: the heel strikes of the frames [a - reach, b + 1 + reach] inside the sequence
GRK_TRANS_HD int contact_lead(const ContactMasks& m, int T, int a, int b, const ContactRule& r, long long* strike) {
    *strike = -1;
    if (b - a + 1 > r.max_frames) return 0;
    const long long lo = a - r.reach < 0 ? 0 : a - r.reach, hi = b + 1 + r.reach > T - 1 ? T - 1 : b + 1 + r.reach;
    const long long l = track_first(m.hs_l, lo, hi + 1), rr = track_first(m.hs_r, lo, hi + 1);
    if ((l >= 0) == (rr >= 0)) return 0;                       // both feet strike, or neither
    *strike = l >= 0 ? l : rr;
    return l >= 0 ? 1 : -1;
}

GRK_TRANS_HD ContactRun contact_run(const ContactMasks& m, const double* s, long long stride, int T, int a, int b, double thr, const ContactRule& r) {
    ContactRun run;
    run.closed = contact_closed(m.finite, T, a, b);
    run.lead = 0;
    run.strike = -1;
    run.t_start = run.t_end = gait_detail::nan();
    if (run.closed) {
        contact_edges(s, stride, a, b, thr, &run.t_start, &run.t_end);
        run.lead = contact_lead(m, T, a, b, r, &run.strike);
    }
    double least = s[(long long)a * stride];
    for (int k = a + 1; k <= b; ++k) {
        const double v = s[(long long)k * stride];
        least = v < least ? v : least;
    }
    run.least = least;
    return run;
}

GRK_TRANS_HD void contact_row(const ContactRun& run, double fps, double* row) {
    row[0] = run.t_start;
    row[1] = run.t_end;
    row[2] = (double)run.lead;
    row[3] = run.lead ? (double)run.strike : gait_detail::nan();
    row[4] = run.closed ? (run.t_end - run.t_start) / fps : gait_detail::nan();
    row[5] = run.least;
}

GRK_TRANS_HD int contact_phase(int lead) { return lead > 0 ? kContactLeft : lead < 0 ? kContactRight : kContactUnattributed; }

// the lead of the run that begins at interval a, from the masks
GRK_TRANS_HD int contact_lead_at(const ContactMasks& m, long long a) { return gait_detail::bit(m.lead_l, a) ? 1 : gait_detail::bit(m.lead_r, a) ? -1 : 0; }

// The walk through the runs of one sequence in time order: begin with {-1, 0}; true and the next run's lead and, where it is led, its edges, or false
// behind the last run.  A kept run costs four loads; another is found by word in the static mask from where the run before it ended.
struct ContactWalk { long long index; int behind; };
GRK_TRANS_HD bool contact_next(const ContactMasks& m, const ContactKept& kept, const double* s, long long stride, int T, double thr, ContactWalk* w, int* lead,
                               double* t_start, double* t_end) {
    if (++w->index >= kept.runs) return false;
    if (w->index < kept.slots) {
        const double* row = kept.rows + w->index * kContactKeptCols;
        *t_start = row[0]; *t_end = row[1]; *lead = (int)row[2]; w->behind = (int)row[3];
        return true;
    }
    const long long a = track_first(m.is_static, w->behind, T);
    w->behind = contact_run_end(m.is_static, T, a);
    *lead = contact_lead_at(m, a);
    if (*lead) contact_edges(s, stride, (int)a, w->behind - 1, thr, t_start, t_end);
    return true;
}

// columns 2 .. 5
GRK_TRANS_HD void contact_counts(const ContactMasks& m, int T, double* out) {
    const long long runs = contact_runs_before(m.is_static, T), left = turn_popcount(m.lead_l, 0, T), right = turn_popcount(m.lead_r, 0, T);
    out[kContactColRuns] = (double)runs;
    out[kContactColLeft] = (double)left;
    out[kContactColRight] = (double)right;
    out[kContactColUnattributed] = (double)(runs - left - right);
}

// columns 6 .. 10: the double-support time over the attributed runs in time order
GRK_TRANS_HD void contact_support(const ContactMasks& m, const ContactKept& kept, const double* s, long long stride, int T, double thr, double fps, double* out) {
    double mean = 0., acc = 0., side[2] = {0., 0.};
    long long n = 0, n_side[2] = {0, 0};
    for (int pass = 0; pass < 2; ++pass) {
        acc = 0.;
        ContactWalk w{-1, 0};
        int lead;
        double t0, t1;
        while (contact_next(m, kept, s, stride, T, thr, &w, &lead, &t0, &t1)) {
            if (lead) {
                const double x = (t1 - t0) / fps;
                if (pass == 0) {
                    acc = acc + x; ++n;
                    const int f = lead > 0 ? 0 : 1;
                    side[f] = side[f] + x; ++n_side[f];
                } else {
                    const double d = x - mean;
                    acc = acc + d * d;
                }
            }
        }
        if (n == 0) break;
        if (pass == 0) mean = acc / (double)n;
    }
    const double none = gait_detail::nan();
    const double L = n_side[0] ? side[0] / (double)n_side[0] : none, R = n_side[1] ? side[1] / (double)n_side[1] : none;
    out[kContactColSupport] = n ? mean : none;
    out[kContactColSupportSd] = n ? __builtin_sqrt(acc / (double)n) : none;
    out[kContactColSupportL] = L;
    out[kContactColSupportR] = R;
    out[kContactColAsymmetry] = n_side[0] && n_side[1] ? (100. * __builtin_fabs(L - R)) / (0.5 * (L + R)) : none;
}

// columns 11 .. 19: three consecutive static runs led by X, the other foot, X make a stride of X; the left foot's strides first
GRK_TRANS_HD void contact_strides(const ContactMasks& m, const ContactKept& kept, const double* s, long long stride, int T, double thr, double fps, double* out) {
    struct Edge { int lead; double t0, t1; };
    double mean[6] = {0., 0., 0., 0., 0., 0.}, acc[6], sq = 0.;
    long long n = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int k = 0; k < 6; ++k) acc[k] = 0.;
        sq = 0.;
        for (int foot = 0; foot < 2; ++foot) {
            const int X = foot ? -1 : 1;
            Edge r0{0, 0., 0.}, r1{0, 0., 0.}, c{0, 0., 0.};
            ContactWalk w{-1, 0};
            while (contact_next(m, kept, s, stride, T, thr, &w, &c.lead, &c.t0, &c.t1)) {
                if (r0.lead == X && r1.lead == -X && c.lead == X) {
                    const double len = c.t0 - r0.t0;
                    if (pass == 0) {                           // the second pass needs the stride time alone: a division is the dear part of a link
                        const double x[6] = {len / fps, (r1.t1 - r0.t0) / fps, (c.t0 - r1.t1) / fps, (r1.t0 - r0.t1) / fps, (100. * (r1.t1 - r0.t0)) / len,
                                             (100. * ((r0.t1 - r0.t0) + (r1.t1 - r1.t0))) / len};
                        for (int k = 0; k < 6; ++k) acc[k] = acc[k] + x[k];
                        ++n;
                    } else {
                        const double d = len / fps - mean[0];
                        sq = sq + d * d;
                    }
                }
                r0 = r1; r1 = c;
            }
        }
        if (n == 0) break;
        if (pass == 0) for (int k = 0; k < 6; ++k) mean[k] = acc[k] / (double)n;
    }
    const double none = gait_detail::nan(), sd = n ? __builtin_sqrt(sq / (double)n) : none;
    out[kContactColStrides] = (double)n;
    out[kContactColStride] = n ? mean[0] : none;
    out[kContactColStrideSd] = sd;
    out[kContactColStance] = n ? mean[1] : none;
    out[kContactColSwing] = n ? mean[2] : none;
    out[kContactColSingle] = n ? mean[3] : none;
    out[kContactColStanceShare] = n ? mean[4] : none;
    out[kContactColSupportShare] = n ? mean[5] : none;
    out[kContactColStrideCv] = n ? (100. * sd) / mean[0] : none;
}

}  // namespace grk
