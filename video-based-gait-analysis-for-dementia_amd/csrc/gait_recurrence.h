// Recurrence quantification of four body signals in float64 and integers (Webber and Zbilut, J. Appl. Physiol. 76, 1994; Marwan et al.,
// Phys. Rep. 438, 2007): every pair of points of the delay-embedded signal against one radius, and the runs of recurrent pairs along each diagonal
// counted by their length.  No HIP and nothing of the library, so gait_recurrence_kernels.hip uses it on the device and the stand-alone checker
// tests/helpers/gait_recurrence_check.cpp on the host.  Whoever includes it compiles WITHOUT fma contraction (-ffp-contract=off): every operation
// below rounds once, in the order the parentheses show.  The four signals, their validity, the differenced signal y and its spread are
// gait_regularity.h's and gait_entropy.h's (reg_frame, reg_valid, ent_diff, ent_spread), the embedding and the distance gait_stability.h's
// (stab_points with horizon 0, stab_dist2): an invalid y is NaN and "valid" is "finite".
//
// rec_eps2         -- the squared radius of a call: (r r) dim.
// rec_pair         -- ONE pair of points: whether it is comparable and whether it is recurrent (D2 finite and at most eps2).
// rec_offsets      -- how many circular offsets a sequence of M points has; rec_parts -- over how many workgroups they are dealt.
// rec_offset_walk  -- ONE circular offset s: the M pairs (i, (i + s) mod M) in rising i, that is diagonal s and behind the wrap diagonal M - s, with
//                     the counts and the lines of both.  On the device a lane owns an offset, in the checker a loop walks them.
// rec_rule_error   -- what a call refuses about its scalars (host only).  A sequence too long is ent_long_sequence's.
#pragma once

#include "gait_stability.h"

namespace grk {

constexpr int kRecBins = 255;             // hist[l - 1]: the lines of length l = 1 .. 255; longer ones are counted and summed
constexpr int kRecSeqCols = 5;            // n, mu, SD, r, eps2
constexpr int kRecCountCols = 6;          // points, comparable, recurrent, long_lines, long_points, longest
constexpr int kRecSumCols = 5;            // what the walk of an offset adds to: the counts without `points`
constexpr int kRecPartOffsets = 256;      // offsets of one round of a part: a lane each
constexpr int kRecMaxParts = 16;          // workgroups of one (sequence, channel)
constexpr int kRecPartCols = kRecBins + kRecSumCols;      // int64 values of one workgroup's partial in the call's scratch
constexpr double kRecMaxRadius = 10.;

struct RecRule { int derivative, dim, lag, theiler; double radius; };

// null, or what is wrong with a call's scalars: the refusals of DESIGN 4.20 beyond those of every call over sequences (host only)
inline const char* rec_rule_error(const RecRule& r) {
    if (r.derivative < 0 || r.derivative > 2) return "derivative outside [0, 2]";
    if (r.dim < 2 || r.dim > kStabMaxDim) return "dim outside [2, 8]";
    if (r.lag < 1 || r.lag > kStabMaxLag) return "lag outside [1, 16]";
    if (r.theiler < 0 || r.theiler > kStabMaxTheiler) return "theiler outside [0, 4096]";
    if (!translation_detail::finite(r.radius) || !(r.radius > 0.) || !(r.radius <= kRecMaxRadius)) return "radius must be finite and within (0, 10]";
    return nullptr;
}
static_assert(kStabMaxDim == 8 && kStabMaxLag == 16 && kStabMaxTheiler == 4096 && kRecMaxRadius == 10., "rec_rule_error's messages name the limits");
static_assert(kRecBins == 255, "DESIGN 4.20 and pipeline.RECURRENCE_BINS name it");

// r: ent_spread's fourth column.  NaN stays NaN, and a standing body's 0 stays 0: the walk is told r > 0 beside it (`on`), and eps2 alone decides nothing
GRK_TRANS_HD double rec_eps2(double r, int dim) { return (r * r) * (double)dim; }

// the points of a sequence of T frames: stab_points with no horizon
GRK_TRANS_HD int rec_points(int T, const RecRule& r) {
    const StabRule s{r.derivative, r.dim, r.lag, r.theiler, 0};
    return stab_points(T, s).M;
}

// what D2 is compared with: eps2, or the largest finite double where eps2 is infinite, so that an infinite D2 never recurs and every finite one does
GRK_TRANS_HD double rec_limit(double eps2) { return eps2 > 1.7976931348623157e308 ? 1.7976931348623157e308 : eps2; }

// a: the DIM values of one point; y: the first value of the other, whose next lie `lag` apart; limit: rec_limit(eps2); on: r > 0.  Every value is finite
// or NaN, so D2 is NaN exactly where one of the 2 DIM values is invalid (differences, squares and sums of finite values are finite or +inf, never NaN):
// D2 == D2 IS the validity of both points, and an infinite D2 is comparable and not recurrent.  & and not &&, as in stab_scan: no branch parts one
// pair from the next
template <int DIM>
GRK_TRANS_HD void rec_pair(const double* a, const double* y, int lag, double limit, bool on, bool* comparable, bool* recurrent) {
    const double d2 = stab_dist2<DIM>(a, y, lag);
    *comparable = d2 == d2;
    *recurrent = on & (d2 <= limit);
}

GRK_TRANS_HD int rec_offsets(int M) { return M > 0 ? M / 2 : 0; }      // s = 1 .. (M - 1) div 2, and M / 2 where M is even

GRK_TRANS_HD int rec_parts(int M) {
    const int p = (rec_offsets(M) + kRecPartOffsets - 1) / kRecPartOffsets;
    return p < 1 ? 1 : p > kRecMaxParts ? kRecMaxParts : p;
}

// what the offsets of a lane, a workgroup or a sequence add up to: sums, and `longest` a maximum
struct RecSums {
    long long comparable = 0, recurrent = 0, long_lines = 0, long_points = 0;
    int longest = 0;
};

// a line of `len` >= 1 pairs has ended.  Bins: add(bin) adds one line to bin 0 .. kRecBins - 1
template <class Bins>
GRK_TRANS_HD void rec_line(int len, RecSums* c, Bins& bins) {
    const bool is_long = len > kRecBins;
    if (!is_long) bins.add(len - 1);
    c->long_lines += is_long;
    c->long_points += is_long ? len : 0;
    c->longest = len > c->longest ? len : c->longest;
}

// y: the sequence's T = M + span values; 1 <= s <= rec_offsets(M).  Step i pairs point i with point j = (i + s) mod M: while i < M - s that is the pair
// (i, i + s) of diagonal s, behind the wrap the pair (i + s - M, i) of diagonal M - s, both in rising first index.  Offset M / 2 of an even M walks its
// first half only: the second would be the same diagonal again.  The run is CLOSED AT THE WRAP: the two diagonals are different lines.  The Theiler
// test takes the true distance of the two points, s or M - s.  Every index is bounded without the data: i < M and j < M, so i + span < T and
// j + span < T.  The pair's loads and distance do not depend on the run before it: the run is chosen, not branched on, and only a line's end -- rare
// beside the pairs -- is a branch
template <int DIM, class Bins>
GRK_TRANS_HD void rec_offset_walk(const double* y, int M, const RecRule& r, int s, double eps2, bool on, RecSums* c, Bins& bins) {
    const double limit = rec_limit(eps2);
    const int wrap = M - s, steps = 2 * s == M ? s : M;
    const bool near_ok = s > r.theiler, far_ok = wrap > r.theiler;
    if (!far_ok) return;                                        // s <= M - s: no pair of this offset passes the Theiler test
    int run = 0;
    long long comparable = 0, recurrent = 0;
    GRK_STAB_UNROLL4
    for (int i = 0; i < steps; ++i) {
        const bool behind = i >= wrap;
        const int j = behind ? i - wrap : i + s;
        double a[DIM];
        for (int k = 0; k < DIM; ++k) a[k] = y[i + k * r.lag];
        bool cmp, rec;
        rec_pair<DIM>(a, y + j, r.lag, limit, on, &cmp, &rec);
        const bool counted = behind ? far_ok : near_ok;
        cmp = cmp & counted;
        rec = rec & counted;
        comparable += cmp;
        recurrent += rec;
        const bool ends = (i == wrap) | !rec;
        const int closed = ends ? run : 0;
        run = rec ? (i == wrap ? 1 : run + 1) : 0;
        if (closed > 0) rec_line(closed, c, bins);
    }
    if (run > 0) rec_line(run, c, bins);
    c->comparable += comparable;
    c->recurrent += recurrent;
}

// the same with dim a variable
template <class Bins>
GRK_TRANS_HD void rec_offset_walk_dim(const double* y, int M, const RecRule& r, int s, double eps2, bool on, RecSums* c, Bins& bins) {
    switch (r.dim) {
        case 2: rec_offset_walk<2>(y, M, r, s, eps2, on, c, bins); break;
        case 3: rec_offset_walk<3>(y, M, r, s, eps2, on, c, bins); break;
        case 4: rec_offset_walk<4>(y, M, r, s, eps2, on, c, bins); break;
        case 5: rec_offset_walk<5>(y, M, r, s, eps2, on, c, bins); break;
        case 6: rec_offset_walk<6>(y, M, r, s, eps2, on, c, bins); break;
        case 7: rec_offset_walk<7>(y, M, r, s, eps2, on, c, bins); break;
        default: rec_offset_walk<8>(y, M, r, s, eps2, on, c, bins); break;
    }
}

// the offsets of part p of `parts`, lane by lane and round by round, as rec_pairs_kernel deals them: s = 1 + p 256 + lane + round (parts 256)
template <class Bins>
GRK_TRANS_HD void rec_lane_walk(const double* y, int M, const RecRule& r, int p, int parts, int lane, double eps2, bool on, RecSums* c, Bins& bins) {
    const int n_off = rec_offsets(M);
    for (int s = 1 + p * kRecPartOffsets + lane; s <= n_off; s += parts * kRecPartOffsets) rec_offset_walk_dim(y, M, r, s, eps2, on, c, bins);
}

// whether point i of y is valid: its dim values all are
GRK_TRANS_HD bool rec_point_valid(const double* y, int i, int dim, int lag) {
    bool ok = true;
    for (int k = 0; k < dim; ++k) ok = ok & translation_detail::finite(y[i + k * lag]);
    return ok;
}

}  // namespace grk
