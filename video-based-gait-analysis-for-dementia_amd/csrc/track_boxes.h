// Per-frame boxes from 2D joints in float64 (the reference's lib/utils/smooth_bbox.py): no HIP and nothing of the library, so
// track_kernels.hip uses it on the device and the stand-alone checker tests/helpers/track_boxes_check.cpp on the host.  Whoever includes it compiles
// WITHOUT fma contraction (-ffp-contract=off): every operation below rounds once, in the order the parentheses show.
//
// track_frame    -- kp_to_bbox_param(squared=True): a joint counts where score > vis_thresh (false for a NaN score); min and max of x and of y over
//                   those joints, height = sqrt(dx^2 + dy^2); detected where a joint counts, every counting x and y is finite, and height >= 0.5 and
//                   height - height == 0 -- all of them comparisons that are FALSE FOR NaN (and the last for an infinity too), so a frame whose min,
//                   max or height is not finite has no detection and is interpolated like any other dead frame (the reference would carry the NaN
//                   on).  Then [cx, cy, scale] = [(min_x + max_x) / 2, (min_y + max_y) / 2, 150 / height].
// track_first / track_last / track_prev / track_next -- searches in a bitmask of detected frames, bit g & 63 of word g >> 6 for frame g, BY WORD:
//                   a dead stretch of n frames costs n / 64 steps, not n.  prev / next assume that a detected frame exists on that side (the fill
//                   runs inside [start, end) alone, whose ends are detected).
// track_fill     -- frame i of a gap between two detected values by translation3_fill, the statement that equals numpy.linspace bit for bit; the
//                   reference interpolates column by column (scalars), so the zero-step branch is taken per column: the column is handed over alone.
// track_reflect  -- scipy.ndimage's mode 'reflect' (d c b a | a b c d | d c b a): index j of the extension of [0, n), period 2n, for any j.
// track_median   -- scipy.signal.medfilt at position i of x[0, n): the window of k values, zeros (or with `edge` the first / last value) outside
//                   [0, n), and of them the one whose RANK is k / 2 -- rank = the values below it plus the equal ones before it in the window.  A
//                   selection, no arithmetic: it is the middle of the sorted window, exactly.
// track_gauss    -- scipy.ndimage.gaussian_filter1d at position l with the weights w[0 .. r] (w[i] for offsets -i and +i): the centre term first,
//                   then the pairs (x[l - i] + x[l + i]) * w[i] from i = r down to 1, one sum -- the order of scipy's own loop for a symmetric
//                   kernel (with scipy's weights the result equals scipy's bit for bit); the extension is track_reflect.
#pragma once

#include "translation3.h"

namespace grk {

constexpr int kTrackDetected = 0, kTrackInterpolated = 1, kTrackOutside = 2, kTrackBadScale = 3;
constexpr int kTrackPadZero = 0, kTrackPadEdge = 1;
constexpr double kTrackMinHeight = 0.5, kTrackPersonPixels = 150.;

// rows: the frame's (K,3) float64 rows (x, y, score); out = [cx, cy, scale] where detected, untouched otherwise
GRK_TRANS_HD bool track_frame(const double* rows, int K, double vis_thresh, double* out) {
    using translation_detail::finite;
    double x0 = 0., x1 = 0., y0 = 0., y1 = 0.;
    bool any = false, good = true;
    for (int j = 0; j < K; ++j) {
        const double x = rows[3 * j], y = rows[3 * j + 1], s = rows[3 * j + 2];
        if (!(s > vis_thresh)) continue;
        good = good && finite(x) && finite(y);
        if (!any) { x0 = x1 = x; y0 = y1 = y; any = true; continue; }
        x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1;
        y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
    }
    if (!any || !good) return false;
    const double dx = x1 - x0, dy = y1 - y0;
    const double height = __builtin_sqrt(dx * dx + dy * dy);
    if (!(height >= kTrackMinHeight) || !finite(height)) return false;
    out[0] = (x0 + x1) / 2.;
    out[1] = (y0 + y1) / 2.;
    out[2] = kTrackPersonPixels / height;
    return true;
}

// the first / last detected frame of [lo, hi), or -1
GRK_TRANS_HD long long track_first(const unsigned long long* words, long long lo, long long hi) {
    for (long long w = lo >> 6; w <= (hi - 1) >> 6 && lo < hi; ++w) {
        unsigned long long v = words[w];
        if (w == lo >> 6) v &= ~0ull << (lo & 63);
        if (v) { const long long g = w * 64 + __builtin_ctzll(v); return g < hi ? g : -1; }
    }
    return -1;
}
GRK_TRANS_HD long long track_last(const unsigned long long* words, long long lo, long long hi) {
    for (long long w = (hi - 1) >> 6; lo < hi && w >= lo >> 6; --w) {
        unsigned long long v = words[w];
        if (w == (hi - 1) >> 6 && (hi & 63)) v &= ~(~0ull << (hi & 63));
        if (v) { const long long g = w * 64 + 63 - __builtin_clzll(v); return g >= lo ? g : -1; }
    }
    return -1;
}
// the nearest detected frame below / above g; one exists
GRK_TRANS_HD long long track_prev(const unsigned long long* words, long long g) {
    long long w = g >> 6;
    unsigned long long v = (g & 63) ? words[w] & ~(~0ull << (g & 63)) : 0ull;
    while (!v) v = words[--w];
    return w * 64 + 63 - __builtin_clzll(v);
}
GRK_TRANS_HD long long track_next(const unsigned long long* words, long long g) {
    long long w = g >> 6;
    unsigned long long v = (g & 63) != 63 ? words[w] & (~0ull << ((g & 63) + 1)) : 0ull;
    while (!v) v = words[++w];
    return w * 64 + __builtin_ctzll(v);
}

// numpy.linspace(prev, next, gap + 2)[i] of two scalars, 1 <= i <= gap
GRK_TRANS_HD double track_fill(double prev, double next, int gap, int i) {
    const double p[3] = {prev, prev, prev}, n[3] = {next, next, next};
    double out[3];
    translation3_fill(p, n, gap, i, out);
    return out[0];
}

GRK_TRANS_HD int track_reflect(long long j, int n) {
    const long long period = 2ll * n;
    long long m = j % period;
    if (m < 0) m += period;
    return (int)(m < n ? m : period - 1 - m);
}

GRK_TRANS_HD double track_median(const double* x, int n, int i, int k, int pad) {
    const int half = k / 2;
    auto at = [&](int m) {                                     // window entry m = 0 .. k - 1; no branch: the load is of a clamped index, then a select
        const int j = i - half + m;
        const double v = x[j < 0 ? 0 : j >= n ? n - 1 : j];
        return (j >= 0 && j < n) || pad == kTrackPadEdge ? v : 0.;
    };
    for (int a = 0; a < k; ++a) {
        const double v = at(a);
        int rank = 0;
        for (int b = 0; b < k; ++b) {
            const double u = at(b);
            rank += (u < v || (u == v && b < a)) ? 1 : 0;
        }
        if (rank == half) return v;
    }
    return at(half);                                           // not reached for finite values: the ranks are a permutation of 0 .. k - 1
}

GRK_TRANS_HD double track_gauss(const double* x, int n, int l, const double* w, int r) {
    double acc = x[l] * w[0];
    for (int i = r; i >= 1; --i) acc = acc + (x[track_reflect((long long)l - i, n)] + x[track_reflect((long long)l + i, n)]) * w[i];
    return acc;
}

}  // namespace grk
