// Per-step and per-stride tables of the gait call, and bootstrap intervals of any per-step table (Efron 1979, the circular block
// bootstrap of Politis and Romano 1992, the mixer of splitmix64, Steele, Lea and Flood 2014): no HIP and nothing of the library, so
// gait_bootstrap_kernels.hip uses it on the device and the stand-alone checker tests/helpers/gait_bootstrap_check.cpp on the host.  Whoever includes
// it compiles WITHOUT fma contraction (-ffp-contract=off): every floating-point operation below rounds once, in the order the parentheses show.
// The generator is integers alone (uint64, wrapping), so it has the same bits everywhere.
//
// boot_step_rows / boot_stride_rows -- the walks of gait_steps and gait_strides (gait_events.h) and, with a not-straight mask, of turn_steps and
//                     turn_strides (gait_turns.h), RESTATED here so that the samples they add up are written down instead: the searches by word
//                     (gait_next_strike, track_first, turn_straight) are theirs, the loop around them is this header's.  That replicate 0 of the
//                     bootstrap of these rows equals those functions' columns in every bit is what pins the restatement (the identity tests).
// boot_mix / boot_stream_key / boot_replicate_key / boot_u / boot_index -- u(seed, stream, r, j) = mix(mix(mix(seed + G (stream + 1)) + G (r + 1))
//                     + G (j + 1)); index(u, n) = ((u >> 32) n) >> 32, whose bias is below n / 2^32 and is stated, not corrected.
// boot_statistics   -- mean, SD and CV of replicate r of one column's n rows: gait_strides' operations in its order, NaN rows skipped.
// boot_before / boot_quantile_rank / boot_select -- the order (value under <, then replicate number) and the element a quantile names.
// boot_rule_error   -- what a call refuses about its rule (host only; null: nothing), so that the stand-alone checker runs every refusal too.
#pragma once

#include "gait_turns.h"

namespace grk {

constexpr int kBootStepCols = 6;          // t_prev, t, landing foot (0 left, 1 right), step time, step length, step width
constexpr int kBootStrideCols = 4;        // t0, t1, foot, stride time
constexpr int kBootMaxRows = 1024;        // rows of a sequence's table, at most: a column's samples are 8 KB
constexpr int kBootMaxTableCols = 16;     // columns of a table
constexpr int kBootMaxCols = 8;           // columns resampled in one call
constexpr int kBootMaxReplicates = 4096;  // B
constexpr int kBootMaxQuantiles = 5;
constexpr int kBootMaxStream = 65535;
constexpr int kBootStats = 3;             // mean, SD, CV
constexpr unsigned long long kBootGolden = 0x9E3779B97F4A7C15ull;

// what a call of the bootstrap is told beyond its pointers; a kernel argument
struct BootRule {
    int max_rows, C, n_cols, B, block, stream, n_q;
    unsigned long long seed;
    int cols[kBootMaxCols], q[kBootMaxQuantiles];
};

// null, or what is wrong with a call's rule (host only)
inline const char* boot_rule_error(const BootRule& r) {
    if (r.max_rows < 1 || r.max_rows > kBootMaxRows) return "max_rows outside [1, 1024]";
    if (r.C < 1 || r.C > kBootMaxTableCols) return "C outside [1, 16]";
    if (r.n_cols < 1 || r.n_cols > kBootMaxCols) return "n_cols outside [1, 8]";
    for (int k = 0; k < r.n_cols; ++k)
        if (r.cols[k] < 0 || r.cols[k] >= r.C) return "column outside [0, C)";
    if (r.B < 1 || r.B > kBootMaxReplicates) return "B outside [1, 4096]";
    if (r.block < 1 || r.block > kBootMaxRows) return "block outside [1, 1024]";
    if (r.stream < 0 || r.stream > kBootMaxStream) return "stream outside [0, 65535]";
    if (r.n_q < 0 || r.n_q > kBootMaxQuantiles) return "n_q outside [0, 5]";
    for (int k = 0; k < r.n_q; ++k)
        if (r.q[k] < 0 || r.q[k] > 10000) return "quantile outside [0, 10000] basis points";
    return nullptr;
}
static_assert(kBootMaxRows == 1024 && kBootMaxTableCols == 16 && kBootMaxCols == 8 && kBootMaxReplicates == 4096 && kBootMaxQuantiles == 5 && kBootMaxStream == 65535,
              "boot_rule_error's messages name the limits");

// The steps of one sequence in time order: consecutive strikes of gait_next_strike on different feet and, where ns (the not-straight mask) is not
// null, with no frame of [pt, t] set in it.  rows: the gait call's (T,7) per-frame rows.  Row i < max_rows of table (max_rows,6) is written for step
// i; the steps past it are counted, not stored.  Returns the count.
GRK_TRANS_HD long long boot_step_rows(const unsigned long long* hs_l, const unsigned long long* hs_r, const unsigned long long* ns, int T, const double* rows,
                                      double fps, int max_rows, double* table) {
    long long n = 0;
    int t = -1, foot = 1, pt = -1, pf = -1;
    while (gait_next_strike(hs_l, hs_r, T, &t, &foot)) {
        if (pt >= 0 && pf != foot && (!ns || turn_straight(ns, pt, t))) {
            if (n < max_rows) {
                const double* row = rows + (long long)t * kGaitFrameCols;
                double* out = table + n * kBootStepCols;
                out[0] = (double)pt;
                out[1] = (double)t;
                out[2] = (double)foot;
                out[3] = (double)(t - pt) / fps;
                out[4] = row[foot] - row[1 - foot];
                out[5] = row[4];
            }
            ++n;
        }
        pt = t; pf = foot;
    }
    return n;
}

// The strides of one sequence: the left foot's in time order, then the right foot's, as gait_strides adds them
GRK_TRANS_HD long long boot_stride_rows(const unsigned long long* hs_l, const unsigned long long* hs_r, const unsigned long long* ns, int T, double fps, int max_rows,
                                        double* table) {
    long long n = 0;
    for (int foot = 0; foot < 2; ++foot) {
        const unsigned long long* words = foot ? hs_r : hs_l;
        long long prev = -1;
        for (long long t = track_first(words, 0, T); t >= 0; t = track_first(words, t + 1, T)) {
            if (prev >= 0 && (!ns || turn_straight(ns, prev, t))) {
                if (n < max_rows) {
                    double* out = table + n * kBootStrideCols;
                    out[0] = (double)prev;
                    out[1] = (double)t;
                    out[2] = (double)foot;
                    out[3] = (double)(t - prev) / fps;
                }
                ++n;
            }
            prev = t;
        }
    }
    return n;
}

GRK_TRANS_HD unsigned long long boot_mix(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
GRK_TRANS_HD unsigned long long boot_stream_key(unsigned long long seed, int stream) { return boot_mix(seed + kBootGolden * ((unsigned long long)stream + 1ull)); }
GRK_TRANS_HD unsigned long long boot_replicate_key(unsigned long long stream_key, int r) { return boot_mix(stream_key + kBootGolden * ((unsigned long long)r + 1ull)); }
GRK_TRANS_HD unsigned long long boot_u(unsigned long long replicate_key, unsigned long long j) { return boot_mix(replicate_key + kBootGolden * (j + 1ull)); }
GRK_TRANS_HD int boot_index(unsigned long long u, int n) { return (int)(((u >> 32) * (unsigned long long)n) >> 32); }

// out = [mean, SD, CV] of replicate r of x[0, n): replicate 0 is the sample itself, replicate r >= 1 reads x[(index(u(.., r, p / block), n) + p % block)
// % n] at p = 0 .. n - 1.  The draw of a block is made once, where p % block == 0; start < n and p % block <= p < n, so one subtraction is the `% n`.
// The second pass makes the same draws again: no index is stored.
GRK_TRANS_HD void boot_statistics(const double* x, int n, int block, unsigned long long stream_key, int r, double* out) {
    const unsigned long long key = boot_replicate_key(stream_key, r);
    double mean = 0., acc = 0.;
    long long m = 0;
    for (int pass = 0; pass < 2; ++pass) {
        acc = 0.;
        int start = 0, o = block;
        unsigned long long j = 0;
        for (int p = 0; p < n; ++p) {
            int at = p;
            if (r > 0) {
                if (o == block) { start = boot_index(boot_u(key, j), n); ++j; o = 0; }
                at = start + o;
                if (at >= n) at -= n;
                ++o;
            }
            const double v = x[at];
            if (v != v) continue;
            if (pass == 0) { acc = acc + v; ++m; }
            else { const double d = v - mean; acc = acc + d * d; }
        }
        if (m == 0) break;
        if (pass == 0) mean = acc / (double)m;
    }
    const double none = gait_detail::nan(), sd = m ? __builtin_sqrt(acc / (double)m) : none;
    out[0] = m ? mean : none;
    out[1] = sd;
    out[2] = m ? (100. * sd) / mean : none;
}

// whether replicate j with the value b stands in front of replicate i with the value a: by the value under <, then by the number.  Neither is NaN
// where it matters: a NaN b is in front of nothing (both comparisons are false), and a NaN a is never asked about.
GRK_TRANS_HD bool boot_before(double b, int j, double a, int i) { return b < a || (b == a && j < i); }

// the rank a quantile of q basis points names among f ordered values, f >= 1
GRK_TRANS_HD int boot_quantile_rank(int q, int f) { return (int)(((long long)q * (long long)(f - 1)) / 10000); }

// v[0, B): one statistic of the replicates 1 .. B.  out = [f, the n_q quantiles]: f the count of values that are not NaN, each quantile the value
// whose rank among them is boot_quantile_rank (every rank is held by exactly one replicate), NaN where f = 0.  The host's statement of what the
// kernel does with a lane per replicate.
GRK_TRANS_HD void boot_select(const double* v, int B, const int* q, int n_q, double* out) {
    int f = 0;
    for (int i = 0; i < B; ++i) f += !(v[i] != v[i]);
    out[0] = (double)f;
    for (int k = 0; k < n_q; ++k) out[1 + k] = gait_detail::nan();
    for (int i = 0; i < B && f > 0; ++i) {
        if (v[i] != v[i]) continue;
        int rank = 0;
        for (int j = 0; j < B; ++j) rank += boot_before(v[j], j, v[i], i);
        for (int k = 0; k < n_q; ++k)
            if (rank == boot_quantile_rank(q[k], f)) out[1 + k] = v[i];
    }
}

}  // namespace grk
