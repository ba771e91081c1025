// csrc/gait_recurrence.h on the host: a stand-alone program (its own main, no HIP, nothing of the library but that header and the ones it includes),
// built with AddressSanitizer and UBSan by tests/test_recurrence_host_cpu.py and run directly on one file per case, which the test writes: the inputs
// of ONE sequence and what pipeline.gait_recurrence (or, of a case on signals, pipeline.gait_recurrence_counts) made of them with sigma = 0.  The
// program runs the chain the kernels run -- reg_frame, ent_diff, ent_spread, rec_eps2, rec_lane_walk with loops over parts and lanes where the device
// has workgroups and lanes, the parts added in part order -- in buffers of exactly the sizes the call states, so that an index outside them is
// caught.  The offsets are dealt as the sequence's own rec_parts deals them, and again to 1 and to kRecMaxParts parts: the sums cannot tell.  Every
// integer and every bit must be equal (a NaN equals a NaN).  A case that the rules refuse is answered with a line "refused <file>: <why>", in the
// words the library and the statement use.
//
// The file, little-endian: int32 [T, J, has_trans, has_exclude, derivative, dim, lag, theiler, has_data], int32 table[8], float64 radius; then, where
// has_data, float32 joints[T J 3] or, where J is 0, float64 signals[T 4]; float64 trans[T 3] and int32 exclude[T] where stated; then the expected
// float64 per_frame[T 4] (not where J is 0), float64 per_seq[4 5], int64 hist[4 255], int64 counts[4 6].  Prints what differs, and "ok" as its last
// line if nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gait_recurrence.h"

using namespace grk;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

template <class V>
static bool read_n(std::FILE* f, std::vector<V>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(V), n, f) == n;
}

static bool same(double a, double b) {
    if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
    return std::memcmp(&a, &b, sizeof a) == 0;
}

// a workgroup's histogram: exactly kRecBins bins on the heap
struct Bins {
    std::vector<unsigned> h = std::vector<unsigned>(kRecBins, 0u);
    void add(int bin) { ++h.at((size_t)bin); }
};

// the two kernels behind the spread for one channel, the offsets dealt to `parts` workgroups; y: exactly T values
static void channel(const std::vector<double>& y, const RecRule& r, double rr, int parts, long long* hist, long long* counts) {
    const int T = (int)y.size(), M = rec_points(T, r);
    const double eps2 = rec_eps2(rr, r.dim);
    for (int b = 0; b < kRecBins; ++b) hist[b] = 0;
    RecSums all;
    for (int p = 0; p < parts; ++p) {                           // a workgroup each, added in part order
        Bins bins;
        RecSums c;
        for (int lane = 0; lane < kRecPartOffsets; ++lane) rec_lane_walk(y.data(), M, r, p, parts, lane, eps2, rr > 0., &c, bins);
        for (int b = 0; b < kRecBins; ++b) hist[b] += bins.h[b];
        all.comparable += c.comparable;
        all.recurrent += c.recurrent;
        all.long_lines += c.long_lines;
        all.long_points += c.long_points;
        all.longest = c.longest > all.longest ? c.longest : all.longest;
    }
    long long points = 0;
    for (int i = 0; i < M; ++i) points += rec_point_valid(y.data(), i, r.dim, r.lag);
    counts[0] = points;
    counts[1] = all.comparable;
    counts[2] = all.recurrent;
    counts[3] = all.long_lines;
    counts[4] = all.long_points;
    counts[5] = all.longest;
}

static int check_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); ++failures; return 1; }
    std::vector<int32_t> head, table, exclude;
    std::vector<double> radius, signals, trans, want_frame, want_seq;
    std::vector<long long> want_hist, want_counts;
    std::vector<float> joints;
    bool ok = read_n(f, head, 9) && read_n(f, table, 8) && read_n(f, radius, 1);
    if (!ok) { std::printf("%s: short header\n", path); std::fclose(f); ++failures; return 1; }
    const int T = head[0], J = head[1];
    const RecRule r{head[4], head[5], head[6], head[7], radius[0]};
    const int off[2] = {0, T};
    if (const char* why = rec_rule_error(r)) {
        EXPECT(!head[8], "%s: its rule is refused: %s", path, why);
        std::printf("refused %s: %s\n", path, why);
        std::fclose(f);
        return 0;
    }
    if (ent_long_sequence(off, 1) >= 0) {
        EXPECT(!head[8], "%s: its length is refused", path);
        std::printf("refused %s: sequence %d has %d frames, more than %d (the work is quadratic in them)\n", path, ent_long_sequence(off, 1), T, kEntMaxFrames);
        std::fclose(f);
        return 0;
    }
    EXPECT(head[8], "%s: a case without data is not refused", path);
    if (!head[8]) { std::fclose(f); return 1; }
    ok = (J ? read_n(f, joints, (size_t)T * J * 3) : read_n(f, signals, (size_t)T * kRegChannels)) && read_n(f, trans, head[2] ? (size_t)T * 3 : 0) &&
         read_n(f, exclude, head[3] ? (size_t)T : 0) && read_n(f, want_frame, J ? (size_t)T * kRegChannels : 0) && read_n(f, want_seq, kRegChannels * kRecSeqCols) &&
         read_n(f, want_hist, kRegChannels * kRecBins) && read_n(f, want_counts, kRegChannels * kRecCountCols);
    std::fclose(f);
    if (!ok) { std::printf("%s: short file\n", path); ++failures; return 1; }

    const int before = failures;
    if (J) {
        int tab[kGaitTable];
        for (int k = 0; k < kGaitTable; ++k) tab[k] = table[k];
        signals.assign((size_t)T * kRegChannels, -7.);
        for (int t = 0; t < T; ++t)
            reg_frame(joints.data() + (size_t)t * J * 3, tab, head[2] ? trans.data() + (size_t)t * 3 : nullptr, signals.data() + (size_t)t * kRegChannels);
        for (size_t i = 0; i < signals.size(); ++i)
            EXPECT(same(signals[i], want_frame[i]), "%s: per_frame[%zu][%zu] = %.17g, not %.17g", path, i / kRegChannels, i % kRegChannels, signals[i], want_frame[i]);
    }
    const int own = rec_parts(rec_points(T, r));
    for (int ch = 0; ch < kRegChannels; ++ch) {
        std::vector<double> y((size_t)T);
        for (int t = 0; t < T; ++t) y[t] = ent_diff(signals.data() + ch, head[3] ? exclude.data() : nullptr, t, T, r.derivative);
        double seq[kRecSeqCols];
        ent_spread(y.data(), T, r.radius, seq);
        seq[4] = rec_eps2(seq[3], r.dim);
        for (int k = 0; k < kRecSeqCols; ++k)
            EXPECT(same(seq[k], want_seq[ch * kRecSeqCols + k]), "%s: per_seq[%d][%d] = %.17g, not %.17g", path, ch, k, seq[k], want_seq[ch * kRecSeqCols + k]);
        for (int parts : {own, 1, kRecMaxParts}) {
            std::vector<long long> hist(kRecBins, -7), counts(kRecCountCols, -7);
            channel(y, r, seq[3], parts, hist.data(), counts.data());
            for (int b = 0; b < kRecBins; ++b)
                EXPECT(hist[b] == want_hist[ch * kRecBins + b], "%s: %d parts: hist[%d][%d] = %lld, not %lld", path, parts, ch, b, hist[b], want_hist[ch * kRecBins + b]);
            for (int k = 0; k < kRecCountCols; ++k)
                EXPECT(counts[k] == want_counts[ch * kRecCountCols + k], "%s: %d parts: counts[%d][%d] = %lld, not %lld", path, parts, ch, k, counts[k],
                       want_counts[ch * kRecCountCols + k]);
        }
    }
    return failures - before;
}

// what no file reaches: the rule at its limits, the parts of every length, and the circular offsets of M = 1 .. 12 against the plain triangle
static void check_rules() {
    const RecRule limits[] = {{1, 5, 2, 8, 0.8}, {0, 2, 1, 0, 1e-300}, {2, 8, 16, 4096, 10.}};
    for (const auto& r : limits) EXPECT(rec_rule_error(r) == nullptr, "a rule at the limits is refused: %s", rec_rule_error(r));
    const double inf = HUGE_VAL;
    const struct { RecRule r; const char* word; } bad[] = {
        {{-1, 5, 2, 8, 0.8}, "derivative"}, {{3, 5, 2, 8, 0.8}, "derivative"}, {{1, 1, 2, 8, 0.8}, "dim"}, {{1, 9, 2, 8, 0.8}, "dim"}, {{1, 5, 0, 8, 0.8}, "lag"},
        {{1, 5, 17, 8, 0.8}, "lag"}, {{1, 5, 2, -1, 0.8}, "theiler"}, {{1, 5, 2, 4097, 0.8}, "theiler"}, {{1, 5, 2, 8, 0.}, "radius"}, {{1, 5, 2, 8, -1.}, "radius"},
        {{1, 5, 2, 8, 10.5}, "radius"}, {{1, 5, 2, 8, inf}, "radius"}, {{1, 5, 2, 8, std::nan("")}, "radius"}};
    for (const auto& b : bad) {
        const char* why = rec_rule_error(b.r);
        EXPECT(why && std::strstr(why, b.word) == why, "a bad %s is %s", b.word, why ? why : "not refused");
    }
    EXPECT(rec_points(400, limits[0]) == 392 && rec_points(8, limits[0]) == 0 && rec_points(kEntMaxFrames, limits[2]) == kEntMaxFrames - kStabMaxSpan, "rec_points");
    EXPECT(rec_parts(0) == 1 && rec_parts(1) == 1 && rec_parts(513) == 1 && rec_parts(514) == 2 && rec_parts(8192) == 16 && rec_parts(8194) == 16 &&
           rec_parts(kEntMaxFrames) == kRecMaxParts, "rec_parts");
    EXPECT(rec_offsets(0) == 0 && rec_offsets(1) == 0 && rec_offsets(2) == 1 && rec_offsets(3) == 1 && rec_offsets(4) == 2, "rec_offsets");
    EXPECT(same(rec_eps2(0.5, 2), 0.5) && std::isnan(rec_eps2(std::nan(""), 5)) && rec_eps2(0., 8) == 0., "rec_eps2");
    // a signal of small integers with a hole, dim 2, lag 1: every M from 1 to 12, every Theiler window up to M, 1 and 16 parts
    const double nan = std::nan("");
    const double x[13] = {0, 1, 0, 1, 1, 0, nan, 0, 0, 1, 0, 0, 1};
    for (int M = 1; M <= 12; ++M)
        for (int w = 0; w <= M; ++w) {
            const RecRule r{0, 2, 1, w, 1.};
            const std::vector<double> y(x, x + M + 1);
            const double rr = 0.75, eps2 = rec_eps2(rr, 2);     // 1.125, exactly: points that differ in one value recur, in both do not
            long long want[kRecCountCols] = {0, 0, 0, 0, 0, 0};
            std::vector<long long> want_hist(kRecBins, 0);
            for (int i = 0; i < M; ++i) want[0] += rec_point_valid(y.data(), i, 2, 1);
            for (int s = w + 1; s < M; ++s) {
                int run = 0;
                for (int i = 0; i + s <= M; ++i) {              // one step past the diagonal's end closes its last line
                    bool hit = false;
                    if (i + s < M && rec_point_valid(y.data(), i, 2, 1) && rec_point_valid(y.data(), i + s, 2, 1)) {
                        ++want[1];
                        const double a = y[i] - y[i + s], b = y[i + 1] - y[i + s + 1];
                        hit = a * a + b * b <= eps2;
                    }
                    if (hit) { ++want[2]; ++run; continue; }
                    if (run) { ++want_hist[(size_t)run - 1]; want[5] = run > want[5] ? run : want[5]; }
                    run = 0;
                }
            }
            for (int parts : {1, kRecMaxParts}) {
                long long counts[kRecCountCols];
                std::vector<long long> hist(kRecBins, -7);
                channel(y, r, rr, parts, hist.data(), counts);
                for (int k = 0; k < kRecCountCols; ++k) EXPECT(counts[k] == want[k], "M %d, theiler %d, %d parts: counts[%d] = %lld, not %lld", M, w, parts, k, counts[k], want[k]);
                for (int b = 0; b < kRecBins; ++b) EXPECT(hist[b] == want_hist[b], "M %d, theiler %d, %d parts: hist[%d] = %lld, not %lld", M, w, parts, b, hist[b], want_hist[b]);
            }
        }
}

int main(int argc, char** argv) {
    check_rules();
    for (int i = 1; i < argc; ++i) check_file(argv[i]);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
