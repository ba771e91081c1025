// csrc/gait_balance.h on the host: a stand-alone program (its own main, no HIP, nothing of the library but that header and the ones it includes),
// built with AddressSanitizer and UBSan by tests/test_balance_host_cpu.py and run directly on one file per case, which the test writes: the inputs of
// ONE sequence and what pipeline.gait_balance (or, of a case on rel, pipeline.gait_balance_steps) made of them.  The program runs the chain the
// kernels run -- balance_com per frame, the two heel-strike bitmasks and the marks in front of each word, the list of marks, balance_pair per pair,
// balance_chain, balance_stride per step, the step table, balance_row, balance_path per frame -- in buffers of exactly the sizes the call states, so
// that an index outside them is caught.  Every bit must be equal (a NaN equals a NaN).
//
// The file, little-endian: int32 [T, J, n_seg, window, settle, max_step, max_steps], int32 table[8], float64 [fps, gravity], int32 segments[n_seg 2],
// float64 weights[n_seg 2], then float32 joints[T J 3] or, where J is 0, float64 rel[T 9]; int32 events[T]; then the expected float64 rel[T 9] (not
// where J is 0), per_frame[T 8], steps[max_steps 15], per_seq[24].  Prints what differs, and "ok" as its last line if nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gait_balance.h"

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

// the stages of balance_steps_kernel and balance_path_kernel, a loop where the device has a lane each
static void sequence(int T, const BalanceRule& r, const double* rel, const int32_t* events, double* per_frame, double* steps, double* out) {
    const int words = ((T - 1) >> 6) + 1;
    std::vector<unsigned long long> left((size_t)words, 0ull), right((size_t)words, 0ull), before((size_t)words, 0ull);
    for (int t = 0; t < T; ++t) {
        if (events[t] & kBalanceLeft) left[t >> 6] |= 1ull << (t & 63);
        if (events[t] & kBalanceRight) right[t >> 6] |= 1ull << (t & 63);
    }
    long long n_marks = 0, strikes = 0;
    for (int w = 0; w < words; ++w) {
        before[w] = (unsigned long long)n_marks;
        n_marks += __builtin_popcountll(left[w] | right[w]);
        strikes += __builtin_popcountll(left[w] ^ right[w]);
    }
    EXPECT(balance_mark_count(left.data(), right.data(), before.data(), T) == n_marks, "the count of marks");
    std::vector<int> list((size_t)n_marks, -7);
    for (int t = 0; t < T; ++t) {
        const int ev = events[t] & (kBalanceLeft | kBalanceRight);
        if (ev) list[(size_t)balance_marks_before(left.data(), right.data(), before.data(), t)] = (t << 2) | ev;
    }
    const long long n_pairs = n_marks > 0 ? n_marks - 1 : 0;
    std::vector<double> pairs((size_t)n_pairs * kBalancePairCols, -7.);
    for (long long i = 0; i < n_pairs; ++i) balance_pair(rel, T, list[(size_t)i], list[(size_t)i + 1], r, pairs.data() + i * kBalancePairCols);
    long long counts[2];
    balance_chain(pairs.data(), n_pairs, counts);
    for (long long i = 0; i < n_pairs; ++i) {
        double* row = pairs.data() + i * kBalancePairCols;
        const double number = row[kBalanceColNumber];
        if (!(number >= 0.)) continue;
        balance_stride(rel, pairs.data(), i);
        if (number < (double)r.max_steps)
            for (int k = 0; k < kBalanceStepCols; ++k) steps[(long long)number * kBalanceStepCols + k] = row[k];
    }
    for (int i = 0; i < r.max_steps * kBalanceStepCols; ++i)
        if (i / kBalanceStepCols >= counts[0]) steps[i] = gait_detail::nan();
    balance_row(pairs.data(), n_pairs, strikes, counts[0], counts[1], r.fps, out);
    for (int t = 0; t < T; ++t) {
        const bool at = gait_detail::bit(left.data(), t) || gait_detail::bit(right.data(), t);
        balance_path(rel, pairs.data(), n_marks, balance_marks_before(left.data(), right.data(), before.data(), t), at, t, per_frame + (size_t)t * kBalanceFrameCols);
    }
}

static int check_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); ++failures; return 1; }
    std::vector<int32_t> head, table, segments, events;
    std::vector<double> scalars, weights, rel_in, want_rel, want_frame, want_steps, want_seq;
    std::vector<float> joints;
    bool ok = read_n(f, head, 7) && read_n(f, table, 8) && read_n(f, scalars, 2);
    if (!ok || head[0] < 1 || head[1] < 0 || head[2] < 0 || head[2] > kBalanceMaxSegments) { std::printf("%s: bad header\n", path); std::fclose(f); ++failures; return 1; }
    const int T = head[0], J = head[1], n_seg = head[2];
    const BalanceRule r{scalars[0], scalars[1], head[3], head[4], head[5], head[6]};
    EXPECT(balance_rule_error(r) == nullptr, "%s: its rule is refused: %s", path, balance_rule_error(r));
    if (balance_rule_error(r)) { std::fclose(f); return 1; }
    ok = read_n(f, segments, (size_t)n_seg * 2) && read_n(f, weights, (size_t)n_seg * 2) &&
         (J ? read_n(f, joints, (size_t)T * J * 3) : read_n(f, rel_in, (size_t)T * kBalanceRelCols)) && read_n(f, events, (size_t)T) &&
         read_n(f, want_rel, J ? (size_t)T * kBalanceRelCols : 0) && read_n(f, want_frame, (size_t)T * kBalanceFrameCols) &&
         read_n(f, want_steps, (size_t)r.max_steps * kBalanceStepCols) && read_n(f, want_seq, (size_t)kBalanceSeqCols);
    std::fclose(f);
    if (!ok) { std::printf("%s: short file\n", path); ++failures; return 1; }

    const int before = failures;
    std::vector<double> rel;
    if (J) {
        BalanceSegments seg{};
        const char* why = balance_segments_error(segments.data(), weights.data(), n_seg, J, &seg);
        EXPECT(why == nullptr, "%s: its segments are refused: %s", path, why);
        if (why) return 1;
        rel.assign((size_t)T * kBalanceRelCols, -7.);
        for (int t = 0; t < T; ++t) balance_com(joints.data() + (size_t)t * J * 3, seg, table[4], table[5], rel.data() + (size_t)t * kBalanceRelCols);
        for (size_t i = 0; i < rel.size(); ++i)
            EXPECT(same(rel[i], want_rel[i]), "%s: rel[%zu][%zu] = %.17g, not %.17g", path, i / kBalanceRelCols, i % kBalanceRelCols, rel[i], want_rel[i]);
    } else {
        rel = rel_in;
    }
    std::vector<double> frame((size_t)T * kBalanceFrameCols, -7.), steps((size_t)r.max_steps * kBalanceStepCols, -7.), seq((size_t)kBalanceSeqCols, -7.);
    sequence(T, r, rel.data(), events.data(), frame.data(), steps.data(), seq.data());
    for (size_t i = 0; i < frame.size(); ++i)
        EXPECT(same(frame[i], want_frame[i]), "%s: per_frame[%zu][%zu] = %.17g, not %.17g", path, i / kBalanceFrameCols, i % kBalanceFrameCols, frame[i], want_frame[i]);
    for (size_t i = 0; i < steps.size(); ++i)
        EXPECT(same(steps[i], want_steps[i]), "%s: steps[%zu][%zu] = %.17g, not %.17g", path, i / kBalanceStepCols, i % kBalanceStepCols, steps[i], want_steps[i]);
    for (int c = 0; c < kBalanceSeqCols; ++c) EXPECT(same(seq[c], want_seq[c]), "%s: per_seq[%d] = %.17g, not %.17g", path, c, seq[c], want_seq[c]);
    return failures - before;
}

// what no file reaches: the marks in front of a frame over word boundaries, and every refusal
static void check_rules() {
    std::vector<unsigned long long> l(3, 0ull), r(3, 0ull), before(3, 0ull);
    const int left_at[] = {0, 63, 64, 130}, right_at[] = {5, 63, 127, 128};        // frame 63 carries both bits: one mark
    for (int t : left_at) l[t >> 6] |= 1ull << (t & 63);
    for (int t : right_at) r[t >> 6] |= 1ull << (t & 63);
    long long n = 0;
    for (int w = 0; w < 3; ++w) { before[w] = (unsigned long long)n; n += __builtin_popcountll(l[w] | r[w]); }
    EXPECT(n == 7 && balance_mark_count(l.data(), r.data(), before.data(), 131) == 7, "seven marks");
    const int frames[] = {0, 1, 5, 6, 63, 64, 65, 127, 128, 129, 130}, wants[] = {0, 1, 1, 2, 2, 3, 4, 4, 5, 6, 6};
    for (int i = 0; i < 11; ++i)
        EXPECT(balance_marks_before(l.data(), r.data(), before.data(), frames[i]) == wants[i], "marks before frame %d", frames[i]);
    const double nan = std::nan(""), inf = INFINITY;
    const BalanceRule good{20., 9.81, 4, 1, 30, 256};
    const struct { BalanceRule r; const char* word; } bad[] = {
        {{0., 9.81, 4, 1, 30, 256}, "fps"}, {{-1., 9.81, 4, 1, 30, 256}, "fps"}, {{nan, 9.81, 4, 1, 30, 256}, "fps"}, {{inf, 9.81, 4, 1, 30, 256}, "fps"},
        {{20., 0., 4, 1, 30, 256}, "gravity"}, {{20., -9.81, 4, 1, 30, 256}, "gravity"}, {{20., nan, 4, 1, 30, 256}, "gravity"}, {{20., inf, 4, 1, 30, 256}, "gravity"},
        {{20., 9.81, 0, 1, 30, 256}, "window"}, {{20., 9.81, 17, 1, 30, 256}, "window"}, {{20., 9.81, 4, -1, 30, 256}, "settle"}, {{20., 9.81, 4, 5, 30, 256}, "settle"},
        {{20., 9.81, 4, 1, 0, 256}, "max_step"}, {{20., 9.81, 4, 1, -3, 256}, "max_step"}, {{20., 9.81, 4, 1, 30, 0}, "max_steps"}, {{20., 9.81, 4, 1, 30, 1025}, "max_steps"}};
    EXPECT(balance_rule_error(good) == nullptr, "the default rule is refused: %s", balance_rule_error(good));
    for (const auto& b : bad) {
        const char* why = balance_rule_error(b.r);
        EXPECT(why && std::strstr(why, b.word) == why, "a bad %s is %s", b.word, why ? why : "not refused");
    }
    const BalanceRule limits[] = {{20., 9.81, 1, 0, 1, 1}, {20., 9.81, 16, 4, 1 << 20, 1024}};
    for (const auto& x : limits) EXPECT(balance_rule_error(x) == nullptr, "a rule at the limits is refused: %s", balance_rule_error(x));
    BalanceSegments seg{};
    std::vector<int> idx(2 * 17, 1);
    std::vector<double> w(2 * 17, 0.5);
    EXPECT(balance_segments_error(idx.data(), w.data(), 16, 2, &seg) == nullptr && seg.n == 16, "sixteen segments are refused");
    const char* why = balance_segments_error(idx.data(), w.data(), 17, 2, &seg);
    EXPECT(why && std::strstr(why, "n_seg") == why, "seventeen segments");
    why = balance_segments_error(idx.data(), w.data(), 0, 2, &seg);
    EXPECT(why && std::strstr(why, "n_seg") == why, "no segment");
    idx[3] = 2;
    why = balance_segments_error(idx.data(), w.data(), 2, 2, &seg);
    EXPECT(why && std::strstr(why, "segment joint") == why, "a joint past J");
    idx[3] = -1;
    why = balance_segments_error(idx.data(), w.data(), 2, 2, &seg);
    EXPECT(why && std::strstr(why, "segment joint") == why, "a negative joint");
    idx[3] = 1;
    for (double m : {0., -1., nan, inf}) {
        w[2] = m;
        why = balance_segments_error(idx.data(), w.data(), 2, 2, &seg);
        EXPECT(why && std::strstr(why, "segment mass") == why, "a mass of %g", m);
    }
    w[2] = 0.5;
    for (double p : {nan, inf, -inf}) {
        w[3] = p;
        why = balance_segments_error(idx.data(), w.data(), 2, 2, &seg);
        EXPECT(why && std::strstr(why, "segment fraction") == why, "a fraction of %g", p);
    }
    w[3] = -0.25;                                              // a fraction outside [0, 1] is a point beyond the joint: allowed
    EXPECT(balance_segments_error(idx.data(), w.data(), 2, 2, &seg) == nullptr, "a negative fraction is refused");
}

int main(int argc, char** argv) {
    check_rules();
    for (int i = 1; i < argc; ++i) check_file(argv[i]);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
