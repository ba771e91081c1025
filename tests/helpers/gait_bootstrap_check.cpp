// csrc/gait_bootstrap.h on the host: a stand-alone program (its own main, no HIP, nothing of the library but that header and the ones it includes),
// built with AddressSanitizer and UBSan by tests/test_bootstrap_host_cpu.py and run directly on one file per case, which the test writes.  The
// program runs what the kernels run -- the masks by frame, boot_step_rows and boot_stride_rows; a column's samples, boot_statistics per replicate,
// boot_select per statistic -- in buffers of exactly the sizes the call states, so that an index outside them is caught.  Every bit must be equal
// (a NaN equals a NaN).
//
// A file, little-endian, begins with an int32 kind.
//   kind 0, a bootstrap call: int32 [n_seq, max_rows, C, n_cols, B, block, stream, n_q], uint64 seed, int32 cols[n_cols], int32 q[n_q], int32
//           counts[n_seq], float64 table[n_seq max_rows C]; then the expected float64 out[n_seq n_cols 3 (2 + n_q)] and replicates[n_seq n_cols 3 B].
//   kind 1, the tables of ONE sequence: int32 [T, max_rows, masked], float64 fps, int32 events[T], int32 phase[T] where masked, float64 rows[T 7];
//           then the expected float64 steps[max_rows 6], strides[max_rows 4], int32 counts[2] and float64 row[9]: what the gait call (masked: the turn
//           call's straight columns) reports as mean and SD of step time, length and width and mean, SD and CV of stride time, which replicate 0 of
//           the tables must meet where the counts are within max_rows.
// Prints what differs, and "ok" as its last line if nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gait_bootstrap.h"

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

static void check_bootstrap(const char* path, std::FILE* f) {
    std::vector<int32_t> head, cols, q, counts;
    std::vector<uint64_t> seed;
    std::vector<double> table, want_out, want_reps;
    if (!read_n(f, head, 8) || !read_n(f, seed, 1) || head[0] < 1 || head[3] < 0 || head[3] > kBootMaxCols || head[7] < 0 || head[7] > kBootMaxQuantiles) {
        std::printf("%s: bad header\n", path); ++failures; return;
    }
    BootRule r{};
    const int n_seq = head[0];
    r.max_rows = head[1]; r.C = head[2]; r.n_cols = head[3]; r.B = head[4]; r.block = head[5]; r.stream = head[6]; r.n_q = head[7]; r.seed = seed[0];
    bool ok = read_n(f, cols, (size_t)r.n_cols) && read_n(f, q, (size_t)r.n_q);
    for (int k = 0; ok && k < r.n_cols; ++k) r.cols[k] = cols[(size_t)k];
    for (int k = 0; ok && k < r.n_q; ++k) r.q[k] = q[(size_t)k];
    EXPECT(ok && boot_rule_error(r) == nullptr, "%s: its rule is refused: %s", path, ok ? boot_rule_error(r) : "short file");
    if (!ok || boot_rule_error(r)) return;
    const size_t width = 2 + (size_t)r.n_q;
    ok = read_n(f, counts, (size_t)n_seq) && read_n(f, table, (size_t)n_seq * r.max_rows * r.C) && read_n(f, want_out, (size_t)n_seq * r.n_cols * kBootStats * width) &&
         read_n(f, want_reps, (size_t)n_seq * r.n_cols * kBootStats * r.B);
    if (!ok) { std::printf("%s: short file\n", path); ++failures; return; }
    const unsigned long long key = boot_stream_key(r.seed, r.stream);
    for (int s = 0; s < n_seq; ++s) {
        int n = counts[(size_t)s];
        n = n < 0 ? 0 : n > r.max_rows ? r.max_rows : n;
        for (int c = 0; c < r.n_cols; ++c) {
            std::vector<double> x((size_t)n);                   // exactly n samples: a draw outside [0, n) is caught
            for (int p = 0; p < n; ++p) x[(size_t)p] = table[((size_t)s * r.max_rows + p) * r.C + r.cols[c]];
            std::vector<double> v[kBootStats];
            for (auto& one : v) one.assign((size_t)r.B, -7.);
            double first[kBootStats];
            for (int rep = 0; rep <= r.B; ++rep) {
                double st[kBootStats];
                boot_statistics(x.data(), n, r.block, key, rep, st);
                for (int k = 0; k < kBootStats; ++k) {
                    if (rep == 0) first[k] = st[k]; else v[k][(size_t)rep - 1] = st[k];
                }
            }
            const size_t at = (size_t)s * r.n_cols + c;
            for (int k = 0; k < kBootStats; ++k) {
                std::vector<double> sel(1 + (size_t)r.n_q, -7.);
                boot_select(v[k].data(), r.B, r.q, r.n_q, sel.data());
                const double* want = want_out.data() + (at * kBootStats + k) * width;
                EXPECT(same(first[k], want[0]), "%s: sequence %d column %d statistic %d: replicate 0 = %.17g, not %.17g", path, s, c, k, first[k], want[0]);
                for (size_t i = 0; i < sel.size(); ++i)
                    EXPECT(same(sel[i], want[1 + i]), "%s: sequence %d column %d statistic %d: out[%zu] = %.17g, not %.17g", path, s, c, k, 1 + i, sel[i], want[1 + i]);
                const double* reps = want_reps.data() + (at * kBootStats + k) * r.B;
                int differ = 0;
                for (int i = 0; i < r.B; ++i) differ += !same(v[k][(size_t)i], reps[i]);
                EXPECT(differ == 0, "%s: sequence %d column %d statistic %d: %d replicates differ", path, s, c, k, differ);
            }
        }
    }
}

static void check_tables(const char* path, std::FILE* f) {
    std::vector<int32_t> head, events, phase, want_counts;
    std::vector<double> fps, rows, want_steps, want_strides, want_row;
    if (!read_n(f, head, 3) || !read_n(f, fps, 1) || head[0] < 1 || head[1] < 1 || head[1] > kBootMaxRows) { std::printf("%s: bad header\n", path); ++failures; return; }
    const int T = head[0], max_rows = head[1];
    const bool masked = head[2] != 0;
    const bool ok = read_n(f, events, (size_t)T) && read_n(f, phase, masked ? (size_t)T : 0) && read_n(f, rows, (size_t)T * kGaitFrameCols) &&
                    read_n(f, want_steps, (size_t)max_rows * kBootStepCols) && read_n(f, want_strides, (size_t)max_rows * kBootStrideCols) &&
                    read_n(f, want_counts, 2) && read_n(f, want_row, 9);
    if (!ok) { std::printf("%s: short file\n", path); ++failures; return; }
    const size_t words = (size_t)((T - 1) >> 6) + 1;
    std::vector<unsigned long long> left(words, 0ull), right(words, 0ull), busy(words, 0ull);
    for (int t = 0; t < T; ++t) {
        if (events[(size_t)t] & kGaitHeelL) left[(size_t)t >> 6] |= 1ull << (t & 63);
        if (events[(size_t)t] & kGaitHeelR) right[(size_t)t >> 6] |= 1ull << (t & 63);
        if (masked && phase[(size_t)t] != kTurnStraight) busy[(size_t)t >> 6] |= 1ull << (t & 63);
    }
    const unsigned long long* ns = masked ? busy.data() : nullptr;
    std::vector<double> steps((size_t)max_rows * kBootStepCols, -7.), strides((size_t)max_rows * kBootStrideCols, -7.);
    const long long n_steps = boot_step_rows(left.data(), right.data(), ns, T, rows.data(), fps[0], max_rows, steps.data());
    const long long n_strides = boot_stride_rows(left.data(), right.data(), ns, T, fps[0], max_rows, strides.data());
    for (size_t i = 0; i < steps.size(); ++i)
        if ((long long)(i / kBootStepCols) >= n_steps) steps[i] = gait_detail::nan();
    for (size_t i = 0; i < strides.size(); ++i)
        if ((long long)(i / kBootStrideCols) >= n_strides) strides[i] = gait_detail::nan();
    EXPECT(n_steps == want_counts[0] && n_strides == want_counts[1], "%s: %lld steps and %lld strides, not %d and %d", path, n_steps, n_strides, want_counts[0], want_counts[1]);
    for (size_t i = 0; i < steps.size(); ++i)
        EXPECT(same(steps[i], want_steps[i]), "%s: steps[%zu][%zu] = %.17g, not %.17g", path, i / kBootStepCols, i % kBootStepCols, steps[i], want_steps[i]);
    for (size_t i = 0; i < strides.size(); ++i)
        EXPECT(same(strides[i], want_strides[i]), "%s: strides[%zu][%zu] = %.17g, not %.17g", path, i / kBootStrideCols, i % kBootStrideCols, strides[i], want_strides[i]);
    if (n_steps > max_rows || n_strides > max_rows) return;
    // the identity: replicate 0 of the tables' columns IS what gait_steps and gait_strides (masked: turn_steps and turn_strides) report
    double got[9];
    for (int k = 0; k < 3; ++k) {
        std::vector<double> x((size_t)n_steps);
        for (long long i = 0; i < n_steps; ++i) x[(size_t)i] = steps[(size_t)i * kBootStepCols + 3 + k];
        double st[kBootStats];
        boot_statistics(x.data(), (int)n_steps, 1, 0ull, 0, st);
        got[2 * k] = st[0]; got[2 * k + 1] = st[1];
    }
    std::vector<double> x((size_t)n_strides);
    for (long long i = 0; i < n_strides; ++i) x[(size_t)i] = strides[(size_t)i * kBootStrideCols + 3];
    boot_statistics(x.data(), (int)n_strides, 1, 0ull, 0, got + 6);
    for (int k = 0; k < 9; ++k) EXPECT(same(got[k], want_row[(size_t)k]), "%s: replicate 0, value %d = %.17g, the call's row says %.17g", path, k, got[k], want_row[(size_t)k]);
    // and the headers' own walks on the same masks
    double gait_row[kGaitSeqCols];
    if (masked) {
        TurnMasks m{};
        m.hs_l = left.data(); m.hs_r = right.data(); m.not_straight = busy.data();
        turn_steps(m, T, rows.data(), fps[0], gait_row);
        turn_strides(m, T, fps[0], gait_row);
    } else {
        gait_steps(left.data(), right.data(), T, rows.data(), fps[0], gait_row);
        gait_strides(left.data(), right.data(), T, fps[0], gait_row);
    }
    const int at[9] = {kGaitColStepTime, kGaitColStepTimeSd, kGaitColStepLen, kGaitColStepLenSd, kGaitColStepWidth, kGaitColStepWidthSd, kGaitColStride, kGaitColStrideSd,
                       kGaitColStrideCv};
    for (int k = 0; k < 9; ++k) EXPECT(same(got[k], gait_row[at[k]]), "%s: replicate 0, value %d = %.17g, the header's walk says %.17g", path, k, got[k], gait_row[at[k]]);
    EXPECT((double)n_steps == gait_row[kGaitColSteps], "%s: %lld steps, the header's walk counts %g", path, n_steps, gait_row[kGaitColSteps]);
}

// what no file reaches: the generator's known answers, the indices' known answers through boot_statistics' own draws, and every refusal
static void check_rules() {
    const struct { unsigned long long seed; int stream, r; unsigned long long j, u; int i7, i1024; } known[] = {
        {0ull, 0, 1, 0ull, 0x2f101fe21496ea20ull, 1, 188}, {0ull, 0, 1, 1ull, 0xa00624088f65d5b6ull, 4, 640}, {0ull, 1, 1, 0ull, 0x882821205babc31full, 3, 544},
        {0ull, 0, 2, 0ull, 0x0b91752fd22fb56aull, 0, 46}, {2023ull, 3, 4096, 1023ull, 0x507689e32221dafdull, 2, 321}, {~0ull, 0, 1, 0ull, 0x85d74c1255584cabull, 3, 535}};
    for (const auto& k : known) {
        const unsigned long long u = boot_u(boot_replicate_key(boot_stream_key(k.seed, k.stream), k.r), k.j);
        EXPECT(u == k.u && boot_index(u, 7) == k.i7 && boot_index(u, 1024) == k.i1024, "u(%llu, %d, %d, %llu) = %#llx", k.seed, k.stream, k.r, k.j, u);
    }
    // x[p] = 2^p: a replicate's sum tells which rows it drew -- n = 10, seed 0, stream 0
    std::vector<double> x(10);
    for (int p = 0; p < 10; ++p) x[(size_t)p] = (double)(1 << p);
    const struct { int block, r, idx[10]; } draws[] = {{1, 1, {1, 6, 4, 9, 3, 3, 1, 5, 7, 6}}, {1, 2, {0, 4, 6, 9, 0, 3, 4, 1, 4, 4}}, {3, 1, {1, 2, 3, 6, 7, 8, 4, 5, 6, 9}}};
    for (const auto& d : draws) {
        double sum = 0., st[kBootStats];
        for (int p = 0; p < 10; ++p) sum += x[(size_t)d.idx[p]];
        boot_statistics(x.data(), 10, d.block, boot_stream_key(0ull, 0), d.r, st);
        EXPECT(st[0] == sum / 10., "block %d replicate %d: mean %.17g, not %.17g", d.block, d.r, st[0], sum / 10.);
    }
    BootRule good{};
    good.max_rows = 256; good.C = 6; good.n_cols = 3; good.B = 2000; good.block = 1; good.stream = 0; good.n_q = 3; good.seed = 0;
    good.cols[0] = 3; good.cols[1] = 4; good.cols[2] = 5; good.q[0] = 250; good.q[1] = 5000; good.q[2] = 9750;
    EXPECT(boot_rule_error(good) == nullptr, "the default rule is refused: %s", boot_rule_error(good));
    const struct { int BootRule::*field; int value; const char* word; } bad[] = {
        {&BootRule::max_rows, 0, "max_rows"}, {&BootRule::max_rows, 1025, "max_rows"}, {&BootRule::C, 0, "C "}, {&BootRule::C, 17, "C "}, {&BootRule::C, 5, "column"},
        {&BootRule::n_cols, 0, "n_cols"}, {&BootRule::n_cols, 9, "n_cols"}, {&BootRule::B, 0, "B "}, {&BootRule::B, 4097, "B "}, {&BootRule::block, 0, "block"},
        {&BootRule::block, 1025, "block"}, {&BootRule::stream, -1, "stream"}, {&BootRule::stream, 65536, "stream"}, {&BootRule::n_q, -1, "n_q"}, {&BootRule::n_q, 6, "n_q"}};
    for (const auto& b : bad) {
        BootRule r = good;
        r.*(b.field) = b.value;
        const char* why = boot_rule_error(r);
        EXPECT(why && std::strstr(why, b.word) == why, "a bad %s is %s", b.word, why ? why : "not refused");
    }
    for (int v : {-1, 6}) { BootRule r = good; r.cols[1] = v; const char* why = boot_rule_error(r); EXPECT(why && std::strstr(why, "column") == why, "column %d", v); }
    for (int v : {-1, 10001}) { BootRule r = good; r.q[2] = v; const char* why = boot_rule_error(r); EXPECT(why && std::strstr(why, "quantile") == why, "quantile %d", v); }
    BootRule most = good;
    most.max_rows = 1024; most.C = 16; most.n_cols = 8; most.B = 4096; most.block = 1024; most.stream = 65535; most.n_q = 5; most.seed = ~0ull;
    for (int k = 0; k < 8; ++k) most.cols[k] = 15;
    for (int k = 0; k < 5; ++k) most.q[k] = k ? 10000 : 0;
    EXPECT(boot_rule_error(most) == nullptr, "a rule at the limits is refused: %s", boot_rule_error(most));
    BootRule least = good;
    least.max_rows = 1; least.C = 1; least.n_cols = 1; least.cols[0] = 0; least.B = 1; least.n_q = 0;
    EXPECT(boot_rule_error(least) == nullptr, "a rule at the lower limits is refused: %s", boot_rule_error(least));
}

int main(int argc, char** argv) {
    check_rules();
    for (int i = 1; i < argc; ++i) {
        std::FILE* f = std::fopen(argv[i], "rb");
        std::vector<int32_t> kind;
        if (!f || !read_n(f, kind, 1)) { std::printf("cannot read %s\n", argv[i]); ++failures; if (f) std::fclose(f); continue; }
        if (kind[0] == 0) check_bootstrap(argv[i], f); else check_tables(argv[i], f);
        std::fclose(f);
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
