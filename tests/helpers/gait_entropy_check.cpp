// csrc/gait_entropy.h on the host: a stand-alone program (its own main, no HIP, nothing of the library but that header and the ones it includes),
// built with AddressSanitizer and UBSan by tests/test_entropy_host_cpu.py and run directly on one file per case, which the test writes: the inputs of
// ONE sequence and what pipeline.gait_entropy (or, of a case on signals, pipeline.gait_sampen) made of them with sigma = 0.  The program runs the
// chain the kernels run -- reg_frame, ent_diff, ent_spread, ent_coarse, ent_template_valid, ent_partners_m with a loop where the device has a lane --
// in buffers of exactly the sizes the call states, so that an index outside them is caught.  Every integer and every bit must be equal (a NaN equals
// a NaN).  A case that the rules refuse is answered with a line "refused <file>: <why>", in the words the library and the statement use.
//
// The file, little-endian: int32 [T, J, has_trans, has_exclude, m, derivative, scales, has_data], int32 table[8], float64 [fraction]; then, where
// has_data, float32 joints[T J 3] or, where J is 0, float64 signals[T 4]; float64 trans[T 3] and int32 exclude[T] where stated; then the expected
// float64 per_frame[T 4] (not where J is 0), int64 counts[4 scales 3], float64 per_seq[4 4].  Prints what differs, and "ok" as its last line if nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gait_entropy.h"

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

// the two kernels for one channel; x: the channel's T values, 4 apart
static void channel(int T, const EntRule& r, const double* x, const int32_t* exclude, long long* counts, double* out) {
    std::vector<double> y((size_t)T);
    for (int t = 0; t < T; ++t) y[t] = ent_diff(x, exclude, t, T, r.derivative);
    ent_spread(y.data(), T, r.fraction, out);
    for (int tau = 1; tau <= r.scales; ++tau) {
        const int N = T / tau, Nt = N - r.m;
        std::vector<double> z((size_t)N);
        for (int j = 0; j < N; ++j) z[j] = ent_coarse(y.data(), j, tau);
        long long* c = counts + (size_t)(tau - 1) * kEntCountCols;
        c[0] = c[1] = c[2] = 0;
        for (int i = 0; i < Nt; ++i) {
            if (!ent_template_valid(z.data(), i, r.m)) continue;
            ++c[0];
            if (out[3] > 0.) ent_partners_m(r.m, z.data(), Nt, i, out[3], &c[1], &c[2]);
        }
    }
}

static int check_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); ++failures; return 1; }
    std::vector<int32_t> head, table, exclude;
    std::vector<double> scalars, signals, trans, want_frame, want_seq;
    std::vector<long long> want_counts;
    std::vector<float> joints;
    bool ok = read_n(f, head, 8) && read_n(f, table, 8) && read_n(f, scalars, 1);
    if (!ok) { std::printf("%s: short header\n", path); std::fclose(f); ++failures; return 1; }
    const int T = head[0], J = head[1];
    const EntRule r{head[4], scalars[0], head[5], head[6]};
    const int off[2] = {0, T};
    if (const char* why = ent_rule_error(r)) {
        EXPECT(!head[7], "%s: its rule is refused: %s", path, why);
        std::printf("refused %s: %s\n", path, why);
        std::fclose(f);
        return 0;
    }
    if (ent_long_sequence(off, 1) >= 0) {
        EXPECT(!head[7], "%s: its length is refused", path);
        std::printf("refused %s: sequence %d has %d frames, more than %d (the work is quadratic in them)\n", path, ent_long_sequence(off, 1), T, kEntMaxFrames);
        std::fclose(f);
        return 0;
    }
    EXPECT(head[7], "%s: a case without data is not refused", path);
    if (!head[7]) { std::fclose(f); return 1; }
    ok = (J ? read_n(f, joints, (size_t)T * J * 3) : read_n(f, signals, (size_t)T * kRegChannels)) && read_n(f, trans, head[2] ? (size_t)T * 3 : 0) &&
         read_n(f, exclude, head[3] ? (size_t)T : 0) && read_n(f, want_frame, J ? (size_t)T * kRegChannels : 0) &&
         read_n(f, want_counts, (size_t)kRegChannels * r.scales * kEntCountCols) && read_n(f, want_seq, (size_t)kRegChannels * kEntSeqCols);
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
    const size_t per_channel = (size_t)r.scales * kEntCountCols;
    std::vector<long long> counts((size_t)kRegChannels * per_channel, -7);
    std::vector<double> seq((size_t)kRegChannels * kEntSeqCols, -7.);
    for (int ch = 0; ch < kRegChannels; ++ch)
        channel(T, r, signals.data() + ch, head[3] ? exclude.data() : nullptr, counts.data() + ch * per_channel, seq.data() + (size_t)ch * kEntSeqCols);
    for (size_t i = 0; i < counts.size(); ++i)
        EXPECT(counts[i] == want_counts[i], "%s: counts[%zu][%zu][%zu] = %lld, not %lld", path, i / per_channel, i % per_channel / kEntCountCols, i % kEntCountCols,
               counts[i], want_counts[i]);
    for (size_t i = 0; i < seq.size(); ++i)
        EXPECT(same(seq[i], want_seq[i]), "%s: per_seq[%zu][%zu] = %.17g, not %.17g", path, i / kEntSeqCols, i % kEntSeqCols, seq[i], want_seq[i]);
    return failures - before;
}

// what no file reaches: the circular offsets against the plain triangle at every small number of templates, and the rule at its limits
static void check_rules() {
    for (int m = 1; m <= kEntMaxM; ++m)
        for (int Nt = 1; Nt <= 12; ++Nt) {
            std::vector<double> z((size_t)Nt + m);
            for (size_t i = 0; i < z.size(); ++i) z[i] = (double)((i * 7) % 5);
            if (Nt > 3) z[3] = std::nan("");
            long long B = 0, A = 0, wantB = 0, wantA = 0;
            for (int i = 0; i < Nt; ++i) {
                if (!ent_template_valid(z.data(), i, m)) continue;
                ent_partners_m(m, z.data(), Nt, i, 1., &B, &A);
                for (int j = i + 1; j < Nt; ++j) {
                    if (!ent_template_valid(z.data(), j, m)) continue;
                    bool hit = true;
                    for (int k = 0; k < m; ++k) hit = hit && std::fabs(z[i + k] - z[j + k]) <= 1.;
                    wantB += hit;
                    wantA += hit && std::fabs(z[i + m] - z[j + m]) <= 1.;
                }
            }
            EXPECT(B == wantB && A == wantA, "m %d, %d templates: B %lld A %lld by offsets, %lld %lld by the triangle", m, Nt, B, A, wantB, wantA);
        }
    const double nan = std::nan(""), inf = INFINITY;
    const EntRule limits[] = {{2, 0.2, 2, 3}, {1, 10., 0, 1}, {4, 1e-300, 2, 8}};
    for (const auto& r : limits) EXPECT(ent_rule_error(r) == nullptr, "a rule at the limits is refused: %s", ent_rule_error(r));
    const struct { EntRule r; const char* word; } bad[] = {
        {{0, 0.2, 2, 3}, "m "}, {{5, 0.2, 2, 3}, "m "}, {{2, 0., 2, 3}, "fraction"}, {{2, -0.2, 2, 3}, "fraction"}, {{2, 10.5, 2, 3}, "fraction"}, {{2, nan, 2, 3}, "fraction"},
        {{2, inf, 2, 3}, "fraction"}, {{2, 0.2, -1, 3}, "derivative"}, {{2, 0.2, 3, 3}, "derivative"}, {{2, 0.2, 2, 0}, "scales"}, {{2, 0.2, 2, 9}, "scales"}};
    for (const auto& b : bad) {
        const char* why = ent_rule_error(b.r);
        EXPECT(why && std::strstr(why, b.word) == why, "a bad %s is %s", b.word, why ? why : "not refused");
    }
    const int off[] = {0, 5, 5 + kEntMaxFrames, 6 + 2 * kEntMaxFrames, 7 + 2 * kEntMaxFrames};
    EXPECT(ent_long_sequence(off, 2) == -1 && ent_long_sequence(off, 4) == 2, "the first long sequence is %d and %d", ent_long_sequence(off, 2), ent_long_sequence(off, 4));
}

int main(int argc, char** argv) {
    check_rules();
    for (int i = 1; i < argc; ++i) check_file(argv[i]);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
