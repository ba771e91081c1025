// csrc/gait_regularity.h on the host: a stand-alone program (its own main, no HIP, nothing of the library but that header and the ones it includes),
// built with AddressSanitizer and UBSan by tests/test_regularity_host_cpu.py and run directly on one file per case, which the test writes: the inputs
// of ONE sequence and what pipeline.gait_regularity (or, of a case on signals, pipeline.gait_autocorr) made of them with sigma = 0.  The program runs
// the chain the kernels run -- reg_frame, the validity mask, reg_mean, reg_key, reg_lag per lag, reg_rho, the three masks over the lags, reg_row -- in
// buffers of exactly the sizes the call states, so that an index outside them is caught.  Every bit must be equal (a NaN equals a NaN).
//
// The file, little-endian: int32 [T, J, has_trans, has_exclude, max_lag, min_lag, min_pairs], int32 table[8], float64 [fps, min_peak], then float32
// joints[T J 3] or, where J is 0, float64 signals[T 4]; float64 trans[T 3] and int32 exclude[T] where stated; then the expected float64
// per_frame[T 4] (not where J is 0), acf[4 (max_lag+1)], per_seq[4 10].  Prints what differs, and "ok" as its last line if nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gait_regularity.h"

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

static void set_bit(unsigned long long* words, int t) { words[t >> 6] |= 1ull << (t & 63); }

// stages (a) to (e) of reg_sequence_stages for one channel, a loop where the device has a lane each; x: the channel's T values, 4 apart
static void channel(int T, const RegRule& r, bool odd, const double* x, const int32_t* exclude, double* acf, double* out) {
    const int words = ((T - 1) >> 6) + 1;
    std::vector<unsigned long long> valid((size_t)words, 0ull);
    std::vector<long long> prefix((size_t)words, -7);
    std::vector<double> d((size_t)T);
    std::vector<int> key((size_t)T);
    for (int t = 0; t < T; ++t) {
        d[t] = x[(size_t)t * kRegChannels];
        if (reg_valid(d[t], exclude, t)) set_bit(valid.data(), t);
    }
    long long n = 0;
    const double mu = reg_mean(d.data(), valid.data(), T, prefix.data(), &n);
    for (int t = 0; t < T; ++t) {
        key[t] = reg_key(valid.data(), prefix.data(), t);
        if (key[t] >= 0) d[t] = d[t] - mu;
    }
    std::vector<double> sums((size_t)r.max_lag + 1), rho((size_t)r.max_lag + 1);
    std::vector<long long> N((size_t)r.max_lag + 1);
    for (int m = 0; m <= r.max_lag; ++m) sums[m] = reg_lag(d.data(), key.data(), T, m, &N[m]);
    for (int m = 0; m <= r.max_lag; ++m) acf[m] = rho[m] = reg_rho(sums[m], N[m], sums[0], N[0], r.min_pairs);
    unsigned long long lags[3][kRegLagWords] = {};
    for (int m = 0; m <= r.max_lag; ++m) {
        if (reg_first_peak(rho.data(), r, m)) set_bit(lags[0], m);
        if (reg_is_max(rho.data(), r.max_lag, m)) set_bit(lags[1], m);
        if (reg_is_min(rho.data(), r.max_lag, m)) set_bit(lags[2], m);
    }
    reg_row(rho.data(), lags[0], lags[1], lags[2], r, odd, n, sums[0], out);
}

static int check_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); ++failures; return 1; }
    std::vector<int32_t> head, table, exclude;
    std::vector<double> scalars, signals, trans, want_frame, want_acf, want_seq;
    std::vector<float> joints;
    bool ok = read_n(f, head, 7) && read_n(f, table, 8) && read_n(f, scalars, 2);
    if (!ok) { std::printf("%s: short header\n", path); std::fclose(f); ++failures; return 1; }
    const int T = head[0], J = head[1];
    const RegRule r{scalars[0], head[4], head[5], scalars[1], head[6]};
    EXPECT(reg_rule_error(r) == nullptr, "%s: its rule is refused: %s", path, reg_rule_error(r));
    if (reg_rule_error(r)) { std::fclose(f); return 1; }
    ok = (J ? read_n(f, joints, (size_t)T * J * 3) : read_n(f, signals, (size_t)T * kRegChannels)) && read_n(f, trans, head[2] ? (size_t)T * 3 : 0) &&
         read_n(f, exclude, head[3] ? (size_t)T : 0) && read_n(f, want_frame, J ? (size_t)T * kRegChannels : 0) &&
         read_n(f, want_acf, (size_t)kRegChannels * (r.max_lag + 1)) && read_n(f, want_seq, (size_t)kRegChannels * kRegSeqCols);
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
    std::vector<double> acf((size_t)kRegChannels * (r.max_lag + 1), -7.), seq((size_t)kRegChannels * kRegSeqCols, -7.);
    for (int ch = 0; ch < kRegChannels; ++ch)
        channel(T, r, reg_odd(ch), signals.data() + ch, head[3] ? exclude.data() : nullptr, acf.data() + (size_t)ch * (r.max_lag + 1), seq.data() + (size_t)ch * kRegSeqCols);
    for (size_t i = 0; i < acf.size(); ++i)
        EXPECT(same(acf[i], want_acf[i]), "%s: acf[%zu][%zu] = %.17g, not %.17g", path, i / (r.max_lag + 1), i % (r.max_lag + 1), acf[i], want_acf[i]);
    for (size_t i = 0; i < seq.size(); ++i)
        EXPECT(same(seq[i], want_seq[i]), "%s: per_seq[%zu][%zu] = %.17g, not %.17g", path, i / kRegSeqCols, i % kRegSeqCols, seq[i], want_seq[i]);
    return failures - before;
}

// what no file reaches: run numbers over word boundaries, and every refusal of the rule
static void check_rules() {
    std::vector<unsigned long long> valid(3, ~0ull);
    for (int t : {0, 63, 64, 65, 128}) valid[t >> 6] &= ~(1ull << (t & 63));
    std::vector<double> x(130, 1.);
    std::vector<long long> prefix(3, -7);
    valid[2] &= 3ull;                                          // 130 frames
    long long n = 0;
    const double mu = reg_mean(x.data(), valid.data(), 130, prefix.data(), &n);
    EXPECT(n == 125 && mu == 1. && prefix[0] == 0 && prefix[1] == 62 && prefix[2] == 124, "n %lld mu %g prefix %lld %lld %lld", n, mu, prefix[0], prefix[1], prefix[2]);
    const int want[] = {-1, 1, 1, -1, -1, -1, 4, 4, -1, 5};
    const int at[] = {0, 1, 62, 63, 64, 65, 66, 127, 128, 129};
    for (int i = 0; i < 10; ++i) EXPECT(reg_key(valid.data(), prefix.data(), at[i]) == want[i], "run of frame %d is %d, not %d", at[i], reg_key(valid.data(), prefix.data(), at[i]), want[i]);
    const double nan = std::nan(""), inf = INFINITY;
    const RegRule good{20., 60, 4, 0.25, 20};
    const struct { RegRule r; const char* word; } bad[] = {
        {{0., 60, 4, 0.25, 20}, "fps"}, {{-1., 60, 4, 0.25, 20}, "fps"}, {{nan, 60, 4, 0.25, 20}, "fps"}, {{inf, 60, 4, 0.25, 20}, "fps"},
        {{20., 7, 4, 0.25, 20}, "max_lag"}, {{20., 256, 4, 0.25, 20}, "max_lag"}, {{20., 60, 1, 0.25, 20}, "min_lag"}, {{20., 60, 59, 0.25, 20}, "min_lag"},
        {{20., 60, 4, 0., 20}, "min_peak"}, {{20., 60, 4, 1.5, 20}, "min_peak"}, {{20., 60, 4, nan, 20}, "min_peak"}, {{20., 60, 4, -0.25, 20}, "min_peak"},
        {{20., 60, 4, 0.25, 1}, "min_pairs"}, {{20., 60, 4, 0.25, (1 << 20) + 1}, "min_pairs"}};
    EXPECT(reg_rule_error(good) == nullptr, "the default rule is refused: %s", reg_rule_error(good));
    for (const auto& b : bad) {
        const char* why = reg_rule_error(b.r);
        EXPECT(why && std::strstr(why, b.word) == why, "a bad %s is %s", b.word, why ? why : "not refused");
    }
    const RegRule limits[] = {{20., 8, 2, 1., 2}, {20., 255, 253, 0.01, 1 << 20}, {20., 8, 6, 0.25, 20}};
    for (const auto& r : limits) EXPECT(reg_rule_error(r) == nullptr, "a rule at the limits is refused: %s", reg_rule_error(r));
}

int main(int argc, char** argv) {
    check_rules();
    for (int i = 1; i < argc; ++i) check_file(argv[i]);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
