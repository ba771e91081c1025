// csrc/gait_coordination.h on the host: a stand-alone program (its own main, no HIP, nothing of the library but that header and the ones it
// includes), built with AddressSanitizer and UBSan by tests/test_coordination_host_cpu.py and run directly on one file per case, which the test
// writes: the signals of ONE sequence and the call's scalars.  The program runs the chain the kernels run -- coord_valid, the ballot's bitmask,
// spec_runs, spec_mean, har_twiddle, spec_hann, spec_window_power, coord_bin, spec_density, spec_row and coord_pair_row with a loop where the device
// has a lane -- in buffers of exactly the sizes the call states, so that an index outside them is caught, and PRINTS every value's bits: the test
// compares them with the statement's.  A case that the rules refuse is answered with a line "refused <file>: <why>", in the words the library and the
// statement use.  A frame of joints goes through coord_frame and kin_frame side by side in check_frames: the four channels must have kin_frame's bits.
//
// The file, little-endian (gait_spectrum_check.cpp's layout): int32 [T, has_exclude, derivative, segment, hop, nfft, min_segments, has_data], float64
// [fps, f_lo, f_hi]; then, where has_data, float64 signals[T 4] and int32 exclude[T] where stated.  The lines: "auto <file> <ch>" and nfft / 2 + 1
// words of 16 hex digits, "limb <file> <ch>" and 13, "cross <file> <pair>" and 2 (nfft / 2 + 1) (Re, Im of every bin), "pair <file> <pair>" and 10;
// "ok" as the last line if nothing failed.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gait_coordination.h"

using namespace grk;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

template <class V>
static bool read_n(std::FILE* f, std::vector<V>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(V), n, f) == n;
}

static void print_bits(const char* what, const char* path, int at, const double* v, size_t n) {
    std::printf("%s %s %d", what, path, at);
    for (size_t i = 0; i < n; ++i) {
        uint64_t u;
        std::memcpy(&u, &v[i], sizeof u);
        std::printf(" %016" PRIx64, u);
    }
    std::printf("\n");
}

// the two kernels for one sequence; x: its rows (T,4)
static void sequence(const char* path, int T, const SpecRule& r, const double* x, const int32_t* exclude) {
    const int L = r.segment, N = r.nfft, bins = N / 2 + 1;
    std::vector<double> y((size_t)T * kCoordChannels);         // four columns, T apart
    std::vector<unsigned long long> mask((size_t)(T + 63) / 64, 0ull);
    long long n = 0;
    for (int t = 0; t < T; ++t) {
        double v[kCoordChannels];
        const bool ok = coord_valid(x, exclude, t, T, r.derivative, v);
        for (int c = 0; c < kCoordChannels; ++c) y[(size_t)c * T + t] = v[c];
        if (ok) { mask[t >> 6] |= 1ull << (t & 63); ++n; }
    }
    std::vector<int> start((size_t)spec_run_segments(T, L, r.hop));
    const int candidates = spec_runs(mask.data(), T, L, r.hop, [&](int s, int t0) {
        EXPECT((size_t)s < start.size(), "segment %d of at most %zu", s, start.size());
        if ((size_t)s < start.size()) start[s] = t0;
    });
    const int used = spec_used(candidates, r.min_segments);
    std::vector<double> mu((size_t)used * kCoordChannels), sn((size_t)N), cs((size_t)N), w((size_t)L);
    for (int e = 0; e < used * kCoordChannels; ++e) mu[e] = spec_mean(y.data() + (size_t)(e & 3) * T + start[e >> 2], L);
    for (int j = 0; j < N; ++j) har_twiddle(j, N, &sn[j], &cs[j]);
    for (int i = 0; i < L; ++i) {
        double s, c;
        har_twiddle(i, L, &s, &c);
        w[i] = spec_hann(c);
    }
    const double W2 = spec_window_power(w.data(), L);
    std::vector<double> au((size_t)kCoordChannels * bins, -7.), cr((size_t)kCoordPairs * bins * 2, -7.);
    std::vector<double> re((size_t)kCoordPairs * bins, -7.), im((size_t)kCoordPairs * bins, -7.);
    for (int k = 0; k < bins; ++k) {
        double acc[kCoordSums];
        coord_bin(y.data(), (size_t)T, start.data(), mu.data(), used, w.data(), L, sn.data(), cs.data(), N, k, acc);
        for (int c = 0; c < kCoordChannels; ++c) au[(size_t)c * bins + k] = spec_density(acc[c], k, used, r, W2);
        for (int p = 0; p < kCoordPairs; ++p) {
            re[(size_t)p * bins + k] = cr[((size_t)p * bins + k) * 2] = spec_density(acc[kCoordChannels + 2 * p], k, used, r, W2);
            im[(size_t)p * bins + k] = cr[((size_t)p * bins + k) * 2 + 1] = spec_density(acc[kCoordChannels + 2 * p + 1], k, used, r, W2);
        }
    }
    for (int c = 0; c < kCoordChannels; ++c) {
        std::vector<double> row(kSpecSeqCols, -7.);
        spec_row(au.data() + (size_t)c * bins, r, true, n, candidates, used, row.data());
        print_bits("auto", path, c, au.data() + (size_t)c * bins, bins);
        print_bits("limb", path, c, row.data(), row.size());
    }
    for (int p = 0; p < kCoordPairs; ++p) {
        std::vector<double> row(kCoordPairCols, -7.);
        coord_pair_row(au.data() + (size_t)coord_pair_a(p) * bins, au.data() + (size_t)coord_pair_b(p) * bins, re.data() + (size_t)p * bins, im.data() + (size_t)p * bins, r,
                       coord_antiphase(p), used, row.data());
        print_bits("cross", path, p, cr.data() + (size_t)p * bins * 2, (size_t)bins * 2);
        print_bits("pair", path, p, row.data(), row.size());
    }
}

static void check_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); ++failures; return; }
    std::vector<int32_t> head, exclude;
    std::vector<double> scalars, signals;
    if (!(read_n(f, head, 8) && read_n(f, scalars, 3))) { std::printf("%s: short header\n", path); std::fclose(f); ++failures; return; }
    const int T = head[0];
    const SpecRule r{scalars[0], head[2], head[3], head[4], head[5], scalars[1], scalars[2], head[6]};
    const int off[2] = {0, T};
    if (const char* why = coord_rule_error(r)) {
        EXPECT(!head[7], "%s: its rule is refused: %s", path, why);
        std::printf("refused %s: %s\n", path, why);
        std::fclose(f);
        return;
    }
    if (ent_long_sequence(off, 1) >= 0) {
        EXPECT(!head[7], "%s: its length is refused", path);
        std::printf("refused %s: sequence %d has %d frames, more than %d (the work is quadratic in them)\n", path, ent_long_sequence(off, 1), T, kEntMaxFrames);
        std::fclose(f);
        return;
    }
    EXPECT(head[7], "%s: a case without data is not refused", path);
    if (!head[7]) { std::fclose(f); return; }
    const bool ok = read_n(f, signals, (size_t)T * kCoordChannels) && read_n(f, exclude, head[1] ? (size_t)T : 0);
    std::fclose(f);
    if (!ok) { std::printf("%s: short file\n", path); ++failures; return; }
    sequence(path, T, r, signals.data(), head[1] ? exclude.data() : nullptr);
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// coord_frame against kin_frame on made-up bodies, a degenerate one among them: the four channels are kin_frame's 8, 9, 0 and 1 in every bit
static void check_frames() {
    const int J = 25, tab[kKinTable] = {0, 20, 12, 16, 13, 17, 14, 18, 15, 19, 4, 8, 5, 9, 6, 10};
    uint32_t state = 12345u;
    for (int trial = 0; trial < 200; ++trial) {
        float rows[J * 3];
        for (float& v : rows) {
            state = state * 1664525u + 1013904223u;
            v = (float)((double)(state >> 8) / 16777216. - 0.5);
        }
        if (trial % 50 == 7)
            for (int a = 0; a < 3; ++a) rows[3 * 12 + a] = rows[3 * 16 + a];      // the left hip on the right hip: no axes
        double all[kKinChannels], four[kCoordChannels];
        kin_frame(rows, tab, all);
        coord_frame(rows, tab, four);
        EXPECT(same_bits(four[0], all[8]) && same_bits(four[1], all[9]) && same_bits(four[2], all[0]) && same_bits(four[3], all[1]), "trial %d: coord_frame is not kin_frame", trial);
        EXPECT((trial % 50 == 7) == (four[0] != four[0]), "trial %d: validity", trial);
    }
}

// what no file reaches: the pairs' table and the rule at its limits
static void check_rules() {
    const int want[kCoordPairs][2] = {{0, 1}, {2, 3}, {0, 3}, {1, 2}, {0, 2}, {1, 3}};
    for (int p = 0; p < kCoordPairs; ++p)
        EXPECT(coord_pair_a(p) == want[p][0] && coord_pair_b(p) == want[p][1] && coord_antiphase(p) == (p != 2 && p != 3), "pair %d", p);
    const double nan = std::nan("");
    const SpecRule limits[] = {{20., 0, 64, 32, 256, 0.5, 3.0, 4}, {1e-3, 0, 8, 1, 8, 1e-4, 5e-4, 2}, {1e6, 2, 256, 256, 1024, 1., 5e5, 1 << 20}};
    for (const auto& r : limits) EXPECT(coord_rule_error(r) == nullptr, "a rule at the limits is refused: %s", coord_rule_error(r));
    const struct { SpecRule r; const char* word; } bad[] = {
        {{0., 0, 64, 32, 256, 0.5, 3., 4}, "fps"}, {{nan, 0, 64, 32, 256, 0.5, 3., 4}, "fps"}, {{20., 3, 64, 32, 256, 0.5, 3., 4}, "derivative"},
        {{20., 0, 63, 32, 256, 0.5, 3., 4}, "segment"}, {{20., 0, 64, 7, 256, 0.5, 3., 4}, "hop"}, {{20., 0, 64, 32, 1026, 0.5, 3., 4}, "nfft"},
        {{20., 0, 64, 32, 256, 0.5, 10.5, 4}, "f_lo"}, {{20., 0, 64, 32, 256, 0.5, 3., 1}, "min_segments outside [2, 2^20]"}, {{20., 0, 64, 32, 256, 0.5, 3., 0}, "min_segments outside [2"},
        {{20., 0, 64, 32, 256, 0.5, 3., (1 << 20) + 1}, "min_segments"}, {{20., 0, 63, 32, 256, 0.5, 3., 1}, "segment"}};
    for (const auto& b : bad) {
        const char* why = coord_rule_error(b.r);
        EXPECT(why && std::strstr(why, b.word) == why, "a bad %s is %s", b.word, why ? why : "not refused");
    }
}

int main(int argc, char** argv) {
    check_rules();
    check_frames();
    for (int i = 1; i < argc; ++i) check_file(argv[i]);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
