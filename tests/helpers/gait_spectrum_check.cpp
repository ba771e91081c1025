// csrc/gait_spectrum.h on the host: a stand-alone program (its own main, no HIP, nothing of the library but that header and the ones it includes),
// built with AddressSanitizer and UBSan by tests/test_spectrum_host_cpu.py and run directly on one file per case, which the test writes: the signals
// of ONE sequence and the call's scalars.  The program runs the chain the kernels run -- ent_diff, the ballot's bitmask, spec_runs, spec_mean,
// har_twiddle, spec_hann, spec_window_power, spec_bin, spec_density, spec_row with a loop where the device has a lane -- in buffers of exactly the
// sizes the call states, so that an index outside them is caught, and PRINTS every value's bits: the test compares them with the statement's.  A case
// that the rules refuse is answered with a line "refused <file>: <why>", in the words the library and the statement use.
//
// The file, little-endian: int32 [T, has_exclude, derivative, segment, hop, nfft, min_segments, has_data], float64 [fps, f_lo, f_hi]; then, where
// has_data, float64 signals[T 4] and int32 exclude[T] where stated.  Per channel two lines: "psd <file> <ch>" and nfft / 2 + 1 words of 16 hex
// digits, "row <file> <ch>" and 13 of them; "ok" as the last line if nothing failed.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gait_spectrum.h"

using namespace grk;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

template <class V>
static bool read_n(std::FILE* f, std::vector<V>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(V), n, f) == n;
}

static void print_bits(const char* what, const char* path, int ch, const std::vector<double>& v) {
    std::printf("%s %s %d", what, path, ch);
    for (double d : v) {
        uint64_t u;
        std::memcpy(&u, &d, sizeof u);
        std::printf(" %016" PRIx64, u);
    }
    std::printf("\n");
}

// the two kernels for one channel; x: the channel's T values, 4 apart
static void channel(int T, const SpecRule& r, bool odd, const double* x, const int32_t* exclude, std::vector<double>& psd, std::vector<double>& row) {
    const int L = r.segment, N = r.nfft;
    std::vector<double> y((size_t)T);
    std::vector<unsigned long long> mask((size_t)(T + 63) / 64, 0ull);
    long long n = 0;
    for (int t = 0; t < T; ++t) {
        y[t] = ent_diff(x, exclude, t, T, r.derivative);
        if (translation_detail::finite(y[t])) { mask[t >> 6] |= 1ull << (t & 63); ++n; }
    }
    std::vector<int> start((size_t)spec_run_segments(T, L, r.hop));
    const int candidates = spec_runs(mask.data(), T, L, r.hop, [&](int s, int t0) {
        EXPECT((size_t)s < start.size(), "segment %d of at most %zu", s, start.size());
        if ((size_t)s < start.size()) start[s] = t0;
    });
    const int used = spec_used(candidates, r.min_segments);
    std::vector<double> mu((size_t)used), sn((size_t)N), cs((size_t)N), w((size_t)L);
    for (int s = 0; s < used; ++s) mu[s] = spec_mean(y.data() + start[s], L);
    for (int j = 0; j < N; ++j) har_twiddle(j, N, &sn[j], &cs[j]);
    for (int i = 0; i < L; ++i) {
        double s, c;
        har_twiddle(i, L, &s, &c);
        w[i] = spec_hann(c);
    }
    const double W2 = spec_window_power(w.data(), L);
    psd.assign((size_t)N / 2 + 1, -7.);
    for (int k = 0; k <= N / 2; ++k)
        psd[k] = spec_density(spec_bin(y.data(), start.data(), mu.data(), used, w.data(), L, sn.data(), cs.data(), N, k), k, used, r, W2);
    row.assign(kSpecSeqCols, -7.);
    spec_row(psd.data(), r, odd, n, candidates, used, row.data());
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
    if (const char* why = spec_rule_error(r)) {
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
    const bool ok = read_n(f, signals, (size_t)T * kRegChannels) && read_n(f, exclude, head[1] ? (size_t)T : 0);
    std::fclose(f);
    if (!ok) { std::printf("%s: short file\n", path); ++failures; return; }
    for (int ch = 0; ch < kRegChannels; ++ch) {
        std::vector<double> psd, row;
        channel(T, r, reg_odd(ch), signals.data() + ch, head[1] ? exclude.data() : nullptr, psd, row);
        print_bits("psd", path, ch, psd);
        print_bits("row", path, ch, row);
    }
}

// what no file reaches: the segments of a run at its edges, the band, and the rule at its limits
static void check_rules() {
    EXPECT(spec_run_segments(63, 64, 32) == 0 && spec_run_segments(64, 64, 32) == 1 && spec_run_segments(95, 64, 32) == 1 && spec_run_segments(96, 64, 32) == 2,
           "the segments of a run of L - 1, L, L + hop - 1 and L + hop frames");
    const double nan = std::nan(""), inf = INFINITY;
    const SpecRule base{20., 2, 64, 32, 256, 0.5, 3.0, 2};
    int lo, hi;
    spec_band(base, &lo, &hi);
    EXPECT(lo == 7 && hi == 38, "the default band is %d .. %d", lo, hi);      // 7 * 20 / 256 = 0.547, 38 * 20 / 256 = 2.97
    const SpecRule limits[] = {base, {1e-3, 0, 8, 1, 8, 1e-4, 5e-4, 1}, {1e6, 2, 256, 256, 1024, 1., 5e5, 1 << 20}, {20., 1, 256, 32, 256, 0.5, 10., 2}};
    for (const auto& r : limits) EXPECT(spec_rule_error(r) == nullptr, "a rule at the limits is refused: %s", spec_rule_error(r));
    const struct { SpecRule r; const char* word; } bad[] = {
        {{0., 2, 64, 32, 256, 0.5, 3., 2}, "fps"}, {{nan, 2, 64, 32, 256, 0.5, 3., 2}, "fps"}, {{inf, 2, 64, 32, 256, 0.5, 3., 2}, "fps"}, {{20., -1, 64, 32, 256, 0.5, 3., 2}, "derivative"},
        {{20., 3, 64, 32, 256, 0.5, 3., 2}, "derivative"}, {{20., 2, 6, 3, 256, 0.5, 3., 2}, "segment"}, {{20., 2, 63, 32, 256, 0.5, 3., 2}, "segment"},
        {{20., 2, 258, 64, 512, 0.5, 3., 2}, "segment"}, {{20., 2, 64, 7, 256, 0.5, 3., 2}, "hop"}, {{20., 2, 64, 65, 256, 0.5, 3., 2}, "hop"}, {{20., 2, 64, 32, 62, 0.5, 3., 2}, "nfft"},
        {{20., 2, 64, 32, 255, 0.5, 3., 2}, "nfft"}, {{20., 2, 64, 32, 1026, 0.5, 3., 2}, "nfft"}, {{20., 2, 64, 32, 256, 0., 3., 2}, "f_lo"}, {{20., 2, 64, 32, 256, 3., 3., 2}, "f_lo"},
        {{20., 2, 64, 32, 256, 0.5, 10.5, 2}, "f_lo"}, {{20., 2, 64, 32, 256, nan, 3., 2}, "f_lo"}, {{20., 2, 64, 32, 256, 0.5, 3., 0}, "min_segments"},
        {{20., 2, 64, 32, 256, 0.5, 3., (1 << 20) + 1}, "min_segments"}};
    for (const auto& b : bad) {
        const char* why = spec_rule_error(b.r);
        EXPECT(why && std::strstr(why, b.word) == why, "a bad %s is %s", b.word, why ? why : "not refused");
    }
}

int main(int argc, char** argv) {
    check_rules();
    for (int i = 1; i < argc; ++i) check_file(argv[i]);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
