// csrc/gait_smoothness.h on the host: a stand-alone program (its own main, no HIP, nothing of the library but that header and the ones it includes),
// built with AddressSanitizer and UBSan by tests/test_smoothness_host_cpu.py and run directly on one file per case, which the test writes: the signals
// of ONE sequence and the call's scalars.  The program runs the chain the kernels run -- ent_diff, the ballot's bitmask, spec_runs, har_twiddle,
// smo_magnitude, smo_segment, smo_jerk, smo_row with a loop where the device has a lane -- in buffers of exactly the sizes the call states, so that an
// index outside them is caught, and PRINTS every value's bits: the test compares them with the statement's.  A case that the rules refuse is answered
// with a line "refused <file>: <why>", in the words the library and the statement use.
//
// The file, little-endian: int32 [T, has_exclude, derivative, segment, hop, nfft, min_segments, has_data], float64 [fps, f_cut, amplitude]; then, where
// has_data, float64 signals[T 4] and int32 exclude[T] where stated.  Per channel two lines: "seg <file> <ch>" and slots * 8 words of 16 hex digits
// (none where the sequence has no slot), "row <file> <ch>" and 10 of them; "ok" as the last line if nothing failed.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gait_smoothness.h"

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

// the three kernels for one channel; x: the channel's T values, 4 apart
static void channel(int T, const SmoRule& r, const double* x, const int32_t* exclude, std::vector<double>& seg, std::vector<double>& row) {
    const int L = r.segment, N = r.nfft, kc = smo_cut_bin(r), bins = kc + 1, slots = spec_run_segments(T, L, r.hop);
    std::vector<unsigned long long> mask((size_t)(T + 63) / 64, 0ull);
    long long n = 0;
    for (int t = 0; t < T; ++t)
        if (translation_detail::finite(ent_diff(x, exclude, t, T, r.derivative))) { mask[t >> 6] |= 1ull << (t & 63); ++n; }
    seg.assign((size_t)slots * kSmoSegCols, -7.);
    const int candidates = spec_runs(mask.data(), T, L, r.hop, [&](int s, int t0) {
        EXPECT(s < slots, "segment %d of at most %d", s, slots);
        if (s < slots) seg[(size_t)s * kSmoSegCols + kSmoColStart] = (double)t0;
    });
    for (size_t e = (size_t)candidates * kSmoSegCols; e < seg.size(); ++e) seg[e] = std::nan("");
    std::vector<double> tw((size_t)2 * N), xs((size_t)L), ys((size_t)L), M((size_t)bins), term((size_t)kc);
    for (int j = 0; j < N; ++j) har_twiddle(j, N, &tw[2 * j], &tw[2 * j + 1]);
    for (int s = 0; s < candidates; ++s) {
        double* out = &seg[(size_t)s * kSmoSegCols];
        const int t0 = (int)out[kSmoColStart];
        for (int i = 0; i < L; ++i) {
            xs[i] = x[(size_t)(t0 + i) * kRegChannels];
            ys[i] = ent_diff(x, exclude, t0 + i, T, r.derivative);
        }
        for (int k = 0; k < bins; ++k) M[k] = smo_magnitude(ys.data(), L, tw.data(), N, k);
        if (smo_segment(M.data(), bins, r.amplitude, term.data(), out)) smo_jerk(xs.data(), L, &out[kSmoColDj], &out[kSmoColVPeak]);
        else out[kSmoColDj] = out[kSmoColVPeak] = std::nan("");
    }
    row.assign(kSmoSeqCols, -7.);
    const int used = spec_used(candidates, r.min_segments);
    row[kSmoColN] = (double)n;
    row[kSmoColCandidates] = (double)candidates;
    row[kSmoColUsed] = (double)used;
    smo_row(seg.data(), kSmoSegCols, candidates, used, r, row.data());
}

static void check_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); ++failures; return; }
    std::vector<int32_t> head, exclude;
    std::vector<double> scalars, signals;
    if (!(read_n(f, head, 8) && read_n(f, scalars, 3))) { std::printf("%s: short header\n", path); std::fclose(f); ++failures; return; }
    const int T = head[0];
    const SmoRule r{scalars[0], head[2], head[3], head[4], head[5], scalars[1], scalars[2], head[6]};
    const int off[2] = {0, T};
    if (const char* why = smo_rule_error(r)) {
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
        std::vector<double> seg, row;
        channel(T, r, signals.data() + ch, head[1] ? exclude.data() : nullptr, seg, row);
        print_bits("seg", path, ch, seg);
        print_bits("row", path, ch, row);
    }
}

// what no file reaches: the cut-off bin, the peak's merge in either order, the slots, and the rule at its limits
static void check_rules() {
    const double nan = std::nan(""), inf = INFINITY;
    const SmoRule base{20., 1, 64, 32, 1024, 10., 0.05, 2};
    EXPECT(smo_cut_bin(base) == 512, "the default cut-off bin is %d", smo_cut_bin(base));
    EXPECT(smo_cut_bin(SmoRule{20., 1, 8, 4, 64, 3., 0.05, 2}) == 9, "3 Hz of 64 points at 20 fps is bin %d", smo_cut_bin(SmoRule{20., 1, 8, 4, 64, 3., 0.05, 2}));
    const SmoPeak a{2., 5}, b{2., 3}, c{3., 9}, none = smo_peak_none();
    EXPECT(smo_peak_merge(a, b).k == 3 && smo_peak_merge(b, a).k == 3 && smo_peak_merge(a, c).k == 9 && smo_peak_merge(c, a).k == 9, "the peak's merge depends on the order");
    EXPECT(smo_peak_merge(none, a).k == 5 && smo_peak_merge(a, none).k == 5 && !smo_peak_holds(smo_peak_take(none, 0., 0)) && !smo_peak_holds(smo_peak_take(none, nan, 0)) &&
               !smo_peak_holds(smo_peak_take(none, inf, 0)) && smo_peak_holds(a),
           "the peak of nothing, of zeros, of NaN and of infinity");
    const int off[4] = {0, 63, 63 + 64, 63 + 64 + 400};
    long long slots[4];
    smo_slot_offsets(off, 3, 64, 32, slots);
    EXPECT(slots[0] == 0 && slots[1] == 0 && slots[2] == 1 && slots[3] == 12, "the slots of 63, 64 and 400 frames: %lld %lld %lld", slots[1], slots[2], slots[3]);
    const SmoRule limits[] = {base, {1e-3, 0, 8, 1, 8, 5e-4, 1., 1}, {1e6, 2, 256, 256, 4096, 5e5, 1e-300, 1 << 20}, {20., 1, 256, 32, 256, 0.01, 0.05, 2}};
    for (const auto& r : limits) EXPECT(smo_rule_error(r) == nullptr, "a rule at the limits is refused: %s", smo_rule_error(r));
    const struct { SmoRule r; const char* word; } bad[] = {
        {{0., 1, 64, 32, 1024, 10., .05, 2}, "fps"}, {{nan, 1, 64, 32, 1024, 10., .05, 2}, "fps"}, {{inf, 1, 64, 32, 1024, 10., .05, 2}, "fps"},
        {{20., -1, 64, 32, 1024, 10., .05, 2}, "derivative"}, {{20., 3, 64, 32, 1024, 10., .05, 2}, "derivative"}, {{20., 1, 6, 3, 1024, 10., .05, 2}, "segment"},
        {{20., 1, 63, 32, 1024, 10., .05, 2}, "segment"}, {{20., 1, 258, 64, 1024, 10., .05, 2}, "segment"}, {{20., 1, 64, 7, 1024, 10., .05, 2}, "hop"},
        {{20., 1, 64, 65, 1024, 10., .05, 2}, "hop"}, {{20., 1, 64, 32, 1024, 10., .05, 0}, "min_segments"}, {{20., 1, 64, 32, 1024, 10., .05, (1 << 20) + 1}, "min_segments"},
        {{20., 1, 64, 32, 62, 10., .05, 2}, "nfft"}, {{20., 1, 64, 32, 1023, 10., .05, 2}, "nfft"}, {{20., 1, 64, 32, 4098, 10., .05, 2}, "nfft"},
        {{20., 1, 64, 32, 1024, 0., .05, 2}, "f_cut"}, {{20., 1, 64, 32, 1024, 10.5, .05, 2}, "f_cut"}, {{20., 1, 64, 32, 1024, nan, .05, 2}, "f_cut"},
        {{20., 1, 64, 32, 1024, 10., 0., 2}, "amplitude"}, {{20., 1, 64, 32, 1024, 10., 1.5, 2}, "amplitude"}, {{20., 1, 64, 32, 1024, 10., nan, 2}, "amplitude"}};
    for (const auto& b : bad) {
        const char* why = smo_rule_error(b.r);
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
