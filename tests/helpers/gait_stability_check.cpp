// csrc/gait_stability.h on the host: a stand-alone program (its own main, no HIP, nothing of the library but that header and the ones it includes),
// built with AddressSanitizer and UBSan by tests/test_stability_host_cpu.py and run directly on one file per case, which the test writes: the inputs
// of ONE sequence and what pipeline.gait_stability (or, of a case on signals, pipeline.gait_divergence) made of them with sigma = 0.  The program runs
// the chain the kernels run -- reg_frame, ent_diff, stab_scan in tiles of kStabTile, stab_walk_dim with a loop where the device has a lane -- in
// buffers of exactly the sizes the call states, so that an index outside them is caught.  Every integer and every bit must be equal (a NaN equals a
// NaN).  A case that the rules refuse is answered with a line "refused <file>: <why>", in the words the library and the statement use.
//
// The file, little-endian: int32 [T, J, has_trans, has_exclude, derivative, dim, lag, theiler, horizon, has_data], int32 table[8]; then, where
// has_data, float32 joints[T J 3] or, where J is 0, float64 signals[T 4]; float64 trans[T 3] and int32 exclude[T] where stated; then the expected
// float64 per_frame[T 4] (not where J is 0), int32 nn[T 4], int64 pairs[4 (horizon+1) 2], float64 mant[4 (horizon+1)].  Prints what differs, and "ok"
// as its last line if nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gait_stability.h"

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

// the search of one reference as the device runs it: the candidates in tiles, each a buffer of its own of exactly n + span values
template <int DIM>
static int nearest(const double* x, const int32_t* exclude, int T, const StabRule& r, const StabPoints& p, int i) {
    double a[DIM];
    bool mine = true;
    for (int c = 0; c < DIM; ++c) {
        a[c] = ent_diff(x, exclude, i + c * r.lag, T, r.derivative);
        mine = mine && translation_detail::finite(a[c]);
    }
    double best = 0.;
    int best_j = -1;
    for (int j0 = 0; j0 < p.E && mine; j0 += kStabTile) {
        const int n = p.E - j0 < kStabTile ? p.E - j0 : kStabTile;
        std::vector<double> tile((size_t)n + p.span);
        for (int t = 0; t < n + p.span; ++t) tile[t] = ent_diff(x, exclude, j0 + t, T, r.derivative);
        stab_scan<DIM>(a, tile.data(), j0, n, i, r.theiler, r.lag, &best, &best_j);
    }
    return best_j;
}

static int nearest_dim(const double* x, const int32_t* exclude, int T, const StabRule& r, const StabPoints& p, int i) {
    switch (r.dim) {
        case 2: return nearest<2>(x, exclude, T, r, p, i);
        case 3: return nearest<3>(x, exclude, T, r, p, i);
        case 4: return nearest<4>(x, exclude, T, r, p, i);
        case 5: return nearest<5>(x, exclude, T, r, p, i);
        case 6: return nearest<6>(x, exclude, T, r, p, i);
        case 7: return nearest<7>(x, exclude, T, r, p, i);
        default: return nearest<8>(x, exclude, T, r, p, i);
    }
}

// the two kernels for one channel; x: the channel's T values, 4 apart; nn: the channel's T neighbours, 4 apart
static void channel(int T, const StabRule& r, const double* x, const int32_t* exclude, int32_t* nn, long long* pairs, double* mant) {
    const StabPoints p = stab_points(T, r);
    for (int i = 0; i < T; ++i) nn[(size_t)i * kRegChannels] = i < p.E ? nearest_dim(x, exclude, T, r, p, i) : -1;
    std::vector<double> y((size_t)T);
    for (int t = 0; t < T; ++t) y[t] = ent_diff(x, exclude, t, T, r.derivative);
    for (int k = 0; k <= r.horizon; ++k) stab_walk_dim(y.data(), nn, kRegChannels, T, r, k, pairs + (size_t)k * kStabPairCols, mant + k);
}

static int check_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); ++failures; return 1; }
    std::vector<int32_t> head, table, exclude, want_nn;
    std::vector<double> signals, trans, want_frame, want_mant;
    std::vector<long long> want_pairs;
    std::vector<float> joints;
    bool ok = read_n(f, head, 10) && read_n(f, table, 8);
    if (!ok) { std::printf("%s: short header\n", path); std::fclose(f); ++failures; return 1; }
    const int T = head[0], J = head[1];
    const StabRule r{head[4], head[5], head[6], head[7], head[8]};
    const int off[2] = {0, T};
    if (const char* why = stab_rule_error(r)) {
        EXPECT(!head[9], "%s: its rule is refused: %s", path, why);
        std::printf("refused %s: %s\n", path, why);
        std::fclose(f);
        return 0;
    }
    if (ent_long_sequence(off, 1) >= 0) {
        EXPECT(!head[9], "%s: its length is refused", path);
        std::printf("refused %s: sequence %d has %d frames, more than %d (the work is quadratic in them)\n", path, ent_long_sequence(off, 1), T, kEntMaxFrames);
        std::fclose(f);
        return 0;
    }
    EXPECT(head[9], "%s: a case without data is not refused", path);
    if (!head[9]) { std::fclose(f); return 1; }
    const size_t curve = (size_t)r.horizon + 1;
    ok = (J ? read_n(f, joints, (size_t)T * J * 3) : read_n(f, signals, (size_t)T * kRegChannels)) && read_n(f, trans, head[2] ? (size_t)T * 3 : 0) &&
         read_n(f, exclude, head[3] ? (size_t)T : 0) && read_n(f, want_frame, J ? (size_t)T * kRegChannels : 0) && read_n(f, want_nn, (size_t)T * kRegChannels) &&
         read_n(f, want_pairs, kRegChannels * curve * kStabPairCols) && read_n(f, want_mant, kRegChannels * curve);
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
    std::vector<int32_t> nn((size_t)T * kRegChannels, -7);
    std::vector<long long> pairs(kRegChannels * curve * kStabPairCols, -7);
    std::vector<double> mant(kRegChannels * curve, -7.);
    for (int ch = 0; ch < kRegChannels; ++ch)
        channel(T, r, signals.data() + ch, head[3] ? exclude.data() : nullptr, nn.data() + ch, pairs.data() + ch * curve * kStabPairCols, mant.data() + ch * curve);
    for (size_t i = 0; i < nn.size(); ++i)
        EXPECT(nn[i] == want_nn[i], "%s: nn[%zu][%zu] = %d, not %d", path, i / kRegChannels, i % kRegChannels, nn[i], want_nn[i]);
    for (size_t i = 0; i < pairs.size(); ++i)
        EXPECT(pairs[i] == want_pairs[i], "%s: pairs[%zu][%zu][%zu] = %lld, not %lld", path, i / (curve * kStabPairCols), i / kStabPairCols % curve, i % kStabPairCols, pairs[i],
               want_pairs[i]);
    for (size_t i = 0; i < mant.size(); ++i) EXPECT(same(mant[i], want_mant[i]), "%s: mant[%zu][%zu] = %.17g, not %.17g", path, i / curve, i % curve, mant[i], want_mant[i]);
    return failures - before;
}

// what no file reaches: stab_frexp against C's frexp down to the smallest subnormal, and the rule at its limits
static void check_rules() {
    const double values[] = {1., 0.5, 0.75, 3., 1e-300, 1e300, 2.2250738585072014e-308, 2.2250738585072009e-308, 4.9406564584124654e-324, 1.5e-323, 1.7976931348623157e308,
                             0.1, 5., 1e-310, 3.3e-320};
    for (double v : values) {
        int e = 0, want_e = 0;
        const double f = stab_frexp(v, &e), want = std::frexp(v, &want_e);
        EXPECT(same(f, want) && e == want_e, "stab_frexp(%.17g) = %.17g 2^%d, not %.17g 2^%d", v, f, e, want, want_e);
    }
    int e = 0;
    (void)stab_frexp(0., &e);                                   // never used, and nothing undefined either
    (void)stab_frexp(std::nan(""), &e);
    const StabRule limits[] = {{1, 5, 2, 20, 20}, {0, 2, 1, 0, 1}, {2, 8, 16, 4096, 63}};
    for (const auto& r : limits) EXPECT(stab_rule_error(r) == nullptr, "a rule at the limits is refused: %s", stab_rule_error(r));
    const struct { StabRule r; const char* word; } bad[] = {
        {{-1, 5, 2, 20, 20}, "derivative"}, {{3, 5, 2, 20, 20}, "derivative"}, {{1, 1, 2, 20, 20}, "dim"}, {{1, 9, 2, 20, 20}, "dim"}, {{1, 5, 0, 20, 20}, "lag"},
        {{1, 5, 17, 20, 20}, "lag"}, {{1, 5, 2, -1, 20}, "theiler"}, {{1, 5, 2, 4097, 20}, "theiler"}, {{1, 5, 2, 20, 0}, "horizon"}, {{1, 5, 2, 20, 64}, "horizon"}};
    for (const auto& b : bad) {
        const char* why = stab_rule_error(b.r);
        EXPECT(why && std::strstr(why, b.word) == why, "a bad %s is %s", b.word, why ? why : "not refused");
    }
    const StabPoints p = stab_points(400, limits[0]), none = stab_points(8, limits[0]), most = stab_points(kEntMaxFrames, limits[2]);
    EXPECT(p.span == 8 && p.M == 392 && p.E == 372, "400 frames: span %d, M %d, E %d", p.span, p.M, p.E);
    EXPECT(none.M == 0 && none.E == 0, "8 frames: M %d, E %d", none.M, none.E);
    EXPECT(most.span == kStabMaxSpan && most.E == kEntMaxFrames - kStabMaxSpan - kStabMaxHorizon, "the longest: span %d, E %d", most.span, most.E);
}

int main(int argc, char** argv) {
    check_rules();
    for (int i = 1; i < argc; ++i) check_file(argv[i]);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
