// csrc/gait_harmonics.h on the host: a stand-alone program (its own main, no HIP, nothing of the library but that header and the ones it includes),
// built with AddressSanitizer and UBSan by tests/test_harmonics_host_cpu.py and run directly on one file per case, which the test writes: the inputs
// of ONE sequence and what pipeline.gait_harmonics (or, of a case on signals, pipeline.gait_stride_dft) made of them with sigma = 0.  The program runs
// the chain the kernels run -- reg_frame, the two heel-strike masks, har_walk, har_stride into the slots, har_summary, har_spectrum -- in buffers of
// exactly the sizes the call states, so that an index outside them is caught.  Every bit must be equal (a NaN equals a NaN).
//
// The file, little-endian: int32 [T, J, has_trans, has_exclude, n_harmonics, derivative, min_stride, max_stride, max_strides], int32 table[8], float64
// [fps], then float32 joints[T J 3] or, where J is 0, float64 signals[T 4]; int32 events[T]; float64 trans[T 3] and int32 exclude[T] where stated; then
// the expected float64 per_frame[T 4] (not where J is 0), strides[4 max_strides 6], spectrum[4 n_harmonics 2], per_seq[4 12].  Prints what differs,
// and "ok" as its last line if nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gait_harmonics.h"

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

// stages (a) to (c) of har_sequence_stages for one channel, a loop where the device has a wave or a lane each; x: the channel's T values, 4 apart
static void channel(int T, const HarRule& r, bool odd, const double* x, const int32_t* events, const int32_t* exclude, double* rows, double* spectrum, double* out) {
    const int words = ((T - 1) >> 6) + 1, width = r.n_harmonics + kHarSlotTail, room = har_slot_room(T);
    std::vector<unsigned long long> m_l((size_t)words, 0ull), m_r((size_t)words, 0ull);
    for (int t = 0; t < T; ++t) {
        if (events[t] & kGaitHeelL) m_l[t >> 6] |= 1ull << (t & 63);
        if (events[t] & kGaitHeelR) m_r[t >> 6] |= 1ull << (t & 63);
    }
    std::vector<double> slots((size_t)room * width, -7.), y(kHarMaxStride + 1), sn(kHarMaxStride + 1), cs(kHarMaxStride + 1), amp((size_t)r.n_harmonics);
    int eligible = 0;
    const long long candidates = har_walk(m_l.data(), m_r.data(), T, [&](long long c, int foot, int t0, int t1) {
        const int L = t1 - t0;
        double HR, iHR;
        const int H = har_stride(x, kRegChannels, exclude, r, odd, t0, t1, y.data(), sn.data(), cs.data(), amp.data(), &HR, &iHR);
        if (L >= r.min_stride && L <= r.max_stride) {
            EXPECT(eligible < room, "stride %lld is the %d-th of an allowed length: more than the %d slots of %d frames", c, eligible + 1, room, T);
            if (eligible < room) {
                double* s = slots.data() + (size_t)eligible * width;
                for (int k = 0; k < r.n_harmonics; ++k) s[k] = amp[k];
                har_slot_tail(s, r.n_harmonics, HR, iHR, H, foot, L);
            }
            ++eligible;
        }
        if (c < r.max_strides) {
            double* row = rows + (size_t)c * kHarStrideCols;
            row[0] = (double)t0; row[1] = (double)t1; row[2] = foot ? -1. : 1.; row[3] = (double)H; row[4] = HR; row[5] = iHR;
        }
    });
    const long long n_slots = eligible < room ? eligible : room;
    har_summary(slots.data(), n_slots, r.n_harmonics, candidates, r.fps, out);
    for (int k = 1; k <= r.n_harmonics; ++k) har_spectrum(slots.data(), n_slots, r.n_harmonics, k, spectrum + (size_t)(k - 1) * 2);
    for (long long e = (candidates < r.max_strides ? candidates : r.max_strides) * kHarStrideCols; e < (long long)r.max_strides * kHarStrideCols; ++e) rows[e] = std::nan("");
}

static int check_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); ++failures; return 1; }
    std::vector<int32_t> head, table, events, exclude;
    std::vector<double> scalars, signals, trans, want_frame, want_strides, want_spectrum, want_seq;
    std::vector<float> joints;
    bool ok = read_n(f, head, 9) && read_n(f, table, 8) && read_n(f, scalars, 1);
    if (!ok) { std::printf("%s: short header\n", path); std::fclose(f); ++failures; return 1; }
    const int T = head[0], J = head[1];
    const HarRule r{scalars[0], head[4], head[5], head[6], head[7], head[8]};
    EXPECT(har_rule_error(r) == nullptr, "%s: its rule is refused: %s", path, har_rule_error(r));
    if (har_rule_error(r)) { std::fclose(f); return 1; }
    const size_t n_strides = (size_t)kRegChannels * r.max_strides * kHarStrideCols, n_spectrum = (size_t)kRegChannels * r.n_harmonics * 2;
    ok = (J ? read_n(f, joints, (size_t)T * J * 3) : read_n(f, signals, (size_t)T * kRegChannels)) && read_n(f, events, (size_t)T) &&
         read_n(f, trans, head[2] ? (size_t)T * 3 : 0) && read_n(f, exclude, head[3] ? (size_t)T : 0) && read_n(f, want_frame, J ? (size_t)T * kRegChannels : 0) &&
         read_n(f, want_strides, n_strides) && read_n(f, want_spectrum, n_spectrum) && read_n(f, want_seq, (size_t)kRegChannels * kHarSeqCols);
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
    std::vector<double> strides(n_strides, -7.), spectrum(n_spectrum, -7.), seq((size_t)kRegChannels * kHarSeqCols, -7.);
    for (int ch = 0; ch < kRegChannels; ++ch)
        channel(T, r, reg_odd(ch), signals.data() + ch, events.data(), head[3] ? exclude.data() : nullptr, strides.data() + (size_t)ch * r.max_strides * kHarStrideCols,
                spectrum.data() + (size_t)ch * r.n_harmonics * 2, seq.data() + (size_t)ch * kHarSeqCols);
    for (size_t i = 0; i < strides.size(); ++i)
        EXPECT(same(strides[i], want_strides[i]), "%s: strides[%zu] = %.17g, not %.17g", path, i, strides[i], want_strides[i]);
    for (size_t i = 0; i < spectrum.size(); ++i)
        EXPECT(same(spectrum[i], want_spectrum[i]), "%s: spectrum[%zu] = %.17g, not %.17g", path, i, spectrum[i], want_spectrum[i]);
    for (size_t i = 0; i < seq.size(); ++i)
        EXPECT(same(seq[i], want_seq[i]), "%s: per_seq[%zu][%zu] = %.17g, not %.17g", path, i / kHarSeqCols, i % kHarSeqCols, seq[i], want_seq[i]);
    return failures - before;
}

// what no file reaches: the exact twiddles, H at the edges, the slots' places, and every refusal of the rule
static void check_rules() {
    for (int L = kHarMinStrideLimit; L <= kHarMaxStride; ++L) {
        double s, c;
        har_twiddle(0, L, &s, &c);
        EXPECT(s == 0. && c == 1., "L %d: j = 0 gives (%g, %g)", L, s, c);
        if (L % 4 == 0) {
            const double want[4][2] = {{0., 1.}, {1., 0.}, {0., -1.}, {-1., 0.}};
            for (int q = 0; q < 4; ++q) {
                har_twiddle(q * L / 4, L, &s, &c);
                EXPECT(s == want[q][0] && c == want[q][1], "L %d: quarter %d gives (%g, %g)", L, q, s, c);
            }
        }
        for (int j = 0; j < L; ++j) {
            har_twiddle(j, L, &s, &c);
            EXPECT(std::fabs(s * s + c * c - 1.) < 2e-15, "L %d j %d: sin^2 + cos^2 = 1 + %g", L, j, s * s + c * c - 1.);
        }
    }
    EXPECT(har_harmonics(20, 6) == 2 && har_harmonics(20, 7) == 2 && har_harmonics(20, 8) == 2 && har_harmonics(20, 9) == 4 && har_harmonics(20, 255) == 20 &&
           har_harmonics(32, 64) == 30 && har_harmonics(32, 65) == 32 && har_harmonics(2, 255) == 2, "H at the edges");
    // sequences of 1, 7 and 800 frames lying back to back: no two overlap and the last ends inside the call's slots
    const int lens[] = {1, 7, 800, 2, 3, 5}, n_seq = 6;
    int f0 = 0;
    size_t end = 0;
    for (int q = 0; q < n_seq; ++q) {
        EXPECT(har_slot_at(f0, q) >= end, "sequence %d begins at slot %zu, before %zu", q, har_slot_at(f0, q), end);
        end = har_slot_at(f0, q) + (size_t)har_slot_room(lens[q]);
        EXPECT(2 * ((lens[q] - 1) / kHarMinStrideLimit) <= har_slot_room(lens[q]), "%d frames have more strides than slots", lens[q]);
        f0 += lens[q];
    }
    EXPECT(end <= har_slots(f0, n_seq), "the last sequence ends at slot %zu of %zu", end, har_slots(f0, n_seq));
    const double nan = std::nan(""), inf = INFINITY;
    const HarRule good{20., 20, 2, 8, 60, 128};
    const struct { HarRule r; const char* word; } bad[] = {
        {{0., 20, 2, 8, 60, 128}, "fps"}, {{-1., 20, 2, 8, 60, 128}, "fps"}, {{nan, 20, 2, 8, 60, 128}, "fps"}, {{inf, 20, 2, 8, 60, 128}, "fps"},
        {{20., 0, 2, 8, 60, 128}, "n_harmonics"}, {{20., 21, 2, 8, 60, 128}, "n_harmonics"}, {{20., 34, 2, 8, 60, 128}, "n_harmonics"},
        {{20., 20, -1, 8, 60, 128}, "derivative"}, {{20., 20, 3, 8, 60, 128}, "derivative"}, {{20., 20, 2, 8, 256, 128}, "max_stride"},
        {{20., 20, 2, 5, 60, 128}, "min_stride"}, {{20., 20, 2, 61, 60, 128}, "min_stride"}, {{20., 20, 2, 8, 60, 0}, "max_strides"},
        {{20., 20, 2, 8, 60, 513}, "max_strides"}};
    EXPECT(har_rule_error(good) == nullptr, "the default rule is refused: %s", har_rule_error(good));
    for (const auto& b : bad) {
        const char* why = har_rule_error(b.r);
        EXPECT(why && std::strstr(why, b.word) == why, "a bad %s is %s", b.word, why ? why : "not refused");
    }
    const HarRule limits[] = {{20., 2, 0, 6, 6, 1}, {20., 32, 2, 255, 255, 512}, {20., 20, 1, 6, 255, 128}};
    for (const auto& r : limits) EXPECT(har_rule_error(r) == nullptr, "a rule at the limits is refused: %s", har_rule_error(r));
}

int main(int argc, char** argv) {
    check_rules();
    for (int i = 1; i < argc; ++i) check_file(argv[i]);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
