// csrc/gait_events.h on the host: a stand-alone program (its own main, no HIP, nothing of the library but that header and the ones it includes), built
// with AddressSanitizer and UBSan by tests/test_gait_host_cpu.py and run directly on one file per case, which the test writes: the inputs of ONE
// sequence and what pipeline.gait_parameters made of them.  The program runs the chain the kernels run -- gait_frame, track_gauss, gait_frame_events
// and the ballots' bitmasks, the per-sequence columns -- in buffers of exactly the sizes the call states, so that an index outside them is caught.
//
// The file, little-endian: int32 [T, J, window, has_trans, radius (-1: no Gaussian)], int32 table[8], float64 [fps, min_excursion], float64
// bar_frame[7], float64 bar_seq[18], float32 joints[T J 3], float64 trans[T 3] (has_trans), float64 weights[radius + 1] (radius >= 0), then the
// expected float64 per_frame[T 7], int32 events[T], float64 per_seq[18].  A bar of 0: every bit equal (a NaN equals a NaN); the test puts bars > 0
// (tests/helpers/gait_checks.py) on the columns a Gaussian reaches, whose sum the two sides order differently.  The events are always equal.
// Prints what differs, and "ok" as its last line if nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gait_events.h"

using namespace grk;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

template <class V>
static bool read_n(std::FILE* f, std::vector<V>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(V), n, f) == n;
}

static bool same(double a, double b, double tol) {
    if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
    if (tol == 0.) return std::memcmp(&a, &b, sizeof a) == 0;
    return std::fabs(a - b) <= tol;
}

static int check_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); return 1; }
    std::vector<int32_t> head, table, want_events;
    std::vector<double> scalars, bar_frame, bar_seq, trans, weights, want_frame, want_seq;
    std::vector<float> joints;
    bool ok = read_n(f, head, 5) && read_n(f, table, 8) && read_n(f, scalars, 2) && read_n(f, bar_frame, kGaitFrameCols) && read_n(f, bar_seq, kGaitSeqCols);
    if (!ok) { std::printf("%s: short header\n", path); std::fclose(f); return 1; }
    const int T = head[0], J = head[1], window = head[2], has_trans = head[3], radius = head[4];
    const double fps = scalars[0], min_excursion = scalars[1];
    ok = read_n(f, joints, (size_t)T * J * 3) && read_n(f, trans, has_trans ? (size_t)T * 3 : 0) && read_n(f, weights, radius >= 0 ? (size_t)radius + 1 : 0) &&
         read_n(f, want_frame, (size_t)T * kGaitFrameCols) && read_n(f, want_events, (size_t)T) && read_n(f, want_seq, (size_t)kGaitSeqCols);
    std::fclose(f);
    if (!ok) { std::printf("%s: short file\n", path); return 1; }

    int tab[kGaitTable];
    for (int k = 0; k < kGaitTable; ++k) tab[k] = table[k];
    std::vector<double> rows((size_t)T * kGaitFrameCols), raw((size_t)4 * T);
    for (int t = 0; t < T; ++t) {
        double sig[5];
        gait_frame(joints.data() + (size_t)t * J * 3, tab, sig);
        for (int k = 0; k < 4; ++k) raw[(size_t)k * T + t] = sig[k];
        rows[(size_t)t * kGaitFrameCols + 4] = sig[4];
    }
    for (int k = 0; k < 4; ++k)
        for (int t = 0; t < T; ++t)
            rows[(size_t)t * kGaitFrameCols + k] = radius >= 0 ? track_gauss(raw.data() + (size_t)k * T, T, t, weights.data(), radius) : raw[(size_t)k * T + t];
    const size_t n_words = (size_t)((T - 1) >> 6) + 1;
    std::vector<unsigned long long> mask[4];
    for (auto& m : mask) m.assign(n_words, 0ull);
    std::vector<int32_t> events((size_t)T);
    for (int t = 0; t < T; ++t) {
        events[t] = gait_frame_events(rows.data(), T, t, window, min_excursion);
        for (int k = 0; k < 4; ++k)
            if ((events[t] >> k) & 1) mask[k][t >> 6] |= 1ull << (t & 63);
    }
    std::vector<double> seq((size_t)kGaitSeqCols, -7.);
    for (int k = 0; k < 4; ++k) seq[kGaitColCounts + k] = gait_count(mask[k].data(), T);
    gait_steps(mask[0].data(), mask[1].data(), T, rows.data(), fps, seq.data());
    gait_strides(mask[0].data(), mask[1].data(), T, fps, seq.data());
    gait_stance(mask[0].data(), mask[1].data(), mask[2].data(), mask[3].data(), T, seq.data());
    gait_traj_speed(mask[0].data(), mask[1].data(), T, joints.data(), J, tab[0], has_trans ? trans.data() : nullptr, fps, seq.data());

    const int before = failures;
    for (int t = 0; t < T; ++t) {
        EXPECT(events[t] == want_events[t], "%s: events[%d] = %d, not %d", path, t, events[t], want_events[t]);
        for (int c = 0; c < kGaitFrameCols; ++c) {
            const double got = rows[(size_t)t * kGaitFrameCols + c], want = want_frame[(size_t)t * kGaitFrameCols + c];
            EXPECT(same(got, want, bar_frame[c]), "%s: per_frame[%d][%d] = %.17g, not %.17g", path, t, c, got, want);
        }
    }
    for (int c = 0; c < kGaitSeqCols; ++c) EXPECT(same(seq[c], want_seq[c], bar_seq[c]), "%s: per_seq[%d] = %.17g, not %.17g", path, c, seq[c], want_seq[c]);
    return failures - before;
}

// what no file reaches: the searches over word boundaries and the events rule at the ends of a sequence
static void check_rules() {
    const double s[13] = {0, 1, 3, 3, -2, -4, -1, -4, -6, -2, 0, 4, 2};       // the hand-made signal of tests/test_gait_host_cpu.py, window 2
    for (int t = 0; t < 13; ++t) {
        const bool hs = gait_heel_strike(s, 1, 13, t, 2, 1.), to = gait_toe_off(s, 1, 13, t, 2, 1.);
        EXPECT(hs == (t == 2), "heel strike at %d: %d", t, (int)hs);      // the plateau 3, 3: the earlier frame; -1 at frame 6: negative; 4 at frame 11: no whole window
        EXPECT(to == (t == 5 || t == 8), "toe-off at %d: %d", t, (int)to);      // -4 at 5 and 7: the earlier frame
    }
    std::vector<unsigned long long> l(3, 0ull), r(3, 0ull);
    for (int g : {10, 63, 64, 150}) l[g >> 6] |= 1ull << (g & 63);
    for (int g : {40, 64, 130}) r[g >> 6] |= 1ull << (g & 63);
    const int want[7][2] = {{10, 0}, {40, 1}, {63, 0}, {64, 0}, {64, 1}, {130, 1}, {150, 0}};
    int t = -1, foot = 1, n = 0;
    while (gait_next_strike(l.data(), r.data(), 151, &t, &foot)) {
        EXPECT(n < 7 && t == want[n < 7 ? n : 0][0] && foot == want[n < 7 ? n : 0][1], "strike %d = (%d, %d)", n, t, foot);
        ++n;
    }
    EXPECT(n == 7, "%d strikes, not 7", n);
    EXPECT(gait_count(l.data(), 151) == 4. && gait_count(r.data(), 151) == 3., "counts");
}

int main(int argc, char** argv) {
    check_rules();
    for (int i = 1; i < argc; ++i) check_file(argv[i]);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
