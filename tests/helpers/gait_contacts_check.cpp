// csrc/gait_contacts.h on the host: a stand-alone program (its own main, no HIP, nothing of the library but that header and the ones it includes),
// built with AddressSanitizer and UBSan by tests/test_contacts_host_cpu.py and run directly on one file per case, which the test writes: the inputs
// of ONE sequence and what pipeline.gait_contacts (or, of a case on speeds, pipeline.gait_contact_runs) made of them with sigma = 0.  The program
// runs the chain the kernels run -- contact_vector and contact_speed, the block sums and the threshold, the ballots' bitmasks, the runs by the lane at
// their first interval, the phases and the run table, the per-sequence columns -- in buffers of exactly the sizes the call states, so that an index
// outside them is caught.  Every bit must be equal (a NaN equals a NaN).
//
// The file, little-endian: int32 [T, J, reach, max_frames, max_runs], int32 table[8], float64 [fps, fraction, speed], then float32 joints[T J 3]
// or, where J is 0, float64 speeds[T]; int32 events[T]; then the expected float64 per_frame[T 4] (not where J is 0), int32 phase[T], float64
// runs[max_runs 6], float64 per_seq[20].  Prints what differs, and "ok" as its last line if nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gait_contacts.h"

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

struct Masks {
    std::vector<unsigned long long> w[kContactMaskSets];
    explicit Masks(int T) { for (auto& m : w) m.assign((size_t)((T - 1) >> 6) + 1, 0ull); }
    ContactMasks view() { return ContactMasks{w[0].data(), w[1].data(), w[2].data(), w[3].data(), w[4].data(), w[5].data()}; }
};
static void set_bit(unsigned long long* words, int t) { words[t >> 6] |= 1ull << (t & 63); }
constexpr int kKept = 4;                                       // runs the checker keeps, where the kernel keeps kContactKeptRuns

// stages (a) to (d) of contact_sequence_stages, a loop over the intervals where the device has a lane each; s: T - 1 speeds, `stride` values apart
static void sequence(int T, const ContactRule& r, const double* s, long long stride, const int32_t* events, int32_t* phase, double* runs, double* out) {
    Masks masks(T);
    const ContactMasks m = masks.view();
    const int words = ((T - 1) >> 6) + 1;
    std::vector<double> blocks((size_t)words);
    for (int w = 0; w < words; ++w) blocks[w] = contact_block_sum(s, stride, T - 1, w);
    for (int k = 0; k < T; ++k) {
        if (k < T - 1 && translation_detail::finite(s[k * stride])) set_bit(m.finite, k);
        if (events[k] & kGaitHeelL) set_bit(m.hs_l, k);
        if (events[k] & kGaitHeelR) set_bit(m.hs_r, k);
    }
    double mean;
    const double thr = contact_threshold(blocks.data(), m.finite, T, r, &mean);
    std::vector<double> kept_rows((size_t)kContactKeptCols * kKept, -7.);      // fewer than the sequences have runs: the row's walks take both ways to a run
    for (int k = 0; k < T - 1; ++k)
        if (s[k * stride] < thr) set_bit(m.is_static, k);
    for (int k = 0; k < T; ++k) {
        if (k == T - 1) { phase[k] = kContactNan; continue; }
        if (!gait_detail::bit(m.is_static, k)) {
            const double v = s[k * stride];
            phase[k] = v != v ? kContactNan : kContactMoving;
        } else if (contact_run_begins(m.is_static, k)) {
            const int b = contact_run_end(m.is_static, T, k) - 1;
            const ContactRun run = contact_run(m, s, stride, T, k, b, thr, r);
            if (run.lead > 0) set_bit(m.lead_l, k);
            if (run.lead < 0) set_bit(m.lead_r, k);
            for (int i = k; i <= b; ++i) phase[i] = contact_phase(run.lead);
            const long long row = contact_runs_before(m.is_static, k);
            if (row < r.max_runs) contact_row(run, r.fps, runs + row * kContactRunCols);
            if (row < kKept) contact_keep(kept_rows.data(), row, run.lead, run.t_start, run.t_end, b + 1);
        }
    }
    const long long found = contact_runs_before(m.is_static, T);
    for (int i = 0; i < r.max_runs * kContactRunCols; ++i)
        if (i / kContactRunCols >= found) runs[i] = gait_detail::nan();
    out[kContactColThr] = thr;
    out[kContactColMean] = mean;
    contact_counts(m, T, out);
    const ContactKept kept{kept_rows.data(), kKept, found};
    contact_support(m, kept, s, stride, T, thr, r.fps, out);
    contact_strides(m, kept, s, stride, T, thr, r.fps, out);
}

static int check_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); ++failures; return 1; }
    std::vector<int32_t> head, table, events, want_phase;
    std::vector<double> scalars, speeds, want_frame, want_runs, want_seq;
    std::vector<float> joints;
    bool ok = read_n(f, head, 5) && read_n(f, table, 8) && read_n(f, scalars, 3);
    if (!ok) { std::printf("%s: short header\n", path); std::fclose(f); ++failures; return 1; }
    const int T = head[0], J = head[1];
    const ContactRule r{scalars[0], scalars[1], scalars[2], head[2], head[3], head[4]};
    ok = (J ? read_n(f, joints, (size_t)T * J * 3) : read_n(f, speeds, (size_t)T)) && read_n(f, events, (size_t)T) &&
         read_n(f, want_frame, J ? (size_t)T * kContactFrameCols : 0) && read_n(f, want_phase, (size_t)T) &&
         read_n(f, want_runs, (size_t)r.max_runs * kContactRunCols) && read_n(f, want_seq, (size_t)kContactSeqCols);
    std::fclose(f);
    if (!ok) { std::printf("%s: short file\n", path); ++failures; return 1; }
    EXPECT(contact_rule_error(r) == nullptr, "%s: its rule is refused: %s", path, contact_rule_error(r));

    std::vector<double> rows, runs((size_t)r.max_runs * kContactRunCols, -7.), seq((size_t)kContactSeqCols, -7.);
    std::vector<int32_t> phase((size_t)T, -7);
    if (J) {
        int tab[kGaitTable];
        for (int k = 0; k < kGaitTable; ++k) tab[k] = table[k];
        rows.assign((size_t)T * kContactFrameCols, gait_detail::nan());
        for (int t = 0; t < T; ++t) contact_vector(joints.data() + (size_t)t * J * 3, tab, rows.data() + (size_t)t * kContactFrameCols + 1);
        for (int t = 0; t + 1 < T; ++t)
            rows[(size_t)t * kContactFrameCols] = contact_speed(rows.data() + (size_t)t * kContactFrameCols + 1, rows.data() + (size_t)(t + 1) * kContactFrameCols + 1, r.fps);
        sequence(T, r, rows.data(), kContactFrameCols, events.data(), phase.data(), runs.data(), seq.data());
    } else {
        speeds.resize((size_t)T - 1);                          // the last entry is not read: without it here, a read of it is caught
        sequence(T, r, speeds.data(), 1, events.data(), phase.data(), runs.data(), seq.data());
    }

    const int before = failures;
    for (int t = 0; t < T; ++t) {
        EXPECT(phase[t] == want_phase[t], "%s: phase[%d] = %d, not %d", path, t, phase[t], want_phase[t]);
        for (int c = 0; J && c < kContactFrameCols; ++c) {
            const double got = rows[(size_t)t * kContactFrameCols + c], want = want_frame[(size_t)t * kContactFrameCols + c];
            EXPECT(same(got, want), "%s: per_frame[%d][%d] = %.17g, not %.17g", path, t, c, got, want);
        }
    }
    for (size_t i = 0; i < runs.size(); ++i)
        EXPECT(same(runs[i], want_runs[i]), "%s: runs[%zu][%zu] = %.17g, not %.17g", path, i / kContactRunCols, i % kContactRunCols, runs[i], want_runs[i]);
    for (int c = 0; c < kContactSeqCols; ++c) EXPECT(same(seq[c], want_seq[c]), "%s: per_seq[%d] = %.17g, not %.17g", path, c, seq[c], want_seq[c]);
    return failures - before;
}

// what no file reaches: the counts of runs over word boundaries, the tree's shape, and every refusal of the rule
static void check_rules() {
    std::vector<unsigned long long> w(3, 0ull);
    for (int t = 62; t <= 66; ++t) set_bit(w.data(), t);       // one run across a word boundary
    set_bit(w.data(), 0);
    set_bit(w.data(), 63 + 64);
    set_bit(w.data(), 128);                                    // a run across the second boundary
    EXPECT(contact_runs_before(w.data(), 0) == 0 && contact_runs_before(w.data(), 1) == 1 && contact_runs_before(w.data(), 62) == 1 && contact_runs_before(w.data(), 63) == 2, "runs before, first word");
    EXPECT(contact_runs_before(w.data(), 64) == 2 && contact_runs_before(w.data(), 65) == 2 && contact_runs_before(w.data(), 127) == 2 && contact_runs_before(w.data(), 128) == 3, "runs before, over a word");
    EXPECT(contact_runs_before(w.data(), 129) == 3 && contact_runs_before(w.data(), 192) == 3, "runs before, the last word");
    EXPECT(contact_run_begins(w.data(), 62) && !contact_run_begins(w.data(), 64) && !contact_run_begins(w.data(), 128) && contact_run_end(w.data(), 192, 62) == 67 && contact_run_end(w.data(), 192, 127) == 129, "run ends");
    double x[130];
    for (int i = 0; i < 130; ++i) x[i] = 1. + std::ldexp((double)i, -50);      // additions that round: the order shows
    x[5] = std::nan("");
    x[70] = INFINITY;
    double by_hand = 0.;
    for (int b = 0; b < 3; ++b) {
        double v[64];
        for (int i = 0; i < 64; ++i) v[i] = b * 64 + i < 130 && std::isfinite(x[b * 64 + i]) ? x[b * 64 + i] : 0.;
        const double s01 = v[0] + v[1], s23 = v[2] + v[3];
        EXPECT(b != 0 || same(s01 + s23, (x[0] + x[1]) + (x[2] + x[3])), "adjacent pairs first");
        for (int width = 32; width >= 1; width /= 2)
            for (int i = 0; i < width; ++i) v[i] = v[2 * i] + v[2 * i + 1];
        EXPECT(same(v[0], contact_block_sum(x, 1, 130, b)), "block %d", b);
        by_hand = by_hand + v[0];
    }
    const double blocks[3] = {contact_block_sum(x, 1, 130, 0), contact_block_sum(x, 1, 130, 1), contact_block_sum(x, 1, 130, 2)};
    std::vector<unsigned long long> fin(3, 0ull);
    for (int i = 0; i < 130; ++i) if (std::isfinite(x[i])) set_bit(fin.data(), i);
    double mean;
    const ContactRule good{20., 0.25, 0., 2, 20, 128};
    const double thr = contact_threshold(blocks, fin.data(), 131, good, &mean);
    EXPECT(same(mean, by_hand / 128.) && same(thr, 0.25 * mean), "mean %.17g thr %.17g", mean, thr);
    const ContactRule fixed{20., 0.25, 0.5, 2, 20, 128};
    EXPECT(contact_threshold(blocks, fin.data(), 131, fixed, &mean) == 0.5, "speed replaces the relative threshold");
    const double nan = std::nan(""), inf = INFINITY;
    const struct { ContactRule r; const char* word; } bad[] = {
        {{0., 0.25, 0., 2, 20, 128}, "fps"}, {{-20., 0.25, 0., 2, 20, 128}, "fps"}, {{nan, 0.25, 0., 2, 20, 128}, "fps"}, {{inf, 0.25, 0., 2, 20, 128}, "fps"},
        {{20., -0.1, 0., 2, 20, 128}, "fraction"}, {{20., nan, 0., 2, 20, 128}, "fraction"}, {{20., inf, 0., 2, 20, 128}, "fraction"},
        {{20., 0.25, -1., 2, 20, 128}, "speed"}, {{20., 0.25, nan, 2, 20, 128}, "speed"}, {{20., 0.25, inf, 2, 20, 128}, "speed"},
        {{20., 0., 0., 2, 20, 128}, "fraction and speed"}, {{20., 0.25, 0., -1, 20, 128}, "reach"}, {{20., 0.25, 0., 9, 20, 128}, "reach"},
        {{20., 0.25, 0., 2, 0, 128}, "max_frames"}, {{20., 0.25, 0., 2, -4, 128}, "max_frames"}, {{20., 0.25, 0., 2, 20, 0}, "max_runs"},
        {{20., 0.25, 0., 2, 20, 513}, "max_runs"}, {{20., 0.25, 0., 2, 20, -1}, "max_runs"}};
    EXPECT(contact_rule_error(good) == nullptr, "the default rule is refused: %s", contact_rule_error(good));
    for (const auto& b : bad) {
        const char* why = contact_rule_error(b.r);
        EXPECT(why && std::strstr(why, b.word) == why, "a bad %s is %s", b.word, why ? why : "not refused");
    }
    const ContactRule limits[] = {{20., 0., 0.5, 0, 1, 1}, {20., 0.25, 0., 8, 1, 512}};
    for (const auto& r : limits) EXPECT(contact_rule_error(r) == nullptr, "a rule at the limits is refused: %s", contact_rule_error(r));
}

int main(int argc, char** argv) {
    check_rules();
    for (int i = 1; i < argc; ++i) check_file(argv[i]);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
