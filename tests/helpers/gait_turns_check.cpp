// csrc/gait_turns.h on the host: a stand-alone program (its own main, no HIP, nothing of the library but that header and the ones it includes), built
// with AddressSanitizer and UBSan by tests/test_turns_host_cpu.py and run directly on one file per case, which the test writes: the inputs of ONE
// sequence and what pipeline.gait_turns made of them with sigma = 0.  The program runs the chain the kernels run -- turn_frame_step, the ballots'
// bitmasks, the runs by the lane at their first frame, the phases and the turn table, the per-sequence columns -- in buffers of exactly the sizes the
// call states, so that an index outside them is caught.  Every bit must be equal (a NaN equals a NaN).
//
// The file, little-endian: int32 [T, J, min_frames, max_frames, max_turns], int32 table[8], float64 [fps, edge_rate, peak_rate, min_angle], float32
// joints[T J 3], int32 events[T], float64 gait_rows[T 7], then the expected float64 per_frame[T 2], int32 phase[T], float64 turns[max_turns 7],
// float64 per_seq[24].  Prints what differs, and "ok" as its last line if nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gait_turns.h"

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
    std::vector<unsigned long long> w[kTurnMaskSets];
    explicit Masks(int T) { for (auto& m : w) m.assign((size_t)((T - 1) >> 6) + 1, 0ull); }
    TurnMasks view() { return TurnMasks{w[0].data(), w[1].data(), w[2].data(), w[3].data(), w[4].data(), w[5].data(), w[6].data(), w[7].data(), w[8].data(), w[9].data(), w[10].data()}; }
};
static void set_bit(unsigned long long* words, int t) { words[t >> 6] |= 1ull << (t & 63); }

// stages (a) to (d) of turn_sequence_stages, a loop over the frames where the device has a lane each
static void sequence(int T, const TurnRule& r, const double* rows, const int32_t* events, const double* gait_rows, int32_t* phase, double* turns, double* out) {
    Masks masks(T);
    const TurnMasks m = masks.view();
    for (int t = 0; t < T; ++t) {
        const double w = rows[(size_t)t * kTurnFrameCols + 1];
        if (w > r.edge_rate) set_bit(m.left, t);
        if (w < -r.edge_rate) set_bit(m.right, t);
        if (w != w) set_bit(m.unknown, t);
        if (events[t] & kGaitHeelL) set_bit(m.hs_l, t);
        if (events[t] & kGaitHeelR) set_bit(m.hs_r, t);
        if (events[t] & kGaitToeL) set_bit(m.to_l, t);
        if (events[t] & kGaitToeR) set_bit(m.to_r, t);
    }
    for (int t = 0; t < T; ++t) {
        const bool left = turn_run_begins(m.left, t);
        if (!left && !turn_run_begins(m.right, t)) continue;
        double peak, angle;
        if (turn_run(rows, t, turn_run_end(left ? m.left : m.right, T, t), r, &peak, &angle)) set_bit(m.accept, t);
    }
    for (int t = 0; t < T; ++t) {
        int ph = kTurnStraight;
        const bool left = gait_detail::bit(m.left, t);
        if (left || gait_detail::bit(m.right, t)) {
            const unsigned long long* run = left ? m.left : m.right;
            const int a = (int)turn_last_clear(run, 0, t) + 1;
            if (gait_detail::bit(m.accept, a)) ph = left ? kTurnLeft : kTurnRight;
            if (a == t && ph != kTurnStraight) {
                const long long row = turn_popcount(m.accept, 0, t);
                if (row < r.max_turns) {
                    const int e = turn_run_end(run, T, t);
                    double peak, angle;
                    turn_run(rows, t, e, r, &peak, &angle);
                    turn_row(m, t, e, left, peak, angle, r.fps, turns + row * kTurnCols);
                }
            }
        } else if (gait_detail::bit(m.unknown, t)) {
            ph = kTurnUnknown;
        }
        phase[t] = ph;
        if (ph == kTurnLeft) set_bit(m.turn_l, t);
        if (ph == kTurnRight) set_bit(m.turn_r, t);
        if (ph != kTurnStraight) set_bit(m.not_straight, t);
    }
    const long long found = turn_popcount(m.accept, 0, T);
    for (int i = 0; i < r.max_turns * kTurnCols; ++i)
        if (i / kTurnCols >= found) turns[i] = gait_detail::nan();
    turn_counts(m, T, out);
    for (int k = 0; k < 4; ++k) out[kTurnColDuration + k] = turn_mean(m, rows, T, r, k, turns);
    turn_steps(m, T, gait_rows, r.fps, out + kTurnGaitAt);
    turn_strides(m, T, r.fps, out + kTurnGaitAt);
    turn_stance(m, T, out + kTurnGaitAt);
}

static int check_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); ++failures; return 1; }
    std::vector<int32_t> head, table, events, want_phase;
    std::vector<double> scalars, gait_rows, want_frame, want_turns, want_seq;
    std::vector<float> joints;
    bool ok = read_n(f, head, 5) && read_n(f, table, 8) && read_n(f, scalars, 4);
    if (!ok) { std::printf("%s: short header\n", path); std::fclose(f); ++failures; return 1; }
    const int T = head[0], J = head[1];
    const TurnRule r{scalars[0], scalars[1], scalars[2], scalars[3], head[2], head[3], head[4]};
    ok = read_n(f, joints, (size_t)T * J * 3) && read_n(f, events, (size_t)T) && read_n(f, gait_rows, (size_t)T * kGaitFrameCols) &&
         read_n(f, want_frame, (size_t)T * kTurnFrameCols) && read_n(f, want_phase, (size_t)T) && read_n(f, want_turns, (size_t)r.max_turns * kTurnCols) &&
         read_n(f, want_seq, (size_t)kTurnSeqCols);
    std::fclose(f);
    if (!ok) { std::printf("%s: short file\n", path); ++failures; return 1; }

    int tab[kGaitTable];
    for (int k = 0; k < kGaitTable; ++k) tab[k] = table[k];
    std::vector<double> rows((size_t)T * kTurnFrameCols), turns((size_t)r.max_turns * kTurnCols, -7.), seq((size_t)kTurnSeqCols, -7.);
    std::vector<int32_t> phase((size_t)T, -7);
    for (int t = 0; t < T; ++t) {
        const double d = turn_frame_step(joints.data(), J, tab, t);
        rows[(size_t)t * kTurnFrameCols] = d;
        rows[(size_t)t * kTurnFrameCols + 1] = d * r.fps;
    }
    sequence(T, r, rows.data(), events.data(), gait_rows.data(), phase.data(), turns.data(), seq.data());

    const int before = failures;
    for (int t = 0; t < T; ++t) {
        EXPECT(phase[t] == want_phase[t], "%s: phase[%d] = %d, not %d", path, t, phase[t], want_phase[t]);
        for (int c = 0; c < kTurnFrameCols; ++c) {
            const double got = rows[(size_t)t * kTurnFrameCols + c], want = want_frame[(size_t)t * kTurnFrameCols + c];
            EXPECT(same(got, want), "%s: per_frame[%d][%d] = %.17g, not %.17g", path, t, c, got, want);
        }
    }
    for (size_t i = 0; i < turns.size(); ++i) EXPECT(same(turns[i], want_turns[i]), "%s: turns[%zu][%zu] = %.17g, not %.17g", path, i / kTurnCols, i % kTurnCols, turns[i], want_turns[i]);
    for (int c = 0; c < kTurnSeqCols; ++c) EXPECT(same(seq[c], want_seq[c]), "%s: per_seq[%d] = %.17g, not %.17g", path, c, seq[c], want_seq[c]);
    return failures - before;
}

// what no file reaches: the searches for a clear bit and the counts over word boundaries
static void check_rules() {
    std::vector<unsigned long long> w(3, 0ull);
    for (int t = 60; t < 130; ++t) set_bit(w.data(), t);       // one run over two word boundaries
    set_bit(w.data(), 0);
    EXPECT(turn_first_clear(w.data(), 0, 150) == 1 && turn_first_clear(w.data(), 60, 150) == 130 && turn_first_clear(w.data(), 64, 128) == -1, "first clear");
    EXPECT(turn_first_clear(w.data(), 60, 130) == -1 && turn_first_clear(w.data(), 129, 150) == 130 && turn_first_clear(w.data(), 5, 5) == -1, "first clear at the ends");
    EXPECT(turn_last_clear(w.data(), 0, 100) == 59 && turn_last_clear(w.data(), 0, 60) == 59 && turn_last_clear(w.data(), 60, 130) == -1, "last clear");
    EXPECT(turn_last_clear(w.data(), 0, 1) == -1 && turn_last_clear(w.data(), 0, 0) == -1 && turn_last_clear(w.data(), 0, 150) == 149 && turn_last_clear(w.data(), 0, 128) == 59, "last clear at the ends");
    EXPECT(turn_popcount(w.data(), 0, 150) == 71 && turn_popcount(w.data(), 61, 129) == 68 && turn_popcount(w.data(), 64, 128) == 64 && turn_popcount(w.data(), 7, 7) == 0, "popcount");
    EXPECT(turn_run_begins(w.data(), 0) && turn_run_begins(w.data(), 60) && !turn_run_begins(w.data(), 64) && !turn_run_begins(w.data(), 1), "run begins");
    EXPECT(turn_run_end(w.data(), 150, 60) == 130 && turn_run_end(w.data(), 130, 100) == 130 && turn_run_end(w.data(), 128, 64) == 128, "run end");
    EXPECT(turn_straight(w.data(), 1, 59) && !turn_straight(w.data(), 1, 60) && !turn_straight(w.data(), 0, 0) && turn_straight(w.data(), 130, 149), "straight");
    const double g0[2] = {0., -1.}, g1[2] = {1., 0.};              // facing the camera, then facing the camera's right, which is the subject's left
    EXPECT(std::fabs(turn_step(g0, g1) - 90.) < 1e-12 && std::fabs(turn_step(g1, g0) + 90.) < 1e-12 && turn_step(g0, g0) == 0., "step");
    const double z[2] = {0., 0.};
    EXPECT(std::isnan(turn_step(g0, z)) && std::isnan(turn_step(z, g0)), "a vanishing horizontal part");
    // every refusal of the rule, each alone in an otherwise good rule, and the good rules at the limits
    const double nan = std::nan(""), inf = INFINITY;
    const TurnRule good{20., 5., 15., 45., 10, 200, 8};
    const struct { TurnRule r; const char* word; } bad[] = {
        {{0., 5., 15., 45., 10, 200, 8}, "fps"}, {{-20., 5., 15., 45., 10, 200, 8}, "fps"}, {{nan, 5., 15., 45., 10, 200, 8}, "fps"}, {{inf, 5., 15., 45., 10, 200, 8}, "fps"},
        {{20., -1., 15., 45., 10, 200, 8}, "edge_rate"}, {{20., nan, 15., 45., 10, 200, 8}, "edge_rate"}, {{20., inf, 15., 45., 10, 200, 8}, "edge_rate"},
        {{20., 5., 4.9, 45., 10, 200, 8}, "peak_rate"}, {{20., 5., nan, 45., 10, 200, 8}, "peak_rate"}, {{20., 5., inf, 45., 10, 200, 8}, "peak_rate"},
        {{20., 5., 15., -1., 10, 200, 8}, "min_angle"}, {{20., 5., 15., nan, 10, 200, 8}, "min_angle"}, {{20., 5., 15., inf, 10, 200, 8}, "min_angle"},
        {{20., 5., 15., 45., 0, 200, 8}, "min_frames"}, {{20., 5., 15., 45., -3, 200, 8}, "min_frames"}, {{20., 5., 15., 45., 10, 9, 8}, "max_frames"},
        {{20., 5., 15., 45., 10, 200, 0}, "max_turns"}, {{20., 5., 15., 45., 10, 200, 65}, "max_turns"}, {{20., 5., 15., 45., 10, 200, -1}, "max_turns"}};
    EXPECT(turn_rule_error(good) == nullptr, "the default rule is refused: %s", turn_rule_error(good));
    for (const auto& b : bad) {
        const char* why = turn_rule_error(b.r);
        EXPECT(why && std::strstr(why, b.word) == why, "a bad %s is %s", b.word, why ? why : "not refused");
    }
    const TurnRule limits[] = {{20., 0., 0., 0., 1, 1, 1}, {20., 5., 5., 0., 10, 10, 64}};
    for (const auto& r : limits) EXPECT(turn_rule_error(r) == nullptr, "a rule at the limits is refused: %s", turn_rule_error(r));
}

int main(int argc, char** argv) {
    check_rules();
    for (int i = 1; i < argc; ++i) check_file(argv[i]);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
