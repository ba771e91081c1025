// csrc/gait_angles.h on the host: a stand-alone program (its own main, no HIP, nothing of the library but that header and the ones it includes), built
// with AddressSanitizer and UBSan by tests/test_kinematics_host_cpu.py and run directly on one file per case, which the test writes: the inputs of ONE
// sequence and what the statement (pipeline.gait_kinematics, gait_cycles or gait_atan2) made of them.  The program runs the chain the kernels run --
// kin_frame, the ballots' bitmasks, kin_channel with the serial extent, kin_rom for the partner, kin_symmetry -- in buffers of exactly the sizes the
// call states, so that an index outside them is caught.  No Gaussian: with sigma = 0 EVERY BIT must equal the statement's (a NaN equals a NaN).
//
// The file, little-endian: int32 [kind, T, J, min_stride, max_stride], then
//   kind 0: int32 table[16], float32 joints[T J 3], int32 events[T], expected float64 per_frame[T 13], curves[13 101 2], rows[13 6]
//   kind 1: float64 y[T], x[T], expected gait_atan2[T]
//   kind 2: float64 angles[T 13], int32 events[T], expected float64 curves[13 101 2], rows[13 6]
// Prints what differs, and "ok" as its last line if nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gait_angles.h"

using namespace grk;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (++failures < 40) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

template <class V>
static bool read_n(std::FILE* f, std::vector<V>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(V), n, f) == n;
}

static bool same(double a, double b) {
    if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
    return std::memcmp(&a, &b, sizeof a) == 0;
}

// rules 5 to 7 on angles (T,13): curves (13,101,2), rows (13,6)
static void cycles(const std::vector<double>& angles, const std::vector<int32_t>& events, int T, int min_stride, int max_stride, std::vector<double>& curves,
                   std::vector<double>& rows) {
    const size_t n_words = (size_t)((T - 1) >> 6) + 1;
    std::vector<unsigned long long> mask[2];
    for (auto& m : mask) m.assign(n_words, 0ull);
    for (int t = 0; t < T; ++t)
        for (int k = 0; k < 2; ++k)
            if ((events[t] >> k) & 1) mask[k][t >> 6] |= 1ull << (t & 63);
    curves.assign((size_t)kKinChannels * kKinPoints * 2, -7.);
    rows.assign((size_t)kKinChannels * kKinSeqCols, -7.);
    for (int c = 0; c < kKinChannels; ++c) {
        const double* x = angles.data() + c;
        auto extent = [x](int t0, int L, double* mx, double* mn) { return kin_extent_serial(x, kKinChannels, t0, L, mx, mn); };
        double* row = rows.data() + (size_t)c * kKinSeqCols;
        for (int p = 0; p < kKinPoints; ++p)
            kin_channel(mask[kin_foot(c)].data(), x, kKinChannels, T, min_stride, max_stride, extent, p, row, curves.data() + ((size_t)c * kKinPoints + p) * 2);
        row[5] = std::nan("");
        const int o = kin_partner(c);
        if (o >= 0) {
            const double* y = angles.data() + o;
            double n_o, rom_o;
            kin_rom(mask[kin_foot(o)].data(), T, min_stride, max_stride, [y](int t0, int L, double* mx, double* mn) { return kin_extent_serial(y, kKinChannels, t0, L, mx, mn); },
                    &n_o, &rom_o);
            row[5] = (c & 1) ? kin_symmetry(n_o, rom_o, row[0], row[3]) : kin_symmetry(row[0], row[3], n_o, rom_o);
        }
    }
}

static int check_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); return ++failures; }
    std::vector<int32_t> head, table, events;
    std::vector<double> angles, want_frame, want_curves, want_rows, ys, xs, want;
    std::vector<float> joints;
    if (!read_n(f, head, 5)) { std::printf("%s: short header\n", path); std::fclose(f); return ++failures; }
    const int kind = head[0], T = head[1], J = head[2], min_stride = head[3], max_stride = head[4];
    const int before = failures;
    bool ok = true;
    if (kind == 1) {
        ok = read_n(f, ys, (size_t)T) && read_n(f, xs, (size_t)T) && read_n(f, want, (size_t)T);
        std::fclose(f);
        if (!ok) { std::printf("%s: short file\n", path); return ++failures; }
        for (int i = 0; i < T; ++i) {
            const double got = gait_atan2(ys[i], xs[i]);
            EXPECT(same(got, want[i]), "%s: gait_atan2(%.17g, %.17g) = %.17g, not %.17g", path, ys[i], xs[i], got, want[i]);
        }
        return failures - before;
    }
    if (kind == 0) ok = read_n(f, table, kKinTable) && read_n(f, joints, (size_t)T * J * 3);
    else ok = read_n(f, angles, (size_t)T * kKinChannels);
    ok = ok && read_n(f, events, (size_t)T) && (kind != 0 || read_n(f, want_frame, (size_t)T * kKinChannels)) &&
         read_n(f, want_curves, (size_t)kKinChannels * kKinPoints * 2) && read_n(f, want_rows, (size_t)kKinChannels * kKinSeqCols);
    std::fclose(f);
    if (!ok) { std::printf("%s: short file\n", path); return ++failures; }
    if (kind == 0) {
        int tab[kKinTable];
        for (int k = 0; k < kKinTable; ++k) tab[k] = table[k];
        angles.assign((size_t)T * kKinChannels, -7.);
        for (int t = 0; t < T; ++t) kin_frame(joints.data() + (size_t)t * J * 3, tab, angles.data() + (size_t)t * kKinChannels);
        for (size_t i = 0; i < angles.size(); ++i)
            EXPECT(same(angles[i], want_frame[i]), "%s: per_frame[%zu][%zu] = %.17g, not %.17g", path, i / kKinChannels, i % kKinChannels, angles[i], want_frame[i]);
    }
    std::vector<double> curves, rows;
    cycles(angles, events, T, min_stride, max_stride, curves, rows);
    for (size_t i = 0; i < curves.size(); ++i)
        EXPECT(same(curves[i], want_curves[i]), "%s: curves[%zu][%zu][%zu] = %.17g, not %.17g", path, i / (2 * kKinPoints), i / 2 % kKinPoints, i % 2, curves[i], want_curves[i]);
    for (size_t i = 0; i < rows.size(); ++i)
        EXPECT(same(rows[i], want_rows[i]), "%s: rows[%zu][%zu] = %.17g, not %.17g", path, i / kKinSeqCols, i % kKinSeqCols, rows[i], want_rows[i]);
    return failures - before;
}

// what no file reaches
static void check_rules() {
    EXPECT(std::isnan(gait_atan2(0., 0.)) && std::isnan(gait_atan2(-0., 0.)) && std::isnan(gait_atan2(1., INFINITY)) && std::isnan(gait_atan2(NAN, 1.)), "the NaN rule");
    EXPECT(gait_atan2(0., 1.) == 0. && !std::signbit(gait_atan2(-0., 1.)) && gait_atan2(0., -1.) == kKinPi && gait_atan2(1., 0.) == kKinHalfPi && gait_atan2(-1., 0.) == -kKinHalfPi, "the axes");
    const double x[5] = {1., 3., 2., 7., 4.};
    EXPECT(kin_cycle_point(x, 1, 0, 4, 0) == 1. && kin_cycle_point(x, 1, 0, 4, 100) == 4. && kin_cycle_point(x, 1, 0, 4, 25) == 3. && kin_cycle_point(x, 1, 0, 4, 50) == 2., "whole frames");
    EXPECT(kin_cycle_point(x, 1, 1, 2, 25) == 3. + (2. - 3.) * (50. / 100.0), "half a frame");
    EXPECT(kin_foot(12) == 0 && kin_partner(12) == -1 && kin_foot(5) == 1 && kin_partner(5) == 4 && kin_partner(4) == 5, "feet and partners");
    EXPECT(std::isnan(kin_symmetry(0., 1., 2., 1.)) && std::isnan(kin_symmetry(2., 0., 2., 0.)) && kin_symmetry(1., 3., 1., 1.) == 100., "the symmetry index");
}

int main(int argc, char** argv) {
    check_rules();
    for (int i = 1; i < argc; ++i) check_file(argv[i]);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
