// Stand-alone check of the wide-line part of csrc/raster_lines.h (tests/test_raster_wide_host_cpu.py builds it with -fsanitize=address,undefined
// and runs it): the lowest minor index of a line of width w as the skeleton view's kernel computes it -- one division with the width's offset in
// the numerator, then remainder stepping by one major step and by 64 -- against the rule's formula evaluated directly in 128-bit arithmetic,
// over seeded random segments that include the +-2^28 limit, pixel centres and pixel boundaries, for every width 1 .. 16.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "raster_lines.h"            // csrc/, given with -I by the test

using namespace grk;

static int fails = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            if (++fails < 20) printf("line %d: %s\n", __LINE__, #cond);         \
        }                                                                       \
    } while (0)

static long long floor_div(__int128 a, __int128 b) {           // b > 0
    __int128 q = a / b;
    if (a % b < 0) --q;
    return (long long)q;
}

// the rule, read off its text: n0 = floor((Q0 dP + (256 m + 128 - P0) dQ - (w - 1) 128 dP) / (256 dP))
static long long rule_n0(const LineRec& r, int m, int w) {
    const __int128 dP = (__int128)r.P1 - r.P0, dQ = (__int128)r.Q1 - r.Q0, cP = (__int128)256 * m + 128;
    return floor_div((__int128)r.Q0 * dP + (cP - r.P0) * dQ - (__int128)(w - 1) * 128 * dP, 256 * dP);
}

static long long check_segment(int ax, int ay, int bx, int by, int n_major, int w) {
    LineRec r{};
    bool flip = false;
    if (!line_order(ax, ay, bx, by, r, flip)) return 0;
    line_range(r, n_major);
    if (r.m0 > r.m1) return 0;
    long long cols = 0;
    {   // by one major step
        const LineStride st = line_stride(r, 1);
        long long n, rem;
        line_minor_wide(r, r.m0, w, n, rem);
        for (int m = r.m0; m <= r.m1; ++m, line_advance(st, n, rem)) {
            CHECK(n == rule_n0(r, m, w));
            CHECK(rem >= 0 && rem < st.D);
            ++cols;
        }
    }
    const LineStride st = line_stride(r, 64);                  // the whole wave
    for (int lane = 0; lane < 64 && r.m0 + lane <= r.m1; ++lane) {
        long long n, rem, n1, rem1;
        line_minor_wide(r, r.m0 + lane, w, n, rem);
        if (w == 1) {                                          // width 1 is the wireframe's line_minor, bit for bit
            line_minor(r, r.m0 + lane, n1, rem1);
            CHECK(n == n1 && rem == rem1);
        }
        if (w % 2 == 1) {                                      // an odd width is the 1-pixel line moved down by (w - 1) / 2 whole pixels
            line_minor(r, r.m0 + lane, n1, rem1);
            CHECK(n == n1 - (w - 1) / 2 && rem == rem1);
        }
        for (int m = r.m0 + lane; m <= r.m1; m += 64, line_advance(st, n, rem)) {
            CHECK(n == rule_n0(r, m, w));
            CHECK(rem >= 0 && rem < st.D);
        }
    }
    return cols;
}

int main() {
    std::mt19937_64 g(20240923);
    const int limit = 1 << 28;
    auto pick = [&](int kind, int n) -> int {
        switch (kind) {
            case 0: return (int)(g() % (2ull * limit + 1)) - limit;                       // anywhere inside the limit
            case 1: return (g() & 1) ? limit : -limit;                                   // on the limit
            case 2: return 256 * (int)(g() % (unsigned)(n + 8)) - 1024 + 128;            // a pixel centre, some outside the viewport
            case 3: return 256 * (int)(g() % (unsigned)(n + 8)) - 1024;                  // a pixel boundary
            default: return (int)(g() % (unsigned)(256 * n + 4096)) - 2048;               // in and around the viewport
        }
    };
    long long segments = 0, cols = 0;
    const int sizes[] = {1, 5, 7, 48, 64, 97, 1080, 1920, 4096};
    for (int it = 0; it < 20000; ++it) {
        const int n = sizes[g() % 9];
        const int k0 = (int)(g() % 5), k1 = (int)(g() % 5);
        const int ax = pick(k0, n), ay = pick(k0 == 1 ? 0 : k0, n), bx = pick(k1, n), by = pick(k1 == 1 ? 4 : k1, n);
        cols += check_segment(ax, ay, bx, by, n, 1 + (int)(g() % 16));
        ++segments;
    }
    // exact horizontals, verticals and diagonals through centres and boundaries, and the limit's corners, in both directions, every width
    const int fixed[][4] = {{1408, 2560, 7552, 2560}, {2560, 7552, 2560, 1408}, {1408, 1408, 7552, 7552}, {7552, 1408, 1408, 7552}, {1280, 2560, 7680, 2688},
                            {-limit, -limit, limit, limit}, {limit, -limit, -limit, limit}, {-limit, 300, limit, 301}, {77, -limit, 78, limit}};
    for (const auto& e : fixed)
        for (int w = 1; w <= 16; ++w) {
            cols += check_segment(e[0], e[1], e[2], e[3], 4096, w);
            cols += check_segment(e[2], e[3], e[0], e[1], 64, w);
            segments += 2;
        }
    printf("segments: %lld, columns: %lld, failures: %d\n", segments, cols, fails);
    if (fails || cols < 100000) return 1;
    printf("ok\n");
    return 0;
}
