// Stand-alone check of csrc/raster_lines.h (tests/test_raster_lines_host_cpu.py builds it with -fsanitize=address,undefined and runs it): the
// integer arithmetic of the wireframe's line rule as the kernels use it -- one division, then remainder stepping, by one major step (a lane's
// own loop) and by 64 (the whole wave) -- against the rule's formula evaluated directly in 128-bit arithmetic, over seeded random edges that
// include the +-2^28 clamp, pixel centres and pixel boundaries.
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

// the rule, read off its text
static long long rule_minor(const LineRec& r, int m) {
    const __int128 dP = (__int128)r.P1 - r.P0, dQ = (__int128)r.Q1 - r.Q0, cP = (__int128)256 * m + 128;
    return floor_div((__int128)r.Q0 * dP + (cP - r.P0) * dQ, 256 * dP);
}

static long long check_edge(int ax, int ay, int bx, int by, int n_major) {
    LineRec r{}, back{};
    bool flip = false, flip_back = false;
    const bool drawn = line_order(ax, ay, bx, by, r, flip);
    CHECK(drawn == line_order(bx, by, ax, ay, back, flip_back));
    if (!drawn) {
        CHECK(ax == bx && ay == by);
        return 0;
    }
    CHECK(r.P0 == back.P0 && r.Q0 == back.Q0 && r.P1 == back.P1 && r.Q1 == back.Q1 && r.xmajor == back.xmajor && flip != flip_back);
    CHECK(r.P0 < r.P1);
    const long long adx = llabs((long long)bx - ax), ady = llabs((long long)by - ay);
    CHECK(r.xmajor == (adx >= ady));
    CHECK(r.P0 == (r.xmajor ? (ax < bx ? ax : bx) : (ay < by ? ay : by)));
    line_range(r, n_major);
    // the range against the rule's sentence, on the indices around it
    for (int m = (r.m0 > 2 ? r.m0 - 2 : 0); m <= r.m1 + 2 && m < n_major; ++m) {
        const long long c = 256ll * m + 128;
        CHECK((r.P0 <= c && c < r.P1) == (m >= r.m0 && m <= r.m1));
    }
    if (r.m0 > 0) CHECK(256ll * (r.m0 - 1) + 128 < r.P0);
    if (r.m1 < n_major - 1) CHECK(256ll * (r.m1 + 1) + 128 >= r.P1);
    if (r.m0 > r.m1) return 0;
    long long frags = 0;
    // a lane's own loop
    {
        const LineStride st = line_stride(r, 1);
        long long n, rem;
        line_minor(r, r.m0, n, rem);
        for (int m = r.m0; m <= r.m1; ++m, line_advance(st, n, rem)) {
            CHECK(n == rule_minor(r, m));
            CHECK(rem >= 0 && rem < st.D);
            ++frags;
        }
    }
    // the whole wave
    const LineStride st = line_stride(r, 64);
    CHECK(st.sr >= 0 && st.sr < st.D && st.sq >= -64 && st.sq <= 64);
    for (int lane = 0; lane < 64; ++lane) {
        long long n, rem;
        line_minor(r, r.m0 + lane, n, rem);
        for (int m = r.m0 + lane; m <= r.m1; m += 64, line_advance(st, n, rem)) {
            CHECK(n == rule_minor(r, m));
            CHECK(rem >= 0 && rem < st.D);
        }
    }
    return frags;
}

int main() {
    std::mt19937_64 g(20240611);
    const int limit = 1 << 28;
    auto pick = [&](int kind, int n) -> int {
        switch (kind) {
            case 0: return (int)(g() % (2ull * limit + 1)) - limit;                       // anywhere inside the clamp
            case 1: return (g() & 1) ? limit : -limit;                                   // on the clamp
            case 2: return 256 * (int)(g() % (unsigned)(n + 8)) - 1024 + 128;            // a pixel centre, some outside the viewport
            case 3: return 256 * (int)(g() % (unsigned)(n + 8)) - 1024;                  // a pixel boundary
            default: return (int)(g() % (unsigned)(256 * n + 4096)) - 2048;               // in and around the viewport
        }
    };
    long long edges = 0, frags = 0;
    const int sizes[] = {1, 5, 7, 48, 64, 97, 1080, 1920, 4096};
    for (int it = 0; it < 40000; ++it) {
        const int n = sizes[g() % 9];
        const int k0 = (int)(g() % 5), k1 = (int)(g() % 5);
        const int ax = pick(k0, n), ay = pick(k0 == 1 ? 0 : k0, n), bx = pick(k1, n), by = pick(k1 == 1 ? 4 : k1, n);
        frags += check_edge(ax, ay, bx, by, n);
        ++edges;
    }
    // exact horizontals, verticals, diagonals and a point, in both directions
    const int fixed[][4] = {{1408, 2560, 7552, 2560}, {2560, 7552, 2560, 1408}, {1408, 1408, 7552, 7552}, {7552, 1408, 1408, 7552},
                            {-limit, -limit, limit, limit}, {limit, -limit, -limit, limit}, {-limit, 300, limit, 301}, {77, -limit, 78, limit},
                            {500, 500, 500, 500}};
    for (const auto& e : fixed) {
        frags += check_edge(e[0], e[1], e[2], e[3], 4096);
        frags += check_edge(e[2], e[3], e[0], e[1], 64);
        edges += 2;
    }
    printf("edges: %lld, fragments: %lld, failures: %d\n", edges, frags, fails);
    if (fails || frags < 100000) return 1;
    printf("ok\n");
    return 0;
}
