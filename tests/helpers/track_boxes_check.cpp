// csrc/track_boxes.h on the host: a stand-alone program (its own main, no HIP, nothing of the library but that header and the one it includes), built
// with AddressSanitizer and UBSan by tests/test_track_host_cpu.py and run directly.  It needs no input: every expected value is written out here or
// formed by other means (a sort for the median, a spelled-out extension for the Gaussian).  Prints what differs, and "ok" as its last line if nothing.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "track_boxes.h"

using namespace grk;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// position j = -32 .. n + 31 of mode 'reflect' over [0, n), n = 1 .. 5, written out by hand: d c b a | a b c d | d c b a
static const char* const kReflect[5] = {
    "00000000000000000000000000000000000000000000000000000000000000000",
    "011001100110011001100110011001100110011001100110011001100110011001",
    "1001221001221001221001221001221001221001221001221001221001221001221",
    "01233210012332100123321001233210012332100123321001233210012332100123",
    "100123443210012344321001234432100123443210012344321001234432100123443",
};

static void check_reflect() {
    for (int n = 1; n <= 5; ++n)
        for (int j = -32; j < n + 32; ++j) {
            const int want = kReflect[n - 1][j + 32] - '0', got = track_reflect(j, n);
            EXPECT(got == want, "reflect(%d, n = %d) = %d, not %d", j, n, got, want);
        }
}

static void set_bit(std::vector<unsigned long long>& w, int g) { w[g >> 6] |= 1ull << (g & 63); }

static void check_search() {
    std::vector<unsigned long long> w(4, 0ull);                 // frames 0 .. 255
    for (int g : {5, 59, 71, 127, 128, 200}) set_bit(w, g);      // frames 60 .. 70 dead: a gap across the first word boundary; 129 .. 199 across the third
    for (int g = 60; g <= 70; ++g) {
        EXPECT(track_prev(w.data(), g) == 59, "prev(%d) = %lld", g, track_prev(w.data(), g));
        EXPECT(track_next(w.data(), g) == 71, "next(%d) = %lld", g, track_next(w.data(), g));
    }
    EXPECT(track_prev(w.data(), 64) == 59 && track_next(w.data(), 63) == 71, "the boundary frames themselves");
    EXPECT(track_prev(w.data(), 128) == 127 && track_next(w.data(), 127) == 128, "neighbours on either side of a boundary");
    EXPECT(track_prev(w.data(), 199) == 128 && track_next(w.data(), 129) == 200, "a gap over a whole dead word's worth of frames");
    EXPECT(track_prev(w.data(), 127) == 71 && track_next(w.data(), 5) == 59, "inside one word");
    EXPECT(track_first(w.data(), 0, 256) == 5 && track_last(w.data(), 0, 256) == 200, "first / last of the whole");
    EXPECT(track_first(w.data(), 6, 59) == -1 && track_last(w.data(), 6, 59) == -1, "an empty stretch inside a word");
    EXPECT(track_first(w.data(), 6, 60) == 59 && track_last(w.data(), 5, 59) == 5, "the ends are [lo, hi)");
    EXPECT(track_first(w.data(), 60, 71) == -1 && track_first(w.data(), 60, 72) == 71 && track_last(w.data(), 60, 128) == 127, "across a boundary");
    EXPECT(track_first(w.data(), 129, 200) == -1 && track_last(w.data(), 129, 201) == 200 && track_first(w.data(), 128, 129) == 128, "at word starts");
    EXPECT(track_first(w.data(), 64, 64) == -1 && track_last(w.data(), 64, 64) == -1, "an empty range");
}

static double sorted_median(const std::vector<double>& x, int i, int k, int pad) {
    const int n = (int)x.size();
    std::vector<double> win;
    for (int j = i - k / 2; j <= i + k / 2; ++j) win.push_back(j >= 0 && j < n ? x[j] : pad == kTrackPadEdge ? x[j < 0 ? 0 : n - 1] : 0.);
    std::sort(win.begin(), win.end());
    return win[k / 2];
}

static void check_median() {
    const double ties[] = {3., 1., 3., 3., 1., 2., 2., 3., 1., 1., 3., 2., 0., 0., 3.};      // few values, many equal
    {
        const std::vector<double> x(ties, ties + 5);            // {3 1 3 3 1}: written out for k = 3
        const double zero[5] = {1., 3., 3., 3., 1.}, edge[5] = {3., 3., 3., 3., 1.};
        for (int i = 0; i < 5; ++i) {
            EXPECT(track_median(x.data(), 5, i, 3, kTrackPadZero) == zero[i], "median k = 3 zero at %d", i);
            EXPECT(track_median(x.data(), 5, i, 3, kTrackPadEdge) == edge[i], "median k = 3 edge at %d", i);
        }
    }
    unsigned state = 12345u;
    for (int n = 1; n <= 15; ++n) {
        std::vector<double> x(ties, ties + n), y(n);
        for (int i = 0; i < n; ++i) { state = state * 1664525u + 1013904223u; y[i] = (double)((state >> 20) % 5) - 2.; }     // -2 .. 2: signs and zeros
        for (int k : {1, 3, 5, 11, 31})
            for (int pad : {kTrackPadZero, kTrackPadEdge})
                for (int i = 0; i < n; ++i) {
                    EXPECT(track_median(x.data(), n, i, k, pad) == sorted_median(x, i, k, pad), "median n %d k %d pad %d at %d", n, k, pad, i);
                    EXPECT(track_median(y.data(), n, i, k, pad) == sorted_median(y, i, k, pad), "median (signed) n %d k %d pad %d at %d", n, k, pad, i);
                }
    }
}

static void check_gauss() {
    const int r = 32;
    std::vector<double> w(r + 1);
    double sum = 0.;
    for (int i = 0; i <= r; ++i) { w[i] = std::exp(-0.5 / 64. * i * i); sum += (i ? 2. : 1.) * w[i]; }
    for (double& v : w) v /= sum;
    for (int n = 1; n <= 5; ++n) {
        std::vector<double> x(n);
        for (int i = 0; i < n; ++i) x[i] = 100. + 7.5 * i * i;
        for (int l = 0; l < n; ++l) {
            double want = x[l] * w[0];                          // the same order over the table's extension
            for (int i = r; i >= 1; --i) want = want + (x[kReflect[n - 1][l - i + 32] - '0'] + x[kReflect[n - 1][l + i + 32] - '0']) * w[i];
            EXPECT(track_gauss(x.data(), n, l, w.data(), r) == want, "gauss n %d at %d", n, l);
        }
    }
    const double one[1] = {1.};
    const double x3[3] = {1., 2., 4.};
    EXPECT(track_gauss(x3, 3, 1, one, 0) == 2., "radius 0 is the identity");
}

static void check_frame_and_fill() {
    const double nan = std::nan("");
    double p[3] = {-1., -1., -1.};
    const double body[4 * 3] = {100., 50., 0.9, 160., 130., 0.31, 999., 999., 0.3, 130., 10., 0.5};      // the third joint sits exactly at the threshold
    EXPECT(track_frame(body, 4, 0.3, p) && p[0] == 130. && p[1] == 70. && p[2] == 150. / std::sqrt(60. * 60. + 120. * 120.), "a plain frame: %g %g %g", p[0], p[1], p[2]);
    const double point[2 * 3] = {10., 20., 0.9, 10.25, 20.25, 0.9};      // height 0.354 < 0.5
    const double half[2 * 3] = {10., 20., 0.9, 10.5, 20., 0.9};          // height exactly 0.5
    const double unseen[2 * 3] = {10., 20., 0.3, 300., 400., 0.1};
    const double bad_x[2 * 3] = {nan, 20., 0.9, 300., 400., 0.9};
    const double bad_hidden[2 * 3] = {nan, nan, 0.1, 300., 400., 0.9};   // a NaN beside a dead score does no harm, but one joint alone has height 0
    const double bad_score[3 * 3] = {10., 20., nan, 300., 400., 0.9, 100., 100., 0.9};
    const double inf_y[2 * 3] = {10., INFINITY, 0.9, 300., 400., 0.9};
    const double huge[2 * 3] = {-1e300, 0., 0.9, 1e300, 0., 0.9};       // dx^2 overflows: the height is not finite
    EXPECT(!track_frame(point, 2, 0.3, p) && track_frame(half, 2, 0.3, p) && p[2] == 300., "the height bar is >= 0.5");
    EXPECT(!track_frame(unseen, 2, 0.3, p) && !track_frame(bad_x, 2, 0.3, p) && !track_frame(bad_hidden, 2, 0.3, p), "no visible joint, a NaN coordinate");
    EXPECT(track_frame(bad_score, 3, 0.3, p) && p[0] == 200. && p[1] == 250., "a NaN score hides its joint alone");
    EXPECT(!track_frame(inf_y, 2, 0.3, p) && !track_frame(huge, 2, 0.3, p), "an infinite coordinate or height");
    // numpy.linspace(1, 2, 5)[1:-1] and the zero-step branch of equal ends
    EXPECT(track_fill(1., 2., 3, 1) == 1.25 && track_fill(1., 2., 3, 2) == 1.5 && track_fill(1., 2., 3, 3) == 1.75, "fill");
    EXPECT(track_fill(0.1, 0.1, 4, 2) == 0.1, "fill between equal ends");
    const double a = 0.1, b = 0.7, step = (b - a) / 8.;
    for (int i = 1; i <= 7; ++i) EXPECT(track_fill(a, b, 7, i) == (double)i * step + a, "fill %d of 7", i);
}

int main() {
    check_reflect();
    check_search();
    check_median();
    check_gauss();
    check_frame_and_fill();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
