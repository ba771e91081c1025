// Stand-alone run of csrc/translation3.h on the host: its own main, no HIP, nothing of the library but that header.  Built with AddressSanitizer
// and UBSan and -ffp-contract=off and run directly (tests/test_translation_host_cpu.py), on cases the test writes out and whose results it reads
// back: every buffer has exactly the size the case states, so a read outside a frame's rows is a sanitizer report.
//
// translation3_check IN OUT.  IN: int32 [n, K3, K2, P, min_joints, n_fill], int32 pairs (P,2), float64 [f, cx, cy, threshold], float32 joints3d
// (n,K3,3), float32 joints2d (n,K2,3), float64 fill cases (n_fill,7) = [prev (3), next (3), gap].  OUT: float64 (n,6) = [tx, ty, tz, reproj, n_used,
// status], then for every fill case float64 (gap,3): frames 1 .. gap of the run.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "translation3.h"

namespace {

template <typename T>
bool read_n(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: translation3_check IN OUT\n"); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<int32_t> head, pairs;
    std::vector<double> cam, fills;
    std::vector<float> j3, j2;
    if (!read_n(in, head, 6)) { std::fprintf(stderr, "short header\n"); return 2; }
    const int n = head[0], K3 = head[1], K2 = head[2], P = head[3], min_joints = head[4], n_fill = head[5];
    if (n < 0 || K3 < 1 || K2 < 1 || P < 1 || P > 64 || n_fill < 0) { std::fprintf(stderr, "bad header\n"); return 2; }
    if (!read_n(in, pairs, (size_t)P * 2) || !read_n(in, cam, 4) || !read_n(in, j3, (size_t)n * K3 * 3) || !read_n(in, j2, (size_t)n * K2 * 3) ||
        !read_n(in, fills, (size_t)n_fill * 7)) { std::fprintf(stderr, "short input\n"); return 2; }
    std::fclose(in);
    std::vector<int> p3(P), p2(P);
    for (int j = 0; j < P; ++j) {
        p3[j] = pairs[2 * j];
        p2[j] = pairs[2 * j + 1];
        if (p3[j] < 0 || p3[j] >= K3 || p2[j] < 0 || p2[j] >= K2) { std::fprintf(stderr, "pair %d outside the joints\n", j); return 2; }
    }
    std::vector<double> out;
    for (int i = 0; i < n; ++i) {
        // the frame's rows in buffers of their own: the header may read K3 and K2 rows of three floats and nothing else
        const std::vector<float> a(j3.begin() + (size_t)i * K3 * 3, j3.begin() + (size_t)(i + 1) * K3 * 3);
        const std::vector<float> b(j2.begin() + (size_t)i * K2 * 3, j2.begin() + (size_t)(i + 1) * K2 * 3);
        const grk::Translation3 r = grk::translation3_fit(a.data(), b.data(), p3.data(), p2.data(), P, cam[0], cam[1], cam[2], cam[3], min_joints);
        out.insert(out.end(), {r.t[0], r.t[1], r.t[2], r.reproj, (double)r.n_used, (double)r.status});
    }
    for (int k = 0; k < n_fill; ++k) {
        const double* c = fills.data() + (size_t)k * 7;
        const int gap = (int)c[6];
        for (int i = 1; i <= gap; ++i) {
            double t[3];
            grk::translation3_fill(c, c + 3, gap, i, t);
            out.insert(out.end(), {t[0], t[1], t[2]});
        }
    }
    std::FILE* of = std::fopen(argv[2], "wb");
    if (!of || std::fwrite(out.data(), sizeof(double), out.size(), of) != out.size()) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    std::fclose(of);
    std::printf("frames: %d, fill cases: %d\nok\n", n, n_fill);
    return 0;
}
