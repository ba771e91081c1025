// csrc/mesh_moments.h on the host: a stand-alone program (its own main, no HIP, nothing of the library but that header), built with AddressSanitizer
// and UBSan by tests/test_body_host_cpu.py and run directly on one file per case, which the test writes: a face table, the vertices of some frames
// and what pipeline.mesh_moments made of them.  The program runs what the kernel runs -- mesh_origin, mesh_column for each of the 1024 columns,
// the tree, mesh_row -- in buffers of exactly the sizes the file states, so that an index outside them is caught.  Every bit must be equal (a NaN
// equals a NaN).  A table is judged first, as grnet_load_faces and grnet_mesh_moments judge it, and the sentence of a refusal is printed.
//
// The file, little-endian: int32 [n, V, F] (n = 0: the table alone), int32 faces[F 3], float32 verts[n V 3], then the expected float64 rows[n 11]
// and sums[n 11].  Prints "table <file>: closed" or "table <file>: <the refusal>", what differs, and "ok" as its last line if nothing differs.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mesh_moments.h"

using namespace grk;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

template <class T>
static bool read_n(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

static bool same(double a, double b) {
    if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
    return std::memcmp(&a, &b, sizeof a) == 0;
}

// the table as the library judges it: 0 and "closed", or the sentence of the refusal
static bool judge(const char* path, const std::vector<int32_t>& faces, int F, int V) {
    char why[192];
    MeshTableFault w = mesh_table_indices(faces.data(), F, V);
    if (w.kind == kMeshTableFine) {
        std::vector<unsigned long long> keys((size_t)3 * F);
        const long long bad = mesh_unmatched_edges(faces.data(), F, V, keys.data());
        if (bad) w = MeshTableFault{kMeshTableOpen, 0, bad};
    }
    mesh_table_text(w, V, why, sizeof why);
    std::printf("table %s: %s\n", path, w.kind == kMeshTableFine ? "closed" : why);
    return w.kind == kMeshTableFine;
}

static void check_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); ++failures; return; }
    std::vector<int32_t> head, faces;
    std::vector<float> verts;
    std::vector<double> want_rows, want_sums;
    bool ok = read_n(f, head, 3);
    if (!ok || head[0] < 0 || head[1] < 1) { std::printf("%s: bad header\n", path); std::fclose(f); ++failures; return; }
    const int n = head[0], V = head[1], F = head[2];
    ok = read_n(f, faces, F > 0 ? (size_t)F * 3 : 0) && read_n(f, verts, (size_t)n * V * 3) && read_n(f, want_rows, (size_t)n * kMeshRowCols) &&
         read_n(f, want_sums, (size_t)n * kMeshTerms);
    std::fclose(f);
    if (!ok) { std::printf("%s: short file\n", path); ++failures; return; }
    const bool closed = judge(path, faces, F, V);
    if (!n) return;
    EXPECT(closed, "%s: frames behind a table that is refused", path);
    if (!closed) return;
    std::vector<double> col((size_t)kMeshCols * kMeshTerms), row((size_t)kMeshRowCols);
    for (int k = 0; k < n; ++k) {
        const float* v = verts.data() + (size_t)k * V * 3;
        double o[3];
        mesh_origin(v, faces.data(), o);
        for (int l = 0; l < kMeshCols; ++l) mesh_column(v, faces.data(), F, l, o, col.data() + (size_t)l * kMeshTerms);
        mesh_tree(col.data());
        mesh_row(col.data(), o, row.data());
        for (int c = 0; c < kMeshTerms; ++c)
            EXPECT(same(col[c], want_sums[(size_t)k * kMeshTerms + c]), "%s: sums[%d][%d] = %.17g, not %.17g", path, k, c, col[c], want_sums[(size_t)k * kMeshTerms + c]);
        for (int c = 0; c < kMeshRowCols; ++c)
            EXPECT(same(row[c], want_rows[(size_t)k * kMeshRowCols + c]), "%s: rows[%d][%d] = %.17g, not %.17g", path, k, c, row[c], want_rows[(size_t)k * kMeshRowCols + c]);
    }
}

// what no file reaches: the sort, the two axes of every second moment, a row without a volume
static void check_rules() {
    std::vector<unsigned long long> a = {5, 3, 9, 3, 0, 7, 7, 7, 1};
    mesh_detail::sort(a.data(), (long long)a.size());
    for (size_t i = 1; i < a.size(); ++i) EXPECT(a[i - 1] <= a[i], "the sort at %zu", i);
    EXPECT(mesh_detail::lower(a.data(), (long long)a.size(), 7) == 5 && mesh_detail::lower(a.data(), (long long)a.size(), 10) == 9, "the search");
    const int ks[6] = {0, 1, 2, 0, 0, 1}, ls[6] = {0, 1, 2, 1, 2, 2};
    for (int q = 0; q < 6; ++q) EXPECT(mesh_axis_k(q) == ks[q] && mesh_axis_l(q) == ls[q], "the axes of moment %d", q);
    const double o[3] = {1., 2., 3.};
    double S[kMeshTerms], row[kMeshRowCols];
    for (double s0 : {0., -6., (double)NAN}) {
        for (int k = 0; k < kMeshTerms; ++k) S[k] = 1.;
        S[0] = s0;
        mesh_row(S, o, row);
        for (int c = 1; c < 10; ++c) EXPECT(std::isnan(row[c]), "column %d of a frame whose S0 is %g", c, s0);
        EXPECT(same(row[0], s0 / 6.) && row[10] == 0.5, "volume and area of a frame whose S0 is %g", s0);
    }
}

int main(int argc, char** argv) {
    check_rules();
    for (int i = 1; i < argc; ++i) check_file(argv[i]);
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
