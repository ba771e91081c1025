// Stand-alone check of csrc/lane_deps.h (tests/test_lane_deps_cpu.py builds it with -fsanitize=address,undefined and runs it).
// For 200 seeded random op lists and for one HR module's fuse pattern:
//   - the happens-before closure of (FIFO lanes + kept waits) equals the closure of (FIFO lanes + all cross-lane edges);
//   - no kept wait is implied by the lane order and the other kept waits;
//   - record[w] is set exactly when a kept wait names w; kept waits are a subsequence of the producers (first-seen order);
//   - a side lane is joined exactly when its last op is not behind lane 0's last op.
#include "../../video-based-gait-analysis-for-dementia_amd/csrc/lane_deps.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

typedef std::vector<uint64_t> Bits;
bool has(const Bits& b, int i) { return (b[i >> 6] >> (i & 63)) & 1; }
void put(Bits& b, int i) { b[i >> 6] |= 1ull << (i & 63); }
void join(Bits& a, const Bits& b) { for (size_t k = 0; k < a.size(); ++k) a[k] |= b[k]; }

// strict ancestors of every op under the lane order and the given cross-lane edges (the list order is a topological order)
std::vector<Bits> closure(const std::vector<int>& lane_of, const std::vector<std::vector<int>>& edges) {
    const int m = (int)lane_of.size(), lanes = lane_deps::lane_count(lane_of);
    std::vector<Bits> anc(m, Bits((m + 63) / 64 + 1, 0));
    std::vector<int> prev(lanes, -1);
    for (int i = 0; i < m; ++i) {
        const int p = prev[lane_of[i]];
        if (p >= 0) { join(anc[i], anc[p]); put(anc[i], p); }
        for (int w : edges[i]) { join(anc[i], anc[w]); put(anc[i], w); }
        prev[lane_of[i]] = i;
    }
    return anc;
}

int failures = 0;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) {                                                          \
            if (++failures <= 20) { fprintf(stderr, "%s: ", name); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
        }                                                                       \
    } while (0)

struct Totals { size_t all = 0, kept = 0, records = 0; };

Totals check_case(const char* name, const std::vector<int>& lane_of, const std::vector<std::vector<int>>& producers) {
    const int m = (int)lane_of.size(), lanes = lane_deps::lane_count(lane_of);
    const lane_deps::Handoffs all = lane_deps::all_cross_lane_waits(lane_of, producers);
    const lane_deps::Handoffs kept = lane_deps::reduce_cross_lane_waits(lane_of, producers);
    CHECK((int)kept.waits.size() == m && (int)kept.record.size() == m && (int)kept.join.size() == lanes, "result sizes");
    const std::vector<Bits> full = closure(lane_of, all.waits), red = closure(lane_of, kept.waits);
    for (int i = 0; i < m; ++i) CHECK(full[i] == red[i], "op %d: the closure of the kept waits differs from the closure of all edges", i);
    std::vector<char> named(m, 0);
    std::vector<int> prev(lanes, -1), last(lanes, -1);
    size_t n_kept = 0, n_rec = 0;
    for (int i = 0; i < m; ++i) {
        // the kept waits are cross-lane producers of the op, in the producers' order
        size_t at = 0;
        for (int w : kept.waits[i]) {
            CHECK(w >= 0 && w < i && lane_of[w] != lane_of[i], "op %d waits on %d: not an earlier op of another lane", i, w);
            while (at < producers[i].size() && producers[i][at] != w) ++at;
            CHECK(at < producers[i].size(), "op %d waits on %d: not a producer, or out of first-seen order", i, w);
            ++at;
            named[w] = 1;
            ++n_kept;
        }
        // minimal: without one kept wait, the op's ancestors (from its lane predecessor and its other kept waits) no longer contain the producer
        for (size_t k = 0; k < kept.waits[i].size(); ++k) {
            Bits a((m + 63) / 64 + 1, 0);
            const int p = prev[lane_of[i]];
            if (p >= 0) { join(a, red[p]); put(a, p); }
            for (size_t q = 0; q < kept.waits[i].size(); ++q)
                if (q != k) { join(a, red[kept.waits[i][q]]); put(a, kept.waits[i][q]); }
            CHECK(!has(a, kept.waits[i][k]), "op %d: the wait on %d is implied by the others", i, kept.waits[i][k]);
        }
        prev[lane_of[i]] = last[lane_of[i]] = i;
    }
    for (int i = 0; i < m; ++i) {
        CHECK((kept.record[i] != 0) == (named[i] != 0), "op %d: record %d but %s kept wait names it", i, (int)kept.record[i], named[i] ? "a" : "no");
        n_rec += kept.record[i] != 0;
    }
    CHECK(kept.n_waits == n_kept && kept.n_records == n_rec, "counts: %zu / %zu reported, %zu / %zu found", kept.n_waits, kept.n_records, n_kept, n_rec);
    CHECK(kept.n_waits <= all.n_waits && kept.n_records <= kept.n_waits, "more kept than given, or more records than waits");
    for (int l = 1; l < lanes; ++l) {
        const bool behind = last[l] < 0 || (last[0] >= 0 && has(full[last[0]], last[l]));
        CHECK((kept.join[l] != 0) == !behind, "lane %d: join %d, its last op %s behind lane 0's", l, (int)kept.join[l], behind ? "is" : "is not");
    }
    Totals t;
    t.all = all.n_waits; t.kept = kept.n_waits; t.records = kept.n_records;
    return t;
}

// splitmix64: the same cases on every machine
struct Rng {
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    int below(int n) { return (int)(next() % (uint64_t)n); }
};

void random_case(int seed, std::vector<int>& lane_of, std::vector<std::vector<int>>& producers) {
    Rng r{(uint64_t)seed * 0x2545f4914f6cdd1dull + 1};
    const int lanes = 2 + r.below(3), m = 5 + r.below(296), style = r.below(3);
    lane_of.assign(m, 0);
    producers.assign(m, {});
    for (int i = 0; i < m; ++i) {
        // style 0: any lane per op; 1: runs on one lane (chains); 2: mostly the producer's lane
        lane_of[i] = (style == 1 && i && r.below(4)) ? lane_of[i - 1] : r.below(lanes);
        if (!i) continue;
        const int n_prod = r.below(4);
        for (int k = 0; k < n_prod; ++k) {
            const int w = r.below(8) ? std::max(0, i - 1 - r.below(std::min(i, 12))) : r.below(i);      // mostly recent ops, sometimes any earlier one
            if (std::find(producers[i].begin(), producers[i].end(), w) == producers[i].end()) producers[i].push_back(w);
        }
        if (style == 2 && !producers[i].empty() && r.below(3)) lane_of[i] = lane_of[producers[i][0]];
    }
}

// Two consecutive four-branch HR modules as build_plan writes them (hrnet.py:141-265): per module the four BasicBlocks of every branch
// (8 convolutions, branch b on lane b, written block by block), the down chains of the fuse layer behind their source branch, ONE grouped
// launch on lane 3 that finishes outputs 0..2 from all four branch outputs and the finished chains, and the stride-2 convolution on lane 2
// that finishes output 3.  The next module's branches read those outputs.
void hr_case(std::vector<int>& lane_of, std::vector<std::vector<int>>& producers) {
    lane_of.clear();
    producers.clear();
    auto add = [&](int lane, const std::vector<int>& prod) {   // producers in first-seen order, each once (as raw_producers() lists them)
        std::vector<int> p;
        for (int w : prod) if (std::find(p.begin(), p.end(), w) == p.end()) p.push_back(w);
        lane_of.push_back(lane);
        producers.push_back(p);
        return (int)lane_of.size() - 1;
    };
    int in[4] = {-1, -1, -1, -1};                             // the op that wrote branch b's input
    for (int module = 0; module < 2; ++module) {
        int x[4], res[4];
        for (int b = 0; b < 4; ++b) x[b] = res[b] = in[b];
        for (int blk = 0; blk < 4; ++blk) {
            int y[4];
            for (int b = 0; b < 4; ++b) y[b] = add(b, x[b] >= 0 ? std::vector<int>{x[b]} : std::vector<int>{});
            for (int b = 0; b < 4; ++b) {                     // conv2 adds the block's input
                std::vector<int> p{y[b]};
                if (res[b] >= 0) p.push_back(res[b]);
                x[b] = res[b] = add(b, p);
            }
        }
        // down chains D_ij (j < i), first links of one source branch merged into one launch
        const int m0 = add(0, {x[0]});                        // (1,0) whole, first links of (2,0) and (3,0)
        const int d20 = add(0, {m0}), d30a = add(0, {m0}), d30 = add(0, {d30a});
        const int m1 = add(1, {x[1]});                        // (2,1) whole, first link of (3,1)
        const int d31 = add(1, {m1});
        const int up = add(3, {x[0], x[1], x[2], x[3], m0, d20, m1});          // outputs 0..2: up terms, x_i, D_10, D_20, D_21
        const int fin = add(2, {x[2], x[3], d30, d31});                       // output 3
        in[0] = in[1] = in[2] = up;
        in[3] = fin;
    }
    add(0, {in[0], in[1], in[2], in[3]});                     // what follows the stage reads all four outputs on the caller's stream
}

}  // namespace

int main() {
    std::vector<int> lane_of;
    std::vector<std::vector<int>> producers;
    Totals sum;
    char name[64];
    for (int seed = 0; seed < 200; ++seed) {
        random_case(seed, lane_of, producers);
        snprintf(name, sizeof name, "random case %d (%zu ops)", seed, lane_of.size());
        const Totals t = check_case(name, lane_of, producers);
        sum.all += t.all; sum.kept += t.kept; sum.records += t.records;
    }
    printf("random: 200 cases, %zu cross-lane edges -> %zu kept waits, %zu records\n", sum.all, sum.kept, sum.records);
    hr_case(lane_of, producers);
    const char* hr_name = "HR fuse pattern";
    const Totals t = check_case(hr_name, lane_of, producers);
    printf("hr: %zu ops, %zu cross-lane edges -> %zu kept waits, %zu records\n", lane_of.size(), t.all, t.kept, t.records);
    {
        const char* name = hr_name;
        CHECK(t.kept < t.all, "the fuse pattern has redundant edges (the finisher and the next module's branches), none was dropped");
    }
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
