// Cross-lane hand-offs of the lane schedule as a pure function of (lane of every op, producers of every op): no HIP, no plan types, so the
// stand-alone checker tests/helpers/lane_deps_check.cpp includes this file and nothing else of the library.
//
// The model.  The op list is the enqueue order and every lane is a FIFO stream, so an op is ordered behind every earlier op of its own lane.
// A wait of op i on op w (another lane) orders i -- and everything after i on its lane -- behind w and behind everything w is ordered
// behind.  What lane a is ordered behind on lane b is therefore always a prefix of lane b: one index per lane pair, a vector clock.
//
// The reduction.  Walking the list, a candidate wait (i, w) is dropped when i's lane is already ordered behind w: by the lane's clock (an
// earlier op of the lane waited on w, on a later op of w's lane, or on an op of a third lane that is itself behind w), or by another
// candidate of the same op.  "Is implied by" is a strict partial order on the candidates of one op, so dropping every implied one at once
// leaves its maximal elements, which still imply all the rest: the happens-before closure of (FIFO lanes + kept waits) equals that of
// (FIFO lanes + all cross-lane edges), and no kept wait is implied by the others.  Kept waits stay in the producers' first-seen order.
#pragma once
#include <algorithm>
#include <vector>

namespace lane_deps {

struct Handoffs {
    std::vector<std::vector<int>> waits;   // per op: the ops of other lanes whose completion it waits for
    std::vector<char> record;              // per op: some kept wait names it
    std::vector<char> join;                // per lane (entry 0 unused): the caller's stream, lane 0, still has to wait for the lane's end after the list
    size_t n_waits = 0, n_records = 0;
};

inline void count(Handoffs& h) {
    h.n_waits = h.n_records = 0;
    for (const auto& w : h.waits) h.n_waits += w.size();
    for (char r : h.record) h.n_records += r != 0;
}

inline int lane_count(const std::vector<int>& lane_of) {
    int lanes = 1;
    for (int l : lane_of) lanes = std::max(lanes, l + 1);
    return lanes;
}

// Every cross-lane producer edge as a wait, every lane joined: the wait set before the reduction
inline Handoffs all_cross_lane_waits(const std::vector<int>& lane_of, const std::vector<std::vector<int>>& producers) {
    const int m = (int)lane_of.size();
    Handoffs h;
    h.waits.assign(m, {});
    h.record.assign(m, 0);
    h.join.assign(lane_count(lane_of), 0);
    for (int i = 0; i < m; ++i) {
        if (lane_of[i] > 0) h.join[lane_of[i]] = 1;
        for (int w : producers[i])
            if (lane_of[w] != lane_of[i]) {
                h.waits[i].push_back(w);
                h.record[w] = 1;
            }
    }
    count(h);
    return h;
}

// producers[i]: earlier ops (any lane, each once) op i has to run behind.  Same-lane producers need nothing: the stream orders them.
inline Handoffs reduce_cross_lane_waits(const std::vector<int>& lane_of, const std::vector<std::vector<int>>& producers) {
    const int m = (int)lane_of.size(), lanes = lane_count(lane_of);
    Handoffs h;
    h.waits.assign(m, {});
    h.record.assign(m, 0);
    h.join.assign(lanes, 0);
    std::vector<int> clock((size_t)lanes * lanes, -1);     // clock[a * lanes + b]: the latest op of lane b that lane a is ordered behind so far
    std::vector<int> snap((size_t)m * lanes, -1);          // the clock of op i's lane right after op i's waits; its own lane's entry is i
    std::vector<int> last(lanes, -1), cand;
    for (int i = 0; i < m; ++i) {
        const int a = lane_of[i];
        int* mine = &clock[(size_t)a * lanes];
        cand.clear();
        for (int w : producers[i])
            if (lane_of[w] != a) cand.push_back(w);
        for (int w : cand) {
            const int b = lane_of[w];
            bool implied = mine[b] >= w;
            for (size_t k = 0; k < cand.size() && !implied; ++k)
                implied = cand[k] != w && snap[(size_t)cand[k] * lanes + b] >= w;
            if (!implied) {
                h.waits[i].push_back(w);
                h.record[w] = 1;
            }
        }
        for (int w : h.waits[i])
            for (int c = 0; c < lanes; ++c)
                if (c != a) mine[c] = std::max(mine[c], snap[(size_t)w * lanes + c]);
        std::copy(mine, mine + lanes, &snap[(size_t)i * lanes]);
        snap[(size_t)i * lanes + a] = i;
        last[a] = i;
    }
    for (int l = 1; l < lanes; ++l) h.join[l] = last[l] >= 0 && clock[l] < last[l];      // clock[0 * lanes + l]: lane 0 at the end of the list
    count(h);
    return h;
}

}  // namespace lane_deps
