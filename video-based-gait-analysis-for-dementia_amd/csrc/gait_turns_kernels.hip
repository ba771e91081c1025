// Turns and straight-walking gait parameters on the device, for many sequences lying back to back (rules and columns: DESIGN 4.13; the arithmetic:
// gait_turns.h, which the host checker runs too; the axes: gait_events.h; the arctangent: gait_angles.h; the Gaussian and the bitmask searches:
// track_boxes.h).
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  Everything is float64 and every operation rounds once.
//
// TWO launches behind one small upload (the sequences' offsets and the Gaussian weights), whatever the number of sequences or frames.
//
// turn_rate_kernel -- one workgroup per sequence, a lane per frame.  The lane makes the ground heading of its frame AND of the frame before it
// (turn_heading twice: four joints, a cross product, two square roots -- cheaper than a launch of its own and a trip through memory, and the same
// operations give the same bits in both lanes that make a heading), their yaw step and the raw rate.  With a Gaussian the raw rates go to a column
// of the call's scratch and, behind one barrier (a workgroup's own global writes are visible to it there), track_gauss with the weights in LDS
// writes the smoothed rate; without one the raw rate is the rate.
//
// turn_seq_kernel  -- one workgroup of four waves per sequence, as gait_seq_kernel.  (a) a wave takes 64 consecutive frames, a lane a frame:
// __ballot of rate > edge, of rate < -edge, of rate != rate and of the four event bits ARE words of seven bitmasks, aligned to the sequence, in LDS
// where the sequence has at most 64 * kGaitLdsWords frames, else in the call's scratch (gait_mask_at of each).
// (b) behind a barrier the lane at the first frame of a run walks ITS run (turn_run: maximum, sum in time order, length); runs are disjoint, so the
// walks run side by side; the verdicts are balloted into the accept mask at the runs' first frames.  (c) behind a barrier every lane finds the
// first frame of the run it lies in (turn_last_clear) and with it its phase; ballots of the phases are the words of the left-turn, right-turn and
// not-straight masks; the lane at an accepted run's first frame writes the turn's row, whose index is the popcount of the accept mask below it.  Peak
// and angle it kept from (b) in the LDS slot of its own thread, tagged with the frame: a thread that has since walked a later run of its own (a
// sequence of more than 256 frames) walks the earlier one again -- the same operations, the same bits.  The rows past the count become NaN.  (d) behind
// a barrier single lanes make the per-sequence row, SPREAD OVER THE FOUR WAVES, because the lanes of one wave that take different branches run one
// after the other (what section 4.11 measured as its weakness): lane 0 of wave 0 the counts, its lanes 1 and 2 the mean duration and steps in turn,
// lane 0 of wave 1 the straight steps, of wave 2 the straight strides, of wave 3 the straight stance share, lane 1 of waves 2 and 3 the mean angle
// and the mean peak, read from the table's rows (a workgroup's own global writes are visible to it behind the barrier).  Each walks the masks by
// word and adds in time order on its own.  No atomics anywhere; no sum depends on the launch, so a sequence has the same bits alone or among others.
//
// The hook grnet_op_gait_turn_runs launches turn_seq_kernel alone on a caller's rows.
#include "kernels.h"
#include "device.h"
#include "gait_turns.h"

namespace grk {
namespace {

__global__ __launch_bounds__(256) void turn_rate_kernel(const int* __restrict__ off, const double* __restrict__ weights, int radius, int J, GaitTable tab,
                                                        const float* __restrict__ joints, double fps, double* raw, double* per_frame) {
    __shared__ double w_lds[kTrackMaxRadius + 1];
    const int f0 = off[blockIdx.x], T = off[blockIdx.x + 1] - f0;
    if ((int)threadIdx.x <= radius) w_lds[threadIdx.x] = weights[threadIdx.x];
    const float* j = joints + (size_t)f0 * J * 3;
    double* rows = per_frame + (size_t)f0 * kTurnFrameCols;
    for (int i = threadIdx.x; i < T; i += 256) {
        const double d = turn_frame_step(j, J, tab.j, i);
        rows[(size_t)i * kTurnFrameCols] = d;
        if (radius >= 0) raw[(size_t)f0 + i] = d * fps;
        else rows[(size_t)i * kTurnFrameCols + 1] = d * fps;
    }
    if (radius < 0) return;                                    // the same in every thread
    __syncthreads();
    const double* x = raw + f0;
    for (int i = threadIdx.x; i < T; i += 256) rows[(size_t)i * kTurnFrameCols + 1] = track_gauss(x, T, i, w_lds, radius);
}

// Stages (a) to (d) of one sequence on its masks: called once with the LDS arrays and once with the call's scratch, so that in each inlined copy the
// compiler knows the address space (gait_sequence_stages says why).  rows: the sequence's (T,2) [step, rate]; gait_rows: its (T,7) rows of the gait call.
struct TurnKept { int frame; double peak, angle; };             // what a thread keeps of the last run it walked in stage (b)

__device__ __forceinline__ void turn_sequence_stages(const TurnMasks& m, TurnKept* kept, int tid, int T, const TurnRule& r, const double* __restrict__ rows,
                                                     const int* __restrict__ events, const double* __restrict__ gait_rows, int* __restrict__ phase,
                                                     double* turns, double* __restrict__ out) {
    // (a) whole chunks of 64 frames, so that every lane of the wave reaches the ballots
    for (int base = (tid >> 6) * 64; base < T; base += kGaitThreads) {
        const int t = base + (tid & 63);
        const bool in = t < T;
        const double w = in ? rows[(size_t)t * kTurnFrameCols + 1] : 0.;
        const int ev = in ? events[t] : 0;
        const unsigned long long b0 = __ballot(w > r.edge_rate), b1 = __ballot(w < -r.edge_rate), b2 = __ballot(w != w);
        const unsigned long long e0 = __ballot(ev & kGaitHeelL), e1 = __ballot(ev & kGaitHeelR), e2 = __ballot(ev & kGaitToeL), e3 = __ballot(ev & kGaitToeR);
        if ((tid & 63) == 0) {
            const int k = base >> 6;
            m.left[k] = b0; m.right[k] = b1; m.unknown[k] = b2;
            m.hs_l[k] = e0; m.hs_r[k] = e1; m.to_l[k] = e2; m.to_r[k] = e3;
        }
    }
    __syncthreads();
    // (b) the runs, each by the lane at its first frame
    kept[tid].frame = -1;
    for (int base = (tid >> 6) * 64; base < T; base += kGaitThreads) {
        const int t = base + (tid & 63);
        bool ok = false;
        if (t < T) {
            const bool left = turn_run_begins(m.left, t);
            if (left || turn_run_begins(m.right, t)) {
                double peak, angle;
                ok = turn_run(rows, t, turn_run_end(left ? m.left : m.right, T, t), r, &peak, &angle);
                if (ok) kept[tid] = TurnKept{t, peak, angle};
            }
        }
        const unsigned long long acc = __ballot(ok);
        if ((tid & 63) == 0) m.accept[base >> 6] = acc;
    }
    __syncthreads();
    // (c) the phases, the turn table
    for (int base = (tid >> 6) * 64; base < T; base += kGaitThreads) {
        const int t = base + (tid & 63);
        int ph = kTurnStraight;
        if (t < T) {
            const bool left = gait_detail::bit(m.left, t);
            if (left || gait_detail::bit(m.right, t)) {
                const unsigned long long* run = left ? m.left : m.right;
                const int a = (int)turn_last_clear(run, 0, t) + 1;      // -1 where the run begins the sequence
                if (gait_detail::bit(m.accept, a)) ph = left ? kTurnLeft : kTurnRight;
                if (a == t && ph != kTurnStraight) {
                    const long long row = turn_popcount(m.accept, 0, t);
                    if (row < r.max_turns) {
                        const int e = turn_run_end(run, T, t);
                        double peak = kept[tid].peak, angle = kept[tid].angle;
                        if (kept[tid].frame != t) turn_run(rows, t, e, r, &peak, &angle);
                        turn_row(m, t, e, left, peak, angle, r.fps, turns + row * kTurnCols);
                    }
                }
            } else if (gait_detail::bit(m.unknown, t)) {
                ph = kTurnUnknown;
            }
            phase[t] = ph;
        }
        const unsigned long long p1 = __ballot(ph == kTurnLeft), p2 = __ballot(ph == kTurnRight), p3 = __ballot(ph != kTurnStraight);
        if ((tid & 63) == 0) { m.turn_l[base >> 6] = p1; m.turn_r[base >> 6] = p2; m.not_straight[base >> 6] = p3; }
    }
    const long long found = turn_popcount(m.accept, 0, T);
    for (int i = tid; i < r.max_turns * kTurnCols; i += kGaitThreads)
        if (i / kTurnCols >= found) turns[i] = gait_detail::nan();
    __syncthreads();
    // (d) the four long walks in four waves
    const int wave = tid >> 6, lane = tid & 63;
    if (lane == 0) {
        if (wave == 0) turn_counts(m, T, out);
        else if (wave == 1) turn_steps(m, T, gait_rows, r.fps, out + kTurnGaitAt);
        else if (wave == 2) turn_strides(m, T, r.fps, out + kTurnGaitAt);
        else turn_stance(m, T, out + kTurnGaitAt);
    } else if (wave == 0 && lane == 1) {
        out[kTurnColDuration] = turn_mean(m, rows, T, r, 0, turns);
    } else if (wave == 0 && lane == 2) {
        out[kTurnColTurnSteps] = turn_mean(m, rows, T, r, 3, turns);
    } else if (wave == 2 && lane == 1) {
        out[kTurnColAngle] = turn_mean(m, rows, T, r, 1, turns);
    } else if (wave == 3 && lane == 1) {
        out[kTurnColPeak] = turn_mean(m, rows, T, r, 2, turns);
    }
}

__global__ __launch_bounds__(kGaitThreads) void turn_seq_kernel(const int* __restrict__ off, TurnRule r, const double* __restrict__ per_frame,
                                                                const int* __restrict__ events, const double* __restrict__ gait_rows, unsigned long long* words,
                                                                size_t mask_words, int* __restrict__ phase, double* turns, double* __restrict__ per_seq) {
    __shared__ unsigned long long lds[kTurnMaskSets][kGaitLdsWords];
    __shared__ TurnKept kept[kGaitThreads];
    const int q = blockIdx.x, f0 = off[q], T = off[q + 1] - f0, tid = threadIdx.x;
    const double* rows = per_frame + (size_t)f0 * kTurnFrameCols;
    const double* gait = gait_rows + (size_t)f0 * kGaitFrameCols;
    double* table = turns + (size_t)q * r.max_turns * kTurnCols;
    double* out = per_seq + (size_t)q * kTurnSeqCols;
    if (((T - 1) >> 6) < kGaitLdsWords) {
        const TurnMasks m{lds[0], lds[1], lds[2], lds[3], lds[4], lds[5], lds[6], lds[7], lds[8], lds[9], lds[10]};
        turn_sequence_stages(m, kept, tid, T, r, rows, events + f0, gait, phase + f0, table, out);
    } else {
        unsigned long long* g = gait_mask_at(words, f0, q);
        const size_t s = mask_words;
        const TurnMasks m{g, g + s, g + 2 * s, g + 3 * s, g + 4 * s, g + 5 * s, g + 6 * s, g + 7 * s, g + 8 * s, g + 9 * s, g + 10 * s};
        turn_sequence_stages(m, kept, tid, T, r, rows, events + f0, gait, phase + f0, table, out);
    }
}

}  // namespace

hipError_t launch_turn_rates(const int* off, int n_seq, const double* weights, int radius, int J, const GaitTable& tab, const float* joints, double fps,
                             double* raw, double* per_frame, hipStream_t s) {
    return launch_k(turn_rate_kernel, dim3(n_seq), dim3(256), 0, s, off, weights, radius, J, tab, joints, fps, raw, per_frame);
}

hipError_t launch_turn_sequences(const int* off, int n_seq, const TurnRule& rule, const double* per_frame, const int* events, const double* gait_rows,
                                 unsigned long long* words, size_t mask_words, int* phase, double* turns, double* per_seq, hipStream_t s) {
    return launch_k(turn_seq_kernel, dim3(n_seq), dim3(kGaitThreads), 0, s, off, rule, per_frame, events, gait_rows, words, mask_words, phase, turns, per_seq);
}

}  // namespace grk
