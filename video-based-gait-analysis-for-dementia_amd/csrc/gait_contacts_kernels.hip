// Foot contact phases and double support on the device, for many sequences lying back to back (rules and columns: DESIGN 4.14; the arithmetic:
// gait_contacts.h, which the host checker runs too; the Gaussian and the bitmask searches: track_boxes.h, gait_turns.h).
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  Everything is float64 and every operation rounds once.
//
// At most THREE launches (two without a Gaussian) behind one small upload (the sequences' offsets and the Gaussian weights), whatever the number
// of sequences or frames.
//
// contact_frame_kernel  -- ONE LANE PER FRAME over all frames of the call (the reasons of gait_frame_kernel): two joints, one difference vector.
// Without a Gaussian the lane makes the vector of the next frame too and with it s of its interval; whether its frame is the last of a sequence,
// whose s is NaN, it finds by bisection in the offsets.  With one the three columns go to the call's scratch.
//
// sigma > 0 alone      -- seq_gauss_columns_kernel (track_kernels.hip) on the three columns: columns 1 .. 3 of the rows, which are 4 wide.
//
// contact_seq_kernel    -- one workgroup of four waves per sequence.  (0) after a Gaussian the lanes make s from the smoothed vectors, then a
// barrier (a workgroup's own global writes are visible to it there).  (a) a wave takes 64 consecutive intervals, a lane an interval: an xor
// butterfly over the lanes (1, 2, 4, ... 32) adds adjacent pairs, then pairs of those -- contact_block_sum's tree, and since a + b and b + a have
// the same bits every lane ends with the block's sum; __ballot of "s is finite" and of the two heel-strike bits ARE words of three masks, aligned
// to the sequence, in LDS where the sequence has at most 64 * kGaitLdsWords frames, else in the call's scratch (gait_mask_at
// of each).  Behind a barrier one lane adds the blocks in time order and makes the threshold.  (b) behind a barrier
// __ballot(s < thr) is a word of the static mask.  (c) behind a barrier a lane whose interval is not static writes its phase; the lane at a run's
// first interval finds the run's end by word, walks ITS run (contact_run: closed, edges, attribution from the heel-strike masks by word, least s),
// writes the phases of its intervals and the run's row, whose index is the number of runs that begin below it, and keeps lead, edges and end of
// the sequence's first kContactKeptRuns runs in LDS for stage (d), whose walks would else find every run by word in the masks and make its edges
// again -- four loads from memory and two divisions a run, four times over.  Runs are disjoint, so the walks run side by side.  Ballots of
// left-led and right-led at the runs' first intervals are two masks more.  The rows past the count become NaN.  (d) behind a barrier single lanes
// make the per-sequence row, SPREAD OVER THREE WAVES because the lanes of one wave that take different branches run one after the other (DESIGN
// 4.11's weakness): lane 0 of wave 0 the threshold and the counts, of wave 1 the double-support columns, of wave 2 the strides.  Each walks the
// runs in time order on its own (contact_next: the kept rows, then the masks by word).  No atomics anywhere; no sum depends on the launch, so a
// sequence has the same bits alone or among others.  Every value is written with a plain vector store.
//
// The hook grnet_op_gait_contact_runs launches contact_seq_kernel alone on a caller's speeds.
#include "kernels.h"
#include "device.h"
#include "gait_contacts.h"

namespace grk {
namespace {

__global__ __launch_bounds__(256) void contact_frame_kernel(const int* __restrict__ off, int n_seq, const float* __restrict__ joints, int J, int frames,
                                                            GaitTable tab, double fps, double* __restrict__ raw, double* __restrict__ per_frame) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= frames) return;
    double d0[3];
    contact_vector(joints + (size_t)f * J * 3, tab.j, d0);
    if (raw) {
        for (int a = 0; a < 3; ++a) raw[(size_t)a * frames + f] = d0[a];
        return;
    }
    double* row = per_frame + (size_t)f * kContactFrameCols;
    for (int a = 0; a < 3; ++a) row[1 + a] = d0[a];
    int lo = 0, hi = n_seq;                                    // the least q with off[q] > f: off[0] = 0 <= f < frames = off[n_seq]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] > f) hi = mid; else lo = mid + 1;
    }
    double s = gait_detail::nan();
    if (off[lo] != f + 1) {                                    // not the last frame of its sequence, so frame f + 1 exists
        double d1[3];
        contact_vector(joints + (size_t)(f + 1) * J * 3, tab.j, d1);
        s = contact_speed(d0, d1, fps);
    }
    row[0] = s;
}

// Stages (a) to (d) of one sequence on its masks and block sums: called once with the LDS arrays and once with the call's scratch, so that in each
// inlined copy the compiler knows the address space (gait_sequence_stages says why).  s: the sequence's speeds, `stride` values apart.
__device__ __forceinline__ void contact_sequence_stages(const ContactMasks& m, double* blocks, double* shared, double* kept_rows, int tid, int T, const ContactRule& r,
                                                        const double* s, long long stride, const int* __restrict__ events, int* __restrict__ phase,
                                                        double* runs, double* __restrict__ out) {
    const int lane = tid & 63, wave = tid >> 6;
    // (a) whole chunks of 64 intervals, so that every lane of the wave reaches the cross-lane moves and the ballots
    for (int base = wave * 64; base < T; base += kGaitThreads) {
        const int k = base + lane;
        const double v = k < T - 1 ? s[(long long)k * stride] : gait_detail::nan();
        const bool fin = translation_detail::finite(v);
        double x = fin ? v : 0.;
        for (int o = 1; o < kContactBlock; o <<= 1) x = x + __shfl_xor(x, o);
        const int ev = k < T ? events[k] : 0;
        const unsigned long long b0 = __ballot(fin), e0 = __ballot(ev & kGaitHeelL), e1 = __ballot(ev & kGaitHeelR);
        if (lane == 0) { blocks[base >> 6] = x; m.finite[base >> 6] = b0; m.hs_l[base >> 6] = e0; m.hs_r[base >> 6] = e1; }
    }
    __syncthreads();
    if (tid == 0) shared[0] = contact_threshold(blocks, m.finite, T, r, &shared[1]);
    __syncthreads();
    const double thr = shared[0];
    // (b)
    for (int base = wave * 64; base < T; base += kGaitThreads) {
        const int k = base + lane;
        const unsigned long long b = __ballot(k < T - 1 && s[(long long)k * stride] < thr);
        if (lane == 0) m.is_static[base >> 6] = b;
    }
    __syncthreads();
    // (c) the phases, the runs, the run table
    for (int base = wave * 64; base < T; base += kGaitThreads) {
        const int k = base + lane;
        bool left = false, right = false;
        if (k == T - 1) {
            phase[k] = kContactNan;
        } else if (k < T - 1) {
            if (!gait_detail::bit(m.is_static, k)) {
                const double v = s[(long long)k * stride];
                phase[k] = v != v ? kContactNan : kContactMoving;
            } else if (contact_run_begins(m.is_static, k)) {
                const int b = contact_run_end(m.is_static, T, k) - 1;
                const ContactRun run = contact_run(m, s, stride, T, k, b, thr, r);
                left = run.lead > 0; right = run.lead < 0;
                const int ph = contact_phase(run.lead);
                for (int i = k; i <= b; ++i) phase[i] = ph;
                const long long row = contact_runs_before(m.is_static, k);
                if (row < r.max_runs) contact_row(run, r.fps, runs + row * kContactRunCols);
                if (row < kContactKeptRuns) contact_keep(kept_rows, row, run.lead, run.t_start, run.t_end, b + 1);
            }
        }
        const unsigned long long p0 = __ballot(left), p1 = __ballot(right);
        if (lane == 0) { m.lead_l[base >> 6] = p0; m.lead_r[base >> 6] = p1; }
    }
    const long long found = contact_runs_before(m.is_static, T);
    for (int i = tid; i < r.max_runs * kContactRunCols; i += kGaitThreads)
        if (i / kContactRunCols >= found) runs[i] = gait_detail::nan();
    __syncthreads();
    // (d) the three walks in three waves
    if (lane != 0) return;
    const ContactKept kept{kept_rows, kContactKeptRuns, found};
    if (wave == 0) {
        out[kContactColThr] = thr;
        out[kContactColMean] = shared[1];
        contact_counts(m, T, out);
    } else if (wave == 1) {
        contact_support(m, kept, s, stride, T, thr, r.fps, out);
    } else if (wave == 2) {
        contact_strides(m, kept, s, stride, T, thr, r.fps, out);
    }
}

// rows: per_frame (frames,4), or null for the hook, whose speeds lie one value apart; make_s: the vectors were smoothed, so s is made here
__global__ __launch_bounds__(kGaitThreads) void contact_seq_kernel(const int* __restrict__ off, ContactRule r, double* per_frame, const double* speeds, int make_s,
                                                                   const int* __restrict__ events, unsigned long long* words, size_t mask_words,
                                                                   int* __restrict__ phase, double* runs, double* __restrict__ per_seq) {
    __shared__ unsigned long long lds[kContactMaskSets][kGaitLdsWords];
    __shared__ double lds_blocks[kGaitLdsWords];
    __shared__ double shared[2];
    __shared__ double kept_rows[kContactKeptCols * kContactKeptRuns];
    const int q = blockIdx.x, f0 = off[q], T = off[q + 1] - f0, tid = threadIdx.x;
    const double* s = per_frame ? per_frame + (size_t)f0 * kContactFrameCols : speeds + f0;
    const long long stride = per_frame ? kContactFrameCols : 1;
    if (make_s) {
        double* rows = per_frame + (size_t)f0 * kContactFrameCols;
        for (int k = tid; k < T; k += kGaitThreads)
            rows[(size_t)k * kContactFrameCols] = k < T - 1 ? contact_speed(rows + (size_t)k * kContactFrameCols + 1, rows + (size_t)(k + 1) * kContactFrameCols + 1, r.fps)
                                                            : gait_detail::nan();
        __syncthreads();
    }
    double* table = runs + (size_t)q * r.max_runs * kContactRunCols;
    double* out = per_seq + (size_t)q * kContactSeqCols;
    if (((T - 1) >> 6) < kGaitLdsWords) {
        const ContactMasks m{lds[0], lds[1], lds[2], lds[3], lds[4], lds[5]};
        contact_sequence_stages(m, lds_blocks, shared, kept_rows, tid, T, r, s, stride, events + f0, phase + f0, table, out);
    } else {
        unsigned long long* g = gait_mask_at(words, f0, q);
        const size_t n = mask_words;
        const ContactMasks m{g, g + n, g + 2 * n, g + 3 * n, g + 4 * n, g + 5 * n};
        contact_sequence_stages(m, reinterpret_cast<double*>(g + kContactMaskSets * n), shared, kept_rows, tid, T, r, s, stride, events + f0, phase + f0, table, out);
    }
}

}  // namespace

hipError_t launch_contact_frames(const int* off, int n_seq, const float* joints, int J, int frames, const GaitTable& tab, double fps, double* raw,
                                 double* per_frame, hipStream_t s) {
    return launch_k(contact_frame_kernel, dim3((frames + 255) / 256), dim3(256), 0, s, off, n_seq, joints, J, frames, tab, fps, raw, per_frame);
}

hipError_t launch_contact_sequences(const int* off, int n_seq, const ContactRule& rule, double* per_frame, const double* speeds, bool make_s, const int* events,
                                    unsigned long long* words, size_t mask_words, int* phase, double* runs, double* per_seq, hipStream_t s) {
    return launch_k(contact_seq_kernel, dim3(n_seq), dim3(kGaitThreads), 0, s, off, rule, per_frame, speeds, make_s ? 1 : 0, events, words, mask_words, phase, runs,
                    per_seq);
}

}  // namespace grk
