// Gait events and parameters from the 3D joints on the device, for many sequences lying back to back (rules and columns: DESIGN 4.11; the
// arithmetic: gait_events.h, which the host checker runs too; the Gaussian and the bitmask searches: track_boxes.h).
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  Everything is float64 and every operation rounds once.
//
// At most three launches behind one small upload (the sequences' offsets and the Gaussian weights), whatever the number of sequences or frames.
//
// gait_frame_kernel  -- ONE LANE PER FRAME over all frames of the call, sequences ignored: a frame is eight joints, one cross product, two square
// roots and five dot products, far too little for a wave (the reasons of track_frame_kernel).  The four signals go to the call's scratch, one
// column each, where a Gaussian follows, else straight into the per-frame rows; the width goes into its row either way.
//
// sigma > 0 alone    -- seq_gauss_columns_kernel (track_kernels.hip) on the four columns: columns 0 .. 3 of the rows, which are 7 wide.
//
// gait_seq_kernel    -- one workgroup of four waves per sequence.  (a) events: a wave takes 64 consecutive frames of the sequence, a lane a frame;
// the lane's four tests read the 2w + 1 rows around it, and __ballot of each kind IS one word of that kind's bitmask -- the words are aligned
// to the sequence and lie in LDS where the sequence has at most 64 * kGaitLdsWords frames, else in the call's scratch (gait_mask_at of each of the
// four masks there).  The lane writes its events entry and the step length and width of its row.
// (b) behind one barrier (a workgroup's own global writes are visible to it there) wave 0 makes the
// per-sequence row: lanes 0 to 3 the counts, lane 4 the steps, 5 the strides, 6 the stance share, 7 the speed along the trajectory -- each
// walks the masks by word and adds in time order on its own, so no sum depends on the launch.  No atomics anywhere.
//
// gait_events_kernel -- the hook grnet_op_gait_events: stage (a)'s tests alone on a caller's (frames, 4) signals.
#include "kernels.h"
#include "device.h"
#include "gait_events.h"

namespace grk {
namespace {

__global__ __launch_bounds__(256) void gait_frame_kernel(const float* __restrict__ joints, int J, int frames, GaitTable tab, double* __restrict__ raw,
                                                         double* __restrict__ per_frame) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= frames) return;
    double sig[5];
    gait_frame(joints + (size_t)f * J * 3, tab.j, sig);
    double* row = per_frame + (size_t)f * kGaitFrameCols;
    for (int k = 0; k < 4; ++k) {
        if (raw) raw[(size_t)k * frames + f] = sig[k];
        else row[k] = sig[k];
    }
    row[4] = sig[4];
}

// Stages (a) and (b) of one sequence on its four bitmasks m[k][0, ceil(T / 64)): called once with the LDS array and once with the call's scratch, so that
// in each inlined copy the compiler knows the address space (track_sequence_stages says why).  Stage (b) is a chain of dependent loads of mask words
// by single lanes: from LDS a link costs tens of cycles, from memory many hundreds.
__device__ __forceinline__ void gait_sequence_stages(unsigned long long* m0, unsigned long long* m1, unsigned long long* m2, unsigned long long* m3, int tid, int T,
                                                     int J, int pelvis, const float* __restrict__ joints, const double* __restrict__ trans, double fps, int window,
                                                     double min_excursion, double* rows, int* __restrict__ events, double* __restrict__ out) {
    // (a) whole chunks of 64 frames, so that every lane of the wave reaches the ballots
    for (int base = (tid >> 6) * 64; base < T; base += kGaitThreads) {
        const int t = base + (tid & 63);
        int ev = 0;
        if (t < T) {
            ev = gait_frame_events(rows, T, t, window, min_excursion);
            events[t] = ev;
        }
        const unsigned long long b0 = __ballot(ev & kGaitHeelL), b1 = __ballot(ev & kGaitHeelR), b2 = __ballot(ev & kGaitToeL), b3 = __ballot(ev & kGaitToeR);
        if ((tid & 63) == 0) { m0[base >> 6] = b0; m1[base >> 6] = b1; m2[base >> 6] = b2; m3[base >> 6] = b3; }
    }
    __syncthreads();
    // (b)
    if (tid >= 8) return;
    if (tid < 4) out[kGaitColCounts + tid] = gait_count(tid == 0 ? m0 : tid == 1 ? m1 : tid == 2 ? m2 : m3, T);
    else if (tid == 4) gait_steps(m0, m1, T, rows, fps, out);
    else if (tid == 5) gait_strides(m0, m1, T, fps, out);
    else if (tid == 6) gait_stance(m0, m1, m2, m3, T, out);
    else gait_traj_speed(m0, m1, T, joints, J, pelvis, trans, fps, out);
}

__global__ __launch_bounds__(kGaitThreads) void gait_seq_kernel(const int* __restrict__ off, int J, int pelvis, const float* __restrict__ joints,
                                                                const double* __restrict__ trans, double fps, int window, double min_excursion,
                                                                unsigned long long* words, size_t mask_words, double* per_frame, int* __restrict__ events,
                                                                double* __restrict__ per_seq) {
    __shared__ unsigned long long lds[4][kGaitLdsWords];
    const int q = blockIdx.x, f0 = off[q], T = off[q + 1] - f0, tid = threadIdx.x;
    double* rows = per_frame + (size_t)f0 * kGaitFrameCols;
    const float* j = joints + (size_t)f0 * J * 3;
    const double* tr = trans ? trans + (size_t)f0 * 3 : nullptr;
    double* out = per_seq + (size_t)q * kGaitSeqCols;
    if (((T - 1) >> 6) < kGaitLdsWords) {
        gait_sequence_stages(lds[0], lds[1], lds[2], lds[3], tid, T, J, pelvis, j, tr, fps, window, min_excursion, rows, events + f0, out);
    } else {
        unsigned long long* g = gait_mask_at(words, f0, q);
        gait_sequence_stages(g, g + mask_words, g + 2 * mask_words, g + 3 * mask_words, tid, T, J, pelvis, j, tr, fps, window, min_excursion, rows, events + f0, out);
    }
}

__global__ __launch_bounds__(256) void gait_events_kernel(const int* __restrict__ off, const double* __restrict__ signals, int window, double min_excursion,
                                                          int* __restrict__ events) {
    const int f0 = off[blockIdx.x], T = off[blockIdx.x + 1] - f0;
    const double* s = signals + (size_t)f0 * 4;
    for (int t = threadIdx.x; t < T; t += 256) {
        int ev = 0;
        for (int k = 0; k < 2; ++k) {
            if (gait_heel_strike(s + k, 4, T, t, window, min_excursion)) ev |= kGaitHeelL << k;
            if (gait_toe_off(s + 2 + k, 4, T, t, window, min_excursion)) ev |= kGaitToeL << k;
        }
        events[(size_t)f0 + t] = ev;
    }
}

}  // namespace

hipError_t launch_gait_frames(const float* joints, int J, int frames, const GaitTable& tab, double* raw, double* per_frame, hipStream_t s) {
    return launch_k(gait_frame_kernel, dim3((frames + 255) / 256), dim3(256), 0, s, joints, J, frames, tab, raw, per_frame);
}

hipError_t launch_gait_sequences(const int* off, int n_seq, int J, int pelvis, const float* joints, const double* trans, double fps, int window,
                                 double min_excursion, unsigned long long* words, size_t mask_words, double* per_frame, int* events, double* per_seq, hipStream_t s) {
    return launch_k(gait_seq_kernel, dim3(n_seq), dim3(kGaitThreads), 0, s, off, J, pelvis, joints, trans, fps, window, min_excursion, words, mask_words, per_frame,
                    events, per_seq);
}

hipError_t launch_gait_events(const int* off, int n_seq, const double* signals, int window, double min_excursion, int* events, hipStream_t s) {
    return launch_k(gait_events_kernel, dim3(n_seq), dim3(256), 0, s, off, signals, window, min_excursion, events);
}

}  // namespace grk
