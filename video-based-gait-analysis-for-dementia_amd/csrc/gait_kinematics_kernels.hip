// Joint-angle kinematics per gait cycle on the device, for many sequences lying back to back (rules and columns: DESIGN 4.12; the arithmetic:
// gait_angles.h, which the host checker runs too; the Gaussian and the bitmask searches: track_boxes.h).
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  Everything is float64 and every operation rounds once.
//
// At most three launches behind one small upload (the sequences' offsets and the Gaussian weights), whatever the number of sequences or frames.
//
// kin_frame_kernel  -- ONE LANE PER FRAME over all frames of the call, sequences ignored: a frame is 16 joints and 13 angles, each an arctangent of some
// sixty operations without a branch that depends on more than the octant (the reasons of track_frame_kernel).  The 13 angles go to the call's scratch,
// one column each, where a Gaussian follows, else straight into the per-frame rows.
//
// sigma > 0 alone  -- seq_gauss_columns_kernel (track_kernels.hip) on the 13 columns: all of the rows, which are 13 wide.
//
// kin_cycle_kernel  -- one workgroup of four waves per (sequence, channel).  (a) a wave takes 64 consecutive frames of the sequence's events, a lane a
// frame: __ballot of the left and of the right heel strike IS one word of that foot's bitmask -- the words are aligned to the sequence and lie in LDS
// where the sequence has at most 64 * kKinLdsWords frames, else in the call's scratch, where every (channel, foot) has a mask of its own
// (gait_mask_at of it).  (b) behind one barrier EVERY thread walks the channel's foot's
// mask by word (kin_channel): the walk is the same in all of them, so nothing diverges; a stride's finiteness, maximum and minimum are one reduction of
// the workgroup (shuffles inside a wave, twelve doubles of LDS across the four: comparisons and a logical and, exact whatever the order); threads
// 0 .. 100 each add their own cycle point over the used strides in time order, every thread holds the same sums of the row, and thread 0 writes it.
// Two passes: means, then squares.  (c) the symmetry index needs the mean range of motion of the partner channel, which another workgroup makes: the
// workgroup makes it again for itself (kin_rom: the first pass over the partner's column and foot), the same operations in the same order, so that
// both channels of a pair write the same bits and no workgroup waits for another.  No atomics anywhere.
#include "kernels.h"
#include "device.h"
#include "gait_angles.h"

namespace grk {
namespace {

__global__ __launch_bounds__(256) void kin_frame_kernel(const float* __restrict__ joints, int J, int frames, KinTable tab, double* __restrict__ raw,
                                                        double* __restrict__ per_frame) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= frames) return;
    double ang[kKinChannels];
    kin_frame(joints + (size_t)f * J * 3, tab.j, ang);
    for (int k = 0; k < kKinChannels; ++k) {
        if (raw) raw[(size_t)k * frames + f] = ang[k];
        else per_frame[(size_t)f * kKinChannels + k] = ang[k];
    }
}

// Whether column x (frame i at x[i * kKinChannels]) is finite on all of [t0, t0 + L], and its maximum and minimum there: every thread of the workgroup
// calls it with the same (t0, L) and every thread gets the same answer.  red: 12 doubles of LDS.
__device__ __forceinline__ bool kin_extent_workgroup(const double* __restrict__ x, int t0, int L, int tid, double* red, double* mx, double* mn) {
    bool fin = true;
    double a = -__builtin_inf(), b = __builtin_inf();
    for (int i = tid; i <= L; i += kKinThreads) {
        const double v = x[(size_t)(t0 + i) * kKinChannels];
        fin = fin && translation_detail::finite(v);
        a = v > a ? v : a;
        b = v < b ? v : b;
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const double oa = __shfl_xor(a, m), ob = __shfl_xor(b, m);
        a = oa > a ? oa : a;
        b = ob < b ? ob : b;
    }
    const bool wave_fin = __ballot(!fin) == 0ull;
    if ((tid & 63) == 0) { red[tid >> 6] = a; red[4 + (tid >> 6)] = b; red[8 + (tid >> 6)] = wave_fin ? 1. : 0.; }
    __syncthreads();
    a = red[0]; b = red[4];
    bool all = red[8] != 0.;
    for (int k = 1; k < kKinThreads / 64; ++k) {
        a = red[k] > a ? red[k] : a;
        b = red[4 + k] < b ? red[4 + k] : b;
        all = all && red[8 + k] != 0.;
    }
    __syncthreads();                                           // the next stride writes red again
    *mx = a; *mn = b;
    return all;
}

// Stages (a) to (c) of one (sequence, channel) on the two heel-strike bitmasks m_l, m_r[0, ceil(T / 64)): called once with the LDS arrays and once with
// the call's scratch, so that in each inlined copy the compiler knows the address space (gait_sequence_stages says why).
__device__ __forceinline__ void kin_cycle_stages(unsigned long long* m_l, unsigned long long* m_r, int tid, int T, int c, const int* __restrict__ events,
                                                 const double* __restrict__ rows, int min_stride, int max_stride, double* red, double* __restrict__ curve,
                                                 double* __restrict__ row) {
    // (a) whole chunks of 64 frames, so that every lane of the wave reaches the ballots
    for (int base = (tid >> 6) * 64; base < T; base += kKinThreads) {
        const int t = base + (tid & 63);
        const int ev = t < T ? events[t] : 0;
        const unsigned long long b0 = __ballot(ev & kGaitHeelL), b1 = __ballot(ev & kGaitHeelR);
        if ((tid & 63) == 0) { m_l[base >> 6] = b0; m_r[base >> 6] = b1; }
    }
    __syncthreads();
    // (b)
    const double* x = rows + c;
    const int p = tid < kKinPoints ? tid : -1;
    double r[kKinSeqCols], pt[2];
    kin_channel(kin_foot(c) ? m_r : m_l, x, kKinChannels, T, min_stride, max_stride,
                [=](int t0, int L, double* mx, double* mn) { return kin_extent_workgroup(x, t0, L, tid, red, mx, mn); }, p, r, pt);
    if (p >= 0) { curve[2 * p] = pt[0]; curve[2 * p + 1] = pt[1]; }
    // (c)
    const int o = kin_partner(c);
    r[5] = gait_detail::nan();
    if (o >= 0) {
        const double* y = rows + o;
        double n_o, rom_o;
        kin_rom(kin_foot(o) ? m_r : m_l, T, min_stride, max_stride,
                [=](int t0, int L, double* mx, double* mn) { return kin_extent_workgroup(y, t0, L, tid, red, mx, mn); }, &n_o, &rom_o);
        r[5] = (c & 1) ? kin_symmetry(n_o, rom_o, r[0], r[3]) : kin_symmetry(r[0], r[3], n_o, rom_o);
    }
    if (tid == 0)
        for (int k = 0; k < kKinSeqCols; ++k) row[k] = r[k];
}

__global__ __launch_bounds__(kKinThreads) void kin_cycle_kernel(const int* __restrict__ off, const int* __restrict__ events, const double* __restrict__ per_frame,
                                                                int min_stride, int max_stride, unsigned long long* words, size_t mask_words,
                                                                double* __restrict__ curves, double* __restrict__ per_seq) {
    __shared__ unsigned long long lds[2][kKinLdsWords];
    __shared__ double red[12];
    const int q = blockIdx.x, c = blockIdx.y, f0 = off[q], T = off[q + 1] - f0, tid = threadIdx.x;
    const double* rows = per_frame + (size_t)f0 * kKinChannels;
    double* curve = curves + ((size_t)q * kKinChannels + c) * kKinPoints * 2;
    double* row = per_seq + ((size_t)q * kKinChannels + c) * kKinSeqCols;
    if (((T - 1) >> 6) < kKinLdsWords) {
        kin_cycle_stages(lds[0], lds[1], tid, T, c, events + f0, rows, min_stride, max_stride, red, curve, row);
    } else {
        unsigned long long* g = gait_mask_at(words + (size_t)(2 * c) * mask_words, f0, q);
        kin_cycle_stages(g, g + mask_words, tid, T, c, events + f0, rows, min_stride, max_stride, red, curve, row);
    }
}

}  // namespace

hipError_t launch_kin_frames(const float* joints, int J, int frames, const KinTable& tab, double* raw, double* per_frame, hipStream_t s) {
    return launch_k(kin_frame_kernel, dim3((frames + 255) / 256), dim3(256), 0, s, joints, J, frames, tab, raw, per_frame);
}

hipError_t launch_kin_cycles(const int* off, int n_seq, const int* events, const double* per_frame, int min_stride, int max_stride, unsigned long long* words,
                             size_t mask_words, double* curves, double* per_seq, hipStream_t s) {
    return launch_k(kin_cycle_kernel, dim3(n_seq, kKinChannels), dim3(kKinThreads), 0, s, off, events, per_frame, min_stride, max_stride, words, mask_words, curves,
                    per_seq);
}

}  // namespace grk
