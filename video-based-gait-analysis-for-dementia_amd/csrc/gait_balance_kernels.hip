// Footprints, centre of mass and margin of stability on the device, for many sequences lying back to back (rules and columns: DESIGN 4.22; the
// arithmetic: gait_balance.h, which the host checker runs too).
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  Everything is float64 and every operation rounds once.
//
// THREE launches behind one small upload (the sequences' offsets), whatever the number of sequences or frames.
//
// balance_frames_kernel -- ONE LANE PER FRAME over all frames of the call: rule 1, the nine values [c, rL, rR] into the call's scratch.
//
// balance_steps_kernel  -- one workgroup of four waves per sequence.  (a) a wave takes 64 consecutive frames: __ballot of the two heel-strike bits
// ARE words of two masks, aligned to the sequence, in the call's scratch (the path kernel reads them again).  (b) behind a barrier (a workgroup's
// own global writes are visible to it there) one lane counts the marks in front of every word.  (c) behind a barrier a lane whose frame is a
// mark writes it into the list at the count in front of its word plus the popc of the word's bits below it: the list lies in LDS where the
// sequence has at most kBalanceLdsStrikes marks, else in the call's scratch.  (d) behind a barrier a lane per pair of consecutive marks does
// rules 3 and 4 (balance_pair: its loops run over at most max_step + 1 and window + 1 frames) into the pair's row in the scratch.  (e) behind a
// barrier ONE lane adds the footprints in time order (balance_chain): float64 addition is not associative, and the statement adds them one after
// the other.  (f) behind a barrier a lane per step does rules 6 and 8 (balance_stride, at most 2 max_step + 1 frames) and copies its row into the
// step table where its number is below max_steps; the rows past the count become NaN.  (g) behind a barrier one lane makes the per-sequence row
// in time order (balance_row).  No atomics anywhere; no sum depends on the launch, so a sequence has the same bits alone or among others.
// Every value is written with a plain vector store.
//
// balance_path_kernel   -- ONE LANE PER FRAME: its sequence by bisection in the offsets, the marks in front of it from the words, rule 7.
//
// The hook grnet_op_gait_balance_steps launches the last two on a caller's [c, rL, rR].  grnet_gait_balance_com launches balance_com_frames_kernel
// in place of the first: the caller's c (the mesh's centre of mass), the ankles subtracted.
#include "kernels.h"
#include "device.h"
#include "gait_balance.h"

namespace grk {
namespace {

__global__ __launch_bounds__(256) void balance_frames_kernel(const float* __restrict__ joints, int J, int frames, int lankle, int rankle, BalanceSegments seg,
                                                             double* __restrict__ rel) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= frames) return;
    double r[kBalanceRelCols];
    balance_com(joints + (size_t)f * J * 3, seg, lankle, rankle, r);
    for (int k = 0; k < kBalanceRelCols; ++k) rel[(size_t)f * kBalanceRelCols + k] = r[k];
}

// rule 1 with the caller's centre of mass in place of the segment table's (grnet_gait_balance_com): ONE LANE PER FRAME
__global__ __launch_bounds__(256) void balance_com_frames_kernel(const float* __restrict__ joints, int J, int frames, int lankle, int rankle,
                                                                 const double* __restrict__ com, double* __restrict__ rel) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= frames) return;
    double r[kBalanceRelCols];
    balance_rel_of(joints + (size_t)f * J * 3, com + (size_t)f * 3, lankle, rankle, r);
    for (int k = 0; k < kBalanceRelCols; ++k) rel[(size_t)f * kBalanceRelCols + k] = r[k];
}

__global__ __launch_bounds__(kGaitThreads) void balance_steps_kernel(const int* __restrict__ off, BalanceRule r, const double* __restrict__ rel_all,
                                                                     const int* __restrict__ events_all, unsigned long long* words, size_t mask_words,
                                                                     int* list_all, double* pairs_all, double* __restrict__ steps_all,
                                                                     double* __restrict__ per_seq) {
    __shared__ int lds_list[kBalanceLdsStrikes];
    __shared__ long long shared[4];                            // marks, strikes, steps, chains
    const int q = blockIdx.x, f0 = off[q], T = off[q + 1] - f0, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* rel = rel_all + (size_t)f0 * kBalanceRelCols;
    const int* events = events_all + f0;
    unsigned long long* left = gait_mask_at(words, f0, q);
    unsigned long long* right = left + mask_words;
    unsigned long long* before = right + mask_words;
    double* pairs = pairs_all + (size_t)f0 * kBalancePairCols;
    double* steps = steps_all + (size_t)q * r.max_steps * kBalanceStepCols;
    // (a) whole chunks of 64 frames, so that every lane of the wave reaches the ballots
    for (int base = wave * 64; base < T; base += kGaitThreads) {
        const int k = base + lane;
        const int ev = k < T ? events[k] : 0;
        const unsigned long long l = __ballot(ev & kBalanceLeft), rr = __ballot(ev & kBalanceRight);
        if (lane == 0) { left[base >> 6] = l; right[base >> 6] = rr; }
    }
    __syncthreads();
    // (b)
    if (tid == 0) {
        long long n = 0, single = 0;
        for (int w = 0; w <= (T - 1) >> 6; ++w) {
            before[w] = (unsigned long long)n;
            n += __builtin_popcountll(left[w] | right[w]);
            single += __builtin_popcountll(left[w] ^ right[w]);
        }
        shared[0] = n;
        shared[1] = single;
    }
    __syncthreads();
    // (c)
    const long long n_marks = shared[0], n_pairs = n_marks > 0 ? n_marks - 1 : 0;
    int* list = n_marks <= kBalanceLdsStrikes ? lds_list : list_all + f0;
    for (int k = tid; k < T; k += kGaitThreads) {
        const int ev = events[k] & (kBalanceLeft | kBalanceRight);
        if (ev) list[balance_marks_before(left, right, before, k)] = (k << 2) | ev;
    }
    __syncthreads();
    // (d)
    for (long long i = tid; i < n_pairs; i += kGaitThreads) balance_pair(rel, T, list[i], list[i + 1], r, pairs + i * kBalancePairCols);
    __syncthreads();
    // (e)
    if (tid == 0) balance_chain(pairs, n_pairs, shared + 2);
    __syncthreads();
    // (f)
    const long long n_steps = shared[2];
    for (long long i = tid; i < n_pairs; i += kGaitThreads) {
        double* row = pairs + i * kBalancePairCols;
        const double number = row[kBalanceColNumber];
        if (!(number >= 0.)) continue;
        balance_stride(rel, pairs, i);
        if (number < (double)r.max_steps)
            for (int k = 0; k < kBalanceStepCols; ++k) steps[(long long)number * kBalanceStepCols + k] = row[k];
    }
    for (int i = tid; i < r.max_steps * kBalanceStepCols; i += kGaitThreads)
        if (i / kBalanceStepCols >= n_steps) steps[i] = gait_detail::nan();
    __syncthreads();
    // (g)
    if (tid == 0) balance_row(pairs, n_pairs, shared[1], n_steps, shared[3], r.fps, per_seq + (size_t)q * kBalanceSeqCols);
}

__global__ __launch_bounds__(256) void balance_path_kernel(const int* __restrict__ off, int n_seq, int frames, const double* __restrict__ rel_all,
                                                           const unsigned long long* __restrict__ words, size_t mask_words,
                                                           const double* __restrict__ pairs_all, double* __restrict__ per_frame) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= frames) return;
    int lo = 0, hi = n_seq;                                    // the least q with off[q] > f: off[0] = 0 <= f < frames = off[n_seq]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] > f) hi = mid; else lo = mid + 1;
    }
    const int q = lo - 1, f0 = off[q], T = off[q + 1] - f0, t = f - f0;
    const unsigned long long* left = words + (size_t)(f0 >> 6) + q;      // gait_mask_at
    const unsigned long long* right = left + mask_words;
    const unsigned long long* before = right + mask_words;
    const bool at = gait_detail::bit(left, t) || gait_detail::bit(right, t);
    double out[kBalanceFrameCols];
    balance_path(rel_all + (size_t)f0 * kBalanceRelCols, pairs_all + (size_t)f0 * kBalancePairCols, balance_mark_count(left, right, before, T),
                 balance_marks_before(left, right, before, t), at, t, out);
    for (int k = 0; k < kBalanceFrameCols; ++k) per_frame[(size_t)f * kBalanceFrameCols + k] = out[k];
}

}  // namespace

hipError_t launch_balance_frames(const float* joints, int J, int frames, const GaitTable& tab, const BalanceSegments& seg, double* rel, hipStream_t s) {
    return launch_k(balance_frames_kernel, dim3((frames + 255) / 256), dim3(256), 0, s, joints, J, frames, tab.j[4], tab.j[5], seg, rel);
}

hipError_t launch_balance_com_frames(const float* joints, int J, int frames, const GaitTable& tab, const double* com, double* rel, hipStream_t s) {
    return launch_k(balance_com_frames_kernel, dim3((frames + 255) / 256), dim3(256), 0, s, joints, J, frames, tab.j[4], tab.j[5], com, rel);
}

hipError_t launch_balance_steps(const int* off, int n_seq, const BalanceRule& rule, const double* rel, const int* events, unsigned long long* words,
                                size_t mask_words, int* list, double* pairs, double* steps, double* per_seq, hipStream_t s) {
    return launch_k(balance_steps_kernel, dim3(n_seq), dim3(kGaitThreads), 0, s, off, rule, rel, events, words, mask_words, list, pairs, steps, per_seq);
}

hipError_t launch_balance_path(const int* off, int n_seq, int frames, const double* rel, const unsigned long long* words, size_t mask_words,
                               const double* pairs, double* per_frame, hipStream_t s) {
    return launch_k(balance_path_kernel, dim3((frames + 255) / 256), dim3(256), 0, s, off, n_seq, frames, rel, words, mask_words, pairs, per_frame);
}

}  // namespace grk
