// Per-frame boxes from 2D joints on the device: the reference's lib/utils/smooth_bbox.py (kp_to_bbox_param, get_all_bbox_params, smooth_bbox_params)
// and the box of lib/dataset/inference.py:57-66, for many sequences lying back to back (rules, bars and stated differences: DESIGN 4.10; the
// arithmetic: track_boxes.h, which the host checker runs too).
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  Everything is float64 and every operation rounds once.
//
// Two launches behind one small upload (the sequences' offsets and the Gaussian weights), whatever the number of sequences or frames.
//
// track_frame_kernel -- ONE LANE PER FRAME over all frames of the call, sequences ignored: a frame is K <= 64 rows, four running extremes and one
// square root, far too little for a wave, and a lane per frame needs no cross-lane traffic for it (the reasons of translation_fit_kernel: a lane
// walks its own contiguous row, the lines it touches stay in L1 over its following joints, the input is read once, and the call waits for latency,
// not bytes).  The one cross-lane step is free: the wave's 64 frames are 64 consecutive frames of the call, so __ballot of `detected` IS word
// f >> 6 of the validity bitmask.  The words are aligned to the call, not to the sequences; the searches of track_boxes.h take any bit range.
//
// track_seq_kernel -- one workgroup of 1024 threads per sequence: a sequence of 400 frames is 1200 medians and 1200 Gaussians, each a chain of LDS
// reads, and the call waits for the longest thread.  (a) start / end: every thread looks at words of the bitmask, a butterfly and sixteen LDS words give
// the first and last detected frame.  (b) fill: thread per frame of [start, end); a dead frame finds its detected neighbours by word (track_prev /
// track_next) and takes track_fill per column.  (c) median and (d) Gaussian: thread per (column, frame), from one buffer into the other, a barrier
// between the stages -- in LDS where n = end - start <= kTrackLdsFrames (two buffers of three columns: 48 KiB), else in the call's scratch through
// the same code (a workgroup's own writes are visible to it behind __syncthreads).  Each output is a fixed-order sum or a selection of its own:
// no atomics, and nothing depends on which threads there are.  (e) the boxes, statuses and the range, with plain stores.  A window or a
// reflection indexes [0, n) of its own sequence alone, and a sequence's rows have the same bits whatever else is in the call.
//
// track_filter_kernel -- the hooks grnet_op_median1d / grnet_op_gauss1d: stage (c) or (d) alone on a caller's columns, global to global.
//
// seq_gauss_columns_kernel -- the Gaussian of the gait calls (gait, kinematics, contacts, regularity; sigma > 0 alone): a workgroup per (sequence,
// channel), thread per frame, the weights in LDS, track_gauss from the channel's column of the call's scratch into column col0 + channel of the
// call's per-frame rows, `cols` values wide.  Width and first column are arguments: one multiply beside a chain of up to 129 dependent additions.
#include "kernels.h"
#include "device.h"
#include "track_boxes.h"

namespace grk {
namespace {

__global__ __launch_bounds__(256) void track_frame_kernel(const double* __restrict__ joints, int K, int frames, double vis_thresh, double* __restrict__ params,
                                                          unsigned long long* __restrict__ words) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    bool detected = false;
    if (f < frames) {
        double p[3];
        detected = track_frame(joints + (size_t)f * K * 3, K, vis_thresh, p);
        if (detected) { params[(size_t)f * 3] = p[0]; params[(size_t)f * 3 + 1] = p[1]; params[(size_t)f * 3 + 2] = p[2]; }
    }
    const unsigned long long mask = __ballot(detected);        // every lane of the wave is here: frames past the end vote 0
    if ((threadIdx.x & 63) == 0) words[f >> 6] = mask;
}

// Stages (b) to (e) of one sequence on the buffers buf[0, 6n): called once with the LDS array and once with the call's scratch, so that in each
// inlined copy the compiler knows the address space (a pointer chosen at run time between the two is a flat pointer, and a flat load of LDS costs
// several times a ds_read: the first form of this kernel spent 87 of its 108 us there).
__device__ __forceinline__ void track_sequence_stages(double* buf, int tid, int f0, int T, int start, int end, int n, const double* w, int radius, int ksize,
                                                      int pad, const double* __restrict__ params, const unsigned long long* __restrict__ words,
                                                      double* __restrict__ boxes, int* __restrict__ status) {
    double* cur = buf;
    double* other = buf + 3 * (size_t)n;
    // (b)
    for (int i = tid; i < n; i += kTrackThreads) {
        const long long g = (long long)f0 + start + i;
        if ((words[g >> 6] >> (g & 63)) & 1) {
            for (int c = 0; c < 3; ++c) cur[(size_t)c * n + i] = params[g * 3 + c];
        } else {
            const long long p = track_prev(words, g), q = track_next(words, g);
            for (int c = 0; c < 3; ++c) cur[(size_t)c * n + i] = track_fill(params[p * 3 + c], params[q * 3 + c], (int)(q - p - 1), (int)(g - p));
        }
    }
    __syncthreads();
    // (c)
    if (ksize > 1) {
        for (int k = tid; k < 3 * n; k += kTrackThreads) other[k] = track_median(cur + (size_t)(k / n) * n, n, k % n, ksize, pad);
        __syncthreads();
        double* t = cur; cur = other; other = t;
    }
    // (d)
    if (radius >= 0) {
        for (int k = tid; k < 3 * n; k += kTrackThreads) other[k] = track_gauss(cur + (size_t)(k / n) * n, n, k % n, w, radius);
        __syncthreads();
        double* t = cur; cur = other; other = t;
    }
    // (e)
    for (int i = tid; i < T; i += kTrackThreads) {
        const long long g = (long long)f0 + i;
        double cx = 0., cy = 0., side = 0.;
        int st = kTrackOutside;
        if (i >= start && i < end) {
            const int k = i - start;
            const double s = cur[2 * (size_t)n + k];
            if (s > 0. && translation_detail::finite(s)) {
                cx = cur[k]; cy = cur[(size_t)n + k]; side = kTrackPersonPixels / s;
                st = ((words[g >> 6] >> (g & 63)) & 1) ? kTrackDetected : kTrackInterpolated;
            } else {
                st = kTrackBadScale;
            }
        }
        double* box = boxes + g * 4;
        box[0] = cx; box[1] = cy; box[2] = side; box[3] = side;
        status[g] = st;
    }
}

// radius < 0: no Gaussian; ksize 1: no median.  work: (frames, 6) float64 of the call, used by the sequences that do not fit the LDS.
__global__ __launch_bounds__(kTrackThreads) void track_seq_kernel(const int* __restrict__ off, const double* __restrict__ weights, int radius, int ksize, int pad,
                                                                  const double* __restrict__ params, const unsigned long long* __restrict__ words, double* work,
                                                                  double* __restrict__ boxes, int* __restrict__ status, int* __restrict__ range) {
    __shared__ double lds[6 * kTrackLdsFrames];
    __shared__ double w_lds[kTrackMaxRadius + 1];
    __shared__ int wave_first[kTrackThreads / 64], wave_last[kTrackThreads / 64];
    const int tid = threadIdx.x, f0 = off[blockIdx.x], f1 = off[blockIdx.x + 1], T = f1 - f0;
    if (tid <= radius) w_lds[tid] = weights[tid];              // radius <= 64 < the threads; read behind the barrier below
    // (a) thread t looks at words w0 + t, w0 + t + threads, ...
    int first = 0x7fffffff, last = -1;
    for (int w = (f0 >> 6) + tid; w <= (f1 - 1) >> 6; w += kTrackThreads) {
        const long long lo = max(f0, w * 64), hi = min(f1, w * 64 + 64);
        const long long a = track_first(words, lo, hi), b = track_last(words, lo, hi);
        if (a >= 0) first = min(first, (int)a);
        last = max(last, (int)b);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { first = min(first, __shfl_xor(first, o, 64)); last = max(last, __shfl_xor(last, o, 64)); }
    if ((tid & 63) == 0) { wave_first[tid >> 6] = first; wave_last[tid >> 6] = last; }
    __syncthreads();
    first = wave_first[0], last = wave_last[0];
#pragma unroll
    for (int k = 1; k < kTrackThreads / 64; ++k) { first = min(first, wave_first[k]); last = max(last, wave_last[k]); }
    const bool none = last < 0;
    const int start = none ? -1 : first - f0, end = none ? 0 : last + 1 - f0, n = none ? 0 : end - start;
    if (tid == 0) { range[2 * blockIdx.x] = start; range[2 * blockIdx.x + 1] = end; }
    if (n <= kTrackLdsFrames) track_sequence_stages(lds, tid, f0, T, start, end, n, w_lds, radius, ksize, pad, params, words, boxes, status);
    else track_sequence_stages(work + (size_t)f0 * 6, tid, f0, T, start, end, n, w_lds, radius, ksize, pad, params, words, boxes, status);
}

__global__ __launch_bounds__(256) void track_filter_kernel(const int* __restrict__ off, const double* __restrict__ x, const double* __restrict__ weights,
                                                           int radius, int ksize, int pad, double* __restrict__ out) {
    const int f0 = off[blockIdx.x], n = off[blockIdx.x + 1] - f0;
    for (int i = threadIdx.x; i < n; i += 256)
        out[(size_t)f0 + i] = radius >= 0 ? track_gauss(x + f0, n, i, weights, radius) : track_median(x + f0, n, i, ksize, pad);
}

__global__ __launch_bounds__(256) void seq_gauss_columns_kernel(const int* __restrict__ off, const double* __restrict__ weights, int radius, int frames,
                                                                const double* __restrict__ raw, double* __restrict__ out, int cols, int col0) {
    __shared__ double w_lds[kTrackMaxRadius + 1];
    const int f0 = off[blockIdx.x], T = off[blockIdx.x + 1] - f0, k = blockIdx.y;
    if ((int)threadIdx.x <= radius) w_lds[threadIdx.x] = weights[threadIdx.x];
    __syncthreads();
    const double* x = raw + (size_t)k * frames + f0;
    for (int i = threadIdx.x; i < T; i += 256) out[((size_t)f0 + i) * cols + col0 + k] = track_gauss(x, T, i, w_lds, radius);
}

}  // namespace

hipError_t launch_track_frames(const double* joints, int K, int frames, double vis_thresh, double* params, unsigned long long* words, hipStream_t s) {
    return launch_k(track_frame_kernel, dim3((frames + 255) / 256), dim3(256), 0, s, joints, K, frames, vis_thresh, params, words);
}

hipError_t launch_track_sequences(const int* off, int n_seq, const double* weights, int radius, int ksize, int pad, const double* params,
                                  const unsigned long long* words, double* work, double* boxes, int* status, int* range, hipStream_t s) {
    return launch_k(track_seq_kernel, dim3(n_seq), dim3(kTrackThreads), 0, s, off, weights, radius, ksize, pad, params, words, work, boxes, status, range);
}

hipError_t launch_track_filter(const int* off, int n_seq, const double* x, const double* weights, int radius, int ksize, int pad, double* out, hipStream_t s) {
    return launch_k(track_filter_kernel, dim3(n_seq), dim3(256), 0, s, off, x, weights, radius, ksize, pad, out);
}

hipError_t launch_seq_gauss_columns(const int* off, int n_seq, int channels, const double* weights, int radius, int frames, const double* raw, double* out,
                                    int cols, int col0, hipStream_t s) {
    return launch_k(seq_gauss_columns_kernel, dim3(n_seq, channels), dim3(256), 0, s, off, weights, radius, frames, raw, out, cols, col0);
}

}  // namespace grk
