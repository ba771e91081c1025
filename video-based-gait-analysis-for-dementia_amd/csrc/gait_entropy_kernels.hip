// Sample entropy of four body signals at several scales on the device, for many sequences lying back to back (rules and columns: DESIGN 4.17; the
// arithmetic: gait_entropy.h, which the host checker runs too).
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  Every floating-point value is float64 and every operation rounds once; the counts
// are 64-bit integers, so no result depends on the order in which the lanes' counts are added.
//
// The call's frame kernel is gait_regularity's (launch_reg_frames) and its Gaussian seq_gauss_columns_kernel; this file holds the two launches behind.
//
// ent_spread_kernel -- the grid is (n_seq, 4): one workgroup of four waves per (sequence, channel).  A lane per frame makes y, the signal differenced
// `derivative` times, NaN where a frame it reads does not count: into the call's scratch, where the counting kernel reads it, and into LDS where the
// sequence has at most kRegLdsFrames frames.  Behind a barrier one lane walks y twice in time order -- the mean, then the squares -- from LDS, or
// from the scratch of a longer sequence through the same code, and writes n, mu, SD and r.
//
// ent_count_kernel  -- the grid is (n_seq, 4, scales): one workgroup per (sequence, channel, scale tau).  (a) a lane per j makes z_tau(j) from tau
// frames of y, into LDS where N = T / tau <= kRegLdsFrames, else into the call's scratch through the same code.  (b) behind a barrier A LANE OWNS
// TEMPLATE i, strided by the workgroup, and keeps its m + 1 values in registers.  Its partners are i + s modulo the N - m templates, s = 1 .. about
// half of them (ent_partners): every pair of the sequence is met once and no lane has more than one partner more than another, where the plain
// triangle j > i gives the first lane all and the last none.  s is one value for the wave, so the partners' values are consecutive doubles across its
// lanes -- no bank conflict -- and slide through registers: one LDS load a pair.  A template with an invalid value is skipped by its owner and fails
// as a partner by the comparisons themselves (a NaN matches nothing).  (c) the three counts of a lane -- valid templates, B, A -- are added across
// the wave by __shfl_xor, across the waves through LDS, and one lane each writes them.  No atomics anywhere.  Every value is written with a plain
// vector store.
//
// The hook grnet_op_gait_sampen launches the two kernels on a caller's signals.
#include "kernels.h"
#include "device.h"
#include "gait_entropy.h"

namespace grk {
namespace {

// rows: per_frame (frames,4), or the hook's signals; y_all: (4,frames)
__global__ __launch_bounds__(kGaitThreads) void ent_spread_kernel(const int* __restrict__ off, EntRule r, const double* __restrict__ rows,
                                                                  const int* __restrict__ exclude, int frames, double* y_all, double* __restrict__ per_seq) {
    __shared__ double lds_y[kRegLdsFrames];
    const int q = blockIdx.x, ch = blockIdx.y, f0 = off[q], T = off[q + 1] - f0, tid = threadIdx.x;
    const double* x = rows + (size_t)f0 * kRegChannels + ch;
    const int* ex = exclude ? exclude + f0 : nullptr;
    double* y = y_all + (size_t)ch * frames + f0;
    const bool fits = T <= kRegLdsFrames;
    for (int t = tid; t < T; t += kGaitThreads) {
        const double v = ent_diff(x, ex, t, T, r.derivative);
        y[t] = v;
        if (fits) lds_y[t] = v;
    }
    __syncthreads();
    if (tid != 0) return;
    double* out = per_seq + ((size_t)q * kRegChannels + ch) * kEntSeqCols;
    if (fits) ent_spread(lds_y, T, r.fraction, out);           // two calls, so that in each inlined copy the compiler knows the address space
    else ent_spread(y, T, r.fraction, out);
}

// Stages (a) to (c) of one (sequence, channel, scale): called once with the LDS array and once with the call's scratch, as reg_sequence_stages is.
// y: the sequence's differenced signal; z: room for N values; counts: the three of this workgroup
__device__ __forceinline__ void ent_count_stages(double* z, long long (*part)[kEntCountCols], int tid, int N, int tau, int m, double r,
                                                 const double* __restrict__ y, long long* __restrict__ counts) {
    for (int j = tid; j < N; j += kGaitThreads) z[j] = ent_coarse(y, j, tau);
    __syncthreads();
    const int Nt = N - m;
    long long c[kEntCountCols] = {0, 0, 0};
    for (int i = tid; i < Nt; i += kGaitThreads) {
        if (!ent_template_valid(z, i, m)) continue;
        ++c[0];
        if (r > 0.) ent_partners_m(m, z, Nt, i, r, &c[1], &c[2]);
    }
    for (int k = 0; k < kEntCountCols; ++k) {
        long long v = c[k];
        for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
        if ((tid & 63) == 0) part[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < kEntCountCols) counts[tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
}

// y_all: (4,frames); z_long: (4 * scales,frames) where a sequence of the call has more than kRegLdsFrames frames, else null; counts (n_seq,4,scales,3)
__global__ __launch_bounds__(kGaitThreads) void ent_count_kernel(const int* __restrict__ off, EntRule r, int frames, const double* __restrict__ y_all, double* z_long,
                                                                 const double* __restrict__ per_seq, long long* __restrict__ counts) {
    __shared__ double lds_z[kRegLdsFrames];
    __shared__ long long part[kGaitThreads / 64][kEntCountCols];
    const int q = blockIdx.x, ch = blockIdx.y, tau = blockIdx.z + 1, f0 = off[q], T = off[q + 1] - f0, tid = threadIdx.x, N = T / tau;
    const size_t at = (size_t)q * kRegChannels + ch;
    const double rr = per_seq[at * kEntSeqCols + 3];           // the scale-1 r at every scale
    const double* y = y_all + (size_t)ch * frames + f0;
    long long* out = counts + (at * r.scales + blockIdx.z) * kEntCountCols;
    if (N <= kRegLdsFrames) ent_count_stages(lds_z, part, tid, N, tau, r.m, rr, y, out);
    else ent_count_stages(z_long + ((size_t)ch * r.scales + blockIdx.z) * frames + f0, part, tid, N, tau, r.m, rr, y, out);      // N <= T: inside the sequence's span
}

}  // namespace

hipError_t launch_ent_spread(const int* off, int n_seq, int derivative, double fraction, const double* rows, const int* exclude, int frames, double* y,
                             double* per_seq, hipStream_t s) {
    const EntRule rule{1, fraction, derivative, 1};             // the kernel reads the derivative and the fraction alone
    return launch_k(ent_spread_kernel, dim3(n_seq, kRegChannels), dim3(kGaitThreads), 0, s, off, rule, rows, exclude, frames, y, per_seq);
}

hipError_t launch_ent_sequences(const int* off, int n_seq, const EntRule& rule, const double* rows, const int* exclude, int frames, double* y, double* z_long,
                                long long* counts, double* per_seq, hipStream_t s) {
    hipError_t e = launch_k(ent_spread_kernel, dim3(n_seq, kRegChannels), dim3(kGaitThreads), 0, s, off, rule, rows, exclude, frames, y, per_seq);
    if (e != hipSuccess) return e;
    return launch_k(ent_count_kernel, dim3(n_seq, kRegChannels, rule.scales), dim3(kGaitThreads), 0, s, off, rule, frames, (const double*)y, z_long,
                    (const double*)per_seq, counts);
}

}  // namespace grk
