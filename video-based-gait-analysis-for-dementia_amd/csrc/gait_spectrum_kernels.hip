// Welch power spectral density of four body signals on the device, for many sequences lying back to back (rules and columns: DESIGN 4.19; the
// arithmetic: gait_spectrum.h, which the host checker runs too).
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  Every floating-point value is float64 and every operation rounds once.  A lane owns
// a bin and nothing is added across lanes, so no result depends on an order the hardware chooses, nor on the shape of the grid.
//
// The call's frame kernel is gait_regularity's (launch_reg_frames) and its Gaussian seq_gauss_columns_kernel; this file holds the two launches behind.
//
// spec_psd_kernel -- the grid is (n_seq, 4, ceil((N / 2 + 1) / 64)): ONE WAVE per (sequence, channel, block of 64 bins), so that the 513 bins of one
// long sequence at N = 1024 are 36 workgroups and not 4.  Every workgroup of a (sequence, channel) makes the same tables for itself: (a) a lane per
// frame makes y with ent_diff, 64 frames a round, and the round's ballot IS the word of the validity bitmask; y goes into LDS where the sequence has at
// most kRegLdsFrames frames, else into this workgroup's own span of the call's scratch through the same code.  A lane per entry makes the N twiddles
// (har_twiddle(j, N)) and the L Hann values.  (b) one lane walks the runs of the bitmask by word (spec_runs) and lays the segment starts: into LDS
// where the sequence can hold at most kSpecLdsSegments of them (spec_run_segments of its length), else into the scratch.  (c) a lane per segment adds
// its mean serially in time order.  (d) A LANE OWNS BIN k and walks the segments in order and each segment's samples in rising i (spec_bin): y, the
// mean and the window are one address for the wave, a broadcast.  THE TWIDDLE GATHER at (k i) mod N is lane-dependent: consecutive lanes are i
// doubles apart, so within a half-wave of ds_read_b64 (64 banks of 4 bytes: 32 doubles a row) an odd i is free of conflicts and an even i costs
// 2^v2(i) cycles for one, less where (k i) mod N repeats and the lanes broadcast.  Over i = 0 .. L - 1 that is about 1 + log2(L) / 2 cycles per
// read on average (3 to 4 at L = 64), for two reads per sample beside six float64 operations per lane.  That count comes from the bank rule alone: no
// counter was read, and what sets the loop's time is not measured (DESIGN 4.19 says what is supposed).  It is accepted because a layout that
// removed the conflicts (a table per i) would not fit, and both of the longest calls stay under the sibling calls' time.  The loop keeps its own index j += k, one compare and subtract.
// Every value is written with a plain vector store.  No atomics anywhere.
//
// spec_row_kernel -- the grid is (n_seq, 4): the wave copies the finished row of psd into LDS and one lane walks it in rising k (spec_row), as
// stab_curve_kernel and ent_spread_kernel do work of this shape.
//
// The hook grnet_op_gait_welch launches the two kernels on a caller's signals.
#include "kernels.h"
#include "device.h"
#include "gait_spectrum.h"

namespace grk {
namespace {

struct SpecTables {
    double* sn;
    double* cs;
    double* w;
    unsigned long long* mask;
    int* shared;                                               // [0]: the candidates
};

// Stages (a) to (d) of one (sequence, channel, block of bins): called with the LDS arrays or with the workgroup's scratch for y and for the segments,
// as ent_count_stages is.  x, ex: the channel's column and the exclude entries of the sequence; psd: the (sequence, channel)'s row; row: its columns
__device__ __forceinline__ void spec_psd_stages(double* y, int* start, double* mu, const SpecTables& tb, int tid, int T, const SpecRule& r,
                                                const double* __restrict__ x, const int* __restrict__ ex, double* __restrict__ psd, double* __restrict__ row) {
    const int L = r.segment, N = r.nfft, words = (T + 63) >> 6;
    long long n = 0;
    for (int w = 0; w < words; ++w) {
        const int t = w * 64 + tid;
        const double v = t < T ? ent_diff(x, ex, t, T, r.derivative) : gait_detail::nan();
        if (t < T) y[t] = v;
        const unsigned long long word = __ballot(translation_detail::finite(v));
        if (tid == 0) tb.mask[w] = word;
        n += __builtin_popcountll(word);
    }
    for (int j = tid; j < N; j += kSpecThreads) har_twiddle(j, N, tb.sn + j, tb.cs + j);
    for (int i = tid; i < L; i += kSpecThreads) {
        double s, c;
        har_twiddle(i, L, &s, &c);
        tb.w[i] = spec_hann(c);
    }
    __syncthreads();
    if (tid == 0) tb.shared[0] = spec_runs(tb.mask, T, L, r.hop, [&](int s, int t0) { start[s] = t0; });
    __syncthreads();
    const int candidates = tb.shared[0], used = spec_used(candidates, r.min_segments);
    for (int s = tid; s < used; s += kSpecThreads) mu[s] = spec_mean(y + start[s], L);
    __syncthreads();
    const int k = blockIdx.z * kSpecThreads + tid;
    if (k <= N / 2) {
        const double W2 = spec_window_power(tb.w, L);
        psd[k] = spec_density(spec_bin(y, start, mu, used, tb.w, L, tb.sn, tb.cs, N, k), k, used, r, W2);
    }
    if (blockIdx.z == 0 && tid == 0) {
        row[kSpecColN] = (double)n;
        row[kSpecColCandidates] = (double)candidates;
        row[kSpecColUsed] = (double)used;
    }
}

// rows: per_frame (frames,4), or the hook's signals; y_long (gridDim.z * 4,frames) float64 where a sequence of the call has more than kRegLdsFrames
// frames, else null; start_long int32 and mu_long float64 of the same shape where a sequence can hold more than kSpecLdsSegments segments, else null;
// psd (n_seq,4,N/2+1); per_seq (n_seq,4,13), of which the first three columns are written here
__global__ __launch_bounds__(kSpecThreads) void spec_psd_kernel(const int* __restrict__ off, SpecRule r, const double* __restrict__ rows, const int* __restrict__ exclude,
                                                                int frames, double* y_long, int* start_long, double* mu_long, double* __restrict__ psd,
                                                                double* __restrict__ per_seq) {
    __shared__ double lds_y[kRegLdsFrames];
    __shared__ double lds_sn[kSpecMaxNfft], lds_cs[kSpecMaxNfft], lds_w[kSpecMaxSegment], lds_mu[kSpecLdsSegments];
    __shared__ unsigned long long lds_mask[kEntMaxFrames / 64];
    __shared__ int lds_start[kSpecLdsSegments], lds_shared[2];
    const int q = blockIdx.x, ch = blockIdx.y, f0 = off[q], T = off[q + 1] - f0, tid = threadIdx.x;
    const size_t at = (size_t)q * kRegChannels + ch, mine = ((size_t)blockIdx.z * kRegChannels + ch) * frames + f0;
    const double* x = rows + (size_t)f0 * kRegChannels + ch;
    const int* ex = exclude ? exclude + f0 : nullptr;
    double* out = psd + at * (r.nfft / 2 + 1);
    double* row = per_seq + at * kSpecSeqCols;
    const SpecTables tb{lds_sn, lds_cs, lds_w, lds_mask, lds_shared};
    const bool y_fits = T <= kRegLdsFrames, seg_fits = spec_run_segments(T, r.segment, r.hop) <= kSpecLdsSegments;
    if (y_fits && seg_fits) spec_psd_stages(lds_y, lds_start, lds_mu, tb, tid, T, r, x, ex, out, row);
    else if (y_fits) spec_psd_stages(lds_y, start_long + mine, mu_long + mine, tb, tid, T, r, x, ex, out, row);      // at most T segments: inside the sequence's span
    else if (seg_fits) spec_psd_stages(y_long + mine, lds_start, lds_mu, tb, tid, T, r, x, ex, out, row);
    else spec_psd_stages(y_long + mine, start_long + mine, mu_long + mine, tb, tid, T, r, x, ex, out, row);
}

__global__ __launch_bounds__(kSpecThreads) void spec_row_kernel(SpecRule r, const double* __restrict__ psd, double* __restrict__ per_seq) {
    __shared__ double P[kSpecMaxNfft / 2 + 1];
    const int ch = blockIdx.y, tid = threadIdx.x, bins = r.nfft / 2 + 1;
    const size_t at = (size_t)blockIdx.x * kRegChannels + ch;
    for (int k = tid; k < bins; k += kSpecThreads) P[k] = psd[at * bins + k];
    __syncthreads();
    if (tid != 0) return;
    double* row = per_seq + at * kSpecSeqCols;
    spec_row(P, r, reg_odd(ch), (long long)row[kSpecColN], (int)row[kSpecColCandidates], (int)row[kSpecColUsed], row);
}

}  // namespace

int spec_bin_blocks(int nfft) { return (nfft / 2 + 1 + kSpecThreads - 1) / kSpecThreads; }

hipError_t launch_spec_sequences(const int* off, int n_seq, const SpecRule& rule, const double* rows, const int* exclude, int frames, double* y_long, int* start_long,
                                 double* mu_long, double* psd, double* per_seq, hipStream_t s) {
    hipError_t e = launch_k(spec_psd_kernel, dim3(n_seq, kRegChannels, spec_bin_blocks(rule.nfft)), dim3(kSpecThreads), 0, s, off, rule, rows, exclude, frames, y_long,
                            start_long, mu_long, psd, per_seq);
    if (e != hipSuccess) return e;
    return launch_k(spec_row_kernel, dim3(n_seq, kRegChannels), dim3(kSpecThreads), 0, s, rule, (const double*)psd, per_seq);
}

}  // namespace grk
