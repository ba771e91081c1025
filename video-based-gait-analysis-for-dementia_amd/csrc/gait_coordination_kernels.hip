// Arm swing and inter-limb coordination on the device, for many sequences lying back to back (rules and columns: DESIGN 4.21; the arithmetic:
// gait_coordination.h, which the host checker runs too; the segments, the window, the twiddles and the density: gait_spectrum.h).
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  Every floating-point value is float64 and every operation rounds once.  A lane owns
// a bin and nothing is added across lanes, so no result depends on an order the hardware chooses, nor on the shape of the grid.
//
// coord_frames_kernel -- ONE LANE PER FRAME over all frames of the call, sequences ignored (coord_frame: two arctangents for the arms and two for the
// legs, kin_frame's operations for those four channels alone, so a third of its work).  The four angles go to the call's scratch, a column each,
// where a Gaussian follows (seq_gauss_columns_kernel), else straight into the per-frame rows.  This is the frame kernel chosen, not launch_kin_frames
// and a gather: that would compute thirteen channels, keep 13 columns of scratch and need one more launch.
//
// coord_csd_kernel -- the grid is (n_seq, ceil((N / 2 + 1) / 64)): ONE WAVE per (sequence, block of 64 bins), and A LANE OWNS A BIN FOR ALL FOUR
// CHANNELS AND ALL SIX PAIRS.  Every workgroup of a sequence makes the same tables for itself: (a) a lane per frame makes the four differenced values
// (coord_valid), 64 frames a round, and the round's ballot of "all four finite" IS the word of the call's one validity bitmask; the four columns of y
// go into LDS where the sequence has at most kCoordLdsFrames frames, else into this workgroup's own span of the call's scratch through the same code.
// A lane per entry makes the N twiddles and the L Hann values.  (b) one lane walks the runs of the bitmask by word (spec_runs) and lays the segment
// starts: into LDS where the sequence can hold at most kCoordLdsSegments of them, else into the scratch.  (c) a lane per (segment, channel) adds its
// mean serially in time order.  (d) the lane walks the segments in order and each segment's samples in rising i (coord_bin): the window, the four
// values of y and the four means are one address for the wave, a broadcast; THE TWIDDLE GATHER at (k i) mod N is lane-dependent and is the costly
// read -- the bank argument is gait_spectrum_kernels.hip's, unchanged: consecutive lanes are i doubles apart, an odd i is free of conflicts, an even
// i costs 2^v2(i) cycles for one, about 1 + log2(L) / 2 cycles a read on average.  It is paid ONCE for four channels and ten spectra (sixteen
// float64 multiply-adds of the sample behind two reads), where four gait_spectrum calls pay it four times.  The sixteen running sums and the eight
// sums of a segment stay in registers.  Every value is written with a plain vector store.  No atomics anywhere.
//
// Static LDS of coord_csd_kernel: y 4 x 1024 x 8 = 32 768, twiddles 2 x 1024 x 8 = 16 384, window 256 x 8 = 2 048, bitmask 512 x 8 = 4 096, starts
// 128 x 4 = 512, means 128 x 4 x 8 = 4 096, shared 8: 59 912 bytes, below the 64 KB of a static allocation.  A 400-frame video at the defaults (11
// segments) lies in LDS entirely.
//
// coord_row_kernel -- the grid is (n_seq, 10): a wave per (sequence, row) copies the finished rows it needs into LDS -- one row of auto for a limb,
// the pair's P_aa, P_bb and its (Re, Im) for a pair -- and one lane walks them in rising k (spec_row, coord_pair_row).  One wave for all ten rows of
// a sequence would need 16 rows of 513 doubles, 65 664 bytes, more than a static allocation holds; a wave per row holds 16 416.
//
// The hook grnet_op_gait_cross_welch launches the last two kernels on a caller's signals.
#include "kernels.h"
#include "device.h"
#include "gait_coordination.h"

namespace grk {
namespace {

__global__ __launch_bounds__(256) void coord_frames_kernel(const float* __restrict__ joints, int J, int frames, KinTable tab, double* __restrict__ raw,
                                                           double* __restrict__ per_frame) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= frames) return;
    double ang[kCoordChannels];
    coord_frame(joints + (size_t)f * J * 3, tab.j, ang);
    for (int k = 0; k < kCoordChannels; ++k) {
        if (raw) raw[(size_t)k * frames + f] = ang[k];
        else per_frame[(size_t)f * kCoordChannels + k] = ang[k];
    }
}

struct CoordTables {
    double* sn;
    double* cs;
    double* w;
    unsigned long long* mask;
    int* shared;                                               // [0]: the candidates
};

// Stages (a) to (d) of one (sequence, block of bins): called with the LDS arrays or with the workgroup's scratch for y and for the segments, as
// spec_psd_stages is.  y: four columns `stride` apart; x, ex: the sequence's rows and exclude entries; au, cr: the sequence's auto and cross rows
__device__ __forceinline__ void coord_csd_stages(double* y, size_t stride, int* start, double* mu, const CoordTables& tb, int tid, int T, const SpecRule& r,
                                                 const double* __restrict__ x, const int* __restrict__ ex, double* __restrict__ au, double* __restrict__ cr,
                                                 double* __restrict__ limb, double* __restrict__ pair) {
    const int L = r.segment, N = r.nfft, words = (T + 63) >> 6, bins = N / 2 + 1;
    long long n = 0;
    for (int w = 0; w < words; ++w) {
        const int t = w * 64 + tid;
        double v[kCoordChannels];
        const bool ok = t < T && coord_valid(x, ex, t, T, r.derivative, v);
        if (t < T)
            for (int c = 0; c < kCoordChannels; ++c) y[c * stride + t] = v[c];
        const unsigned long long word = __ballot(ok);
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
    for (int e = tid; e < used * kCoordChannels; e += kSpecThreads) mu[e] = spec_mean(y + (e & 3) * stride + start[e >> 2], L);
    __syncthreads();
    const int k = blockIdx.y * kSpecThreads + tid;
    if (k <= N / 2) {
        const double W2 = spec_window_power(tb.w, L);
        double acc[kCoordSums];
        coord_bin(y, stride, start, mu, used, tb.w, L, tb.sn, tb.cs, N, k, acc);
        for (int c = 0; c < kCoordChannels; ++c) au[(size_t)c * bins + k] = spec_density(acc[c], k, used, r, W2);
        for (int p = 0; p < kCoordPairs; ++p) {
            cr[((size_t)p * bins + k) * 2] = spec_density(acc[kCoordChannels + 2 * p], k, used, r, W2);
            cr[((size_t)p * bins + k) * 2 + 1] = spec_density(acc[kCoordChannels + 2 * p + 1], k, used, r, W2);
        }
    }
    if (blockIdx.y == 0 && tid < kCoordChannels) {
        limb[tid * kSpecSeqCols + kSpecColN] = (double)n;
        limb[tid * kSpecSeqCols + kSpecColCandidates] = (double)candidates;
        limb[tid * kSpecSeqCols + kSpecColUsed] = (double)used;
    }
    if (blockIdx.y == 0 && tid < kCoordPairs) pair[tid * kCoordPairCols + kCoordColUsed] = (double)used;
}

// rows: per_frame (frames,4), or the hook's signals; y_long (gridDim.y * 4 * frames) float64 where a sequence of the call has more than
// kCoordLdsFrames frames, else null; start_long (gridDim.y * frames) int32 and mu_long (gridDim.y * 4 * frames) float64 where a sequence can hold
// more than kCoordLdsSegments segments, else null; au (n_seq,4,N/2+1); cr (n_seq,6,N/2+1,2); limbs (n_seq,4,13) and pairs (n_seq,6,10), of which
// the first three columns and the first are written here
__global__ __launch_bounds__(kSpecThreads) void coord_csd_kernel(const int* __restrict__ off, SpecRule r, const double* __restrict__ rows, const int* __restrict__ exclude,
                                                                 int frames, double* y_long, int* start_long, double* mu_long, double* __restrict__ au,
                                                                 double* __restrict__ cr, double* __restrict__ limbs, double* __restrict__ pairs) {
    __shared__ double lds_y[kCoordChannels * kCoordLdsFrames];
    __shared__ double lds_sn[kSpecMaxNfft], lds_cs[kSpecMaxNfft], lds_w[kSpecMaxSegment], lds_mu[kCoordChannels * kCoordLdsSegments];
    __shared__ unsigned long long lds_mask[kEntMaxFrames / 64];
    __shared__ int lds_start[kCoordLdsSegments], lds_shared[2];
    const int q = blockIdx.x, f0 = off[q], T = off[q + 1] - f0, tid = threadIdx.x, bins = r.nfft / 2 + 1;
    const size_t span = (size_t)blockIdx.y * frames + f0;      // this workgroup's frames of the sequence: four values a frame in y_long and mu_long
    const double* x = rows + (size_t)f0 * kCoordChannels;
    const int* ex = exclude ? exclude + f0 : nullptr;
    double* a = au + (size_t)q * kCoordChannels * bins;
    double* c = cr + (size_t)q * kCoordPairs * bins * 2;
    double* limb = limbs + (size_t)q * kCoordChannels * kSpecSeqCols;
    double* pair = pairs + (size_t)q * kCoordPairs * kCoordPairCols;
    const CoordTables tb{lds_sn, lds_cs, lds_w, lds_mask, lds_shared};
    const bool y_fits = T <= kCoordLdsFrames, seg_fits = spec_run_segments(T, r.segment, r.hop) <= kCoordLdsSegments;
    double* y = y_fits ? lds_y : y_long + span * kCoordChannels;
    const size_t stride = y_fits ? (size_t)kCoordLdsFrames : (size_t)T;
    if (seg_fits) coord_csd_stages(y, stride, lds_start, lds_mu, tb, tid, T, r, x, ex, a, c, limb, pair);
    else coord_csd_stages(y, stride, start_long + span, mu_long + span * kCoordChannels, tb, tid, T, r, x, ex, a, c, limb, pair);      // at most T segments
}

__global__ __launch_bounds__(kSpecThreads) void coord_row_kernel(SpecRule r, const double* __restrict__ au, const double* __restrict__ cr, double* __restrict__ limbs,
                                                                 double* __restrict__ pairs) {
    __shared__ double P[4][kSpecMaxNfft / 2 + 1];
    const int q = blockIdx.x, e = blockIdx.y, tid = threadIdx.x, bins = r.nfft / 2 + 1;
    const double* a = au + (size_t)q * kCoordChannels * bins;
    double* limb = limbs + (size_t)q * kCoordChannels * kSpecSeqCols;
    if (e < kCoordChannels) {
        for (int k = tid; k < bins; k += kSpecThreads) P[0][k] = a[(size_t)e * bins + k];
        __syncthreads();
        if (tid != 0) return;
        double* row = limb + e * kSpecSeqCols;
        spec_row(P[0], r, true, (long long)row[kSpecColN], (int)row[kSpecColCandidates], (int)row[kSpecColUsed], row);
        return;
    }
    const int p = e - kCoordChannels;
    const double* c = cr + ((size_t)q * kCoordPairs + p) * bins * 2;
    for (int k = tid; k < bins; k += kSpecThreads) {
        P[0][k] = a[(size_t)coord_pair_a(p) * bins + k];
        P[1][k] = a[(size_t)coord_pair_b(p) * bins + k];
        P[2][k] = c[2 * k];
        P[3][k] = c[2 * k + 1];
    }
    __syncthreads();
    if (tid != 0) return;
    double* row = pairs + ((size_t)q * kCoordPairs + p) * kCoordPairCols;
    coord_pair_row(P[0], P[1], P[2], P[3], r, coord_antiphase(p), (int)row[kCoordColUsed], row);
}

}  // namespace

hipError_t launch_coord_frames(const float* joints, int J, int frames, const KinTable& tab, double* raw, double* per_frame, hipStream_t s) {
    return launch_k(coord_frames_kernel, dim3((frames + 255) / 256), dim3(256), 0, s, joints, J, frames, tab, raw, per_frame);
}

hipError_t launch_coord_sequences(const int* off, int n_seq, const SpecRule& rule, const double* rows, const int* exclude, int frames, double* y_long, int* start_long,
                                  double* mu_long, double* au, double* cr, double* limbs, double* pairs, hipStream_t s) {
    hipError_t e = launch_k(coord_csd_kernel, dim3(n_seq, spec_bin_blocks(rule.nfft)), dim3(kSpecThreads), 0, s, off, rule, rows, exclude, frames, y_long, start_long,
                            mu_long, au, cr, limbs, pairs);
    if (e != hipSuccess) return e;
    return launch_k(coord_row_kernel, dim3(n_seq, kCoordChannels + kCoordPairs), dim3(kSpecThreads), 0, s, rule, (const double*)au, (const double*)cr, limbs, pairs);
}

}  // namespace grk
