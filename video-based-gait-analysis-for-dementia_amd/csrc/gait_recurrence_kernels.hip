// Recurrence quantification of four body signals on the device, for many sequences lying back to back (rules and columns: DESIGN 4.20; the
// arithmetic: gait_recurrence.h, which the host checker runs too).
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  Every floating-point value is float64 and every operation rounds once; everything
// that is added across lanes is an integer, so no result depends on an order the hardware chooses.
//
// The call's frame kernel is gait_regularity's (launch_reg_frames), its Gaussian seq_gauss_columns_kernel, and its differences and spread
// gait_entropy's ent_spread_kernel as it is (launch_ent_spread): y lies in the call's scratch, n, mu, SD and r beside it.  This file holds the two
// launches behind.
//
// rec_pairs_kernel -- the grid is (n_seq, 4, parts of the call's sequence with the most): one workgroup of four waves per (sequence, channel, part);
// one past its sequence's rec_parts returns at once.  The workgroup copies y into LDS where the sequence has at most kRegLdsFrames frames, else it
// reads the scratch through the same code.  A LANE OWNS A CIRCULAR OFFSET s = 1 + part 256 + lane + round (parts 256) and walks i = 0 .. M - 1 with
// partner (i + s) mod M (rec_offset_walk): diagonal s, and behind the wrap diagonal M - s, so every lane has the same M pairs.  The reference point's
// values are one address for the wave, a broadcast; the partner's are CONSECUTIVE DOUBLES across the lanes: 64 lanes read 128 consecutive dwords, which
// a ds_read_b64 serves in its passes of 32 dwords over the 64 banks without a conflict, whatever the lag (the lag moves all lanes alike).  A line that
// ends goes into the workgroup's LDS histogram of kRecBins unsigned 32-bit bins by an integer atomicAdd on LDS, a vector LDS instruction: a part walks
// at most 2^25 pairs, so no bin overflows, and integer addition commutes, so the order the hardware serves the lanes in cannot change a bit.  These
// are the only atomics of the gait kernels; there are NO GLOBAL ATOMICS AND NO FLOATING-POINT ATOMICS.  The lane's 64-bit sums (comparable, recurrent,
// long lines and their points) are added across the wave by __shfl_xor and across the waves through LDS, `longest` as a maximum.  Every workgroup
// writes its partial -- kRecBins bins and five sums, widened to int64 -- to its own span of the call's scratch with plain vector stores.
//
// rec_rows_kernel  -- the grid is (n_seq, 4): one workgroup per (sequence, channel), a lane per bin.  It adds the sequence's parts in part order,
// counts the valid points by a ballot, and writes hist, counts and per_seq (ent_spread's four columns and eps2).
//
// Where a sequence's parts begin in the scratch: at the sum of the part counts of the sequences in front of it (rec_part_base), which every
// workgroup adds up from the offsets by itself -- n_seq / 256 loads a lane.
//
// The hook grnet_op_gait_recurrence_counts launches ent_spread_kernel and the two kernels on a caller's signals.
#include "kernels.h"
#include "device.h"
#include "gait_recurrence.h"

namespace grk {
namespace {

static_assert(kRecPartOffsets == kGaitThreads, "a lane of the workgroup owns an offset of the round");
static_assert(kRecBins < kGaitThreads && kRecCountCols <= 64, "rec_rows_kernel: a lane per bin, and the counts in one wave");
// a part has at most ceil(16 384 / (16 * 256)) = 4 rounds of 256 offsets, each of at most 32 768 pairs: 2^25 pairs, and no more lines
static_assert((long long)kEntMaxFrames * ((kEntMaxFrames / 2 + kRecMaxParts * kRecPartOffsets - 1) / (kRecMaxParts * kRecPartOffsets)) * kRecPartOffsets <= (1LL << 25),
              "a bin of the LDS histogram cannot overflow");

struct RecLdsBins {
    unsigned* h;
    __device__ void add(int bin) { atomicAdd(h + bin, 1u); }      // ds_add_u32
};

// the parts of the sequences in front of q, the same in every lane; four: room for a value a wave.  k < q <= n_seq - 1, so off[k + 1] is in the table
__device__ __forceinline__ int rec_part_base(const int* __restrict__ off, int q, const RecRule& r, int tid, int* four) {
    int v = 0;
    for (int k = tid; k < q; k += kGaitThreads) v += rec_parts(rec_points(off[k + 1] - off[k], r));
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((tid & 63) == 0) four[tid >> 6] = v;
    __syncthreads();
    return ((four[0] + four[1]) + four[2]) + four[3];
}

// One (sequence, channel, part): called once with the LDS copy of y and once with the call's scratch, as ent_count_stages is.  hist: kRecBins zeroed
// bins behind a barrier; out: the workgroup's kRecPartCols values
__device__ __forceinline__ void rec_pairs_stages(const double* y, unsigned* hist, long long (*part)[kRecSumCols], int tid, int M, const RecRule& r, int p, int parts,
                                                 double eps2, bool on, long long* __restrict__ out) {
    RecSums c;
    RecLdsBins bins{hist};
    rec_lane_walk(y, M, r, p, parts, tid, eps2, on, &c, bins);
    long long v[kRecSumCols] = {c.comparable, c.recurrent, c.long_lines, c.long_points, (long long)c.longest};
    for (int k = 0; k < kRecSumCols; ++k) {
        long long x = v[k];
        for (int d = 32; d; d >>= 1) {
            const long long o = __shfl_xor(x, d, 64);
            x = k == kRecSumCols - 1 ? (o > x ? o : x) : x + o;
        }
        if ((tid & 63) == 0) part[tid >> 6][k] = x;
    }
    __syncthreads();                                            // the waves' sums, and every lane's lines in the histogram
    if (tid < kRecBins) out[tid] = (long long)hist[tid];
    if (tid < kRecSumCols - 1) out[kRecBins + tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    if (tid == kRecSumCols - 1) {
        long long m = part[0][tid];
        for (int w = 1; w < kGaitThreads / 64; ++w) m = part[w][tid] > m ? part[w][tid] : m;
        out[kRecBins + tid] = m;
    }
}

// y_all (4,frames) and spread (n_seq,4,4): ent_spread_kernel's; partials: (sum of the sequences' parts,4,kRecPartCols)
__global__ __launch_bounds__(kGaitThreads) void rec_pairs_kernel(const int* __restrict__ off, RecRule r, int frames, const double* __restrict__ y_all,
                                                                 const double* __restrict__ spread, long long* __restrict__ partials) {
    __shared__ double lds_y[kRegLdsFrames];
    __shared__ unsigned hist[kRecBins];
    __shared__ long long part[kGaitThreads / 64][kRecSumCols];
    __shared__ int four[kGaitThreads / 64];
    const int q = blockIdx.x, ch = blockIdx.y, p = blockIdx.z, f0 = off[q], T = off[q + 1] - f0, tid = threadIdx.x;
    const int M = rec_points(T, r), parts = rec_parts(M);
    if (p >= parts) return;
    const int base = rec_part_base(off, q, r, tid, four);
    const double rr = spread[((size_t)q * kRegChannels + ch) * kEntSeqCols + 3];
    const double eps2 = rec_eps2(rr, r.dim);
    const double* y = y_all + (size_t)ch * frames + f0;
    const bool fits = T <= kRegLdsFrames;
    if (fits)
        for (int t = tid; t < T; t += kGaitThreads) lds_y[t] = y[t];
    if (tid < kRecBins) hist[tid] = 0u;
    __syncthreads();
    long long* out = partials + ((size_t)(base + p) * kRegChannels + ch) * kRecPartCols;      // base + p < the sum of all parts: the host sized it so
    if (fits) rec_pairs_stages(lds_y, hist, part, tid, M, r, p, parts, eps2, rr > 0., out);    // two calls: in each inlined copy the address space is known
    else rec_pairs_stages(y, hist, part, tid, M, r, p, parts, eps2, rr > 0., out);
}

// per_seq (n_seq,4,5), hist (n_seq,4,kRecBins) int64, counts (n_seq,4,6) int64.  Every index is bounded without the data: a bin by tid < kRecBins, a
// part by p < rec_parts(M) behind the sequence's base, a point's values by i < M = T - span, so i + span < T
__global__ __launch_bounds__(kGaitThreads) void rec_rows_kernel(const int* __restrict__ off, RecRule r, int frames, const double* __restrict__ y_all,
                                                                const double* __restrict__ spread, const long long* __restrict__ partials,
                                                                double* __restrict__ per_seq, long long* __restrict__ hist, long long* __restrict__ counts) {
    __shared__ int four[kGaitThreads / 64];
    __shared__ int pts[kGaitThreads / 64];
    const int q = blockIdx.x, ch = blockIdx.y, f0 = off[q], T = off[q + 1] - f0, tid = threadIdx.x;
    const int M = rec_points(T, r), parts = rec_parts(M);
    const int base = rec_part_base(off, q, r, tid, four);
    const size_t at = (size_t)q * kRegChannels + ch;
    const long long* in = partials + ((size_t)base * kRegChannels + ch) * kRecPartCols;
    const size_t step = (size_t)kRegChannels * kRecPartCols;   // from a part to the next of the same channel
    if (tid < kRecBins) {
        long long v = 0;
        for (int p = 0; p < parts; ++p) v += in[p * step + tid];
        hist[at * kRecBins + tid] = v;
    }
    const double* y = y_all + (size_t)ch * frames + f0;
    int n = 0;
    for (int i0 = 0; i0 < M; i0 += kGaitThreads) {              // the same trips in every lane: the ballot is of whole waves
        const int i = i0 + tid;
        const bool ok = i < M && rec_point_valid(y, i, r.dim, r.lag);
        n += __popcll(__ballot(ok));
    }
    if ((tid & 63) == 0) pts[tid >> 6] = n;
    __syncthreads();
    long long* c = counts + at * kRecCountCols;
    if (tid == 0) c[0] = ((pts[0] + pts[1]) + pts[2]) + pts[3];
    if (tid >= 1 && tid < kRecCountCols) {
        const int k = kRecBins + tid - 1;
        long long v = in[k];
        for (int p = 1; p < parts; ++p) {
            const long long o = in[p * step + k];
            v = tid == kRecCountCols - 1 ? (o > v ? o : v) : v + o;
        }
        c[tid] = v;
    }
    if (tid < kEntSeqCols) per_seq[at * kRecSeqCols + tid] = spread[at * kEntSeqCols + tid];
    if (tid == kEntSeqCols) per_seq[at * kRecSeqCols + tid] = rec_eps2(spread[at * kEntSeqCols + 3], r.dim);
}

}  // namespace

hipError_t launch_rec_sequences(const int* off, int n_seq, int max_parts, const RecRule& rule, const double* rows, const int* exclude, int frames, double* y,
                                double* spread, long long* partials, double* per_seq, long long* hist, long long* counts, hipStream_t s) {
    hipError_t e = launch_ent_spread(off, n_seq, rule.derivative, rule.radius, rows, exclude, frames, y, spread, s);
    if (e != hipSuccess) return e;
    e = launch_k(rec_pairs_kernel, dim3(n_seq, kRegChannels, max_parts), dim3(kGaitThreads), 0, s, off, rule, frames, (const double*)y, (const double*)spread,
                 partials);
    if (e != hipSuccess) return e;
    return launch_k(rec_rows_kernel, dim3(n_seq, kRegChannels), dim3(kGaitThreads), 0, s, off, rule, frames, (const double*)y, (const double*)spread,
                    (const long long*)partials, per_seq, hist, counts);
}

}  // namespace grk
