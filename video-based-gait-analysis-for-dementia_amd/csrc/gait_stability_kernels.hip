// Local dynamic stability of four body signals on the device, for many sequences lying back to back (rules and columns: DESIGN 4.18; the
// arithmetic: gait_stability.h, which the host checker runs too).
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  Every floating-point value is float64 and every operation rounds once; the
// neighbours and the exponents are integers, and nothing is added across lanes, so no result depends on an order the hardware chooses.
//
// The call's frame kernel is gait_regularity's (launch_reg_frames) and its Gaussian seq_gauss_columns_kernel; this file holds the two launches behind.
//
// stab_nn_kernel    -- the grid is (n_seq, 4, blocks): one workgroup of four waves per (sequence, channel, block of kGaitThreads reference points),
// the blocks sized by the call's LONGEST sequence; a workgroup whose block lies past its sequence's eligible points writes -1 to its frames and
// returns, one past its frames returns at once.  A LANE OWNS REFERENCE POINT i and keeps its dim values in registers (dim is a template parameter
// behind a switch).  The workgroup walks the sequence's candidates in tiles of kStabTile: a lane per frame makes y with ent_diff straight from the
// rows into an LDS tile of tile + span values, and behind a barrier every lane scans the tile's j in increasing order (stab_scan).  All lanes of a
// wave read the same j: every LDS read is a broadcast, free of bank conflicts.  A lane keeps (best D2, best j) under a strict <: scanning j upwards
// IS the tie rule, and there is no cross-lane reduction.  One int32 vector store per lane at the end.
//
// stab_curve_kernel -- the grid is (n_seq, 4): one workgroup per (sequence, channel).  A lane per frame makes y and copies nn into LDS where the
// sequence has at most kRegLdsFrames frames (32 KB + 16 KB); else y goes into the call's scratch through the same code and nn is read from the
// output.  Behind a barrier A LANE OWNS A k, horizon + 1 <= 64 lanes, one wave, and walks the references in order with the serial mantissa product
// (stab_walk): nn(i) is one address for the wave, the values consecutive across its lanes.  No atomics anywhere.  Every value is written with a
// plain vector store.
//
// The hook grnet_op_gait_divergence launches the two kernels on a caller's signals.
#include "kernels.h"
#include "device.h"
#include "gait_stability.h"

namespace grk {
namespace {

// x, ex: the channel's column and the exclude entries of the sequence; i: this lane's point, which may lie past the eligible ones
template <int DIM>
__device__ __forceinline__ int stab_nn_search(double* tile, const double* __restrict__ x, const int* __restrict__ ex, int T, const StabRule& r, const StabPoints& p,
                                              int i, int tid) {
    bool mine = i < p.E;
    double a[DIM];
    for (int c = 0; c < DIM; ++c) {
        a[c] = mine ? ent_diff(x, ex, i + c * r.lag, T, r.derivative) : gait_detail::nan();      // i + span < T where i < E
        mine = mine && translation_detail::finite(a[c]);
    }
    double best = 0.;
    int best_j = -1;
    for (int j0 = 0; j0 < p.E; j0 += kStabTile) {
        const int n = p.E - j0 < kStabTile ? p.E - j0 : kStabTile;
        for (int t = tid; t < n + p.span; t += kGaitThreads) tile[t] = ent_diff(x, ex, j0 + t, T, r.derivative);      // j0 + t < E + span <= T
        __syncthreads();
        if (mine) stab_scan<DIM>(a, tile, j0, n, i, r.theiler, r.lag, &best, &best_j);
        __syncthreads();
    }
    return best_j;
}

// rows: per_frame (frames,4), or the hook's signals; nn (frames,4)
__global__ __launch_bounds__(kGaitThreads) void stab_nn_kernel(const int* __restrict__ off, StabRule r, const double* __restrict__ rows, const int* __restrict__ exclude,
                                                               int* __restrict__ nn) {
    __shared__ double tile[kStabTile + kStabMaxSpan];
    const int q = blockIdx.x, ch = blockIdx.y, f0 = off[q], T = off[q + 1] - f0, tid = threadIdx.x, first = blockIdx.z * kGaitThreads, i = first + tid;
    if (first >= T) return;
    const StabPoints p = stab_points(T, r);
    int* out = nn + (size_t)f0 * kRegChannels + ch;
    if (first >= p.E) {
        if (i < T) out[(size_t)i * kRegChannels] = -1;
        return;
    }
    const double* x = rows + (size_t)f0 * kRegChannels + ch;
    const int* ex = exclude ? exclude + f0 : nullptr;
    int j;
    switch (r.dim) {
        case 2: j = stab_nn_search<2>(tile, x, ex, T, r, p, i, tid); break;
        case 3: j = stab_nn_search<3>(tile, x, ex, T, r, p, i, tid); break;
        case 4: j = stab_nn_search<4>(tile, x, ex, T, r, p, i, tid); break;
        case 5: j = stab_nn_search<5>(tile, x, ex, T, r, p, i, tid); break;
        case 6: j = stab_nn_search<6>(tile, x, ex, T, r, p, i, tid); break;
        case 7: j = stab_nn_search<7>(tile, x, ex, T, r, p, i, tid); break;
        default: j = stab_nn_search<8>(tile, x, ex, T, r, p, i, tid); break;
    }
    if (i < T) out[(size_t)i * kRegChannels] = j;
}

// One (sequence, channel): called once with the LDS arrays and once with the call's scratch and the output, as ent_count_stages is.  y: room for T
// values; nn_copy: room for T neighbours or null; nn_out: the channel's column of the sequence's rows of the output
__device__ __forceinline__ void stab_curve_stages(double* y, int* nn_copy, int tid, int T, const StabRule& r, const double* __restrict__ x, const int* __restrict__ ex,
                                                  const int* nn_out, long long* __restrict__ pairs, double* __restrict__ mant) {
    for (int t = tid; t < T; t += kGaitThreads) {
        y[t] = ent_diff(x, ex, t, T, r.derivative);
        if (nn_copy) nn_copy[t] = nn_out[(size_t)t * kRegChannels];
    }
    __syncthreads();
    if (tid > r.horizon) return;
    if (nn_copy) stab_walk_dim(y, nn_copy, 1, T, r, tid, pairs + (size_t)tid * kStabPairCols, mant + tid);
    else stab_walk_dim(y, nn_out, kRegChannels, T, r, tid, pairs + (size_t)tid * kStabPairCols, mant + tid);
}

// nn (frames,4), written by stab_nn_kernel; y_long: (4,frames) where a sequence of the call has more than kRegLdsFrames frames, else null;
// pairs (n_seq,4,horizon+1,2); mant (n_seq,4,horizon+1)
__global__ __launch_bounds__(kGaitThreads) void stab_curve_kernel(const int* __restrict__ off, StabRule r, const double* __restrict__ rows, const int* __restrict__ exclude,
                                                                  int frames, const int* nn, double* y_long, long long* __restrict__ pairs, double* __restrict__ mant) {
    __shared__ double lds_y[kRegLdsFrames];
    __shared__ int lds_nn[kRegLdsFrames];
    const int q = blockIdx.x, ch = blockIdx.y, f0 = off[q], T = off[q + 1] - f0, tid = threadIdx.x;
    const size_t at = ((size_t)q * kRegChannels + ch) * (r.horizon + 1);
    const double* x = rows + (size_t)f0 * kRegChannels + ch;
    const int* ex = exclude ? exclude + f0 : nullptr;
    const int* nn_out = nn + (size_t)f0 * kRegChannels + ch;
    if (T <= kRegLdsFrames) stab_curve_stages(lds_y, lds_nn, tid, T, r, x, ex, nn_out, pairs + at * kStabPairCols, mant + at);
    else stab_curve_stages(y_long + (size_t)ch * frames + f0, nullptr, tid, T, r, x, ex, nn_out, pairs + at * kStabPairCols, mant + at);
}

}  // namespace

hipError_t launch_stab_sequences(const int* off, int n_seq, int longest, const StabRule& rule, const double* rows, const int* exclude, int frames, int* nn,
                                 double* y_long, long long* pairs, double* mant, hipStream_t s) {
    const int blocks = (longest + kGaitThreads - 1) / kGaitThreads;
    hipError_t e = launch_k(stab_nn_kernel, dim3(n_seq, kRegChannels, blocks), dim3(kGaitThreads), 0, s, off, rule, rows, exclude, nn);
    if (e != hipSuccess) return e;
    return launch_k(stab_curve_kernel, dim3(n_seq, kRegChannels), dim3(kGaitThreads), 0, s, off, rule, rows, exclude, frames, (const int*)nn, y_long, pairs, mant);
}

}  // namespace grk
