// Gait regularity and symmetry from the autocorrelation of four body signals on the device, for many sequences lying back to back (rules and
// columns: DESIGN 4.15; the arithmetic: gait_regularity.h, which the host checker runs too; the Gaussian and the bitmask searches: track_boxes.h).
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  Everything is float64 and every operation rounds once.
//
// At most THREE launches (two without a Gaussian) behind one small upload (the sequences' offsets and the Gaussian weights), whatever the number
// of sequences or frames.
//
// reg_frame_kernel  -- ONE LANE PER FRAME over all frames of the call (the reasons of gait_frame_kernel): six joints, one cross product, three square
// roots, three dot products.  The four signals go to the call's scratch, one column each, where a Gaussian follows, else into the per-frame rows.
//
// sigma > 0 alone  -- seq_gauss_columns_kernel (track_kernels.hip) on the four columns: all of the rows, which are 4 wide.
//
// reg_seq_kernel    -- the grid is (n_seq, 4): one workgroup of four waves per (sequence, channel).  The signal and the run numbers of the sequence
// lie in LDS where it has at most kRegLdsFrames frames, else in the call's scratch, through the same code.  (a) a wave takes 64 consecutive frames,
// a lane a frame: the value goes to d[], __ballot of "the frame counts" IS a word of the validity mask.  (b) behind a barrier one lane adds the valid
// values in time order, word by word, and keeps the count of valid frames before every word.  (c) behind a barrier a lane per frame centres its
// value and makes its run number: the frame's index less the popcount of the mask below it.  (d) behind a barrier LANE m OWNS LAG m, 0 .. 255: every
// lane walks t in time order, so d[t] and key[t] are one address for the whole wave -- a broadcast -- and d[t + m], key[t + m] are consecutive
// across its lanes -- no bank conflict; both are loaded whether the pair counts or not and the addition is chosen, so no load waits for another.
// A lane's sum is its own, in time order: no sum depends on the launch, so a sequence has the same bits alone or among others.  A wave whose
// lags all lie beyond max_lag skips the walk.  Lane 0 shares lag 0's sum and count; behind a barrier every
// lane makes rho of its lag, into LDS and into acf.  (e) behind a barrier __ballot of rule 6's three tests ARE the words of three masks over the lags;
// behind a last barrier one lane makes the row: a first-set-bit search for the first peak, a walk over the set bits of a window for the other lag.
// No atomics anywhere.  Every value is written with a plain vector store.
//
// The hook grnet_op_gait_autocorr launches reg_seq_kernel alone on a caller's signals.
#include "kernels.h"
#include "device.h"
#include "gait_regularity.h"

namespace grk {
namespace {

__global__ __launch_bounds__(256) void reg_frame_kernel(const float* __restrict__ joints, int J, int frames, GaitTable tab, const double* __restrict__ trans,
                                                        double* __restrict__ raw, double* __restrict__ per_frame) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= frames) return;
    double sig[kRegChannels];
    reg_frame(joints + (size_t)f * J * 3, tab.j, trans ? trans + (size_t)f * 3 : nullptr, sig);
    for (int k = 0; k < kRegChannels; ++k) {
        if (raw) raw[(size_t)k * frames + f] = sig[k];
        else per_frame[(size_t)f * kRegChannels + k] = sig[k];
    }
}

struct RegShared { double mu, sum_0; long long n, N_0; };

// Stages (a) to (e) of one (sequence, channel): called once with the LDS arrays and once with the call's scratch, so that in each inlined copy the
// compiler knows the address space (gait_sequence_stages says why).  x: the channel's column of the sequence's rows, kRegChannels values apart.
__device__ __forceinline__ void reg_sequence_stages(double* d, int* key, unsigned long long* valid, long long* prefix, double* rho,
                                                    unsigned long long (*lags)[kRegLagWords], RegShared* shared, int tid, int T, const RegRule& r, bool odd,
                                                    const double* __restrict__ x, const int* __restrict__ exclude, double* __restrict__ acf,
                                                    double* __restrict__ out) {
    const int lane = tid & 63, wave = tid >> 6;
    // (a) whole chunks of 64 frames, so that every lane of the wave reaches the ballot
    for (int base = wave * 64; base < T; base += kGaitThreads) {
        const int t = base + lane;
        bool v = false;
        if (t < T) {
            const double xv = x[(size_t)t * kRegChannels];
            v = reg_valid(xv, exclude, t);
            d[t] = xv;
        }
        const unsigned long long b = __ballot(v);
        if (lane == 0) valid[base >> 6] = b;
    }
    __syncthreads();
    // (b)
    if (tid == 0) shared->mu = reg_mean(d, valid, T, prefix, &shared->n);
    __syncthreads();
    // (c)
    const double mu = shared->mu;
    for (int t = tid; t < T; t += kGaitThreads) {
        const int k = reg_key(valid, prefix, t);
        key[t] = k;
        if (k >= 0) d[t] = d[t] - mu;
    }
    __syncthreads();
    // (d) lane = lag
    const int m = tid;
    double sum = 0.;
    long long N = 0;
    if (m <= r.max_lag) sum = reg_lag(d, key, T, m, &N);
    if (tid == 0) { shared->sum_0 = sum; shared->N_0 = N; }
    __syncthreads();
    if (m <= r.max_lag) {
        const double v = reg_rho(sum, N, shared->sum_0, shared->N_0, r.min_pairs);
        rho[m] = v;
        acf[m] = v;
    }
    __syncthreads();
    // (e) the three masks over the lags, then the row
    const bool in = m <= r.max_lag;
    const unsigned long long b0 = __ballot(in && reg_first_peak(rho, r, m)), b1 = __ballot(in && reg_is_max(rho, r.max_lag, m)),
                             b2 = __ballot(in && reg_is_min(rho, r.max_lag, m));
    if (lane == 0) { lags[0][wave] = b0; lags[1][wave] = b1; lags[2][wave] = b2; }
    __syncthreads();
    if (tid == 0) reg_row(rho, lags[0], lags[1], lags[2], r, odd, shared->n, shared->sum_0, out);
}

// rows: per_frame (frames,4), or the hook's signals
__global__ __launch_bounds__(kGaitThreads) void reg_seq_kernel(const int* __restrict__ off, RegRule r, const double* __restrict__ rows, const int* __restrict__ exclude,
                                                               int frames, double* long_d, int* long_key, unsigned long long* words, size_t mask_words,
                                                               double* __restrict__ acf, double* __restrict__ per_seq) {
    __shared__ double lds_d[kRegLdsFrames];
    __shared__ int lds_key[kRegLdsFrames];
    __shared__ unsigned long long lds_valid[kRegLdsFrames / 64];
    __shared__ long long lds_prefix[kRegLdsFrames / 64];
    __shared__ double rho[kRegMaxLag + 1];
    __shared__ unsigned long long lags[3][kRegLagWords];
    __shared__ RegShared shared;
    const int q = blockIdx.x, ch = blockIdx.y, f0 = off[q], T = off[q + 1] - f0, tid = threadIdx.x;
    const double* x = rows + (size_t)f0 * kRegChannels + ch;
    const int* ex = exclude ? exclude + f0 : nullptr;
    double* a = acf + ((size_t)q * kRegChannels + ch) * (size_t)(r.max_lag + 1);
    double* out = per_seq + ((size_t)q * kRegChannels + ch) * kRegSeqCols;
    if (T <= kRegLdsFrames) {
        reg_sequence_stages(lds_d, lds_key, lds_valid, lds_prefix, rho, lags, &shared, tid, T, r, reg_odd(ch), x, ex, a, out);
    } else {                                                   // the host gave the scratch: a sequence of the call is longer than the LDS arrays
        const size_t at = (size_t)ch * frames + f0;
        unsigned long long* g = gait_mask_at(words + (size_t)ch * 2 * mask_words, f0, q);
        reg_sequence_stages(long_d + at, long_key + at, g, reinterpret_cast<long long*>(g + mask_words), rho, lags, &shared, tid, T, r, reg_odd(ch), x, ex, a, out);
    }
}

}  // namespace

hipError_t launch_reg_frames(const float* joints, int J, int frames, const GaitTable& tab, const double* trans, double* raw, double* per_frame, hipStream_t s) {
    return launch_k(reg_frame_kernel, dim3((frames + 255) / 256), dim3(256), 0, s, joints, J, frames, tab, trans, raw, per_frame);
}

hipError_t launch_reg_sequences(const int* off, int n_seq, const RegRule& rule, const double* rows, const int* exclude, int frames, double* long_d, int* long_key,
                                unsigned long long* words, size_t mask_words, double* acf, double* per_seq, hipStream_t s) {
    return launch_k(reg_seq_kernel, dim3(n_seq, kRegChannels), dim3(kGaitThreads), 0, s, off, rule, rows, exclude, frames, long_d, long_key, words, mask_words, acf,
                    per_seq);
}

}  // namespace grk
