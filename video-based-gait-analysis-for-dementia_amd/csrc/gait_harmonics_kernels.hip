// Harmonic ratios per stride of four body signals on the device, for many sequences lying back to back (rules and columns: DESIGN 4.16; the
// arithmetic: gait_harmonics.h, which the host checker runs too; the bitmask searches: track_boxes.h).
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  Everything is float64 and every operation rounds once.
//
// The call's frame kernel is gait_regularity's (launch_reg_frames) and its Gaussian seq_gauss_columns_kernel; this file holds the third launch.
//
// har_seq_kernel    -- the grid is (n_seq, 4): one workgroup of four waves per (sequence, channel).  (a) a wave takes 64 consecutive frames of the
// sequence's events, a lane a frame: __ballot of the left and of the right heel strike IS one word of that foot's bitmask, in LDS where the sequence
// has at most 64 * kGaitLdsWords frames, else in the call's scratch (gait_mask_at).  (b) behind one barrier EVERY thread walks the two masks by word
// (har_walk): the walk is the same in all of them, so every thread knows every candidate's number and, of those whose length is allowed, the slot.
// WAVE c mod 4 TAKES CANDIDATE c.  In its own 6 KB of LDS it builds y and the two twiddle tables, a lane per frame (the tables are kept while the
// next stride of the wave has the same length), then walks i in time order with LANE = (HARMONIC, COSINE | SINE): y(i) is one address for the wave,
// the table read a gather.  One __shfl_xor brings sine to cosine for the amplitude; the wave then reads the amplitudes in rising k by __shfl, so every
// lane holds rule 7's four sums, and lane 0 writes the stride's row and the slot's tail, the even lanes the slot's amplitudes.  A slot -- the
// amplitudes, HR, iHR, H, the signed length -- lies in the call's scratch at a place that depends on the sequence alone (har_slot_at), so no sum
// depends on the launch and a sequence has the same bits alone or among others.  A stride has at most 256 frames whatever the sequence's length.
// (c) behind a barrier the slots' tails go to LDS, a thread a value, where the sequence has at most 256 slots (the waves' y arrays, which nobody reads
// any more); behind another thread 0 makes the row of per_seq from them in order -- fourteen passes, which took 21 us longer at 400 frames while they
// read the scratch -- threads 64 .. 64 + n_harmonics a harmonic's spectrum entry each, and all fill the rows behind the last stored stride with NaN.
// No atomics anywhere.  Every value is written with a plain vector store.
//
// The hook grnet_op_gait_stride_dft launches har_seq_kernel alone on a caller's signals.
#include "kernels.h"
#include "device.h"
#include "gait_harmonics.h"

namespace grk {
namespace {

constexpr int kHarTable = kHarMaxStride + 1;
constexpr int kHarLdsTails = 4 * kHarTable / kHarSlotTail;     // slots whose tails fit the four waves' y arrays: 256

// what a wave wrote to its LDS, every lane of it may read afterwards, and the other way round
__device__ __forceinline__ void har_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Stages (a) to (c) of one (sequence, channel) on the two heel-strike bitmasks m_l, m_r[0, ceil(T / 64)): called once with the LDS arrays and once with
// the call's scratch, so that in each inlined copy the compiler knows the address space (gait_sequence_stages says why).  x: the channel's column of
// the sequence's rows, kRegChannels values apart; slots: har_slot_room(T) of them; rows: (max_strides, 6); spectrum: (n_harmonics, 2)
__device__ __forceinline__ void har_sequence_stages(unsigned long long* m_l, unsigned long long* m_r, double (*y)[kHarTable], double (*sn)[kHarTable],
                                                    double (*cs)[kHarTable], int tid, int T, const HarRule& r, bool odd, const int* __restrict__ events,
                                                    const double* __restrict__ x, const int* __restrict__ exclude, double* slots, double* __restrict__ rows,
                                                    double* __restrict__ spectrum, double* __restrict__ out) {
    const int lane = tid & 63, wave = tid >> 6, n_h = r.n_harmonics, width = n_h + kHarSlotTail, room = har_slot_room(T);
    const double none = gait_detail::nan();
    // (a) whole chunks of 64 frames, so that every lane of the wave reaches the ballots
    for (int base = wave * 64; base < T; base += kGaitThreads) {
        const int t = base + lane;
        const int ev = t < T ? events[t] : 0;
        const unsigned long long b0 = __ballot(ev & kGaitHeelL), b1 = __ballot(ev & kGaitHeelR);
        if (lane == 0) { m_l[base >> 6] = b0; m_r[base >> 6] = b1; }
    }
    __syncthreads();
    // (b) the same walk in every thread; a wave works on its own candidates
    double* my_y = y[wave];
    double* my_sn = sn[wave];
    double* my_cs = cs[wave];
    const int k = (lane >> 1) + 1;                             // the lane's harmonic; the even lane has the cosine, the odd one the sine
    const double* my_tab = (lane & 1) ? my_sn : my_cs;
    int eligible = 0, table_L = 0;
    const long long candidates = har_walk(m_l, m_r, T, [&](long long c, int foot, int t0, int t1) {
        const int L = t1 - t0;
        const bool allowed = L >= r.min_stride && L <= r.max_stride && L >= kHarMinStrideLimit && L <= kHarMaxStride;
        const int slot = allowed ? eligible++ : -1;
        if ((int)(c & 3) != wave) return;
        int H = 0;
        double HR = none, iHR = none, a = none;
        if (allowed) {
            const double x0 = x[(size_t)t0 * kRegChannels], x1 = x[(size_t)t1 * kRegChannels];
            har_wave_sync();                                   // the wave's last stride has been read
            bool bad = false;
            for (int base = 0; base <= L; base += 64) {
                const int i = base + lane;
                if (i <= L) {                                  // t0 + i <= t1 < T
                    const double xi = x[(size_t)(t0 + i) * kRegChannels];
                    bad = bad || !reg_valid(xi, exclude, t0 + i);
                    if (i < L) {
                        my_y[i] = har_detrend(xi, x0, x1, i, L);
                        if (L != table_L) har_twiddle(i, L, my_sn + i, my_cs + i);
                    }
                }
            }
            table_L = L;
            har_wave_sync();
            if (__ballot(bad) == 0ull) {
                H = har_harmonics(n_h, L);
                double acc = 0.;
                if (k <= H)
                    for (int i = 0, j = 0; i < L; ++i) {
                        acc = acc + my_y[i] * my_tab[j];
                        j += k;
                        if (j >= L) j -= L;
                    }
                const double other = __shfl_xor(acc, 1, 64);
                a = (lane & 1) ? har_amplitude(other, acc, L) : har_amplitude(acc, other, L);
                HarSums sums;
                for (int h = 1; h <= H; ++h) har_add(sums, h, __shfl(a, 2 * (h - 1), 64), r.derivative);
                if (!har_ratio(sums, odd, &HR, &iHR)) { H = 0; HR = iHR = none; }
            }
            if (slot < room) {
                double* s = slots + (size_t)slot * width;
                if (!(lane & 1) && k <= n_h) s[k - 1] = k <= H ? a : none;
                if (lane == 0) har_slot_tail(s, n_h, HR, iHR, H, foot, L);
            }
        }
        if (lane == 0 && c < r.max_strides) {
            double* row = rows + (size_t)c * kHarStrideCols;
            row[0] = (double)t0; row[1] = (double)t1; row[2] = foot ? -1. : 1.; row[3] = (double)H; row[4] = HR; row[5] = iHR;
        }
    });
    __syncthreads();
    // (c) the row's passes over the slots' tails read LDS where the tails fit the waves' y arrays, which nobody reads any more: a thread a value
    const long long n_slots = eligible < room ? eligible : room;
    double* tails = &y[0][0];
    const bool tails_fit = n_slots <= kHarLdsTails;
    if (tails_fit)
        for (int e = tid; e < (int)n_slots * kHarSlotTail; e += kGaitThreads) tails[e] = slots[(size_t)(e / kHarSlotTail) * width + n_h + e % kHarSlotTail];
    __syncthreads();
    if (tid == 0) {
        if (tails_fit) har_summary(tails, n_slots, 0, candidates, r.fps, out);      // a slot without amplitudes is its tail
        else har_summary(slots, n_slots, n_h, candidates, r.fps, out);
    }
    if (tid >= 64 && tid < 64 + n_h) har_spectrum(slots, n_slots, n_h, tid - 63, spectrum + (size_t)(tid - 64) * 2);
    const long long stored = candidates < r.max_strides ? candidates : r.max_strides;
    for (long long e = stored * kHarStrideCols + tid; e < (long long)r.max_strides * kHarStrideCols; e += kGaitThreads) rows[e] = none;
}

// rows: per_frame (frames,4), or the hook's signals
__global__ __launch_bounds__(kGaitThreads) void har_seq_kernel(const int* __restrict__ off, HarRule r, const double* __restrict__ rows, const int* __restrict__ events,
                                                               const int* __restrict__ exclude, int frames, int n_seq, unsigned long long* words, size_t mask_words,
                                                               double* slots, double* __restrict__ strides, double* __restrict__ spectrum,
                                                               double* __restrict__ per_seq) {
    __shared__ unsigned long long lds_l[kGaitLdsWords], lds_r[kGaitLdsWords];
    __shared__ double y[4][kHarTable], sn[4][kHarTable], cs[4][kHarTable];
    const int q = blockIdx.x, ch = blockIdx.y, f0 = off[q], T = off[q + 1] - f0, tid = threadIdx.x;
    const double* x = rows + (size_t)f0 * kRegChannels + ch;
    const int* ex = exclude ? exclude + f0 : nullptr;
    const size_t at = (size_t)q * kRegChannels + ch;
    double* sl = slots + ((size_t)ch * har_slots(frames, n_seq) + har_slot_at(f0, q)) * (size_t)(r.n_harmonics + kHarSlotTail);
    double* st = strides + at * (size_t)r.max_strides * kHarStrideCols;
    double* sp = spectrum + at * (size_t)r.n_harmonics * 2;
    double* out = per_seq + at * kHarSeqCols;
    if (T <= 64 * kGaitLdsWords) {
        har_sequence_stages(lds_l, lds_r, y, sn, cs, tid, T, r, reg_odd(ch), events + f0, x, ex, sl, st, sp, out);
    } else {                                                   // the host gave the scratch: a sequence of the call is longer than the LDS masks
        unsigned long long* g = gait_mask_at(words + (size_t)ch * 2 * mask_words, f0, q);
        har_sequence_stages(g, g + mask_words, y, sn, cs, tid, T, r, reg_odd(ch), events + f0, x, ex, sl, st, sp, out);
    }
}

}  // namespace

hipError_t launch_har_sequences(const int* off, int n_seq, const HarRule& rule, const double* rows, const int* events, const int* exclude, int frames,
                                unsigned long long* words, size_t mask_words, double* slots, double* strides, double* spectrum, double* per_seq, hipStream_t s) {
    return launch_k(har_seq_kernel, dim3(n_seq, kRegChannels), dim3(kGaitThreads), 0, s, off, rule, rows, events, exclude, frames, n_seq, words, mask_words, slots,
                    strides, spectrum, per_seq);
}

}  // namespace grk
