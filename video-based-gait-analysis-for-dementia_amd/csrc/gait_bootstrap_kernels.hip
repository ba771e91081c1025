// The gait call's per-step and per-stride tables, and bootstrap intervals of a per-step table, on the device (rules and columns: DESIGN 4.23; the
// arithmetic and the generator: gait_bootstrap.h, which the host checker runs too).
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  Everything is float64 and every operation rounds once; the generator is uint64.
//
// step_tables_kernel -- one workgroup of four waves per sequence.  (a) a wave takes 64 consecutive frames: __ballot of the two heel-strike bits
// and (where a phase is given and straight_only) of phase != 0 ARE words of three masks, aligned to the sequence, in LDS where the sequence has at
// most 64 * kGaitLdsWords frames, else in the call's scratch (gait_mask_at of each of the three masks there).  (b) behind one barrier lane 0 of
// wave 0 walks the steps and lane 0 of wave 1 the strides (boot_step_rows, boot_stride_rows: the walks gait_seq_kernel makes, with the rows written
// down) and each writes its count.  (c) behind a barrier every lane writes NaN into the rows past the counts.  No atomics.
//
// bootstrap_kernel   -- ONE launch whatever n_seq: a workgroup of kBootThreads = 1024 lanes per (sequence, column, statistic).  (a) the column's
// n <= 1024 samples into LDS (8 KB).  (b) LANES RUN OVER REPLICATES: lane i takes the replicates i, i + 1024, ... of 0 .. B (at most kBootRounds =
// 5) and keeps its statistic of each IN REGISTERS; each is boot_statistics, a serial pass over the n samples in the order p = 0 .. n - 1 and a
// second one that makes the same draws again, so no index is stored and no float sum crosses a lane.  The three workgroups of a column make the same
// replicates, each for its own statistic: the passes are short beside the selection, and a call of few sequences ends three times sooner.  (c) the
// B values of the replicates 1 .. B into ONE LDS array of 4096 doubles (32 KB; with the samples 40 KB and a few counters.  A workgroup is 16 waves and
// a CU holds 32, so TWO workgroups fit a CU, and 80 KB of its 160 KB of LDS hold them -- all three statistics in one workgroup's LDS would be 96 KB
// and one workgroup a CU; the call's scratch would be 96 KB a column of
// memory traffic for values a lane already has); f by __ballot and popc per wave and a sum of the sixteen wave counts in LDS; then SELECTION BY
// COUNTING RANKS: a lane counts the values in front of each of its own (boot_before: value under <, then replicate number; every lane reads the
// same v[j], a broadcast), and the lane whose rank a quantile names writes its value.  The ranks of the f values are a permutation of 0 .. f - 1, so
// exactly one lane writes each quantile: no atomics.  Counting is B^2 comparisons a statistic (a sort on (value, number) would be B log^2 B and
// name the same bits; it is the next step if calls of thousands of sequences matter).  Replicate 0 is lane 0's first.  Every value is written with
// a plain vector store.
#include "kernels.h"
#include "device.h"
#include "gait_bootstrap.h"

namespace grk {
namespace {

__device__ __forceinline__ void step_tables_stages(unsigned long long* m0, unsigned long long* m1, unsigned long long* m2, bool masked, int tid, int T,
                                                   const int* __restrict__ events, const int* __restrict__ phase, const double* __restrict__ rows, double fps,
                                                   int max_rows, int* found, double* __restrict__ steps, double* __restrict__ strides, int* __restrict__ counts) {
    // (a) whole chunks of 64 frames, so that every lane of the wave reaches the ballots
    for (int base = (tid >> 6) * 64; base < T; base += kGaitThreads) {
        const int t = base + (tid & 63);
        const int ev = t < T ? events[t] : 0;
        const int busy = masked && t < T ? phase[t] != kTurnStraight : 0;
        const unsigned long long b0 = __ballot(ev & kGaitHeelL), b1 = __ballot(ev & kGaitHeelR), b2 = __ballot(busy);
        if ((tid & 63) == 0) { m0[base >> 6] = b0; m1[base >> 6] = b1; m2[base >> 6] = b2; }
    }
    __syncthreads();
    // (b)
    const unsigned long long* ns = masked ? m2 : nullptr;
    if (tid == 0 || tid == 64) {
        const long long n = tid == 0 ? boot_step_rows(m0, m1, ns, T, rows, fps, max_rows, steps) : boot_stride_rows(m0, m1, ns, T, fps, max_rows, strides);
        found[tid >> 6] = (int)n;
        counts[tid >> 6] = (int)n;
    }
    __syncthreads();
    // (c)
    const int n_steps = found[0], n_strides = found[1];
    for (int i = tid; i < max_rows * kBootStepCols; i += kGaitThreads)
        if (i / kBootStepCols >= n_steps) steps[i] = gait_detail::nan();
    for (int i = tid; i < max_rows * kBootStrideCols; i += kGaitThreads)
        if (i / kBootStrideCols >= n_strides) strides[i] = gait_detail::nan();
}

__global__ __launch_bounds__(kGaitThreads) void step_tables_kernel(const int* __restrict__ off, const int* __restrict__ events, const int* __restrict__ phase,
                                                                   const double* __restrict__ per_frame, double fps, int max_rows, unsigned long long* words,
                                                                   size_t mask_words, double* __restrict__ steps, double* __restrict__ strides,
                                                                   int* __restrict__ counts) {
    __shared__ unsigned long long lds[kStepMaskSets][kGaitLdsWords];
    __shared__ int found[2];
    const int q = blockIdx.x, f0 = off[q], T = off[q + 1] - f0, tid = threadIdx.x;
    const double* rows = per_frame + (size_t)f0 * kGaitFrameCols;
    const int* ph = phase ? phase + f0 : nullptr;
    double* st = steps + (size_t)q * max_rows * kBootStepCols;
    double* sr = strides + (size_t)q * max_rows * kBootStrideCols;
    if (((T - 1) >> 6) < kGaitLdsWords) {
        step_tables_stages(lds[0], lds[1], lds[2], phase != nullptr, tid, T, events + f0, ph, rows, fps, max_rows, found, st, sr, counts + 2 * q);
    } else {
        unsigned long long* g = gait_mask_at(words, f0, q);
        step_tables_stages(g, g + mask_words, g + 2 * mask_words, phase != nullptr, tid, T, events + f0, ph, rows, fps, max_rows, found, st, sr, counts + 2 * q);
    }
}

// rank[k] += the values of v[0, B) in front of the lane's value a[k] of replicate number tid + k * kBootThreads, for the R rounds a call of this B has:
// R is a template argument so that a call of B = 2 000 does the work of two rounds, not of five
template <int R>
__device__ __forceinline__ void boot_count_ranks(const double* v, int B, const double (&a)[kBootRounds], int tid, int (&rank)[kBootRounds]) {
    for (int j = 0; j < B; ++j) {
        const double b = v[j];
#pragma unroll
        for (int k = 0; k < R; ++k) rank[k] += boot_before(b, j, a[k], tid + k * kBootThreads - 1);
    }
}

__global__ __launch_bounds__(kBootThreads) void bootstrap_kernel(const double* __restrict__ table, const int* __restrict__ counts, BootRule r,
                                                                 double* __restrict__ out, double* __restrict__ replicates) {
    __shared__ double x[kBootMaxRows];
    __shared__ double v[kBootMaxReplicates];
    __shared__ int kept[kBootThreads / 64];
    const int q = blockIdx.x, c = blockIdx.y, s = blockIdx.z, tid = threadIdx.x;
    int n = counts[q];
    n = n < 0 ? 0 : n > r.max_rows ? r.max_rows : n;
    // (a)
    const double* column = table + (size_t)q * r.max_rows * r.C + r.cols[c];
    for (int p = tid; p < n; p += kBootThreads) x[p] = column[(size_t)p * r.C];
    __syncthreads();
    // (b)
    const unsigned long long key = boot_stream_key(r.seed, r.stream);
    const int rounds = (r.B + kBootThreads) / kBootThreads;     // ceil((B + 1) / 1024): the replicates 0 .. B
    double st[kBootRounds];
#pragma unroll
    for (int k = 0; k < kBootRounds; ++k) {
        st[k] = gait_detail::nan();
        const int rep = tid + k * kBootThreads;
        if (k < rounds && rep <= r.B) {
            double all[kBootStats];
            boot_statistics(x, n, r.block, key, rep, all);
            st[k] = s == 0 ? all[0] : s == 1 ? all[1] : all[2];
        }
    }
    // (c)
    const int width = 2 + r.n_q;
    double* row = out + (((size_t)q * r.n_cols + c) * kBootStats + s) * width;
    double* reps = replicates ? replicates + (((size_t)q * r.n_cols + c) * kBootStats + s) * r.B : nullptr;
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kBootRounds; ++k) {
        const int rep = tid + k * kBootThreads;
        const bool have = k < rounds && rep >= 1 && rep <= r.B;
        if (have) {
            v[rep - 1] = st[k];
            if (reps) reps[rep - 1] = st[k];
        }
        mine += __builtin_popcountll(__ballot(have && st[k] == st[k]));
    }
    if ((tid & 63) == 0) kept[tid >> 6] = mine;
    __syncthreads();
    int f = 0;
    for (int w = 0; w < kBootThreads / 64; ++w) f += kept[w];
    if (tid == 0) {
        row[0] = st[0];
        row[1] = (double)f;
        if (f == 0)
            for (int i = 0; i < r.n_q; ++i) row[2 + i] = gait_detail::nan();
    }
    if (f == 0) return;
    int rank[kBootRounds] = {0, 0, 0, 0, 0};
    switch (rounds) {
        case 1: boot_count_ranks<1>(v, r.B, st, tid, rank); break;
        case 2: boot_count_ranks<2>(v, r.B, st, tid, rank); break;
        case 3: boot_count_ranks<3>(v, r.B, st, tid, rank); break;
        case 4: boot_count_ranks<4>(v, r.B, st, tid, rank); break;
        default: boot_count_ranks<5>(v, r.B, st, tid, rank); break;
    }
#pragma unroll
    for (int k = 0; k < kBootRounds; ++k) {
        const int rep = tid + k * kBootThreads;
        if (!(k < rounds && rep >= 1 && rep <= r.B) || st[k] != st[k]) continue;
        for (int i = 0; i < r.n_q; ++i)
            if (rank[k] == boot_quantile_rank(r.q[i], f)) row[2 + i] = st[k];
    }
}
static_assert(kBootRounds * kBootThreads >= kBootMaxReplicates + 1 && kBootRounds == 5, "a lane's rounds cover the replicates 0 .. B");

}  // namespace

hipError_t launch_step_tables(const int* off, int n_seq, const int* events, const int* phase, const double* per_frame, double fps, int max_rows,
                              unsigned long long* words, size_t mask_words, double* steps, double* strides, int* counts, hipStream_t s) {
    return launch_k(step_tables_kernel, dim3(n_seq), dim3(kGaitThreads), 0, s, off, events, phase, per_frame, fps, max_rows, words, mask_words, steps, strides, counts);
}

hipError_t launch_bootstrap(const double* table, const int* counts, int n_seq, const BootRule& rule, double* out, double* replicates, hipStream_t s) {
    return launch_k(bootstrap_kernel, dim3(n_seq, rule.n_cols, kBootStats), dim3(kBootThreads), 0, s, table, counts, rule, out, replicates);
}

}  // namespace grk
