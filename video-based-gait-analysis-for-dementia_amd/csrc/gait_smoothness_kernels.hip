// Movement smoothness of four body signals on the device, for many sequences lying back to back: the spectral arc length and the dimensionless jerk
// of every segment (rules and columns: DESIGN 4.24; the arithmetic: gait_smoothness.h, which the host checker runs too).
//
// THIS FILE IS COMPILED WITH -ffp-contract=off (csrc/Makefile).  Every floating-point value is float64 and every operation rounds once.  A lane owns
// a bin; across lanes nothing is joined but a maximum with its smallest bin, a first and a last index, none of which depends on the order; every sum
// is one lane's, in rising index.  So no result depends on an order the hardware chooses, nor on the shape of the grid.  No atomics anywhere, and
// every value is written with a plain vector store.
//
// The call's frame kernel is gait_regularity's (launch_reg_frames) and its Gaussian seq_gauss_columns_kernel; this file holds the three launches behind.
//
// smo_starts_kernel -- the grid is (n_seq, 4): ONE WAVE per (sequence, channel).  A lane per frame makes y with ent_diff, 64 frames a round, and the
// round's ballot IS the word of the validity bitmask: 512 words at most (kEntMaxFrames), always in LDS; y itself is not kept, the segment kernel
// makes its own L values again.  The sequence's first slot is the sum of spec_run_segments over the sequences in front (integers: a lane per
// sequence, then one lane adds the 64 parts).  One lane walks the runs of the bitmask by word (spec_runs) and writes `start` into the slot rows; the
// wave fills the slots behind the candidates with NaN, tells every slot its sequence (channel 0's wave) and writes n, candidates and used.  The
// launch also makes the call's twiddle table, (sine, cosine) of har_twiddle(j, N), each workgroup a part: it is read by the next launch only.
//
// smo_segment_kernel -- the grid is (slots, 4): ONE WORKGROUP of kSmoThreads per (slot, channel); it exits where the slot holds no segment.  LDS
// (dynamic): the segment's x and y (2 L), the magnitudes (k_c + 1) and the arc's terms (k_c + 1): 9.2 KB at the defaults (L = 64, 513 bins), 36.9 KB
// at the limits (L = 256, 2049 bins); with 160 KB a CU that is 17 and 4 workgroups, and the waves allow 8 (32 waves a CU), so at the defaults the
// waves bound the occupancy and at the limits LDS does (16 waves a CU, 4 a SIMD).  A LANE OWNS BIN k and takes rounds of the workgroup's width over
// the k_c + 1 bins: y is one address for the wave, a broadcast.  THE TWIDDLE GATHER at (k i) mod N is lane-dependent.  The table is the call's, in
// the scratch, 16 bytes an entry so that one load brings sine and cosine: 16 KB at N = 1024 and 64 KB at N = 4096, read through L1 and L2 by every
// workgroup of the launch.  (In a diagnostic build GRNET_SMO_TWIDDLES = 1 copies it into LDS per workgroup and = 2 makes every twiddle again with
// har_twiddle: the forms that DESIGN 4.24 measures against it; the bits are har_twiddle's in every case.  The product build has form 0 as a
// constant.)  Consecutive lanes are i entries apart, so a round's gather touches at most 64 cache lines at large i and one at i = 0.  Then M_max and its bin by wave shuffles and four LDS entries, m_k = M_k / M_max in
// place, k_a and k_b the same way, the arc's terms by all lanes, their sum by lane 0 in rising k, and the jerk by lane 64 meanwhile.
//
// smo_row_kernel -- the grid is (n_seq, 4): the wave stages 64 slots' sparc, k_last and dj at a time in LDS and one lane walks them in time order,
// twice (the mean, then the spread), with gait_smoothness.h's steps.
//
// The hook grnet_op_gait_sparc launches the three kernels on a caller's signals.
#include "kernels.h"
#include "device.h"
#include "gait_smoothness.h"

namespace grk {
namespace {

__global__ __launch_bounds__(kSmoWave) void smo_starts_kernel(const int* __restrict__ off, SmoRule r, const double* __restrict__ rows, const int* __restrict__ exclude,
                                                             double* __restrict__ tw, int* __restrict__ slot_seq, int* __restrict__ slot_base,
                                                             double* __restrict__ per_seg, double* __restrict__ per_seq) {
    __shared__ unsigned long long mask[kEntMaxFrames / 64];
    __shared__ int part[kSmoWave], shared[2];
    const int q = blockIdx.x, ch = blockIdx.y, tid = threadIdx.x, L = r.segment, hop = r.hop;
    const int block = q * kRegChannels + ch, blocks = gridDim.x * kRegChannels;
    for (int j = block * kSmoWave + tid; j < r.nfft; j += blocks * kSmoWave) har_twiddle(j, r.nfft, tw + 2 * j, tw + 2 * j + 1);
    int mine = 0;
    for (int p = tid; p < q; p += kSmoWave) mine += spec_run_segments(off[p + 1] - off[p], L, hop);
    part[tid] = mine;
    const int f0 = off[q], T = off[q + 1] - f0, words = (T + 63) >> 6;
    const double* x = rows + (size_t)f0 * kRegChannels + ch;
    const int* ex = exclude ? exclude + f0 : nullptr;
    long long n = 0;
    for (int w = 0; w < words; ++w) {
        const int t = w * 64 + tid;
        const double v = t < T ? ent_diff(x, ex, t, T, r.derivative) : gait_detail::nan();
        const unsigned long long word = __ballot(translation_detail::finite(v));
        if (tid == 0) mask[w] = word;
        n += __builtin_popcountll(word);
    }
    __syncthreads();
    if (tid == 0) {
        int base = 0;
        for (int i = 0; i < kSmoWave; ++i) base += part[i];
        double* seg = per_seg + ((size_t)base * kRegChannels + ch) * kSmoSegCols;
        shared[0] = base;
        shared[1] = spec_runs(mask, T, L, hop, [&](int s, int t0) { seg[(size_t)s * kRegChannels * kSmoSegCols + kSmoColStart] = (double)t0; });
    }
    __syncthreads();
    const int base = shared[0], candidates = shared[1], slots = spec_run_segments(T, L, hop);      // candidates <= slots: a split only loses some
    for (int e = candidates * kSmoSegCols + tid; e < slots * kSmoSegCols; e += kSmoWave)
        per_seg[((size_t)(base + e / kSmoSegCols) * kRegChannels + ch) * kSmoSegCols + e % kSmoSegCols] = gait_detail::nan();
    if (ch == 0) {
        for (int s = tid; s < slots; s += kSmoWave) slot_seq[base + s] = q;
        if (tid == 0) slot_base[q] = base;
    }
    if (tid == 0) {
        double* row = per_seq + ((size_t)q * kRegChannels + ch) * kSmoSeqCols;
        row[kSmoColN] = (double)n;
        row[kSmoColCandidates] = (double)candidates;
        row[kSmoColUsed] = (double)spec_used(candidates, r.min_segments);
    }
}

// M_k of one bin with the twiddles where kForm puts them: 0 the call's table (tw in the scratch), 1 its copy in LDS (tw there), 2 har_twiddle
// itself.  The operations on y are smo_magnitude's in its order
template <int kForm>
__device__ __forceinline__ double smo_bin(const double* y, int L, const double* tw, int N, int k) {
    if (kForm != 2) return smo_magnitude(y, L, tw, N, k);
    double C = 0., S = 0.;
    for (int i = 0, j = 0; i < L; ++i) {
        const double v = y[i];
        double sn, cs;
        har_twiddle(j, N, &sn, &cs);
        C = C + v * cs;
        S = S + v * sn;
        j += k;
        if (j >= N) j -= N;
    }
    return __builtin_sqrt(C * C + S * S);
}

template <int kForm>
__global__ __launch_bounds__(kSmoThreads) void smo_segment_kernel(const int* __restrict__ off, SmoRule r, int kc, const double* __restrict__ rows,
                                                                  const int* __restrict__ exclude, const double* __restrict__ tw, const int* __restrict__ slot_seq,
                                                                  double* __restrict__ per_seg) {
    extern __shared__ double lds[];
    __shared__ double wave_m[kSmoThreads / kSmoWave];
    __shared__ int wave_k[kSmoThreads / kSmoWave], wave_a[kSmoThreads / kSmoWave], wave_b[kSmoThreads / kSmoWave];
    const int slot = blockIdx.x, ch = blockIdx.y, tid = threadIdx.x, wave = tid / kSmoWave, L = r.segment, N = r.nfft, bins = kc + 1;
    double* row = per_seg + ((size_t)slot * kRegChannels + ch) * kSmoSegCols;
    const double start = row[kSmoColStart];
    if (!(start >= 0.)) return;                                // a slot behind the candidates: the whole workgroup leaves
    const int q = slot_seq[slot], f0 = off[q], T = off[q + 1] - f0, t0 = (int)start;
    double *x = lds, *y = x + L, *M = y + L, *term = M + bins, *table = term + bins;
    const double* col = rows + (size_t)f0 * kRegChannels + ch;
    const int* ex = exclude ? exclude + f0 : nullptr;
    for (int i = tid; i < L; i += kSmoThreads) {               // t0 + L <= T: spec_runs laid the segment inside a run
        x[i] = col[(size_t)(t0 + i) * kRegChannels];
        y[i] = ent_diff(col, ex, t0 + i, T, r.derivative);
    }
    if (kForm == 1)
        for (int j = tid; j < 2 * N; j += kSmoThreads) table[j] = tw[j];
    __syncthreads();
    SmoPeak p = smo_peak_none();
    for (int k = tid; k < bins; k += kSmoThreads) {
        const double Mk = smo_bin<kForm>(y, L, kForm == 1 ? table : tw, N, k);
        M[k] = Mk;
        p = smo_peak_take(p, Mk, k);
    }
    for (int o = kSmoWave / 2; o > 0; o >>= 1) p = smo_peak_merge(p, SmoPeak{__shfl_xor(p.m, o, kSmoWave), __shfl_xor(p.k, o, kSmoWave)});
    if (tid % kSmoWave == 0) { wave_m[wave] = p.m; wave_k[wave] = p.k; }
    __syncthreads();
    p = smo_peak_none();
    for (int w = 0; w < kSmoThreads / kSmoWave; ++w) p = smo_peak_merge(p, SmoPeak{wave_m[w], wave_k[w]});
    if (!smo_peak_holds(p)) {                                  // the same for every lane
        if (tid >= kSmoColSparc && tid < kSmoSegCols) row[tid] = gait_detail::nan();
        return;
    }
    int ka = bins, kb = -1;
    for (int k = tid; k < bins; k += kSmoThreads) {            // a lane turns the magnitudes it made itself
        const double m = M[k] / p.m;
        M[k] = m;
        if (m >= r.amplitude) {
            if (k < ka) ka = k;
            kb = k;
        }
    }
    for (int o = kSmoWave / 2; o > 0; o >>= 1) {
        ka = min(ka, __shfl_xor(ka, o, kSmoWave));
        kb = max(kb, __shfl_xor(kb, o, kSmoWave));
    }
    if (tid % kSmoWave == 0) { wave_a[wave] = ka; wave_b[wave] = kb; }
    __syncthreads();
    for (int w = 0; w < kSmoThreads / kSmoWave; ++w) {
        ka = min(ka, wave_a[w]);
        kb = max(kb, wave_b[w]);
    }
    if (kb > ka) {                                             // the peak's bin has m = 1 >= amplitude: k_a <= k_b exist
        const double u = 1.0 / (double)(kb - ka);
        for (int k = ka + tid; k < kb; k += kSmoThreads) term[k - ka] = smo_arc_term(u, M[k], M[k + 1]);
    }
    __syncthreads();
    if (tid == 0) {
        row[kSmoColSparc] = kb > ka ? smo_arc(term, kb - ka) : 0.;
        row[kSmoColFirst] = (double)ka;
        row[kSmoColLast] = (double)kb;
        row[kSmoColPeakBin] = (double)p.k;
        row[kSmoColPeakMagnitude] = p.m;
    }
    if (tid == kSmoWave) {                                     // the second wave's first lane, beside the first's sum
        double dj, v_peak;
        smo_jerk(x, L, &dj, &v_peak);
        row[kSmoColDj] = dj;
        row[kSmoColVPeak] = v_peak;
    }
}

__global__ __launch_bounds__(kSmoWave) void smo_row_kernel(const int* __restrict__ off, SmoRule r, const int* __restrict__ slot_base,
                                                          const double* __restrict__ per_seg, double* __restrict__ per_seq) {
    __shared__ double sparc[kSmoWave], last[kSmoWave], dj[kSmoWave];
    const int q = blockIdx.x, ch = blockIdx.y, tid = threadIdx.x;
    double* row = per_seq + ((size_t)q * kRegChannels + ch) * kSmoSeqCols;
    const int candidates = (int)row[kSmoColCandidates], used = (int)row[kSmoColUsed];
    const double* seg = used > 0 ? per_seg + ((size_t)slot_base[q] * kRegChannels + ch) * kSmoSegCols : nullptr;
    const size_t stride = (size_t)kRegChannels * kSmoSegCols;
    const SpecRule sr = smo_spec(r);
    SmoSums a = smo_row_none();
    double Q = 0., mean = 0.;
    for (int pass = 0; pass < 2 && used > 0; ++pass) {
        for (int s0 = 0; s0 < candidates; s0 += kSmoWave) {
            const int here = min(kSmoWave, candidates - s0);
            __syncthreads();
            if (tid < here) {
                const double* e = seg + (size_t)(s0 + tid) * stride;
                sparc[tid] = e[kSmoColSparc];
                last[tid] = e[kSmoColLast];
                dj[tid] = e[kSmoColDj];
            }
            __syncthreads();
            if (tid == 0)
                for (int s = 0; s < here; ++s) {
                    if (pass == 0) smo_row_take(a, sparc[s], last[s], dj[s], sr);
                    else Q = smo_row_spread(Q, sparc[s], mean);
                }
        }
        if (pass == 0 && tid == 0) {
            if (a.defined < 1) break;
            mean = smo_row_mean(a);
        }
    }
    if (tid == 0) smo_row_write(a, Q, used, row);
}

}  // namespace

size_t smo_lds_bytes(const SmoRule& r, int kc, int form) { return (2 * (size_t)r.segment + 2 * (size_t)(kc + 1) + (form == 1 ? 2 * (size_t)r.nfft : 0)) * sizeof(double); }

hipError_t launch_smo_sequences(const int* off, int n_seq, int slots, const SmoRule& rule, int kc, int form, const double* rows, const int* exclude, double* tw,
                                int* slot_seq, int* slot_base, double* per_seg, double* per_seq, hipStream_t s) {
    hipError_t e = launch_k(smo_starts_kernel, dim3(n_seq, kRegChannels), dim3(kSmoWave), 0, s, off, rule, rows, exclude, tw, slot_seq, slot_base, per_seg, per_seq);
    if (e != hipSuccess) return e;
    if (slots > 0) {
        const size_t lds = smo_lds_bytes(rule, kc, form);
        const dim3 grid(slots, kRegChannels), block(kSmoThreads);
        if (form == 1) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(smo_segment_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e == hipSuccess) e = launch_k(smo_segment_kernel<1>, grid, block, lds, s, off, rule, kc, rows, exclude, (const double*)tw, (const int*)slot_seq, per_seg);
        } else if (form == 2) {
            e = launch_k(smo_segment_kernel<2>, grid, block, lds, s, off, rule, kc, rows, exclude, (const double*)tw, (const int*)slot_seq, per_seg);
        } else {
            e = launch_k(smo_segment_kernel<0>, grid, block, lds, s, off, rule, kc, rows, exclude, (const double*)tw, (const int*)slot_seq, per_seg);
        }
        if (e != hipSuccess) return e;
    }
    return launch_k(smo_row_kernel, dim3(n_seq, kRegChannels), dim3(kSmoWave), 0, s, off, rule, (const int*)slot_base, (const double*)per_seg, per_seq);
}

}  // namespace grk
