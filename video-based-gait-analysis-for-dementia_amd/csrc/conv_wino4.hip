// Winograd F(4x4, 3x3) on the fp32 matrix cores for the widest 3x3 stride-1 layers on 56x56 maps (upsample head 256 -> 256, PARE head
// 480 -> 256: hrnet.py:444-451, pare.py:197-210 -- Conv2d 3x3 pad 1 + BatchNorm2d(eval) + ReLU).  A 4x4 output tile is 36 independent
// products instead of 144 multiplies: 2.25 per output against 4 for F(2x2, 3x3) (round 2; source in the history: commit 8d3a931) and 9 for the direct kernel.  The
// transforms have non-trivial coefficients (4, 5, 2, 8 and sixths in the filter transform, which is applied in fp64 at load):
// measured on a 256-channel layer in fp32 the result is 7.8e-6 of the output rms away from the exact sum (F(2x2,3x3): 8e-7, the
// direct fma chain: 1.9e-6) -- two orders of magnitude inside the 1e-3 bar, covered by the same parity tests.
//
// Loop discipline (worked out on the round-2 F(2x2,3x3) kernel): on gfx950 every vector instruction between fp32 MFMAs is matrix-pipe time: few of them,
// clustered).  One workgroup (4 waves): one image, ONE tile row = 14 tiles (output rows 4r .. 4r+3; one MFMA row tile, 2 rows
// idle), 64 output channels, all 36 points -- wave w owns points 9w .. 9w+8 = 9 x 4 accumulator tiles (144 registers).  Per chunk of
// 8 input channels: the 6 input rows of the chunk by LDS-DMA (rows contiguous in the NCHW plane, 16-byte units); thread (channel, tile, half)
// transforms HALF of a 6x6 patch -- 6 16-byte LDS reads + DPP for the two edge columns, three rows of B^T d and their 18 products
// with B, 18 LDS writes into V[point][channel][16 tiles]; 72 MFMAs per wave, A fragment = one LDS dword, the 4 B fragments = one
// 16-byte load straight from L2, requested a chunk ahead.
#include "kernels.h"
#include "device.h"
#include "conv_wino4_tile.h"

#include <cstdio>
#include <cstdlib>

namespace grk {

namespace {

#ifdef GRNET_ABLATION
__device__ unsigned long long g_w4phase[8];      // diagnostic build, dbg bit 3: ticks summed over workgroups (tools/wino_phases.py)
#endif

constexpr int kCK = 8;                       // input channels per chunk
constexpr size_t kLdsB = Wino4Geom<56, kCK, 256>::lds_bytes;      // 58 368 B (56-wide maps; 28-wide ones need less and take the same)

template <typename T>
__device__ __forceinline__ void landed(T& x) { asm volatile("" : "+v"(x)); }

// NB: 16-channel blocks per workgroup: 4, or 2 = HALF a 64-channel block of the same packed weights (the half-size workgroups of a
// layer's last round, ConvArgs::wsplit)
// WD: map width, 56 or 28 (Wino4Geom).
// WSPLIT: the 32-channel kernel on HALF a 64-channel block of weights packed for the 64-channel kernel (last-round workgroups).  The
// standalone 32-channel layers (NB = 2, !WSPLIT) have their own packing with the two k-steps of a chunk interleaved (pack_wino4_weights):
// one 16-byte load brings a point's B fragments of BOTH k-steps, 9 weight loads per chunk and wave instead of 18.
template <int NB, int WD, int ABL, bool WSPLIT>
__device__ __forceinline__ void conv_wino4_body(const ConvArgs& a) {
    constexpr bool PAIR = NB == 2 && !WSPLIT;
    constexpr int NLD = PAIR ? 9 : 18;                   // weight loads per chunk and wave
    typedef Wino4Geom<WD, kCK, 256> G;
    constexpr int TPR = G::TPR, TRG = G::TRG, kRawW = G::RAWW, UPC = G::UPC, kV = G::V, kMrow = G::MROW;
    extern __shared__ __align__(16) float smem[];
    float* raw = smem;                                  // [2][8][RAWW]
    float* V = raw + G::VOFF;                           // [2][36][8][16]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lq = lane >> 4;

    const int id = a.blk0 + (WSPLIT ? (int)(blockIdx.x >> 1) : (int)blockIdx.x), nb0 = WSPLIT ? 2 * (int)(blockIdx.x & 1) : 0;
    int img, r, by;
    G::decode(a, id, img, r, by);
    const int co0 = WSPLIT ? by * 64 : by * (NB * 16);      // first channel of the weight block; channel n*16 + l sits at l*cstr + n
    constexpr int cstr = WSPLIT ? 4 : NB;
    set_wave_prio(a.prio);
    const int HW = a.H * a.W;
    const float* inb = a.in + ((size_t)img * a.in_ctot + a.in_coff) * HW;
    const int g0 = (4 * TRG * r - 1) * WD;               // plane index of raw[.][0]

    const __amdgpu_buffer_rsrc_t u_rsrc = buffer_rsrc(a.w, 36 * a.CinPad * a.CoutPad * 4), r_rsrc = buffer_rsrc(inb, a.Cin * HW * 4);
    typedef float bfrag __attribute__((ext_vector_type(PAIR ? 4 : NB)));   // PAIR: {k-step 0: n0 n1, k-step 1: n0 n1}
    const int nchunks_u = a.CinPad / kCK;
    // byte offsets: a lane's part (VGPR) + point / chunk part (scalar)
    const int ub = PAIR ? ((lq * a.CoutPad * 2 + co0 * 2 + l15 * 4) * 4 + wave * 9 * nchunks_u * 4 * a.CoutPad * 2 * 4)
                        : ((wave * 9 * a.CinPad + lq) * a.CoutPad + co0 + l15 * cstr + nb0) * 4;
    const int u_point = PAIR ? nchunks_u * 4 * a.CoutPad * 2 * 4 : a.CinPad * a.CoutPad * 4;
    const int u_kstep = 4 * a.CoutPad * 4, u_chunk = PAIR ? 4 * a.CoutPad * 2 * 4 : kCK * a.CoutPad * 4;
    auto load_u = [&](int chunk, int g) -> bfrag {       // !PAIR: group g = (point wave*9 + g/2, k-step g%2); PAIR: g = point
        const int soff = PAIR ? chunk * u_chunk + g * u_point : chunk * u_chunk + (g >> 1) * u_point + (g & 1) * u_kstep;
        if constexpr (PAIR || NB == 4) return __builtin_bit_cast(bfrag, __builtin_amdgcn_raw_buffer_load_b128(u_rsrc, ub, soff, 0));
        else return __builtin_bit_cast(bfrag, __builtin_amdgcn_raw_buffer_load_b64(u_rsrc, ub, soff, 0));
    };
    int roff[G::NRU];                                    // raw rows: 672 units per chunk; -1 = no unit or a row outside the image
#pragma unroll
    for (int i = 0; i < G::NRU; ++i) {
        const int u = i * G::NT + tid, ch = u / UPC, k = u - ch * UPC, gi = g0 + 4 * k;
        const bool unit = u < kCK * UPC, inside = gi >= 0 && gi < HW;
        roff[i] = unit && inside ? (ch * HW + gi) * 4 : -1;
        if (unit && !inside) {                           // rows above / below the image: zero once in both buffers, the DMA never writes there
            *reinterpret_cast<f32x4*>(raw + u * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(raw + kCK * kRawW + u * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    auto issue_raw = [&](int chunk) { G::issue_raw(roff, r_rsrc, raw, chunk, wave, HW); };

    // ---- input transform (Wino4Patch).  16 rows of 16 lanes: row = (channel 0..7, half 0..1), lane = tile 0..13 (lanes 14, 15 idle: their
    // zeros are the right neighbour of tile 13 and they write into the two padding tile slots)
    const int row16 = tid >> 4, px = tid & 15, chn = row16 & 7;
    const int half = __builtin_amdgcn_readfirstlane(row16 >> 3);                         // wave-uniform: waves 0, 1 / 2, 3
    // WD = 28: the 16 lanes are two tile rows of 7 tiles + 1 idle lane each; idle lanes supply the zero on BOTH sides there
    const int pc = WD == 56 ? px : (px & 7), trl = WD == 56 ? 0 : (px >> 3);
    const bool real = pc < TPR;
    const int rpos = chn * kRawW + (4 * trl) * WD + 4 * (real ? pc : TPR - 1);
    const int slot = real ? trl * TPR + pc : 14 + (WD == 56 ? px - 14 : trl);            // tile slot in V (14, 15: padding)
    const int vpos = (half * 18) * (kCK * 16) + chn * 16 + slot;                         // + (rr * 6 + c) * 128 for row rr of the half, column c
    typedef Wino4Patch<G> Tf;

    f32x4 acc[9][NB];                                    // [point of this wave][channel block]
#pragma unroll
    for (int p = 0; p < 9; ++p)
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[p][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nchunks = a.CinPad / kCK;
    bfrag bq[NLD];                                       // B fragments of the 18 MFMA groups (PAIR: of the 9 points); each is re-requested for the next chunk behind its group
    abl::Ticks<5> ticks(abl::bit(a.dbg, 8));          // [0] prologue, [1] first transform, [2] chunk loop, [3] epilogue, [4] workgroups
    issue_raw(0);
    if (nchunks > 1) issue_raw(1);
#pragma unroll
    for (int g = 0; g < NLD; ++g) bq[g] = load_u(0, g);
    if constexpr (PAIR) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");   // the raw rows (requested before the weight loads) have landed
    else asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
    __syncthreads();
    ticks.mark(0);
    {
        Tf t;
        t.read(raw + rpos);
        t.halo(real);
        t.rows(half);
        t.cols(V + vpos);
    }
    ticks.mark(1);
    // ---- the chunk loop: three clusters of 24 MFMAs (three points x two k-steps x four channel blocks)
    float av[2][6];
    auto load_a = [&](int buf, int c, int set) {         // A fragments of cluster c: points 3c .. 3c+2 of this wave, both k-steps
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int p = wave * 9 + 3 * c + (k >> 1), ks = k & 1;
            av[set][k] = V[buf * kV + p * (kCK * 16) + (ks * 4 + lq) * 16 + l15];
        }
    };
    auto chunk = [&](int buf, bool with_transform, int next) {
        Tf t;
        const float* rp = raw + (next & 1) * (kCK * kRawW) + rpos;
        float* vp = V + (next & 1) * kV + vpos;
        if (ABL != 3) load_a(buf, 0, 0);
        if (with_transform && ABL != 1 && next + 1 < nchunks) issue_raw(next + 1);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // cluster c: (1) everything requested one cluster ago has landed
#pragma unroll
            for (int k = 0; k < 6; ++k) landed(av[c & 1][k]);
            if (with_transform && ABL != 2) {
                if (c == 1) { t.halo(real); t.rows(half); }
                if (c == 2) t.cols(vp);
            }
            __builtin_amdgcn_sched_barrier(0);
            // (2) requests: the next cluster's A fragments, the next chunk's B fragments of the previous cluster, the next chunk's input rows
            if (c < 2 && ABL != 3) load_a(buf, c + 1, (c + 1) & 1);
            if (with_transform && ABL != 1 && c > 0) {
#pragma unroll
                for (int k = 0; k < NLD / 3; ++k) bq[(NLD / 3) * (c - 1) + k] = load_u(next, (NLD / 3) * (c - 1) + k);
            }
            if (with_transform && ABL != 2 && c == 0) t.read(rp);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < 6; ++k)
#pragma unroll
                for (int n = 0; n < NB; ++n) {
                    const int pi = 3 * c + (k >> 1);
                    const float bfr = PAIR ? bq[pi][(k & 1) * 2 + n] : bq[6 * c + k][n];
                    acc[pi][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c & 1][k], bfr, acc[pi][n], 0, 0, 0);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (with_transform && ABL != 1) {
#pragma unroll
            for (int k = 0; k < NLD / 3; ++k) bq[2 * (NLD / 3) + k] = load_u(next, 2 * (NLD / 3) + k);
        }
    };
    auto meet = [&](bool last) {
        // this wave's share of raw(ch+1) has landed: it was requested before the 18 weight loads of the previous iteration, which may stay
        // in flight (loads return in order)
        if (last) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if constexpr (PAIR) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
        __syncthreads();
    };
    for (int ch = 0; ch + 1 < nchunks; ++ch) {
        meet(false);
        chunk(ch & 1, true, ch + 1);
    }
    const bool has_add = a.n_add == 1;
    meet(nchunks > 1);
    // thread (channel c of the pass's 16, tile t): 4 output rows of 4 pixels.  The residual rows of a pass are requested a pass ahead
    // (pass 0's before the accumulators go to LDS): their round trip used to sit between the inverse transform and the stores of every
    // pass -- twice per launch of the 32-channel branch layers, which are the longest dependency chain of stages 2-4.
    typename G::Epi ep;
    G::epi(tid, r, a.H, ep);
    f32x4 radd[4] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    auto fetch_res = [&](int nt) {
        const int co = co0 + (nb0 + nt) * 16 + ep.ec;
        if (has_add && ep.on && co < a.Cout) G::fetch_res(radd, a, ep, img, co, HW);
    };
    fetch_res(0);                                       // under the last chunk's MFMAs
    chunk((nchunks - 1) & 1, false, 0);

    ticks.mark(2);
    // ---- epilogue: inverse transform A^T M A (A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]), + bias, + residual, ReLU
    float* Mx = smem;                                    // [36 points][16 channels][20]
    for (int nt = 0; nt < NB; ++nt) {
        __syncthreads();
#pragma unroll
        for (int pi = 0; pi < 9; ++pi) {
            f32x4 v;
            if constexpr (NB == 4) v = nt == 0 ? acc[pi][0] : nt == 1 ? acc[pi][1] : nt == 2 ? acc[pi][2] : acc[pi][3];
            else v = nt == 0 ? acc[pi][0] : acc[pi][1];
            *reinterpret_cast<f32x4*>(Mx + ((wave * 9 + pi) * 16 + l15) * kMrow + lq * 4) = v;
        }
        __syncthreads();
        const f32x4 rcur[4] = {radd[0], radd[1], radd[2], radd[3]};
        if (nt + 1 < NB) fetch_res(nt + 1);
        if (ep.on) {
            const int co = co0 + (nb0 + nt) * 16 + ep.ec;
            if (co < a.Cout) {
                float s[4][6];                           // A^T M: rows of the 4x6 intermediate
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    float m[6];
#pragma unroll
                    for (int i = 0; i < 6; ++i) m[i] = Mx[((i * 6 + j) * 16 + ep.ec) * kMrow + ep.et];
                    at_f43(m, s[0][j], s[1][j], s[2][j], s[3][j]);
                }
                const float b = a.bias[co];
                const size_t obase = ((size_t)img * a.out_ctot + a.out_coff + co) * HW + ep.eorow * WD + 4 * ep.etx;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float y0, y1, y2, y3;
                    at_f43<true>(s[i], y0, y1, y2, y3, b);
                    f32x4 y = f32x4{y0, y1, y2, y3};
                    if (has_add) y += rcur[i];
                    if (a.relu) { y[0] = fmaxf(y[0], 0.f); y[1] = fmaxf(y[1], 0.f); y[2] = fmaxf(y[2], 0.f); y[3] = fmaxf(y[3], 0.f); }
                    *reinterpret_cast<f32x4*>(a.out + obase + i * WD) = y;
                }
            }
        }
    }
    ticks.mark(3);
    ticks.count(4);
    ticks.flush(GRK_ABL_COUNTERS(g_w4phase), tid == 0);
}

template <int NB, int WD = 56, int ABL = 0, bool WSPLIT = false>
__global__ __launch_bounds__(256) void conv_wino4_f32(const ConvArgs a) { conv_wino4_body<NB, WD, ABL, WSPLIT>(a); }

// ---------------------------------------------------------------------------------------------------------------------------------
// conv_wino4w_f32: the same F(4x4,3x3) convolution for the WIDE layers on 56x56 maps (output channels in 128s: 480 -> 256, 256 -> 256,
// 128 -> 128 -- the upsample heads and the PARE head, 0.9 ms of a 3.7 ms step), round 4.  What the 4-wave kernel above loses on them is
// not the matrix pipe (its chunk loop is ~53 % MFMA) but everything a workgroup does per 64 output channels: the input transform, the
// raw-row DMA and the chunk skeleton are paid again by every 64-channel workgroup of the same tile row, and with one wave per SIMD every
// LDS / L2 round trip is dead time.  Here a workgroup is EIGHT waves = 128 output channels on one tile row:
//   * V (the transformed chunk) is built once and shared by both 64-channel halves: transform and DMA per output channel halve;
//   * two waves per SIMD: wave w and wave w+4 share a SIMD (waves go to SIMDs cyclically) and run the two halves of an iteration in
//     OPPOSITE order -- waves 0-3 transform chunk c+1, then multiply chunk c; waves 4-7 multiply first -- so a SIMD's two waves are in
//     different phases and each one's LDS / memory latencies are covered by the other's MFMAs;
//   * chunks of 16 input channels (all 512 threads transform: thread = (channel, tile, half of the patch)), one barrier per 16 channels;
//   * at most 256 registers per wave (two waves per SIMD): hipcc then keeps the 144 accumulators in ordinary VGPRs (no AGPR split), the
//     B fragments live in a ring of two clusters (48 registers) instead of a whole chunk (72), re-requested right behind their MFMAs.
// Wave w: points 9 (w & 3) .. + 8, output channels 64 (w >> 2) .. + 63 of the workgroup's 128 (4 accumulator tiles per point).
// LDS: raw rows [2][16][336] + V [2][36][16][16] = 116.7 KB (one workgroup per CU); the epilogue's [2 halves][36][16][20] reuses it.
constexpr int kCKW = 16;                              // input channels per chunk
constexpr size_t kLdsW = Wino4Geom<56, kCKW, 512>::lds_bytes;      // 116 736 B

// WD: map width, 56 (one tile row of 14 tiles) or 28 (two tile rows of 7, as in the 4-wave kernel).  NPW: 16-channel blocks per wave:
// 4 = 128 output channels per workgroup, 2 = 64 (the 64 -> 64 layers: HR branch 1 on 28x28 maps -- until round 4 two 32-channel
// workgroups, each transforming the same input -- and layer1 / the first upsample head on 56x56 maps).  Weights are packed as for the
// 4-wave kernel's 64-channel blocks: a lane's 16 bytes hold its channel of the four 16-channel blocks; with NPW = 2 a wave reads its 8.
template <int WD, int NPW>
__device__ __forceinline__ void conv_wino4w_body(const ConvArgs& a) {
    typedef Wino4Geom<WD, kCKW, 512> G;
    constexpr int TPR = G::TPR, TRG = G::TRG, kRawW = G::RAWW, UPC = G::UPC, kVW = G::V, kMrow = G::MROW;
    constexpr int COUTW = 2 * NPW * 16;                  // output channels per workgroup
    static_assert(NPW == 4 || NPW == 2, "geometry");
    typedef float bfrag __attribute__((ext_vector_type(NPW)));
    extern __shared__ __align__(16) float smem[];
    float* raw = smem;                                  // [2][16][RAWW]
    float* V = raw + G::VOFF;                           // [2][36][16][16]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, lq = lane >> 4;
    const int pg = wave & 3, hf = wave >> 2;            // point group; half of the workgroup's output channels = half of the patch it transforms

    const int id = blockIdx.x;
    int img, r, by;
    G::decode(a, id, img, r, by);
    // first output channel of this wave and where it sits in the packed weights: channel n*16 + l of a 64-block is at l*4 + n
    const int co0 = by * COUTW + hf * (NPW * 16);
    const int wpos = NPW == 4 ? co0 : (co0 & ~63) + ((co0 >> 5) & 1) * 2;
    set_wave_prio(a.prio);
    const int HW = a.H * a.W;
    const float* inb = a.in + ((size_t)img * a.in_ctot + a.in_coff) * HW;
    const int g0 = (4 * TRG * r - 1) * WD;               // plane index of raw[.][0]

    const __amdgpu_buffer_rsrc_t u_rsrc = buffer_rsrc(a.w, 36 * a.CinPad * a.CoutPad * 4), r_rsrc = buffer_rsrc(inb, a.Cin * HW * 4);
    const int ub = ((pg * 9 * a.CinPad + lq) * a.CoutPad + wpos + l15 * 4) * 4;       // a lane's part of a B-fragment address (bytes)
    const int u_point = a.CinPad * a.CoutPad * 4, u_kstep = 4 * a.CoutPad * 4, u_chunk = kCKW * a.CoutPad * 4;
    // B fragments of cluster q of a chunk: q = 2 * (point third t) + (k-step pair kp); entry e = 2 * (point in third) + (k-step in pair)
    auto load_u = [&](int chunk, int q, int e) -> bfrag {
        const int soff = chunk * u_chunk + (3 * (q >> 1) + (e >> 1)) * u_point + (2 * (q & 1) + (e & 1)) * u_kstep;
        if constexpr (NPW == 4) return __builtin_bit_cast(bfrag, __builtin_amdgcn_raw_buffer_load_b128(u_rsrc, ub, soff, 0));
        else return __builtin_bit_cast(bfrag, __builtin_amdgcn_raw_buffer_load_b64(u_rsrc, ub, soff, 0));
    };
    int roff[G::NRU];                                    // -1 = no unit or a row outside the image
#pragma unroll
    for (int i = 0; i < G::NRU; ++i) {
        const int u = i * G::NT + tid, ch = u / UPC, k = u - ch * UPC, gi = g0 + 4 * k;
        const bool unit = u < kCKW * UPC, inside = gi >= 0 && gi < HW;
        roff[i] = unit && inside ? (ch * HW + gi) * 4 : -1;
        if (unit && !inside) {                           // rows above / below the image: zero once in both buffers, the DMA never writes there
            *reinterpret_cast<f32x4*>(raw + u * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(raw + kCKW * kRawW + u * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    auto issue_raw = [&](int chunk) { G::issue_raw(roff, r_rsrc, raw, chunk, wave, HW); };

    // ---- input transform: thread = (channel 0..15, tile slot 0..15, half), as in the 4-wave kernel (WD = 28: the 16 lanes are two tile rows of
    // 7 tiles + 1 idle lane each; idle lanes supply the zero on both sides there)
    const int row16 = tid >> 4, px = tid & 15, chn = row16 & 15;
    const int pc = WD == 56 ? px : (px & 7), trl = WD == 56 ? 0 : (px >> 3);
    const bool real = pc < TPR;
    const int rpos = chn * kRawW + (4 * trl) * WD + 4 * (real ? pc : TPR - 1);
    const int slot = real ? trl * TPR + pc : 14 + (WD == 56 ? px - 14 : trl);
    const int vpos = (hf * 18) * (kCKW * 16) + chn * 16 + slot;            // + (rr * 6 + c) * 256 for row rr of the half, column c
    auto transform = [&](const float* rp, float* vp) {
        Wino4Patch<G> t;
        t.read(rp);
        t.halo(real);
        t.rows(hf);
        t.cols(vp);
    };

    f32x4 acc[9][NPW];                                   // [point of this wave][16-channel block of its half]
#pragma unroll
    for (int p = 0; p < 9; ++p)
#pragma unroll
        for (int n = 0; n < NPW; ++n) acc[p][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nchunks = a.CinPad / kCKW;
    bfrag bq[6];                                         // B fragments of ONE cluster; every entry is re-requested for the next cluster right behind its MFMAs
    float av[2][6];
    auto load_a = [&](int buf, int q, int set) {         // A fragments of cluster q: points 3 (q >> 1) .. + 2 of this wave, k-steps 2 (q & 1), + 1
#pragma unroll
        for (int e = 0; e < 6; ++e) {
            const int p = pg * 9 + 3 * (q >> 1) + (e >> 1), ks = 2 * (q & 1) + (e & 1);
            av[set][e] = V[buf * kVW + p * (kCKW * 16) + (ks * 4 + lq) * 16 + l15];
        }
    };
    // the six clusters of a chunk: 6 x NPW MFMAs each (three points x two k-steps x NPW channel blocks).  Entry e of bq is consumed by NPW
    // MFMAs and re-requested at once for the next cluster (of the next chunk after cluster 5): the other entries' MFMAs and the SIMD's
    // other wave cover the L2 round trip.
    auto multiply = [&](int buf, int ch, bool more) {
        load_a(buf, 0, 0);
#pragma unroll
        for (int q = 0; q < 6; ++q) {
#pragma unroll
            for (int e = 0; e < 6; ++e) landed(av[q & 1][e]);
            __builtin_amdgcn_sched_barrier(0);
            if (q < 5) load_a(buf, q + 1, (q + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 6; ++e) {
                const int pi = 3 * (q >> 1) + (e >> 1);
#pragma unroll
                for (int n = 0; n < NPW; ++n) acc[pi][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q & 1][e], bq[e][n], acc[pi][n], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (q < 5) bq[e] = load_u(ch, q + 1, e);
                else if (more) bq[e] = load_u(ch + 1, 0, e);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    // thread (half h, channel c of the pass's 16, tile t) of the epilogue: 4 output rows of 4 pixels; the residual rows of a pass are requested a pass ahead
    const bool has_add = a.n_add == 1;
    const int eh = tid >> 8;
    typename G::Epi ep;
    G::epi(tid & 255, r, a.H, ep);
    f32x4 radd[4] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    auto fetch_res = [&](int nt) {
        const int co = by * COUTW + eh * (NPW * 16) + nt * 16 + ep.ec;
        if (has_add && ep.on && co < a.Cout) G::fetch_res(radd, a, ep, img, co, HW);
    };

    issue_raw(0);
    if (nchunks > 1) issue_raw(1);
#pragma unroll
    for (int e = 0; e < 6; ++e) bq[e] = load_u(0, 0, e);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");        // this wave's shares of raw(0), raw(1) (requested before the 6 weight loads) have landed
    __syncthreads();
    // Barrier #k separates "every wave has transformed chunk k" from "any wave multiplies chunk k".  Between two barriers waves 0-3 run
    // [transform k+1, multiply k] and waves 4-7 [multiply k, transform k+1]: the two waves of a SIMD are never both in their transform, and
    // each one's LDS / memory latencies are covered by the other's MFMAs.  Written as ONE loop with ONE multiply -- waves 0-3 take the
    // barrier in front of their transform, waves 4-7 behind it -- because with the two orders spelled out hipcc copied the 144 accumulators
    // at every merge point and spilled 127 registers.  raw(k + 2) is requested right behind barrier #k (its buffer held chunk k, which every
    // wave transformed before that barrier) and has landed when its requester reaches barrier #(k + 1).
    if (hf == 0) transform(raw + rpos, V + vpos);
    for (int k = 0; k < nchunks; ++k) {
        if (hf == 0) {
            asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            __syncthreads();
            if (k + 2 < nchunks) issue_raw(k + 2);
        }
        const int tk = k + 1 - hf;                            // the chunk this wave transforms in this iteration
        if (tk < nchunks) transform(raw + (tk & 1) * (kCKW * kRawW) + rpos, V + (tk & 1) * kVW + vpos);
        if (hf != 0) {
            asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            __syncthreads();
            if (k + 2 < nchunks) issue_raw(k + 2);
        }
        if (k + 1 == nchunks) fetch_res(0);                  // under the last chunk's MFMAs
        __builtin_amdgcn_sched_barrier(0);
        multiply(k & 1, k, k + 1 < nchunks);
        __builtin_amdgcn_sched_barrier(0);
    }

    // ---- epilogue: inverse transform A^T M A, + bias, + residual, ReLU; both halves go through LDS together, 16 channels each per pass
    float* Mx = smem + hf * G::MTILE;                    // this wave's half: [36 points][16 channels][20]
    const float* Mr = smem + eh * G::MTILE;              // the half this thread reads
    for (int nt = 0; nt < NPW; ++nt) {
        __syncthreads();
#pragma unroll
        for (int pi = 0; pi < 9; ++pi) {
            f32x4 v;
            if constexpr (NPW == 4) v = nt == 0 ? acc[pi][0] : nt == 1 ? acc[pi][1] : nt == 2 ? acc[pi][2] : acc[pi][3];
            else v = nt == 0 ? acc[pi][0] : acc[pi][1];
            *reinterpret_cast<f32x4*>(Mx + ((pg * 9 + pi) * 16 + l15) * kMrow + lq * 4) = v;
        }
        __syncthreads();
        const f32x4 rcur[4] = {radd[0], radd[1], radd[2], radd[3]};
        if (nt + 1 < NPW) fetch_res(nt + 1);
        if (ep.on) {
            const int co = by * COUTW + eh * (NPW * 16) + nt * 16 + ep.ec;
            if (co < a.Cout) {
                float s4[4][6];
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    float m[6];
#pragma unroll
                    for (int i = 0; i < 6; ++i) m[i] = Mr[((i * 6 + j) * 16 + ep.ec) * kMrow + ep.et];
                    at_f43(m, s4[0][j], s4[1][j], s4[2][j], s4[3][j]);
                }
                const float b = a.bias[co];
                const size_t obase = ((size_t)img * a.out_ctot + a.out_coff + co) * HW + ep.eorow * WD + 4 * ep.etx;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float y0, y1, y2, y3;
                    at_f43<true>(s4[i], y0, y1, y2, y3, b);
                    f32x4 y = f32x4{y0, y1, y2, y3};
                    if (has_add) y += rcur[i];
                    if (a.relu) { y[0] = fmaxf(y[0], 0.f); y[1] = fmaxf(y[1], 0.f); y[2] = fmaxf(y[2], 0.f); y[3] = fmaxf(y[3], 0.f); }
                    *reinterpret_cast<f32x4*>(a.out + obase + i * WD) = y;
                }
            }
        }
    }
}

template <int WD, int NPW>
__global__ __launch_bounds__(512) void conv_wino4w_f32(const ConvArgs a) { conv_wino4w_body<WD, NPW>(a); }

}  // namespace

// 16-channel blocks per workgroup: 4 where the output channels come in 64s -- except for exactly 64 channels on a 28x28 map, where
// 32-channel workgroups double a grid that would otherwise be 64 workgroups for 256 CUs (in context, 16 frames: 3 693 frames/s
// against 3 310 with 64-channel workgroups there)
// Eight-wave workgroups (conv_wino4w_f32): 16-channel blocks per wave, 0 = the 4-wave kernel.  GRNET_WINO_WIDE is a mask (default 1):
// bit 0 the 56x56 layers whose output channels come in 128s (upsample heads, PARE head): 480 -> 256 459 -> 357 us, 256 -> 256 264 -> 202,
// 128 -> 128 78 -> 57 at 16 frames, the step 3.71 -> 3.52 ms.  The other shapes the kernel is instantiated for were measured and stay off:
// bit 1 the 64 -> 64 layers of HR branch 1 on 28x28 maps (64 workgroups instead of 128: 18.7 us alone against 15.6, the step 3.53 -> 3.74 ms --
// the branch chains need the short launches), bit 2 the 28x28 layers with output channels in 128s (half the CUs: 95 / 51 us against 74 / 39,
// step unchanged), bit 3 the 64-channel layers on 56x56 maps (21.6 us alone against 24.2, but 3.530 -> 3.549 ms in the step).
int conv_wino4_wide(int cout, int w) {
    static const int wide_env = GRNET_AB(WINO_WIDE, 1);
    if (w == 56) return cout % 128 == 0 ? ((wide_env & 1) ? 4 : 0) : cout == 64 ? ((wide_env & 8) ? 2 : 0) : 0;
    if (w == 28) return cout % 128 == 0 ? ((wide_env & 4) ? 4 : 0) : cout == 64 ? ((wide_env & 2) ? 2 : 0) : 0;
    return 0;
}
int conv_wino4_blocks(int cout, int w) { return (cout % 64 == 0 && !(w == 28 && cout == 64 && !conv_wino4_wide(cout, w))) ? 4 : 2; }

bool conv_wino4_eligible(int cin, int cout, int ks, int stride, int h, int w, int n_add) {
    return ks == 3 && stride == 1 && ((h == 56 && w == 56) || (h == 28 && w == 28)) && n_add <= 1 && cin % kCK == 0 && cout % 32 == 0 && cin >= 32;
}

// GRNET_WINO_LDS_PAD (diagnostic): extra bytes of LDS the 4-wave launches ask for -- how sensitive the step is to the workgroups per CU
static size_t wino4_lds() {
    static const size_t pad = (size_t)GRNET_AB(WINO_LDS_PAD, 0);
    return kLdsB + pad;
}

// The launch form of layer `a` in a call of a.N frames: ONE place, read by the launchers below and by grnet_conv_launch_form.  Four-wave
// workgroups: TRG tile rows of one image x nb 16-channel blocks; eight-wave ones (conv_wino4w_f32; test hint 2003, dbg bit 5, forces the 4-wave
// kernel): npw blocks per wave.  XCD-aware workgroup order where the tile count is a multiple of the 8 XCDs; a last round of 4-wave workgroups
// that is at most half full runs as twice as many half-size workgroups (the 32-channel kernel on half a 64-channel block).
hipError_t conv_wino4_form(const ConvArgs& a, Wino4Form* f) {
    *f = Wino4Form{};
    f->nb = conv_wino4_blocks(a.Cout, a.W);
    if (!conv_wino4_eligible(a.Cin, a.Cout, a.ks, a.stride, a.H, a.W, a.n_add) || a.CinPad % kCK != 0 || a.CoutPad % (f->nb * 16) != 0) return hipErrorInvalidValue;
    if (a.n_add == 1 && a.add_shift[0] != 0) return hipErrorInvalidValue;
    const int npw = conv_wino4_wide(a.Cout, a.W);
    const bool wide = npw && a.CinPad % kCKW == 0 && a.CoutPad % (npw * 32) == 0 && !(a.dbg & 32);
    const int trg = wino4_tile_rows(a.W);                // both kernels: a workgroup is one group of 14 tiles
    f->waves = wide ? 8 : 4;
    f->npw = wide ? npw : 0;
    f->gx = a.N * (((a.H >> 2) + trg - 1) / trg);
    f->gy = a.CoutPad / (wide ? npw * 32 : f->nb * 16);
    f->xcd = f->gx % 8 == 0 && f->gx >= 16 ? 1 : 0;
    const int total = f->gx * f->gy;
    f->full = total;
    if (wide || f->nb == 2) return hipSuccess;
    static const int split_env = GRNET_AB(WINO_SPLIT, 1);
    int kCUs = 0;                                        // workgroups per round = CUs of this device (one workgroup fits a CU)
    if (hipError_t e = device_cu_count(&kCUs); e != hipSuccess) return e;
    const int full = total / kCUs * kCUs, rest = total - full;
    if (split_env && full > 0 && rest > 0 && 2 * rest <= kCUs && (!f->xcd || full % 8 == 0)) {
        f->split = 1;
        f->full = full;
        f->rest = rest;
    }
    return hipSuccess;
}

// the grid of form f in the kernel arguments: one launch, unless the caller adds the half-size last round
static void apply_form(ConvArgs& a, const Wino4Form& f, int* n_launches) {
    a.gx = f.gx;
    a.gy = f.gy;
    a.xcd = f.xcd;
    a.blk0 = 0;
    a.wsplit = 0;
    if (n_launches) *n_launches = 1;
}

template <int WD>
static hipError_t launch_wino4_w(ConvArgs a, hipStream_t s, const Wino4Form& f, int* n_launches) {
    const size_t kLdsB = wino4_lds();
    apply_form(a, f, n_launches);
    const int total = a.gx * a.gy;
#ifdef GRNET_ABLATION
    if constexpr (WD == 56) {
        if (a.dbg >= 1 && a.dbg <= 3) {
            auto go = [&](auto kern) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsB); return launch_k(kern, dim3(total), dim3(256), kLdsB, s, a); };
            if (a.dbg == 1) return go(conv_wino4_f32<4, 56, 1>);
            if (a.dbg == 2) return go(conv_wino4_f32<4, 56, 2>);
            return go(conv_wino4_f32<4, 56, 3>);
        }
    }
#endif
    if (f.nb == 2) return launch_k(conv_wino4_f32<2, WD>, dim3(total), dim3(256), kLdsB, s, a);
    if (f.split) {
        hipError_t e = launch_k(conv_wino4_f32<4, WD>, dim3(f.full), dim3(256), kLdsB, s, a);
        if (e != hipSuccess) return e;
        a.blk0 = f.full;
        a.wsplit = 1;
        if (n_launches) *n_launches = 2;
        return launch_k(conv_wino4_f32<2, WD, 0, true>, dim3(2 * f.rest), dim3(256), kLdsB, s, a);
    }
    return launch_k(conv_wino4_f32<4, WD>, dim3(total), dim3(256), kLdsB, s, a);
}

// a.w: transformed weights [36][CinPad][CoutPad] (pack_wino4_weights), CoutPad % 64 == 0 (or 32: the 32-channel variant)
hipError_t launch_conv_wino4(ConvArgs a, hipStream_t s, int* n_launches) {
    static PerDeviceOnce attr;
    int dev = 0;
    if (hipError_t e = current_device(&dev); e != hipSuccess) return e;
    if (hipError_t e = once_per_device(attr, dev, [](int*) {
            hipError_t e = hipSuccess;
            const size_t l4 = wino4_lds();
            auto set = [&](auto kern, size_t lds) { if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); };
            set(conv_wino4_f32<4, 56>, l4); set(conv_wino4_f32<2, 56>, l4); set(conv_wino4_f32<4, 28>, l4); set(conv_wino4_f32<2, 28>, l4);
            set(conv_wino4_f32<2, 56, 0, true>, l4); set(conv_wino4_f32<2, 28, 0, true>, l4);
            set(conv_wino4w_f32<56, 4>, kLdsW); set(conv_wino4w_f32<56, 2>, kLdsW); set(conv_wino4w_f32<28, 4>, kLdsW); set(conv_wino4w_f32<28, 2>, kLdsW);
            return e;
        }); e != hipSuccess) return e;
    Wino4Form f;
    if (hipError_t e = conv_wino4_form(a, &f); e != hipSuccess) return e;
    if (f.waves == 8) {
        apply_form(a, f, n_launches);
        const dim3 grid(a.gx * a.gy);
        if (a.W == 56) return f.npw == 4 ? launch_k(conv_wino4w_f32<56, 4>, grid, dim3(512), kLdsW, s, a) : launch_k(conv_wino4w_f32<56, 2>, grid, dim3(512), kLdsW, s, a);
        return f.npw == 4 ? launch_k(conv_wino4w_f32<28, 4>, grid, dim3(512), kLdsW, s, a) : launch_k(conv_wino4w_f32<28, 2>, grid, dim3(512), kLdsW, s, a);
    }
#ifdef GRNET_ABLATION
    if (GRNET_AB_SET(W4_PHASES)) {
        a.dbg |= 8;
        const hipError_t e = a.W == 56 ? launch_wino4_w<56>(a, s, f, n_launches) : launch_wino4_w<28>(a, s, f, n_launches);
        unsigned long long h[8] = {};
        abl::take_counters(HIP_SYMBOL(g_w4phase), h, s);
        const double n = h[4] ? (double)h[4] : 1.0;
        fprintf(stderr, "[wino4 phases] %d->%d @%d N%d add %d nb %d wgs %llu: per WG ticks  prologue %.0f  first transform %.0f  chunk loop %.0f (%d chunks)  epilogue %.0f\n",
                a.Cin, a.Cout, a.W, a.N, a.n_add, f.nb, h[4], h[0] / n, h[1] / n, h[2] / n, a.CinPad / kCK, h[3] / n);
        return e;
    }
#endif
    return a.W == 56 ? launch_wino4_w<56>(a, s, f, n_launches) : launch_wino4_w<28>(a, s, f, n_launches);
}

// the filter transform of F(4x4,3x3), U = G g G^T, in fp64: g (3,3) row-major -> u[i * 6 + j]
void wino4_transform_filter(const double* g, double* u) {
    static const double G[6][3] = {{1.0 / 4, 0, 0}, {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                   {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
    double t[6][3];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 3; ++j) t[i][j] = G[i][0] * g[j] + G[i][1] * g[3 + j] + G[i][2] * g[6 + j];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) u[i * 6 + j] = t[i][0] * G[j][0] + t[i][1] * G[j][1] + t[i][2] * G[j][2];
}

// U = G g G^T per (cout, cin) in fp64 -> [36][cin_pad][cout_pad] fp32; w: (cout, cin, 3, 3) folded weights (double)
void pack_wino4_weights(const double* w, int cout, int cin, int cin_pad, int cout_pad, float* out, int wid) {
    const int nb = conv_wino4_blocks(cout, wid), tc = nb * 16;              // the kernel variant launch_conv_wino4 picks for this layer
    for (size_t i = 0; i < (size_t)36 * cin_pad * cout_pad; ++i) out[i] = 0.f;
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci) {
            // within a workgroup's tc channels, channel n*16 + l sits at l*nb + n: lane l's nb MFMA B fragments are one load
            const int cpos = (co / tc) * tc + (co % 16) * nb + (co % tc) / 16;
            double u[36];
            wino4_transform_filter(w + ((size_t)co * cin + ci) * 9, u);
            for (int p = 0; p < 36; ++p) {
                if (nb == 4) out[((size_t)p * cin_pad + ci) * cout_pad + cpos] = (float)u[p];
                else {                                   // 32-channel layers: [point][chunk][k % 4][32-channel block][channel l][k-step][n]
                    const int chunk = ci / kCK, ks = (ci % kCK) / 4, kq = ci % 4;
                    out[(((size_t)p * (cin_pad / kCK) + chunk) * 4 + kq) * ((size_t)cout_pad * 2) + (co / 32) * 64 + (co % 16) * 4 + ks * 2 + (co % 32) / 16] = (float)u[p];
                }
            }
        }
}

}  // namespace grk
