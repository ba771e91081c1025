// bf16 path, round 5: a whole CHAIN of 3x3 stride-1 BasicBlocks of one HR branch (hrnet.py:30-59: conv-BN-ReLU, conv-BN, + x, ReLU;
// 4 blocks = 8 convolutions per branch and module, hrnet.py:141-187) in ONE launch with the frame resident in LDS.
//
// Why: at 256 frames the 64 ch @28x28 / 128 ch @14x14 / 256 ch @7x7 branch convolutions ran 30-31 us per launch at 0.19 of the bf16 matrix
// peak (MFMA-busy 0.24-0.27, SQ_WAIT_ANY 0.45-0.69: profiles/r04_bf16_n256_*): every launch pays a workgroup prologue, an HBM round trip
// for ~2 us of MFMAs per workgroup, an LDS epilogue and a launch boundary, 144 times per step.  All four branches of a module execute the
// SAME 57.8 MFLOP per frame, and a call of 256 frames has exactly one frame per CU.  So: workgroup = one frame, 8 waves; the frame's
// activations (50-100 KB in bf16) stay in LDS from the first convolution of the chain to the last, the weights stream L2 -> registers
// (A fragments, two k-steps ahead), HBM sees the chain's input once and its output once.
//
// LDS image: the zero-padded plane, flattened.  Slot (y, x) = (y + 1) * P + (x + 1) with row pitch P = W + 1: the right halo of row y IS the
// left halo of row y + 1 (one shared zero column), rows -1 and H are zero rows.  A slot holds the pixel's C channels (2C bytes) + 32 bytes of
// padding: slot stride = 2C + 32 bytes = 16 * m with m / 2 odd, which makes every 16-lane group of a ds_read_b128 (lanes with 16 different
// pixels, half of them on k-group q, half on q + 1: MI355X_MICROARCH, LDS table) hit 16 different 16-byte bank groups: conflict-free.
// With the flattened image a tap is a CONSTANT slot offset (dy * P + dx) for every output, so a wave's MFMA column tile is simply 16
// consecutive slots and all operand addresses are one base register + immediates.  Outputs that fall on the halo column (and past the
// plane) are computed and dropped: 811 of 816 (28x28), 209 of 224 (14x14), 55 of 64 (7x7) columns are real.
//
// Roles (as conv_bf16.hip): A[cout l&15][k = 8(l>>4)+j] = W[tap][cout][cin], B[k][pixel l&15] = slot[pixel + tap][cin], D[cout 4(l>>4)+r][pixel l&15].
// Wave (cb, pg) owns CS x 16 output channels x PS column tiles; per k-step (one tap x 32 input channels): CS weight fragments (global, 16 B
// per lane, prefetched two steps ahead in a ring of three register sets), PS pixel fragments (ds_read_b128), CS x PS MFMAs.  The tile geometry and that
// k-loop (plane_kloop) are defined once for this file, conv_bf16_wide.hip and conv_bf16_s2.hip: conv_bf16_plane.h.
//
// In place: a convolution's outputs are all held in accumulators until every wave has finished READING the plane (barrier), then written
// over it (bias, ReLU, bf16, 8 bytes per lane and tile), barrier, next convolution.  The residual of a BasicBlock costs no registers: when
// conv1's result t replaces x in a lane's slots, the lane first reads x from those very slots and seeds conv2's accumulators with
// x + bias2 -- conv2 then ends with relu(acc).  Halo slots are never written, so they stay zero for the whole chain.
//
// Parity: every intermediate is rounded to bf16 exactly where the unfused path stores it, so the chain equals the launch-per-convolution
// path up to fp32 summation order (output-rounding ties); tests/test_gpu_conv_bf16.py compares both and the fp32 oracle on bf16-rounded operands.
#include "kernels.h"
#include "device.h"
#include "conv_bf16_plane.h"

#include <cstdio>
#include <cstdlib>

namespace grk {

namespace {

// F frames per workgroup (round 6; F = 2 for the 256-channel 7x7 chain): the frames are stacked in ONE flattened plane, a zero row between them (plane rows 1 .. W:
// frame 0, W + 1: zero, W + 2 .. 2 W + 1: frame 1), so a workgroup's weight stream -- 9.4 MB per chain from L2, the bound of that chain: two single-frame workgroups
// per CU pulled 46 B/clk of the CU's 64 -- serves two frames.  The separator row is never written (the column mask below), so it stays the zero padding of both.
template <int C, int W, int F = 1>
struct ChainGeom : PlaneGeom<C, C, W, F * W + F - 1, F * W> {
    typedef PlaneGeom<C, C, W, F * W + F - 1, F * W> B;
    static constexpr int H = F * W + F - 1;                 // plane rows that carry outputs (the separator rows included)
    static constexpr int LDS = B::NSLOT * B::SB;
    static constexpr int NU = B::NUO;                       // units per thread of the plane: all of it arrives and leaves
    static_assert(LDS <= 160 * 1024, "the plane must fit the LDS");
    static_assert(F > 1 || B::IMM16, "ds_read immediates");      // (F = 2: 70 KB of plane, hipcc keeps a second base register)
};

// Registers: the 256-channel 7x7 chain (L2-bound on its weight stream, MFMA-busy 0.41) is held to 96 (five waves per SIMD; 32 bytes of scratch): two of its workgroups fit
// a CU -- 158 -> 147 us per chain alone at 256 frames -- and one fits BESIDE a workgroup of the 128-channel 14x14 chain (2 x 96 + 2 x 160 registers, 45 + 74 KB of LDS), which
// is launched on another lane at the same time.  The step did not show the latter (10.59-10.68 ms either way, three pairs on one box).
template <int C, int W, int F = 1>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(C == 256 && F == 1 ? 5 : 2))) void conv_bf16_chain(const ChainArgs a) {
    typedef ChainGeom<C, W, F> G;
    constexpr int P = G::P, SB = G::SB, CS = G::CS, PS = G::PS, UPP = G::UPP, NU = G::NU;
    extern __shared__ __align__(16) unsigned char plane[];
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cb = wave % G::WCB, pg = wave / G::WCB;
    const int n = blockIdx.x * F;                            // first frame of this workgroup; frames n .. n + nf - 1 exist
    if (n >= a.N) return;
    const int nf = a.N - n < F ? a.N - n : F;

    // ---- the frames: HBM -> registers (all loads in flight), zero the plane meanwhile, then registers -> interior slots (frame f: plane rows f (W + 1) + 1 ..)
    const u16* inb = reinterpret_cast<const u16*>(a.in) + (size_t)n * W * W * a.in_ctot + a.in_coff;
    u32x4 stage[NU];
#pragma unroll
    for (int i = 0; i < NU; ++i) {
        const int u = tid + i * 512;
        stage[i] = u32x4{0u, 0u, 0u, 0u};
        if (u < nf * W * W * UPP) {
            const int px = u / UPP, part = u - px * UPP;      // px runs over the frames: they are contiguous in memory
            stage[i] = *reinterpret_cast<const u32x4*>(inb + (size_t)px * a.in_ctot + part * 8);
        }
    }
    for (int u = tid; u < G::LDS / 16; u += 512) reinterpret_cast<u32x4*>(plane)[u] = u32x4{0u, 0u, 0u, 0u};
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NU; ++i) {
        const int u = tid + i * 512;
        if (u < nf * W * W * UPP) {
            const int px = u / UPP, part = u - px * UPP, f = px / (W * W), pf = px - f * W * W, y = pf / W, x = pf - y * W;
            *reinterpret_cast<u32x4*>(plane + ((f * (W + 1) + y + 1) * P + x + 1) * SB + part * 16) = stage[i];
        }
    }

    // ---- per-lane constants
    const int o_first = G::O0 + pg * PS * 16 + l15;                          // this lane's output column of tile 0
    const unsigned char* bread = plane + (o_first - P - 1) * SB + lq * 16;    // B operand of tap (0,0), chunk 0, tile 0
    unsigned char* owrite = plane + o_first * SB + (cb * CS * 16 + lq * 4) * 2;      // this lane's 4 channels of tile 0, block 0
    unsigned valid = 0;                                                       // bit ps: column tile ps of this lane is a real pixel
#pragma unroll
    for (int ps = 0; ps < PS; ++ps) {
        const int o = o_first + ps * 16, row = o / P;      // plane row 1 .. H; rows that are a multiple of W + 1 separate two frames
        if (o % P != 0 && o <= G::H * P + W && row % (W + 1) != 0 && (row - 1) / (W + 1) < nf) valid |= 1u << ps;
    }
    const unsigned wlb = ((cb * CS * 16 + l15) * 32 + lq * 8) * 2;           // byte offset of this lane in a [C][32] weight row block
    const int co = cb * CS * 16 + lq * 4;                                     // first of this lane's 4 output channels (block 0)

    f32x4 acc[CS][PS];
    {
        const float* b0 = a.bias[0];
#pragma unroll
        for (int cs = 0; cs < CS; ++cs) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(b0 + co + cs * 16);
#pragma unroll
            for (int ps = 0; ps < PS; ++ps) acc[cs][ps] = bv;
        }
    }
    // weight fragments of k-step s: element offset (s * C + cs * 16) * 32 from the lane's base; the ring starts with steps 0 .. RING - 2
    constexpr int RING = 3;                                 // (9 for the 256-channel chain, k-steps of 8 MFMAs: 150 us against 145 -- its weight stream is bound by the CU's 64 B/clk vector-memory path, not by latency)
    bf16x8 wr[RING][CS];
    {
        const unsigned char* w0 = reinterpret_cast<const unsigned char*>(a.w[0]);
#pragma unroll
        for (int st = 0; st < RING - 1; ++st)
#pragma unroll
            for (int cs = 0; cs < CS; ++cs) wr[st][cs] = *reinterpret_cast<const bf16x8*>(w0 + (st * C + cs * 16) * 64 + wlb);
    }
    __syncthreads();                                                          // the plane is staged

    for (int ci = 0; ci < a.nconv; ++ci) {
        const u16* wc = reinterpret_cast<const u16*>(a.w[ci]);
        const int cn = ci + 1 < a.nconv ? ci + 1 : ci;                        // the last convolution re-requests itself (nobody waits for it)
        const u16* wn = reinterpret_cast<const u16*>(a.w[cn]);
        plane_kloop<G, CS, PS, RING>(acc, wr, bread, wc, wn, (size_t)C * 32, C / 32, true, wlb);
        // ---- in-place epilogue
        const bool first = (ci & 1) == 0;                                     // conv1 of a BasicBlock: the plane still holds the block's input x
        f32x4 bnext[CS];
#pragma unroll
        for (int cs = 0; cs < CS; ++cs) bnext[cs] = *reinterpret_cast<const f32x4*>(a.bias[cn] + co + cs * 16);
        __syncthreads();                                                      // every wave has read what it needs of the plane
#pragma unroll
        for (int ps = 0; ps < PS; ++ps)
#pragma unroll
            for (int cs = 0; cs < CS; ++cs) {
                unsigned char* pos = owrite + ps * 16 * SB + cs * 32;
                u32x2 r = u32x2{0u, 0u};
                if (first) r = *reinterpret_cast<const u32x2*>(pos);
                const u32x2 pk = pack4_relu(acc[cs][ps]);
                if (valid & (1u << ps)) *reinterpret_cast<u32x2*>(pos) = pk;
                f32x4 nx = bnext[cs];
                if (first) { nx[0] += bf_lo(r[0]); nx[1] += bf_hi(r[0]); nx[2] += bf_lo(r[1]); nx[3] += bf_hi(r[1]); }
                acc[cs][ps] = nx;
            }
        __syncthreads();                                                      // the plane holds this convolution's output
    }

    // ---- the chain's output: interior slots -> HBM, 16 bytes per lane, pixels in memory order
    u16* outb = reinterpret_cast<u16*>(a.out) + (size_t)n * W * W * a.out_ctot + a.out_coff;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
        const int u = tid + i * 512;
        if (u < nf * W * W * UPP) {
            const int px = u / UPP, part = u - px * UPP, f = px / (W * W), pf = px - f * W * W, y = pf / W, x = pf - y * W;
            *reinterpret_cast<u32x4*>(outb + (size_t)px * a.out_ctot + part * 8) = *reinterpret_cast<const u32x4*>(plane + ((f * (W + 1) + y + 1) * P + x + 1) * SB + part * 16);
        }
    }
}


// ---- ONE BasicBlock of the 32-channel 56x56 branch with a BAND of the frame resident in LDS (a whole 56x56x32 frame is 200 KB: it does not fit).
// The plane of a band of R output rows: input rows y0 - 2 .. y0 + R + 1 (rows outside the image are zero) in the flattened, pitch-57 image of the chain
// kernel; conv1 on rows y0 - 1 .. y0 + R (its rows outside the image are conv2's zero padding: not written, the slots keep their zeros), in place; conv2
// reads them; rows y0 .. y0 + R - 1 -> HBM.  (A kernel with the workgroup = one band, one or two per CU, measured 51-53 us per block against 43 for the
// frame-persistent kernel below: NOTES_rejected.md.)
template <int C, int W, int R>
struct BandGeom : PlaneGeom<C, C, W, R + 2, R> {            // outputs on plane rows 1 .. R + 2 (conv1's)
    typedef PlaneGeom<C, C, W, R + 2, R> B;
    static constexpr int ROWS = R + 4;                      // plane rows: image rows y0 - 2 .. y0 + R + 1
    static constexpr int LDS = B::NSLOT * B::SB;
    static_assert(LDS <= 160 * 1024 && B::NSLOT >= ROWS * B::P + 1, "band geometry");
    static_assert(B::IMM16, "ds_read immediates");
};

// ---- The same block with the WORKGROUP = ONE FRAME walking its NB = 56 / R bands, the next band arriving by LDS-DMA under the current band's MFMAs.
// A workgroup per band spends two thirds of its life in its load and store phases (one workgroup per CU: nothing overlaps them; 51 us
// per BasicBlock at 256 frames against 11.8 us of MFMAs at peak and 22 us of HBM time).  A first persistent version kept the next band in
// registers (R = 14): 256 VGPRs + 160-284 bytes of scratch, and hipcc parked the prefetched rows in scratch right behind their loads, i.e.
// waited for them -- no overlap.  So the prefetch takes no registers at all:
//   * the next band's rows travel HBM -> LDS by LDS-DMA into a dense staging area (lane-linear, as the DMA writes) and are copied LDS -> LDS
//     into the padded plane when the current band has left;
//   * vmcnt is in order, and a wave that waits for a weight fragment would wait for every DMA it issued before: the weights of BOTH
//     convolutions (36 KB for C = 32) live in LDS for the whole launch, so the k-loops issue no vector-memory operation at all and the DMAs
//     fly through them.  Weight rows are 64 bytes (no room for padding): the 16-byte part p of row r sits at p ^ 2 (r >> 3 & 1), which puts the
//     16 lanes of every ds_read_b128 group (rows {0-3, 12-15} at part q, rows {4-11} at part q + 1, or the mirror image) on 16 different bank groups;
//   * barriers are raw s_barrier + lgkmcnt(0): __syncthreads() would drain the DMAs (a pending DMA is a pending LDS write to its fence).
// LDS: weights 36 KB + plane (R = 8: 12 rows, 72.7 KB) + staging (12 x 56 x 64 B = 43 KB) = 152 KB.  R = 8 tiles the 56 rows exactly (7 bands);
// 10 of 12 plane rows carry outputs of conv1, 8 of conv2's, 569 of 640 MFMA columns are real: 0.72 of the MFMAs are useful, HBM reads 1.5 x the input.


// k-loop of one 32 -> 32 convolution with the weights in LDS: per tap CS weight fragments (one tap ahead, two register sets) and PS pixel fragments
// (ring as in plane_kloop); no vector-memory operation.  wl: this lane's fragment of tap 0, block 0 (swizzled part); 2 KB per tap, 1 KB per block.
template <int P, int SB, int CS, int PS>
__device__ __forceinline__ void chain_kloop_ldsw(f32x4 (&acc)[CS][PS], const unsigned char* bread, const unsigned char* wl) {
    bf16x8 bfr[PS], wr[2][CS];
#pragma unroll
    for (int cs = 0; cs < CS; ++cs) wr[0][cs] = *reinterpret_cast<const bf16x8*>(wl + cs * 1024);
#pragma unroll
    for (int ps = 0; ps < PS; ++ps) bfr[ps] = *reinterpret_cast<const bf16x8*>(bread + ps * 16 * SB);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        if (tap < 8) {
#pragma unroll
            for (int cs = 0; cs < CS; ++cs) wr[(tap + 1) & 1][cs] = *reinterpret_cast<const bf16x8*>(wl + (tap + 1) * 2048 + cs * 1024);
        }
        const int noff = (((tap + 1) / 3) * P + ((tap + 1) % 3)) * SB;
#pragma unroll
        for (int ps = 0; ps < PS; ++ps) {
#pragma unroll
            for (int cs = 0; cs < CS; ++cs) acc[cs][ps] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[tap & 1][cs], bfr[ps], acc[cs][ps], 0, 0, 0);
            if (tap < 8) bfr[ps] = *reinterpret_cast<const bf16x8*>(bread + ps * 16 * SB + noff);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

template <int W, int R>
struct FrameGeom {
    static constexpr int C = 32;
    typedef BandGeom<C, W, R> B;
    static constexpr int WBYTES = 2 * 9 * C * 64;            // both convolutions' weights, 64-byte rows
    static constexpr int PLANE = B::LDS;
    static constexpr int UR = W * B::UPP;                     // 16-byte units per row
    static constexpr int STAGE_UNITS = B::ROWS * UR;
    static constexpr int LDS = WBYTES + PLANE + STAGE_UNITS * 16;
    static constexpr int NUS = (STAGE_UNITS + 511) / 512, NUO = (R * UR + 511) / 512;
    static_assert(W % R == 0 && LDS <= 160 * 1024 && PLANE % 16 == 0, "frame geometry");
};

template <int W, int R>
__global__ __launch_bounds__(512) void conv_bf16_block_frame(const ChainArgs a) {
    constexpr int C = 32;
    typedef BandGeom<C, W, R> G;
    typedef FrameGeom<W, R> F;
    constexpr int P = G::P, SB = G::SB, CS = G::CS, PS = G::PS, UPP = G::UPP, NB = G::NB, UR = F::UR;
    static_assert(G::WCB == 1, "one channel block of 32");
    extern __shared__ __align__(16) unsigned char lds[];
    unsigned char* wlds = lds;                                 // [conv][tap][row 32][4 parts, swizzled] bf16
    unsigned char* plane = lds + F::WBYTES;
    unsigned char* stg = plane + F::PLANE;                     // [plane row][x][4 parts]: the NEXT band, as it lies in memory
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = blockIdx.x;
    if (n >= a.N) return;
    const u16* inb = reinterpret_cast<const u16*>(a.in) + (size_t)n * W * W * a.in_ctot + a.in_coff;
    u16* outb = reinterpret_cast<u16*>(a.out) + (size_t)n * W * W * a.out_ctot + a.out_coff;

    // (round 5) unit i of this thread = (plane row r, column x, 16-byte part) is the same in every band: kept packed (r : 4 | x : 6 | part : 2 bits, two units per
    // register) instead of two divisions per unit and band in request() and again in deposit()
    unsigned upk[(F::NUS + 1) / 2];
#pragma unroll
    for (int i = 0; i < (F::NUS + 1) / 2; ++i) upk[i] = 0u;
#pragma unroll
    for (int i = 0; i < F::NUS; ++i) {
        const int u = i * 512 + tid, r = u / UR, q = u - r * UR, x = q / UPP, part = q - x * UPP;
        upk[i >> 1] |= (unsigned)((r << 8) | (x << 2) | part) << (16 * (i & 1));
    }
    auto request = [&](int y0) {                               // rows y0 - 2 .. y0 + R + 1 that exist -> staging, by LDS-DMA (rows outside the image are not requested)
#pragma unroll
        for (int i = 0; i < F::NUS; ++i) {
            const int ub = i * 512 + wave * 64, u = ub + lane;
            const unsigned pk = upk[i >> 1] >> (16 * (i & 1));
            const int r = (pk >> 8) & 15, x = (pk >> 2) & 63, part = pk & 3, y = y0 - 2 + r;
            if (u < F::STAGE_UNITS && y >= 0 && y < W) dma16_builtin(inb + ((size_t)y * W + x) * a.in_ctot + part * 8, stg + ub * 16);
        }
    };
    auto deposit = [&](int y0) {                               // staging -> interior slots of every plane row; zeros where the band hangs over the image
#pragma unroll
        for (int i = 0; i < F::NUS; ++i) {
            const int u = i * 512 + tid;
            const unsigned pk = upk[i >> 1] >> (16 * (i & 1));
            const int r = (pk >> 8) & 15, x = (pk >> 2) & 63, part = pk & 3, y = y0 - 2 + r;
            if (u < F::STAGE_UNITS) {
                u32x4 v = u32x4{0u, 0u, 0u, 0u};
                if (y >= 0 && y < W) v = *reinterpret_cast<const u32x4*>(stg + u * 16);
                *reinterpret_cast<u32x4*>(plane + (r * P + x + 1) * SB + part * 16) = v;
            }
        }
    };
    request(0);
    {   // the weights: global -> registers -> LDS (swizzled); the plane's halo columns and spare slots: zero, once
        constexpr int WU = 2 * 9 * C * 4, NWU = (WU + 511) / 512;      // 16-byte units of both convolutions
        u32x4 wv[NWU];
#pragma unroll
        for (int i = 0; i < NWU; ++i) {
            const int v = i * 512 + tid, cv = v / (WU / 2), vv = v - cv * (WU / 2);
            wv[i] = u32x4{0u, 0u, 0u, 0u};
            if (v < WU) wv[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned char*>(a.w[cv]) + vv * 16);
        }
        for (int u = tid; u < F::PLANE / 16; u += 512) reinterpret_cast<u32x4*>(plane)[u] = u32x4{0u, 0u, 0u, 0u};
        // (round 6) the 32 output-channel rows of a tap are PERMUTED on the way in: channel c = 8 q + 4 s + r goes to row s * 16 + 4 q + r, so that lane (pixel, lq) of the
        // two MFMA blocks s = 0, 1 ends up with channels 8 lq .. 8 lq + 3 and 8 lq + 4 .. 8 lq + 7 -- EIGHT consecutive channels: the in-place epilogue, the conv2 seeds and
        // the output stores move 16 bytes per lane and tile instead of two times 8 (the stores were 8.7 of a launch's 50 us as 32-byte pieces: profiles/r06_block_frame_ablation.txt).
        // Every output's dot product is unchanged: bit-identical results.  (The same assignment in the frame-resident chain kernels, whose epilogues are a smaller share of
        // their launches, measured no change: 103.4 / 107.2 / 174 us per chain against 103.4 / 107.7 / 168.5 -- not kept there.)
#pragma unroll
        for (int i = 0; i < NWU; ++i) {
            const int v = i * 512 + tid, c = (v >> 2) & 31, part = v & 3;
            const int row = ((c >> 2) & 1) * 16 + 4 * (c >> 3) + (c & 3);
            if (v < WU) *reinterpret_cast<u32x4*>(wlds + ((v >> 7) * 32 + row) * 64 + ((part ^ (((row >> 3) & 1) << 1)) * 16)) = wv[i];
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's DMAs of band 0 have landed
    lds_barrier();                                             // ... and everybody's; the plane is zero, the weights are in place
    deposit(0);
    lds_barrier();                                             // staging is free, the plane holds band 0
    const int o_first = G::O0 + wave * PS * 16 + l15;
    const unsigned char* bread = plane + (o_first - P - 1) * SB + lq * 16;
    unsigned char* owrite = plane + o_first * SB + lq * 16;       // this lane's 8 channels (8 lq ..) of column tile 0
    const unsigned char* wl0 = wlds + l15 * 64 + ((lq ^ (((l15 >> 3) & 1) << 1)) * 16);
    const unsigned char* wl1 = wl0 + 9 * C * 64;
    const int co = lq * 8;                                        // MFMA block cs holds channels co + 4 cs .. + 3 of this lane's pixel
    // conv2 needs rows 2 .. R + 1 of the plane only (conv1: rows 1 .. R + 2): its own, shorter tile run -- PS2 = 4 column tiles per wave from slot 2 P + 1 on
    // instead of conv1's PS = 5 from P + 1 on (a fifth of conv2's MFMAs and fragment reads computed rows nobody stores)
    constexpr int NOUT2 = R * P - 1, PS2 = ((NOUT2 + 15) / 16 + 7) / 8;
    const int o2_first = 2 * P + 1 + wave * PS2 * 16 + l15;
    const unsigned char* bread2 = plane + (o2_first - P - 1) * SB + lq * 16;
    f32x4 b1[CS], b2[CS];
#pragma unroll
    for (int cs = 0; cs < CS; ++cs) {
        b1[cs] = *reinterpret_cast<const f32x4*>(a.bias[0] + co + cs * 4);
        b2[cs] = *reinterpret_cast<const f32x4*>(a.bias[1] + co + cs * 4);
    }
    if (NB > 1) request(R);                                    // behind the bias loads: waiting for those must not mean waiting for these
    const bool direct_store = !(a.flags & 1);

#pragma unroll 1
    for (int band = 0; band < NB; ++band) {
        const int y0 = band * R;
        unsigned valid1 = 0, valid2 = 0;
#pragma unroll
        for (int ps = 0; ps < PS; ++ps) {
            const int o = o_first + ps * 16, r = o / P, y = y0 - 2 + r;
            const bool px_ok = o - r * P != 0 && r >= 1 && r <= R + 2 && y >= 0 && y < W;
            if (px_ok) valid1 |= 1u << ps;
            if (px_ok && r >= 2 && r <= R + 1) valid2 |= 1u << ps;
        }
        f32x4 acc[CS][PS];
#pragma unroll
        for (int cs = 0; cs < CS; ++cs)
#pragma unroll
            for (int ps = 0; ps < PS; ++ps) acc[cs][ps] = b1[cs];
        if (!abl::bit(a.flags, 16))
        chain_kloop_ldsw<P, SB, CS, PS>(acc, bread, wl0);
        if (direct_store) {
            // conv2's accumulators start from x + bias2, read at conv2's OWN columns while the plane still holds x (nobody has written yet)
            f32x4 acc2[CS][PS2];
            unsigned v2 = 0;
#pragma unroll
            for (int ps = 0; ps < PS2; ++ps) {
                const int o = o2_first + ps * 16, r = o / P, y = y0 - 2 + r;
                if (o - r * P != 0 && r >= 2 && r <= R + 1 && y >= 0 && y < W) v2 |= 1u << ps;
                const u32x4 rr = *reinterpret_cast<const u32x4*>(plane + (o2_first + ps * 16) * SB + lq * 16);
#pragma unroll
                for (int cs = 0; cs < CS; ++cs) {
                    f32x4 nx = b2[cs];
                    nx[0] += bf_lo(rr[2 * cs]); nx[1] += bf_hi(rr[2 * cs]); nx[2] += bf_lo(rr[2 * cs + 1]); nx[3] += bf_hi(rr[2 * cs + 1]);
                    acc2[cs][ps] = nx;
                }
            }
            lds_barrier();                                     // every wave has read what it needs of x
#pragma unroll
            for (int ps = 0; ps < PS; ++ps) {
                const f32x4 A = acc[0][ps], B = acc[1][ps];
                if (valid1 & (1u << ps)) *reinterpret_cast<u32x4*>(owrite + ps * 16 * SB) = u32x4{pack2(relu_bits(A[0]), relu_bits(A[1])), pack2(relu_bits(A[2]), relu_bits(A[3])), pack2(relu_bits(B[0]), relu_bits(B[1])), pack2(relu_bits(B[2]), relu_bits(B[3]))};
            }
            lds_barrier();
            if (!abl::bit(a.flags, 32))
            chain_kloop_ldsw<P, SB, CS, PS2>(acc2, bread2, wl1);
            // the block's output rows leave straight from the accumulators (round 5: was in place through the plane, a barrier, then 16-byte stores): 8 bytes per lane, the
            // four k-groups of a pixel make 32 contiguous bytes, the two channel blocks its 64-byte row; nothing of this band's output is needed in LDS again.
            // The next band's DMAs (issued a whole band ago) and the previous band's stores are the only vector-memory operations in flight: waited for HERE, in front of
            // this band's stores (round-5 advice: a counted wait behind them assumed CS x PS2 stores per wave, but the stores are predicated -- the wave that owns the
            // column tiles past the band issues fewer, and its DMAs could then still be in flight when deposit() reads the staging area)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int ps = 0; ps < PS2; ++ps) {
                int of = o2_first;
                asm volatile("" : "+v"(of));                   // (tile-independent pixel offsets: not to be hoisted out of the band loop into 2 x PS registers)
                const int o = of + ps * 16, r = o / P, x = o - r * P - 1;
                u16* op = outb + ((size_t)(y0 + r - 2) * W + x) * a.out_ctot + lq * 8;
                const f32x4 A = acc2[0][ps], B = acc2[1][ps];
                if (v2 & (1u << ps)) *reinterpret_cast<u32x4*>(op) = u32x4{pack2(relu_bits(A[0]), relu_bits(A[1])), pack2(relu_bits(A[2]), relu_bits(A[3])), pack2(relu_bits(B[0]), relu_bits(B[1])), pack2(relu_bits(B[2]), relu_bits(B[3]))};       // 16 bytes per lane: a pixel's 64-byte row by four lanes
            }
        } else {
        lds_barrier();
#pragma unroll
        for (int ps = 0; ps < PS; ++ps)
#pragma unroll
            for (int cs = 0; cs < CS; ++cs) {
                unsigned char* pos = owrite + ps * 16 * SB + cs * 8;
                const u32x2 r = *reinterpret_cast<const u32x2*>(pos);
                const f32x4 v = acc[cs][ps];
                if (valid1 & (1u << ps)) *reinterpret_cast<u32x2*>(pos) = u32x2{pack2(relu_bits(v[0]), relu_bits(v[1])), pack2(relu_bits(v[2]), relu_bits(v[3]))};
                f32x4 nx = b2[cs];
                nx[0] += bf_lo(r[0]); nx[1] += bf_hi(r[0]); nx[2] += bf_lo(r[1]); nx[3] += bf_hi(r[1]);
                acc[cs][ps] = nx;
            }
        lds_barrier();
        chain_kloop_ldsw<P, SB, CS, PS>(acc, bread, wl1);
        lds_barrier();
#pragma unroll
        for (int ps = 0; ps < PS; ++ps)
#pragma unroll
            for (int cs = 0; cs < CS; ++cs) {
                const f32x4 v = acc[cs][ps];
                if (valid2 & (1u << ps))
                    *reinterpret_cast<u32x2*>(owrite + ps * 16 * SB + cs * 8) = u32x2{pack2(relu_bits(v[0]), relu_bits(v[1])), pack2(relu_bits(v[2]), relu_bits(v[3]))};
            }
        // the next band's DMAs (issued a whole band ago) and the previous band's stores are the only vector-memory operations in flight: wait for
        // them HERE, in front of this band's stores, so that the wait does not include those stores' round trip
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        lds_barrier();                                         // the band's rows are in the plane; the next band is in staging
#pragma unroll
        for (int i = 0; i < F::NUO; ++i) {
            const int u = i * 512 + tid, r = u / UR, q = u - r * UR, x = q / UPP, part = q - x * UPP;
            if (u < R * UR)
                *reinterpret_cast<u32x4*>(outb + ((size_t)(y0 + r) * W + x) * a.out_ctot + part * 8) = *reinterpret_cast<const u32x4*>(plane + ((r + 2) * P + x + 1) * SB + part * 16);
        }
        }
        if (band + 1 < NB) {
            lds_barrier();                                     // the band's rows have been read out of the plane
            if (!abl::bit(a.flags, 64))
            deposit(y0 + R);
            lds_barrier();                                     // staging is free, the plane holds the next band
            if (band + 2 < NB) request(y0 + 2 * R);
        }
    }
}

// ---- The whole 32-channel 56x56 chain (HR branch 0 of a module: 4 BasicBlocks = 8 convolutions, hrnet.py:141-187) as ONE launch: a PIPELINE OF ROWS.
// conv_bf16_block_frame above is bound by its per-band skeleton (57 % of a launch is not the k-loops: profiles/r06_block_frame_ablation.txt) and pays it once per
// BasicBlock.  Here a workgroup owns a frame and each of its 8 waves owns ONE convolution of the chain for the whole launch:
//   * the wave's weights (9 taps x 32 x 32 bf16 = 18 KB) live in its REGISTERS (72 per lane: the A fragments of all 18 (tap, channel block) MFMAs), loaded once;
//   * in step t wave s computes output row t - 2 s of its convolution (4 column tiles x 2 channel blocks x 9 taps = 72 MFMAs) from three rows of its input ring in LDS
//     and leaves the row -- ReLU, bf16 -- in the input ring of wave s + 1 (the last wave stores to HBM); conv2 of a block seeds its accumulators with bias + x from
//     the ring its conv1 reads (the block's input row).  A lag of two rows per stage keeps producer and consumers of a ring on different rows within a step, so ONE
//     barrier per step is all the synchronisation there is; no wave ever waits for weights, addresses are one base + immediates;
//   * rings: 6 rows for the chain's input (arrives by LDS-DMA three steps ahead, one wave-instruction per step from each of waves 0 .. 3), 5 for a block's input
//     (its conv1 reads rows r - 1 .. r + 1 while conv2, two steps behind, still takes row r - 2 as the residual), 4 between conv1 and conv2: 37 rows of 4 KB = 148 KB;
//   * a ring row is 64 slots of 64 bytes (pixel x in slot x + 1, slots 0 and 57 .. 63 zero): no padding between pixels, the 16-byte part p of slot q sits at
//     p ^ 2 (q >> 2 & 1), which puts the 16 lanes of every ds_read_b128 group on 16 different bank groups for every tile start and tap.
// 74 steps per frame (56 rows + 14 of pipeline + 4 of input lead); results bit-identical to the launch-per-block kernels (same seeds, same tap order, same rounding
// points).  HBM sees the chain's input once and its output once (the three intermediates between blocks no longer exist).
struct PipeGeom {
    static constexpr int W = 56, C = 32, NS = 8, ROWB = 4096, TILES = 4;
    static constexpr int ROWS = 6 + 4 * 4 + 3 * 5;             // ring 0: 6 rows; rings 1, 3, 5, 7: 4; rings 2, 4, 6: 5
    static constexpr int LDS = ROWS * ROWB + 512;             // + the two slots a tile's right-most taps reach past the last row
    static_assert(ROWS == 37 && LDS <= 160 * 1024, "ring layout");
};

#ifdef GRNET_ABLATION
__device__ unsigned long long g_pipe_phase[8 * 4];            // diagnostic builds, GRNET_PIPE_PHASES: clock ticks per wave: request / compute + store / DMA wait / barrier
#endif
__global__ __launch_bounds__(512) void conv_bf16_chain_pipe(const ChainArgs a) {
    typedef PipeGeom G;
    constexpr int W = G::W;
    extern __shared__ __align__(16) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // waves w and w + 4 share a SIMD: they get conv1 and conv2 of the same block, whose steps are COMPLEMENTARY (below)
    const int s = wv < 4 ? 2 * wv : 2 * (wv - 4) + 1;         // this wave's convolution
    const int n = blockIdx.x;
    if (n >= a.N) return;
    const u16* inb = reinterpret_cast<const u16*>(a.in) + (size_t)n * W * W * a.in_ctot + a.in_coff;
    u16* outb = reinterpret_cast<u16*>(a.out) + (size_t)n * W * W * a.out_ctot + a.out_coff;
    const bool last = s == G::NS - 1, second = (s & 1) != 0;

    // A fragments of this wave's convolution: lane (row i = l15, k group lq) of channel block cs holds W[tap][channel 8 (i >> 2) + 4 cs + (i & 3)][8 lq .. 8 lq + 7]
    // (the row permutation of conv_bf16_block_frame: a lane's two accumulator blocks are the pixel's channels 8 lq .. 8 lq + 7)
    bf16x8 wf[9][2];
    f32x4 bias[2];
    {
        const u16* wsrc = reinterpret_cast<const u16*>(a.w[s]);
        const float* bsrc = a.bias[s];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int cs = 0; cs < 2; ++cs) wf[tap][cs] = *reinterpret_cast<const bf16x8*>(wsrc + ((size_t)tap * 32 + 8 * (l15 >> 2) + 4 * cs + (l15 & 3)) * 32 + 8 * lq);
#pragma unroll
        for (int cs = 0; cs < 2; ++cs) bias[cs] = *reinterpret_cast<const f32x4*>(bsrc + 8 * lq + 4 * cs);
    }
    for (int u = tid; u < G::LDS / 16; u += 512) reinterpret_cast<u32x4*>(lds)[u] = u32x4{0u, 0u, 0u, 0u};
    // ring k = the input of convolution k; this wave reads ring s (+ ring s - 1, the block's input, for the residual of a second convolution), writes ring s + 1
    auto first_of = [](int k) { return k == 0 ? 0 : 6 + ((k - 1) >> 1) * 9 + (((k - 1) & 1) ? 4 : 0); };      // rings 1, 2, 3, ... = 4, 5, 4, 5, ... rows behind ring 0's 6
    auto rows_of = [](int k) { return k == 0 ? 6 : (k & 1) ? 4 : 5; };
    const int f_in = first_of(s), n_in = rows_of(s), f_res = first_of(s > 0 ? s - 1 : 0), n_res = rows_of(s > 0 ? s - 1 : 0), f_out = first_of(s + 1), n_out = rows_of(s + 1);
    // lane offsets inside a ring row for tap column dx: slot 16 j + l15 + dx, part lq swizzled by the slot's bit 2 (16 j leaves that bit alone)
    unsigned off[3];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) off[dx] = (unsigned)((l15 + dx) * 64 + ((lq ^ ((((l15 + dx) >> 2) & 1) << 1)) * 16));
    // the chain's input, one wave-instruction of a row per step from waves 0 .. 3: unit d = 64 wv + lane of the row = (slot d >> 2, swizzled part d & 3)
    const int dslot = (64 * wv + lane) >> 2, dpart = ((64 * wv + lane) & 3) ^ (((dslot >> 2) & 1) << 1);
    const bool dma_lane = wv < 4 && dslot >= 1 && dslot <= W;
    // The piece is inline asm hipcc does not know of (dma16_masked: uniform row base + 32-bit lane offset, EXEC = the row's real units): with an LDS-DMA it DOES know
    // of in the loop, every wait in front of a fragment's MFMAs is lgkmcnt(0) -- the younger reads included; without, the waits are counted (lgkmcnt(7): one read
    // back of eight).  Its landing is awaited explicitly (vmcnt below, then the step's barrier), as before.
    const unsigned dlane = dma_lane ? (unsigned)(((dslot - 1) * a.in_ctot + dpart * 8) * 2) : 0u;
    const unsigned long long dmask = __ballot(dma_lane);
    const unsigned lds0 = (unsigned)(size_t)lds;
    auto request = [&](int y, int i_row) {                     // row y of the input -> ring 0 (rows outside the image stay zero: the ring starts zeroed, row 56's slot is zeroed below)
        dma16_masked(dlane, reinterpret_cast<const unsigned char*>(inb) + (size_t)y * W * a.in_ctot * 2, lds0 + (unsigned)(i_row * G::ROWB + wv * 1024), dmask);
    };
    f32x4 acc[2][4];
    // row r of this wave's convolution into acc: bias (+ the block's input row r for a second convolution), 9 taps x 4 column tiles x 2 channel blocks
    // ring rows of this step's image rows, kept as counters that wrap (a modulo by a per-wave ring size costs ~40 scalar instructions, six times a step):
    // i_in: row r - 1 in the input ring, i_res: row r in the residual ring, i_out: row r in the output ring, i_dma: row t + 3 in ring 0
    int i_in = 0, i_res = 0, i_out = 0, i_dma = 0;
    auto wrap = [](int i, int nrows) { return i >= nrows ? i - nrows : i; };
    auto compute_row = [&](int r) {
        (void)r;
        if (abl::bit(a.flags, 64)) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { acc[0][j] = bias[0]; acc[1][j] = bias[1]; }
        } else if (second) {
            const unsigned char* xr = lds + (f_res + i_res) * G::ROWB + off[1];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const u32x4 rr = *reinterpret_cast<const u32x4*>(xr + j * 1024);
#pragma unroll
                for (int cs = 0; cs < 2; ++cs) {
                    f32x4 nx = bias[cs];
                    nx[0] += bf_lo(rr[2 * cs]); nx[1] += bf_hi(rr[2 * cs]); nx[2] += bf_lo(rr[2 * cs + 1]); nx[3] += bf_hi(rr[2 * cs + 1]);
                    acc[cs][j] = nx;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) { acc[0][j] = bias[0]; acc[1][j] = bias[1]; }
        }
        if (abl::bit(a.flags, 16)) return;
        const unsigned char* rb[3];
        rb[0] = lds + (f_in + i_in) * G::ROWB;
        rb[1] = lds + (f_in + wrap(i_in + 1, n_in)) * G::ROWB;
        rb[2] = lds + (f_in + wrap(i_in + 2, n_in)) * G::ROWB;
        // pixel fragments as a ring of two sets: fragment j of tap t + 2 is requested right behind the two MFMAs that consumed fragment j of tap t (16 MFMAs = 256
        // cycles ahead of its use), so every wait in front of an MFMA pair is for ONE read with seven younger ones in flight
        bf16x8 px[2][4];
#pragma unroll
        for (int pre = 0; pre < 2; ++pre)
#pragma unroll
            for (int j = 0; j < 4; ++j) px[pre][j] = *reinterpret_cast<const bf16x8*>(rb[0] + off[pre] + j * 1024);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[tap][0], px[tap & 1][j], acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[tap][1], px[tap & 1][j], acc[1][j], 0, 0, 0);
                if (tap + 2 < 9) px[tap & 1][j] = *reinterpret_cast<const bf16x8*>(rb[(tap + 2) / 3] + off[(tap + 2) % 3] + j * 1024);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    // acc (row r) -> ReLU, bf16 -> ring s + 1 (the last convolution: HBM); zero: the padding rows -1 and 56 of the next convolution's input
    auto store_row = [&](int r, int i_row, bool zero) {            // i_row: ring row of image row r in the output ring
        if (abl::bit(a.flags, 32)) return;
        unsigned char* orow = lds + (f_out + i_row) * G::ROWB + off[1];
        if (zero) {
            if (!last) {
#pragma unroll
                for (int j = 0; j < 4; ++j) *reinterpret_cast<u32x4*>(orow + j * 1024) = u32x4{0u, 0u, 0u, 0u};
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // round to bf16, THEN clamp at zero on the packed halves (v_pk_max_i16: a negative bf16 is a negative 16-bit integer, -0 included) -- the bits of
            // relu-then-round (rounding keeps the sign) in 8 vector instructions per tile instead of 12
            const f32x4 A = acc[0][j], B = acc[1][j];
            u32x4 v = u32x4{relu_pk(pack2(A[0], A[1])), relu_pk(pack2(A[2], A[3])), relu_pk(pack2(B[0], B[1])), relu_pk(pack2(B[2], B[3]))};
            const int x = 16 * j + l15;
            if (last) {
                if (j < 3 || x < W) *reinterpret_cast<u32x4*>(outb + ((size_t)r * W + x) * a.out_ctot + lq * 8) = v;
            } else {
                if (j == 3 && x >= W) v = u32x4{0u, 0u, 0u, 0u};     // slots 57 .. 64 (the right halo, the spare slots, the next row's left halo) stay zero
                *reinterpret_cast<u32x4*>(orow + j * 1024) = v;
            }
        }
    };
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // weights and bias are in registers (nothing else of this wave's is in flight from here on but DMAs and stores)
    lds_barrier();                                             // the rings are zero
    // Schedule.  Convolution s works on row t - c(s) in step t, c = 0, 2, 5, 7, 10, 12, 15, 17: a first convolution computes its row and stores it in the same step
    // (matrix pipe, then vector ALU); a second convolution stores the row of the PREVIOUS step first, then seeds and computes the next (vector ALU, then matrix
    // pipe) -- the two waves of a SIMD are in opposite phases.  A second convolution's row therefore appears one step later, and the next block's first
    // convolution follows it by three steps instead of two; within a step no wave reads a row another one writes (ring sizes above), so one barrier per step.
    const int c_s = 5 * (s >> 1) + 2 * (s & 1);
    const int t_end = W + 17 + 2;                              // the last convolution computes row 55 in step 72 and stores it in step 73
    int pending = 0;                                           // second convolutions: 1 = acc holds the previous step's row, 2 = a padding row is due
    {   // the counters at t = -4 (rows below -1 are never touched: only the phase matters; 120 = a multiple of every ring size)
        const int r0 = -4 - c_s;
        i_in = (r0 - 1 + 120) % n_in; i_res = (r0 + 120) % n_res; i_out = (r0 + 120) % n_out; i_dma = (-4 + 3 + 120) % 6;
    }

    abl::Ticks<4> ticks(abl::bit(a.flags, 128));
#pragma unroll 1
    for (int t = -4; t < t_end; ++t) {
        if (t + 3 == W && wv == 0) {                           // ring 0's row for image row 56 (the bottom padding) held row 50: zero it (slots 0 .. 63)
            unsigned char* z = lds + i_dma * G::ROWB;
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(z + (i * 64 + lane) * 16) = u32x4{0u, 0u, 0u, 0u};
        }
        const bool asks = wv < 4 && t + 3 >= 0 && t + 3 < W;
        if (asks) request(t + 3, i_dma);
        const int r = t - c_s;
        ticks.mark(0);
        if (second) {
            if (pending) store_row(r - 1, i_out == 0 ? n_out - 1 : i_out - 1, pending == 2);
            pending = 0;
            if (r >= 0 && r < W) { compute_row(r); pending = 1; }
            else if (r == -1 || r == W) pending = 2;
        } else if (r >= -1 && r <= W) {
            const bool pad = r < 0 || r == W;
            if (!pad) compute_row(r);
            store_row(r, i_out, pad);
        }
        i_in = wrap(i_in + 1, n_in); i_res = wrap(i_res + 1, n_res); i_out = wrap(i_out + 1, n_out); i_dma = wrap(i_dma + 1, 6);
        ticks.mark(1);
        // the row this wave requested one step ago has landed (this step's may still fly; a step without a request leaves nothing in flight)
        if (asks) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
        else if (wv < 4) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ticks.mark(2);
        if (!abl::bit(a.flags, 256))
        lds_barrier();
        ticks.mark(3);
    }
    ticks.flush(GRK_ABL_COUNTERS(g_pipe_phase) + wv * 4, lane == 0);
}

template <int C, int W>
hipError_t set_chain_lds() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(conv_bf16_chain<C, W>), hipFuncAttributeMaxDynamicSharedMemorySize, ChainGeom<C, W>::LDS);
}

}  // namespace

hipError_t conv_bf16_chain_init() {
    GRK_TRY((set_chain_lds<64, 28>()));
    GRK_TRY((set_chain_lds<128, 14>()));
    GRK_TRY((set_chain_lds<256, 7>()));
    GRK_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(conv_bf16_chain<256, 7, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, ChainGeom<256, 7, 2>::LDS));
    GRK_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(conv_bf16_block_frame<56, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, FrameGeom<56, 8>::LDS));
    GRK_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(conv_bf16_chain_pipe), hipFuncAttributeMaxDynamicSharedMemorySize, PipeGeom::LDS));
    GRK_TRY(conv_bf16_wide_init());                          // the two other families of LDS-resident kernels (conv_bf16_wide.hip, conv_bf16_s2.hip)
    return conv_bf16_s2_init();
}

bool conv_bf16_chain_eligible(int c, int w) { return (c == 64 && w == 28) || (c == 128 && w == 14) || (c == 256 && w == 7) || (c == 32 && w == 56); }
// the 56x56 branch: ONE launch for a whole module's chain (conv_bf16_chain_pipe, 8 convolutions), otherwise one launch per BasicBlock (conv_bf16_block_frame)
int conv_bf16_chain_launches(int c, int w, int nconv) { return c == 32 && w == 56 && !(nconv == 8 && GRNET_AB(BF16_PIPE, 1)) ? nconv / 2 : 1; }

// a.in / a.out: NHWC bf16 views of (N, W, W, C) tensors (channel strides in_ctot / out_ctot, first channels in_coff / out_coff, multiples of 8);
// a.w[i]: [C/32][9][C][32] bf16 (pack_conv's bf16 layout with CoutPad = C), a.bias[i]: fp32 [C]; nconv even, <= kMaxChain:
// convolutions 2k, 2k+1 are conv1 / conv2 of BasicBlock k.
hipError_t launch_conv_bf16_chain(const ChainArgs& a, int c, int w, hipStream_t s) {
    if (!conv_bf16_chain_eligible(c, w) || a.nconv < 2 || a.nconv > kMaxChain || (a.nconv & 1) || a.N < 1) return hipErrorInvalidValue;
    if (a.in_ctot % 8 != 0 || a.in_coff % 8 != 0 || a.out_ctot % 8 != 0 || a.out_coff % 8 != 0) return hipErrorInvalidValue;
    if (c == 32 && a.nconv == 8 && GRNET_AB(BF16_PIPE, 1)) {   // the whole chain as one pipeline of rows, a wave per convolution (a.mid is not used)
        ChainArgs b = a;
        b.flags = (GRNET_AB(BF16_FRAME_DBG, 0) << 4) | (GRNET_AB(BF16_PIPE_VSEED, 0) ? 2 : 0);              // (diagnostic builds: timing-only ablation bits 16 / 32 / 64 = no k-loop / no epilogue / no seeds)
#ifdef GRNET_ABLATION
        if (GRNET_AB_SET(PIPE_PHASES)) {
            b.flags |= 128;
            GRK_TRY(launch_k(conv_bf16_chain_pipe, dim3(a.N), dim3(512), PipeGeom::LDS, s, b));
            unsigned long long h[32] = {};
            abl::take_counters(HIP_SYMBOL(g_pipe_phase), h, s);
            const double d = (double)a.N * 79.0;                 // per workgroup and step
            for (int w = 0; w < 8; ++w)
                fprintf(stderr, "[pipe phases] wave %d (conv %d): ticks per step  request %.0f  compute+store %.0f  dma wait %.0f  barrier %.0f\n", w, w < 4 ? 2 * w : 2 * (w - 4) + 1,
                        h[w * 4] / d, h[w * 4 + 1] / d, h[w * 4 + 2] / d, h[w * 4 + 3] / d);
            return hipSuccess;
        }
#endif
        GRK_TRY(launch_k(conv_bf16_chain_pipe, dim3(a.N), dim3(512), PipeGeom::LDS, s, b));
        return hipSuccess;
    }
    if (c == 32) {                                           // one launch per BasicBlock; block k > 0 reads what block k - 1 wrote: a.mid holds the intermediates
        ChainArgs b = a;
        for (int k = 0; k < a.nconv / 2; ++k) {
            b.nconv = 2;
            b.w[0] = a.w[2 * k]; b.w[1] = a.w[2 * k + 1]; b.bias[0] = a.bias[2 * k]; b.bias[1] = a.bias[2 * k + 1];
            if (k > 0) { b.in = a.mid[k - 1]; b.in_ctot = a.mid_ctot[k - 1]; b.in_coff = a.mid_coff[k - 1]; }
            if (k < a.nconv / 2 - 1) {
                if (!a.mid[k] || a.mid_ctot[k] % 8 != 0 || a.mid_coff[k] % 8 != 0) return hipErrorInvalidValue;
                b.out = a.mid[k]; b.out_ctot = a.mid_ctot[k]; b.out_coff = a.mid_coff[k];
            } else { b.out = a.out; b.out_ctot = a.out_ctot; b.out_coff = a.out_coff; }
            // workgroup = frame, seven bands of 8 rows, the next band by LDS-DMA under the current band's MFMAs
            static const int frame_direct = GRNET_AB(BF16_FRAME_DIRECT, 1);
            b.flags = (frame_direct ? 0 : 1) | (GRNET_AB(BF16_FRAME_DBG, 0) << 4);      // (diagnostic builds: timing-only ablation bits 16 / 32 / 64 = no conv1 k-loop / no conv2 k-loop / no deposit)
            GRK_TRY(launch_k(conv_bf16_block_frame<56, 8>, dim3(a.N), dim3(512), FrameGeom<56, 8>::LDS, s, b));
        }
        return hipSuccess;
    }
    if (c == 64) return launch_k(conv_bf16_chain<64, 28>, dim3(a.N), dim3(512), ChainGeom<64, 28>::LDS, s, a);
    if (c == 128) return launch_k(conv_bf16_chain<128, 14>, dim3(a.N), dim3(512), ChainGeom<128, 14>::LDS, s, a);
    if (GRNET_AB(BF16_CHAIN7_PAIR, 1) && a.N >= 2) return launch_k(conv_bf16_chain<256, 7, 2>, dim3((a.N + 1) / 2), dim3(512), ChainGeom<256, 7, 2>::LDS, s, a);
    return launch_k(conv_bf16_chain<256, 7>, dim3(a.N), dim3(512), ChainGeom<256, 7>::LDS, s, a);
}

}  // namespace grk
