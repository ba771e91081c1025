// bf16 path: the wide 3x3 stride-1 layers with a band of the input resident in LDS.  The flattened, padded LDS plane and the MFMA roles are those of the
// frame-resident chain kernels (conv_bf16_chain.hip: its header describes them); the tile geometry and the k-loop with its weight ring are the LDS-plane
// family's one definition (conv_bf16_plane.h).
//
// ---- ONE wide 3x3 stride-1 convolution (upsample heads hrnet.py:440-453, PARE head pare.py:377-400, layer1's 3x3 hrnet.py:80-100) with a band of
// the input resident in LDS.  conv_bf16_nhwc runs these layers at 0.25-0.45 of the matrix peak: 224-pixel x 64-channel tiles, 32 input
// channels per barrier (126 MFMAs per wave between two barriers, each with a vmcnt(0) in front).  Here a workgroup owns R output rows of one
// frame x CT = CP output channels (CP = 128, or 64 for the 64-channel layers): the R + 2 input rows go HBM -> LDS by LDS-DMA straight into the
// padded, flattened plane of the chain kernel (the pad units and every zero -- halo column, rows outside the image -- come from a block of
// zeros: the DMA writes lane-linear, so it cannot skip them), CP input channels per pass; between two barriers a wave issues 9 x CP/32 x 26
// MFMAs (936 for CP = 128).  Layers with more than CP input channels take several passes (480 = 128 + 128 + 128 + 96) into the same
// accumulators; their weights are one contiguous stream ([chunk][tap][CoutPad][32]), so the ring of weight fragments runs across passes.
// The tile leaves through the plane (in place, as in the chain kernel) as whole channel rows.
#include "kernels.h"
#include "device.h"
#include "conv_bf16_plane.h"

namespace grk {

namespace {

// CT output channels per workgroup (CT <= CP: the tile leaves through the first 2 CT bytes of the plane's slots)
template <int CP, int CT, int W, int R>
struct WideGeom : PlaneGeom<CP, CT, W, R, R> {
    typedef PlaneGeom<CP, CT, W, R, R> B;
    static constexpr int UPS = B::SB / 16;
    static constexpr int ROWS = R + 2;                      // plane rows: image rows y0 - 1 .. y0 + R
    static constexpr int LDS = B::NSLOT * B::SB;
    static constexpr int FILL_UNITS = ((ROWS * B::P + 1) * UPS + 63) / 64 * 64;    // slots 0 .. ROWS * P (the last one: the right halo of the last row), whole wave-instructions
    static constexpr int NFILL = (FILL_UNITS / 64 + 7) / 8;                        // wave-instructions per wave
    static_assert(LDS <= 160 * 1024 && FILL_UNITS * 16 <= LDS && CT <= CP, "wide-band geometry");
    // (with CP = 128 the farthest pixel fragment lies 89 KB behind the lane's base: past the 16-bit ds_read immediate, hipcc keeps a second base register)
};

template <int CP, int CT, int W, int R>
__global__ __launch_bounds__(512) void conv_bf16_wide_band(const ConvArgs a) {
    typedef WideGeom<CP, CT, W, R> G;
    constexpr int P = G::P, SB = G::SB, CS = G::CS, PS = G::PS, UPS = G::UPS, UPP = G::UPP;
    extern __shared__ __align__(16) unsigned char plane[];
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wcb = wave % G::WCB, pg = wave / G::WCB;
    const int ncb = a.CoutPad / CT;                            // output-channel tiles of the layer
    int bid = blockIdx.x;
    if (a.xcd) bid = xcd_redeal(bid);
    const int cbo = bid % ncb, nb = bid / ncb, n = nb / G::NB, band = nb - n * G::NB;
    if (n >= a.N) return;
    const int y0 = band * R;
    const u16* inb = reinterpret_cast<const u16*>(a.in) + (size_t)n * W * W * a.in_ctot + a.in_coff;
    const u16* zeros = reinterpret_cast<const u16*>(a.zeros);

    // DMA unit u = (slot, 16-byte part) of the plane in memory order.  The unit -> pixel map does not depend on the pass, and hipcc would hoist it
    // out of the pass loop into 2 x NFILL registers held beside the accumulators (164-212 bytes of scratch): the lane index is laundered through an
    // empty asm per pass, so the map is recomputed (~20 scalar-free instructions per unit, 19 units per pass) instead of kept.
    auto fill = [&](int c0, int cw) {                          // input channels c0 .. c0 + cw - 1 of the band -> plane, by LDS-DMA
        int ln = lane;
        asm volatile("" : "+v"(ln));
#pragma unroll
        for (int i = 0; i < G::NFILL; ++i) {
            const int ub = (i * 8 + wave) * 64;
            if (ub >= G::FILL_UNITS) break;                    // wave-uniform
            const int u = ub + ln, slot = u / UPS, part = u - slot * UPS, r = slot / P, xx = slot - r * P, y = y0 - 1 + r;
            const bool data = r < G::ROWS && xx != 0 && y >= 0 && y < W && part * 8 < cw;
            dma16_builtin(data ? inb + (size_t)(y * W + xx - 1) * a.in_ctot + c0 + part * 8 : zeros, plane + ub * 16);
        }
    };

    const int o_first = G::O0 + pg * PS * 16 + l15;
    const unsigned char* bread = plane + (o_first - P - 1) * SB + lq * 16;
    unsigned char* owrite = plane + o_first * SB + (wcb * CS * 16 + lq * 4) * 2;
    unsigned valid = 0;
#pragma unroll
    for (int ps = 0; ps < PS; ++ps) {
        const int o = o_first + ps * 16, r = o / P;
        if (o - r * P != 0 && r >= 1 && r <= R && y0 + r - 1 < W) valid |= 1u << ps;
    }
    const int co = cbo * CT + wcb * CS * 16;                   // first output channel of this wave
    const unsigned wlb = ((co + l15) * 32 + lq * 8) * 2;
    const size_t wtap = (size_t)a.CoutPad * 32;
    const u16* wg = reinterpret_cast<const u16*>(a.w);
    f32x4 acc[CS][PS];
#pragma unroll
    for (int cs = 0; cs < CS; ++cs) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias + co + cs * 16 + lq * 4);
#pragma unroll
        for (int ps = 0; ps < PS; ++ps) acc[cs][ps] = bv;
    }
    bf16x8 wr[3][CS];
#pragma unroll
    for (int cs = 0; cs < CS; ++cs) {
        wr[0][cs] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const unsigned char*>(wg + cs * 16 * 32) + wlb);
        wr[1][cs] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const unsigned char*>(wg + wtap + cs * 16 * 32) + wlb);
    }
    const int npass = (a.CinPad + CP - 1) / CP;
#pragma unroll 1
    for (int pass = 0; pass < npass; ++pass) {
        const int c0 = pass * CP, cw = a.CinPad - c0 < CP ? a.CinPad - c0 : CP;
        if (pass) __syncthreads();                             // every wave has finished reading the previous pass's plane
        if (!abl::bit(a.dbg, 1) || pass == 0)      // timing-only builds (make ABLATION=1; GRNET_WIDE_DBG bit 0: no fill, bit 1: no k-loop)
        fill(c0, cw);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const u16* wpass = wg + (size_t)(c0 / 32) * 9 * wtap;       // the pass's first k-step; behind the layer's last one the stream ends: its own first steps again
        if (!abl::bit(a.dbg, 2))
        plane_kloop<G>(acc, wr, bread, wpass, wpass, wtap, cw / 32, pass == npass - 1, wlb);
    }
    // ---- the tile: bias is in the accumulators; ReLU, bf16, in place through the plane, rows y0 .. y0 + R - 1 -> HBM as whole channel rows
    __syncthreads();
#pragma unroll
    for (int ps = 0; ps < PS; ++ps)
#pragma unroll
        for (int cs = 0; cs < CS; ++cs)
            if (valid & (1u << ps)) *reinterpret_cast<u32x2*>(owrite + ps * 16 * SB + cs * 32) = pack4_relu_if(acc[cs][ps], a.relu);
    __syncthreads();
    u16* outb = reinterpret_cast<u16*>(a.out) + (size_t)n * W * W * a.out_ctot + a.out_coff + cbo * CT;
    const int cstore = a.Cout - cbo * CT;                      // real channels of this tile (CoutPad may exceed Cout)
#pragma unroll
    for (int i = 0; i < G::NUO; ++i) {
        const int u = i * 512 + tid, px = u / UPP, part = u - px * UPP, r = px / W, x = px - r * W;
        if (u < R * W * UPP && y0 + r < W && part * 8 < cstore)
            *reinterpret_cast<u32x4*>(outb + ((size_t)(y0 + r) * W + x) * a.out_ctot + part * 8) = *reinterpret_cast<const u32x4*>(plane + ((r + 1) * P + x + 1) * SB + part * 16);
    }
}

// ---- The wide 3x3 convolution again, with BOTH operands streamed through LDS by DMA under the MFMAs (round 5).  conv_bf16_wide_band holds CP = 128
// channels of the band in one plane and refills it between passes: fill -> vmcnt(0) -> barrier -> 936 MFMAs per wave -> barrier, nothing overlapped (one
// workgroup per CU owns the whole LDS).  Ablated at 256 frames (make ABLATION=1, GRNET_WIDE_DBG): 480 -> 256 @56 takes 1 277 us, 1 054 without the three
// refills, 177 without any k-loop (first fill + store): the k-loop alone runs at 2.0 PFLOP/s -- the MFMA issue rate at the clock the chip holds under this
// load -- and 0.4 of 1.28 ms is exposed fill and store.
// Here a plane holds ONE 32-channel chunk of the band (slot stride 64 + 32 bytes: 32 * odd, conflict-free b128 reads as before) and two planes alternate:
// chunk c is computed from plane c % 2 while the pieces of chunk c + 1 land in the other one.  ONE barrier per chunk, behind tap 7: every wave's reads of
// chunk c are done by then (tap 8's fragments are in registers) and its pieces of chunk c + 1 have landed, so tap 8 reads ahead into chunk c + 1 and the
// first piece of chunk c + 2 goes out; 234 MFMAs per wave between barriers.
// vmcnt retires in order, and hipcc drains it to ZERO in front of every use of a loaded register while an LDS-DMA it knows of is in flight (seen in the ISA of
// a first version with the weights by global_load: one vmcnt(0) per tap).  So NO register-returning vector load is left in the loop: the weights go through
// LDS too -- every wave DMAs the 2 KiB (32 output channels x 32 k) of its own fragments per k-step into a private ring of three slots, two steps ahead, XOR-
// swizzled like the frame kernel's -- every DMA is inline asm the compiler does not count, and the waits are explicit: per tap the wave issues W(t+2) (two
// pieces) and at most one plane piece, and waits in the middle of the tap with vmcnt(2 + I(t-1) + I(t)) -- everything up to W(t+1) has landed, the plane
// pieces of this and the previous tap may still fly -- then reads W(t+1)'s fragments for the next tap.  I(t) = 1 on the taps that carry a plane piece
// (tap 8 and taps 0 .. NFILL-2: every wave issues the same count -- a wave without an own last piece re-requests the plane's last one, and behind the
// last chunk the pieces fetch zeros into the plane nobody reads any more).
template <int CT, int W, int R, bool DIRECT = false>
struct RingGeom : PlaneGeom<32, CT, W, R, R> {                                      // a plane holds ONE 32-channel chunk: slot stride 96 bytes
    typedef PlaneGeom<32, CT, W, R, R> B;
    static constexpr int UPS = B::SB / 16;
    static constexpr int ROWS = R + 2;
    static constexpr int NPIECE = ((ROWS * B::P + 1) * UPS + 63) / 64;              // one-KiB DMA pieces of a plane: slots 0 .. ROWS * P
    static constexpr int PB = NPIECE * 1024;                                        // plane stride, bytes
    static constexpr int NFILL = (NPIECE + 7) / 8;                                  // pieces per wave and chunk
    static constexpr int WRING = 2 * PB;                                            // the waves' weight rings: 8 x 3 slots x 2 KiB (a plane's dead columns read into them: garbage, never stored)
    static constexpr int OSB = 2 * CT + 32;                                         // slot stride of the output tile (staged over everything)
    static constexpr int LDS = WRING + 8 * 3 * 2048;
    static constexpr bool piece_at(int tap) { return tap == 8 || tap < NFILL - 1; }
    static_assert(LDS <= 160 * 1024 && NFILL >= 2 && NFILL <= 7 && (DIRECT || (B::O0 + B::NT * 16) * OSB <= LDS), "ring geometry");
    static_assert(B::IMM16 && B::NSLOT * B::SB + 64 <= LDS - PB, "ds_read immediates / the farthest dead read stays inside the allocation");
};

template <int CT, int W, int R, bool DIRECT = false>
__global__ __launch_bounds__(512) void conv_bf16_wide_ring(const ConvArgs a) {
    typedef RingGeom<CT, W, R, DIRECT> G;
    constexpr int P = G::P, SB = G::SB, CS = G::CS, PS = G::PS, UPS = G::UPS, UPP = G::UPP, PB = G::PB, NFILL = G::NFILL, OSB = G::OSB;
    extern __shared__ __align__(16) unsigned char plane[];
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wcb = wave % G::WCB, pg = wave / G::WCB;
    const int ncb = a.CoutPad / CT;
    int bid = blockIdx.x;
    if (a.xcd) bid = xcd_redeal(bid);
    const int cbo = bid % ncb, nb = bid / ncb, n = nb / G::NB, band = nb - n * G::NB;
    if (n >= a.N) return;
    const int y0 = band * R;
    const unsigned char* inb = reinterpret_cast<const unsigned char*>(reinterpret_cast<const u16*>(a.in) + (size_t)n * W * W * a.in_ctot + a.in_coff);
    const int nch = a.CinPad / 32, nstep = nch * 9;
    const unsigned lds0 = (unsigned)(size_t)plane;                                  // LDS byte address of the allocation (M0 takes byte addresses)

    // this lane's share of plane piece i: byte offset of its 16 bytes of chunk 0 in the frame (chunk c: + 64 c).  Units that must read zero -- halo column, rows
    // outside the image -- are the same for every chunk: they are zeroed ONCE below and their lanes are switched off in every piece (EXEC), so a piece needs
    // no second source and is `global_load_lds v_off, s[base]`; the pad units (never read) stay on and fetch the frame's first bytes, so that no piece is empty
    // (an instruction without lanes would not count in vmcnt, and the waits below count instructions)
    unsigned poff[NFILL];
    int pdst[NFILL];
    unsigned long long pmask[NFILL];
#pragma unroll
    for (int i = 0; i < NFILL; ++i) {
        int pc = i * 8 + wave;
        pc = pc < G::NPIECE ? pc : G::NPIECE - 1;                                   // no own last piece: the plane's last one again
        const int u = pc * 64 + lane, slot = u / UPS, part = u - slot * UPS, r = slot / P, xx = slot - r * P, y = y0 - 1 + r;
        const bool data = part < 4 && r < G::ROWS && xx != 0 && y >= 0 && y < W;
        poff[i] = data ? (unsigned)(((y * W + xx - 1) * a.in_ctot + part * 8) * 2) : 0u;
        pdst[i] = pc * 1024;
        pmask[i] = __ballot(data || part >= 4);
        if (!data && part < 4) {                                                    // both planes: never written again
            *reinterpret_cast<u32x4*>(plane + pdst[i] + lane * 16) = u32x4{0u, 0u, 0u, 0u};
            *reinterpret_cast<u32x4*>(plane + PB + pdst[i] + lane * 16) = u32x4{0u, 0u, 0u, 0u};
        }
    }
    const bool chunk0 = abl::bit(a.dbg, 8);                                        // (read out here: inside the lambda `a` would become one more capture)
    auto piece = [&](int i, int c, int pl) {                                        // behind the last chunk: chunk 0 again, into the plane nobody reads any more
        int ce = c < nch ? c : 0;
        if (chunk0) ce = 0;                                                                  // bit 3: every piece fetches chunk 0 (cache hits): issue cost without the memory latency
        dma16_masked(poff[i], inb + ce * 64, lds0 + pl + pdst[i], pmask[i]);
    };
    // weights of k-step s for this wave: rows co .. co + 31 of [step][CoutPad][32]; piece cs = 16 rows x 64 B, lane (row = l >> 2, unit = l & 3) fetches the unit
    // (l & 3) ^ 2 (row >> 3 & 1) of its row: the fragment read below finds k-group lq of row l15 at unit lq ^ 2 (l15 >> 3) -- conflict-free b128 reads of 64-byte rows
    const int co = cbo * CT + wcb * CS * 16;
    const unsigned wlane = (unsigned)(((co + (lane >> 2)) * 32 + (((lane & 3) ^ (2 * ((lane >> 5) & 1))) * 8)) * 2);
    const size_t wstep = (size_t)a.CoutPad * 64;                                    // bytes per k-step
    const unsigned char* wg = reinterpret_cast<const unsigned char*>(a.w);
    const unsigned wring = lds0 + G::WRING + wave * (3 * 2048);
    auto wdma = [&](int s, int slot) {                                              // behind the layer's last step the stream ends: its first steps again (nobody reads them)
        const unsigned char* base = wg + (size_t)(s < nstep ? s : s - nstep) * wstep;
#pragma unroll
        for (int cs = 0; cs < CS; ++cs) dma16_uniform(wlane + cs * 1024, base, wring + slot * 2048 + cs * 1024);
    };
    const unsigned char* aread = plane + G::WRING + wave * (3 * 2048) + l15 * 64 + ((lq ^ (2 * (l15 >> 3))) * 16);

    const int o_first = G::O0 + pg * PS * 16 + l15;
    const unsigned char* bread = plane + (o_first - P - 1) * SB + lq * 16;
    unsigned valid = 0;
#pragma unroll
    for (int ps = 0; ps < PS; ++ps) {
        const int o = o_first + ps * 16, r = o / P;
        if (o - r * P != 0 && r >= 1 && r <= R && y0 + r - 1 < W) valid |= 1u << ps;
    }
    f32x4 acc[CS][PS];
#pragma unroll
    for (int cs = 0; cs < CS; ++cs) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias + co + cs * 16 + lq * 4);
#pragma unroll
        for (int ps = 0; ps < PS; ++ps) acc[cs][ps] = bv;
    }
    // ---- prologue: chunk 0 -> plane 0, k-steps 0 and 1, the last piece of chunk 1 (the piece "tap 8 of chunk -1" would have issued)
#pragma unroll
    for (int i = 0; i < NFILL; ++i) piece(i, 0, 0);
    wdma(0, 0);
    wdma(1, 1);
    piece(NFILL - 1, 1, PB);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CS + 1) : "memory");                   // in order: chunk 0 and step 0 have landed; step 1 and the piece of chunk 1 may fly
    __syncthreads();                                                                // (and the zeroed halo units are everybody's)
    bf16x8 bfr[PS], afr[3][CS];                                                     // fragment sets in ring order too: step s0 + tap uses set tap % 3 (9 = 3 x 3)
#pragma unroll
    for (int cs = 0; cs < CS; ++cs) afr[0][cs] = *reinterpret_cast<const bf16x8*>(aread + cs * 1024);
#pragma unroll
    for (int ps = 0; ps < PS; ++ps) bfr[ps] = *reinterpret_cast<const bf16x8*>(bread + ps * 16 * SB);
    int cur = 0, nxt = PB;
#pragma unroll 1
    for (int c = 0; c < nch; ++c) {
        const unsigned char* bc = bread + cur;
        const unsigned char* bn = bread + nxt;
        const int s0 = c * 9;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            // k-step s0 + tap + 2 -> ring slot (tap + 2) % 3 (9 = 3 x 3: the slot is static), then this tap's plane piece: chunk c + 1 on taps 0 .. NFILL-2
            // (pieces 0 .. NFILL-2; into the other plane), chunk c + 2 on tap 8 (piece NFILL-1; into THIS plane, which the barrier behind tap 7 has freed)
            if (!abl::bit(a.dbg, 2))      // timing-only builds (make ABLATION=1; GRNET_WIDE_DBG bit 0: no plane pieces, bit 1: no weight pieces, bit 2: no waits)
            wdma(s0 + tap + 2, (tap + 2) % 3);
            if (!abl::bit(a.dbg, 1)) {
                if (tap == 8) piece(NFILL - 1, c + 2, cur);
                else if (tap < NFILL - 1) piece(tap, c + 1, nxt);
            }
            const unsigned char* nb_ = tap < 8 ? bc + (((tap + 1) / 3) * P + ((tap + 1) % 3)) * SB : bn;
            constexpr int HALF = PS / 2;
#pragma unroll
            for (int ps = 0; ps < PS; ++ps) {
                if (ps == HALF) {
                    // everything up to k-step s0 + tap + 1 has landed (issued one tap ago); behind it: that tap's plane piece, this tap's two weight pieces and plane piece
                    if (!abl::bit(a.dbg, 4))
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CS + (G::piece_at((tap + 8) % 9) ? 1 : 0) + (G::piece_at(tap) ? 1 : 0)) : "memory");
#pragma unroll
                    for (int cs = 0; cs < CS; ++cs) afr[(tap + 1) % 3][cs] = *reinterpret_cast<const bf16x8*>(aread + ((tap + 1) % 3) * 2048 + cs * 1024);
                }
#pragma unroll
                for (int cs = 0; cs < CS; ++cs) acc[cs][ps] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[tap % 3][cs], bfr[ps], acc[cs][ps], 0, 0, 0);
                bfr[ps] = *reinterpret_cast<const bf16x8*>(nb_ + ps * 16 * SB);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (tap == 7) {
                // every read of chunk c has returned (tap 8's fragments included); this wave's pieces of chunk c + 1 landed with the wait in the middle of this tap
                // (the last one went out on tap NFILL-2 <= 5)
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
            }
        }
        const int t = cur; cur = nxt; nxt = t;
    }
    if constexpr (DIRECT) {
        // 256 output channels per workgroup: the tile (R x W pixels x 512 bytes) does not fit the LDS beside nothing -- it leaves straight from the accumulators, 8 bytes per
        // lane and block (a pixel's 64 bytes of this wave are two stores back to back; the eight channel waves complete its 512-byte row in L2)
        const int cstore = a.Cout - cbo * CT;
        u16* outw = reinterpret_cast<u16*>(a.out) + (size_t)n * W * W * a.out_ctot + a.out_coff + cbo * CT + wcb * CS * 16 + lq * 4;
#pragma unroll
        for (int ps = 0; ps < PS; ++ps) {
            const int o = o_first + ps * 16, r = o / P, x = o - r * P - 1;
            u16* op = outw + ((size_t)(y0 + r - 1) * W + x) * a.out_ctot;
#pragma unroll
            for (int cs = 0; cs < CS; ++cs)
                if ((valid & (1u << ps)) && wcb * CS * 16 + cs * 16 + lq * 4 < cstore) *reinterpret_cast<u32x2*>(op + cs * 16) = pack4_relu_if(acc[cs][ps], a.relu);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                           // no piece may land in an LDS that already belongs to somebody else
        return;
    }
    // ---- the tile: ReLU, bf16, staged over planes and rings (every piece has landed, every wave is done reading), rows y0 .. y0 + R - 1 -> HBM as whole channel rows
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned char* owrite = plane + o_first * OSB + (wcb * CS * 16 + lq * 4) * 2;
#pragma unroll
    for (int ps = 0; ps < PS; ++ps)
#pragma unroll
        for (int cs = 0; cs < CS; ++cs)
            if (valid & (1u << ps)) *reinterpret_cast<u32x2*>(owrite + ps * 16 * OSB + cs * 32) = pack4_relu_if(acc[cs][ps], a.relu);
    __syncthreads();
    u16* outb = reinterpret_cast<u16*>(a.out) + (size_t)n * W * W * a.out_ctot + a.out_coff + cbo * CT;
    const int cstore = a.Cout - cbo * CT;
#pragma unroll
    for (int i = 0; i < G::NUO; ++i) {
        const int u = i * 512 + tid, px = u / UPP, part = u - px * UPP, r = px / W, x = px - r * W;
        if (u < R * W * UPP && y0 + r < W && part * 8 < cstore)
            *reinterpret_cast<u32x4*>(outb + ((size_t)(y0 + r) * W + x) * a.out_ctot + part * 8) = *reinterpret_cast<const u32x4*>(plane + ((r + 1) * P + x + 1) * OSB + part * 16);
    }
}

}  // namespace

hipError_t conv_bf16_wide_init() {
    GRK_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(conv_bf16_wide_band<64, 64, 56, 14>), hipFuncAttributeMaxDynamicSharedMemorySize, WideGeom<64, 64, 56, 14>::LDS));
    GRK_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(conv_bf16_wide_ring<128, 56, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, RingGeom<128, 56, 8>::LDS));
    GRK_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(conv_bf16_wide_ring<256, 56, 4, true>), hipFuncAttributeMaxDynamicSharedMemorySize, RingGeom<256, 56, 4, true>::LDS));
    GRK_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(conv_bf16_wide_ring<32, 56, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, RingGeom<32, 56, 8>::LDS));
    GRK_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(conv_bf16_wide_ring<128, 28, 14>), hipFuncAttributeMaxDynamicSharedMemorySize, RingGeom<128, 28, 14>::LDS));
    return hipSuccess;
}

// Wide-band kernel: 3x3, stride 1, no fused addend, 56x56 or 28x28 maps, CinPad a multiple of 32; output channels in tiles of 128 (Cin >= 128) or
// 64 (Cin = 64 -> 64); every 16-byte group of the output view must lie inside the buffer.  (A 32-channel tile for transition1's 256 -> 32 -- 6-row bands,
// 3 column tiles per wave -- measured 245 us against the generic kernel's 228 at 256 frames: every pixel fragment feeds two MFMAs only.  Not instantiated.)
bool conv_bf16_wide_eligible(const ConvArgs& a) {
    if (a.ks != 3 || a.stride != 1 || a.n_add != 0 || a.H != a.W || a.Ho != a.H || a.Wo != a.W || a.CinPad % 32 != 0) return false;
    if (a.in_ctot % 8 != 0 || a.in_coff % 8 != 0 || a.out_ctot % 8 != 0 || a.out_coff % 8 != 0 || a.Cout % 8 != 0) return false;
    if (a.W == 56 && a.CinPad == 64 && a.CoutPad == 64) return true;
    // transition1's 256 -> 32 (hrnet.py:348-387): the ring kernel with ONE 32-channel block, every wave a column group (conv_bf16_nhwc ran it at 0.18 of the peak, 2.0 TB/s)
    static const int ct32_env = GRNET_AB(BF16_WIDE_CT32, 1);
    if (ct32_env && a.W == 56 && a.CinPad >= 128 && a.CoutPad == 32) return true;
    return (a.W == 56 || a.W == 28) && a.CinPad >= 128 && a.CoutPad % 128 == 0;
}
hipError_t launch_conv_bf16_wide(const ConvArgs& a0, hipStream_t s) {
    if (!conv_bf16_wide_eligible(a0) || a0.N < 1) return hipErrorInvalidValue;
    static const int xcd_env = GRNET_AB(BF16_XCD, 1);
    ConvArgs a = a0;
    a.xcd = xcd_env;
#ifdef GRNET_ABLATION
    a.dbg = GRNET_AB(WIDE_DBG, 0);
#endif
    // (64 -> 64 on the ring kernel -- 7-row bands, two chunks: the second streams under the first -- measured 93 us against the band kernel's 79: stays here)
    if (a.CinPad == 64) return launch_k(conv_bf16_wide_band<64, 64, 56, 14>, dim3(a.N * WideGeom<64, 64, 56, 14>::NB), dim3(512), WideGeom<64, 64, 56, 14>::LDS, s, a);
    if (a.CoutPad == 32) return launch_k(conv_bf16_wide_ring<32, 56, 8>, dim3(a.N * RingGeom<32, 56, 8>::NB), dim3(512), RingGeom<32, 56, 8>::LDS, s, a);
    const int ncb = a.CoutPad / 128;
    // the ring of one-chunk planes (the 128-channel plane of conv_bf16_wide_band, refilled between passes, lost to it on every layer: NOTES_rejected.md)
    // 256 output channels at 56x56: ONE workgroup for all channels of a 4-row band (eight channel waves, 15 column tiles each) -- the band is fetched once, not once per
    // 128-channel tile: 6 input rows per 4 output rows instead of 2 x 10 per 8, 5 plane pieces per chunk and wave instead of 7; the tile leaves from the accumulators.
    // Alone it ties the 128-channel tiles (1 222 / 1 221 us for 480 -> 256, 644 / 647 for 256 -> 256 at 256 frames); in the step 10.49 against 10.51-10.53 ms (two pairs).
    // GRNET_BF16_WIDE_CT256=0: 128-channel tiles
    static const int ct256_env = GRNET_AB(BF16_WIDE_CT256, 1);
    if (ct256_env && a.W == 56 && a.CoutPad == 256)
        return launch_k(conv_bf16_wide_ring<256, 56, 4, true>, dim3(a.N * RingGeom<256, 56, 4, true>::NB), dim3(512), RingGeom<256, 56, 4, true>::LDS, s, a);
    // 56x56: 8-row bands (7 per frame, 15 column tiles per wave, 244 registers) measured against 7-row ones (8 per frame): 480 -> 256 1 240 / 1 240 us,
    // 256 -> 256 648 / 666, 128 -> 128 210 / 216 at 256 frames
    if (a.W == 56) return launch_k(conv_bf16_wide_ring<128, 56, 8>, dim3(a.N * RingGeom<128, 56, 8>::NB * ncb), dim3(512), RingGeom<128, 56, 8>::LDS, s, a);
    return launch_k(conv_bf16_wide_ring<128, 28, 14>, dim3(a.N * RingGeom<128, 28, 14>::NB * ncb), dim3(512), RingGeom<128, 28, 14>::LDS, s, a);
}

}  // namespace grk
