// bf16 path: what the LDS-plane kernels share -- conv_bf16_chain (conv_bf16_chain.hip), conv_bf16_wide_band / conv_bf16_wide_ring (conv_bf16_wide.hip) and
// conv_bf16_s2_band (conv_bf16_s2.hip): the tile geometry, the k-loop with its weight ring, the XCD re-deal.  Each is defined ONCE here; the files keep their
// fill / staging schemes, pass loops, prologues and epilogues, the ring kernel's DMA pipeline, launchers and eligibility.  Included by those files after device.h.
// (The four-value ReLU + pack of the epilogues, pack4_relu / pack4_relu_if, is in device.h: conv_bf16_roll.hip uses it too.)
// What is NOT here, on purpose: the per-lane prologue (lane roles, column mask, bias seeds, ring priming), the deposit and row-store loops and the band fill
// are still written out per kernel.  Each was tried as a function; hipcc inlines even a __forceinline__ function only AFTER its first round of scalar
// optimisations, so a piece that moves into one is optimised out of its context first, and the kernels' instruction streams came out different (register
// allocation and scheduling ties; 50 to 3 500 assembly lines per file).  Only what was a function already (the k-loop) or is a pure value function of
// opaque arguments (xcd_redeal, pack4_relu_if) compiles to the same code shared as copied.  Sharing the rest is a kernel change, to be measured as one.
//
// The plane (conv_bf16_chain.hip's header has the long form): the zero-padded image, flattened with row pitch P = W + 1 (one shared halo column), a slot per
// pixel of 2 C + 32 bytes (32 x odd: conflict-free ds_read_b128 of 16 consecutive slots), so a tap is a CONSTANT slot offset and a wave's MFMA column tile is 16
// consecutive slots.  8 waves as a WCB x WPG grid; wave (wcb, pg) owns CS x 16 output channels x PS column tiles; the tile leaves in place through the plane.
#pragma once
#include "device.h"

namespace grk {

// The tile geometry.  CIN: input channels a slot holds, CT: output channels of the workgroup, W: pixels per plane row, NR: plane rows that carry outputs,
// R: image rows the workgroup stores.  A kernel's own struct derives from this and adds its rows, its LDS size and its fill units.
template <int CIN, int CT, int W_, int NR, int R_>
struct PlaneGeom {
    static constexpr int W = W_, R = R_;
    static constexpr int P = W + 1;                         // row pitch in slots
    static constexpr int SB = 2 * CIN + 32;                 // slot stride, bytes
    static constexpr int O0 = P + 1;                        // slot of pixel (0, 0) = first output column (stride 1)
    static constexpr int NOUT = NR * P - 1;                 // output columns: O0 .. the last pixel of the last row
    static constexpr int CS = 2;                            // 16-channel blocks per wave
    static constexpr int WCB = CT / (16 * CS);              // waves along the output channels
    static constexpr int WPG = 8 / WCB;                     // waves along the pixels
    static constexpr int PS = ((NOUT + 15) / 16 + WPG - 1) / WPG;      // column tiles per wave
    static constexpr int NT = WPG * PS;                     // column tiles
    static constexpr int NSLOT = O0 + NT * 16 + P + 2;      // highest slot a tap reads: O0 + 16 NT - 1 + P + 1; + one spare slot (the read-ahead of a convolution's last step)
    static constexpr int UPP = CT / 8;                      // 16-byte units per output pixel
    static constexpr int NUO = (R * W * UPP + 511) / 512;   // units per thread of the rows that leave
    static constexpr int NB = (W + R - 1) / R;              // bands per frame
    // every pixel fragment of a k-loop within the 16-bit ds_read immediate of ONE base register (where not, hipcc keeps a second base)
    static constexpr bool IMM16 = (PS - 1) * 16 * SB + (2 * P + 2) * SB + (CIN / 32) * 64 < 65536;
    static_assert(CT % 32 == 0 && WCB >= 1 && WCB <= 8 && 8 % WCB == 0, "wave grid");
    static_assert((SB / 16) % 2 == 0 && ((SB / 32) % 2) == 1, "slot stride must be 32 * odd bytes (conflict-free b128 reads)");
    static_assert(PS <= 32, "one bit per column tile in the lane's validity mask");
    // byte offset of tap (dy, dx) from the lane's base, stride 1 (the stride-2 geometry has its own: four sub-planes)
    static constexpr int toff(int tap) { return ((tap / 3) * P + tap % 3) * SB; }
};

// Workgroups go to the 8 XCDs round-robin by blockIdx.  Where the grid is a multiple of 8 the ids are re-dealt so that CONSECUTIVE tiles -- the output-channel
// tiles of a band, then the frame's next band (which shares two halo rows) -- run on ONE XCD at about the same time and meet in its L2.  bid: blockIdx.x
__device__ __forceinline__ int xcd_redeal(int bid) {
    if ((gridDim.x & 7) == 0) bid = (bid & 7) * (gridDim.x >> 3) + (bid >> 3);
    return bid;
}

// One k-loop over the LDS plane: nch chunks of 32 input channels x 9 taps into acc.
// Per k-step (tap x 32-channel chunk): CS weight fragments requested two steps ahead (ring of three register sets), and per column tile
// one pixel fragment: tile ps of step s + 1 is requested right behind the MFMAs of tile ps of step s, into the register set they have
// just read -- a read has PS - 1 MFMA pairs (and the SIMD's other wave) to land.  Left to itself hipcc sinks every read and every
// weight load to its first use (one register set, lgkmcnt(0) in front of every MFMA pair, vmcnt(0) per step: the loop ran at LDS
// latency); the sched_barrier behind every group pins the order written here.  The chunk loop stays a loop (9 taps unrolled: the
// ring positions are static, 9 = 3 x 3), so every address is a per-chunk base + immediates.
// bread: the lane's base in the plane (tap t of chunk 0, tile 0 at bread + G::toff(t)); wc: the first k-step of this run, wtap: elements per k-step
// (CoutPad x 32; the chain: C x 32), weights [chunk][tap][CoutPad][32].  wc / wn are UNIFORM pointers: with the lane's share kept apart as the 32-bit
// byte offset wlb every weight load is `global_load v, v_off, s[base]` -- a 64-bit per-lane pointer per k-step cost two registers each, which hipcc
// hoisted out of the band loop of the frame kernel and spilled.  wr[0 .. RING - 2] hold steps 0 .. RING - 2 on entry and the NEXT run's on exit: the
// leading steps of a layer's next pass are simply the next k-steps of the stream; behind the last chunk of a convolution (last) they come from wn -- the
// chain's next convolution, or the layer's own first steps again where the stream ends (nobody waits for them).
// RING: register sets of the weight ring = prefetch distance + 1.  3 (two k-steps ahead) where a k-step is >= 14 MFMAs; 9 (eight ahead) for the
// 256-channel 7x7 chain, whose k-steps are 8 MFMAs = 128 cycles: two steps did not cover an L2 round trip (SQ_WAIT_ANY 0.73 of its wave cycles).
// RING must divide the 9 taps of a chunk (the ring positions are static in the unrolled tap loop).
template <typename G, int CS, int PS, int RING = 3>
__device__ __forceinline__ void plane_kloop(f32x4 (&acc)[CS][PS], bf16x8 (&wr)[RING][CS], const unsigned char* bread, const u16* wc, const u16* wn, size_t wtap, int nch, bool last, unsigned wlb) {
    constexpr int SB = G::SB, D = RING - 1;
    static_assert(9 % RING == 0, "the ring must divide the taps");
    bf16x8 bfr[PS];
#pragma unroll
    for (int ps = 0; ps < PS; ++ps) bfr[ps] = *reinterpret_cast<const bf16x8*>(bread + ps * 16 * SB + G::toff(0));
#pragma unroll 1
    for (int chunk = 0; chunk < nch; ++chunk) {
        const unsigned char* bch = bread + chunk * 64;
        const u16* wch = wc + (size_t)chunk * 9 * wtap;
        const bool lastc = last && chunk == nch - 1;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            {                                                             // weights of step s + D (taps 9 .. = the next chunk's / the next run's first ones)
                const u16* src = wch + (size_t)(tap + D) * wtap;
                if (tap + D >= 9) src = lastc ? wn + (size_t)(tap + D - 9) * wtap : src;
#pragma unroll
                for (int cs = 0; cs < CS; ++cs) wr[(tap + D) % RING][cs] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const unsigned char*>(src + cs * 16 * 32) + wlb);
            }
            // the next step's pixel fragments: tap + 1 of this chunk, or tap 0 of the next (the last step of a convolution reads ahead into
            // the slot padding / the spare slot: nobody uses those values)
            const int noff = tap < 8 ? G::toff(tap + 1) : G::toff(0) + 64;
#pragma unroll
            for (int ps = 0; ps < PS; ++ps) {
#pragma unroll
                for (int cs = 0; cs < CS; ++cs) acc[cs][ps] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[tap % RING][cs], bfr[ps], acc[cs][ps], 0, 0, 0);
                bfr[ps] = *reinterpret_cast<const bf16x8*>(bch + ps * 16 * SB + noff);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

}  // namespace grk
