// fp32 Winograd F(4x4,3x3) on 56x56 / 28x28 maps: what conv_wino4_f32 (4 waves) and conv_wino4w_f32 (8 waves) of conv_wino4.hip share -- the tile
// geometry, the workgroup decode, the epilogue-thread mapping with the residual prefetch, the raw-row DMA request and the half-patch input
// transform.  Each is defined ONCE here; the file keeps the two chunk loops (chunk / meet, and multiply with its barrier choreography: the
// two designs), the weight streams, the epilogue tile loops, launchers and eligibility.  The 1-D transforms bt_lo / bt_hi / at_f43, the wave
// priority and the buffer resource are in device.h: conv_wino4s.hip (small maps, register-resident) uses them too.  Included after device.h.
// How a piece is written here is part of what it compiles to.  hipcc simplifies a function BEFORE it inlines it, even a __forceinline__ one,
// so a piece that was inline text and becomes a function with by-value arguments is optimised out of its context first (an index division
// came out narrower, register allocation ties fell differently); the same piece taking its inputs BY REFERENCE, as a lambda's captures do,
// and filling a struct the caller owns compiles to the code of the inline text.  epi() and issue_raw() are written that way on purpose.
// What is NOT here for that reason -- the raw-row offset table, the lane mapping of the input transform, the epilogue tile -- is still
// written out in both kernels; NOTES_rejected.md 4.2 has the forms tried and by how much each differed.
#pragma once
#include "device.h"

namespace grk {

constexpr int wino4_tile_rows(int wd) { return 14 / (wd / 4); }       // tile rows of a workgroup's 14 tiles: 1 (56-wide maps) or 2 (28-wide)

// WD: map width, 56 or 28.  A workgroup's 14 tiles are one tile row of a 56-wide map (6 input rows) or two tile rows of 7 of a 28-wide one
// (10 input rows; 7 tile rows per image = 3.5 groups: the last group's lower half reads zeros and stores nothing).  CK: input channels per
// chunk, NT: threads per workgroup.  LDS: raw rows [2][CK][RAWW] (second buffer right behind the first), V [2][36][CK][16 tile slots] behind
// the room of two 56-wide raw buffers; the epilogue's [NT / 256][36 points][16 channels][MROW] reuses it.
template <int WD_, int CK_, int NT_>
struct Wino4Geom {
    static constexpr int WD = WD_, CK = CK_, NT = NT_;
    static constexpr int TPR = WD / 4, TRG = wino4_tile_rows(WD);      // tiles per tile row, tile rows per workgroup
    static constexpr int RAWW = (4 * TRG + 2) * WD, UPC = RAWW / 4;    // raw floats / 16-byte units per channel
    static constexpr int NRU = (CK * UPC + NT - 1) / NT;               // units of a chunk's raw rows per thread (3)
    static constexpr int VOFF = 2 * CK * 6 * 56, V = 36 * CK * 16;     // where V starts; floats of one V buffer
    static constexpr int MROW = 20, MTILE = 36 * 16 * MROW;            // epilogue: [point][channel][16 MFMA rows + 4]
    static constexpr size_t lds_bytes = sizeof(float) * (VOFF + 2 * V);      // 58 368 B (CK 8) / 116 736 B (CK 16)
    static_assert(WD == 56 || WD == 28, "tile geometry");
    static_assert(2 * CK * RAWW <= VOFF && sizeof(float) * (NT / 256) * MTILE <= lds_bytes, "the epilogue tiles reuse the staging area");

    // workgroup id -> (image, tile-row group r of the image, channel block by); XCD-aware order where the launch form says so
    static __device__ __forceinline__ void decode(const ConvArgs& a, int id, int& img, int& r, int& by) {
        int bx;
        if (a.xcd) {
            const int j = id >> 3, x = id & 7, q = j / a.gy;
            by = j - q * a.gy;
            bx = x * (a.gx >> 3) + q;
        } else {
            bx = id / a.gy;
            by = id - bx * a.gy;
        }
        const int groups = ((a.H >> 2) + TRG - 1) / TRG;               // tile-row groups per image (14 or 4)
        img = bx / groups;
        r = bx - img * groups;
    }

    // The raw rows of a chunk by LDS-DMA (rows are contiguous in the NCHW plane; 16-byte units, NRU per thread): roff[i] is unit
    // i * NT + tid's byte offset in the chunk's channels, -1 = no unit or a row outside the image
    static __device__ __forceinline__ void issue_raw(const int (&roff)[NRU], const __amdgpu_buffer_rsrc_t& r_rsrc, float* const& raw, int chunk, const int& wave, const int& HW) {
        const int soff = chunk * (CK * 4) * HW;
        float* dst = raw + (chunk & 1) * (CK * RAWW);
#pragma unroll
        for (int i = 0; i < NRU; ++i)
            if (roff[i] >= 0) __builtin_amdgcn_raw_ptr_buffer_load_lds(r_rsrc, (GRNET_LDS_AS void*)(dst + (i * NT + wave * 64) * 4), 16, roff[i], soff, 0, 0);
        asm volatile("" ::: "memory");                   // later loads stay behind these requests: the vmcnt waits of the chunk loops count on the order
    }

    // The epilogue thread t (0..255 of a 64-channel half) = (channel ec of the pass's 16, tile et): 4 output rows of 4 pixels from row eorow,
    // tile column etx; on: it has a tile inside the image
    struct Epi { int ec, et, etx, eorow; bool on; };
    static __device__ __forceinline__ void epi(const int& t, const int& r, const int& H, Epi& e) {
        e.ec = t / 14;
        e.et = t - e.ec * 14;
        const int etro = e.et / TPR;
        e.etx = e.et - etro * TPR;
        e.eorow = 4 * (TRG * r + etro);
        e.on = t < 14 * 16 && e.eorow < H;
    }
    // the residual rows of e's tile of channel co (the caller has checked that there are any): requested a pass ahead of their use
    static __device__ __forceinline__ void fetch_res(f32x4 (&radd)[4], const ConvArgs& a, const Epi& e, int img, int co, int HW) {
        const float* ap = a.add[0] + ((size_t)img * a.add_ctot[0] + a.add_coff[0] + co) * HW + e.eorow * WD + 4 * e.etx;
#pragma unroll
        for (int i = 0; i < 4; ++i) radd[i] = *reinterpret_cast<const f32x4*>(ap + i * WD);
    }
};

// The input transform of HALF a 6x6 patch, in four stages (the 4-wave kernel spreads them over the clusters of a chunk).  A thread reads all
// 6 rows of its tile's patch (own columns 4t .. 4t+3 as one 16-byte read per row, 4t-1 / 4t+4 from the neighbour lanes by DPP, whose
// out-of-row zero is the image's left padding) and produces rows 3*half .. 3*half+2 of B^T d B.
template <typename G>
struct Wino4Patch {
    float d[6][6], e[3][6];
    __device__ __forceinline__ void read(const float* rp) {              // 6 LDS reads
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(rp + i * G::WD);
            d[i][1] = v[0]; d[i][2] = v[1]; d[i][3] = v[2]; d[i][4] = v[3];
        }
    }
    __device__ __forceinline__ void halo(bool real) {                    // real: not an idle lane (those supply the zeros)
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            d[i][0] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(G::WD == 56 || real ? d[i][4] : 0.f), 0x111, 0xf, 0xf, true));   // row_shr:1
            d[i][5] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(real ? d[i][1] : 0.f), 0x101, 0xf, 0xf, true));                  // row_shl:1
        }
    }
    __device__ __forceinline__ void rows(int half) {                     // three rows of B^T d, per column; half: wave-uniform
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const float col[6] = {d[0][j], d[1][j], d[2][j], d[3][j], d[4][j], d[5][j]};
            if (half == 0) bt_lo(col, e[0][j], e[1][j], e[2][j]);
            else bt_hi(col, e[0][j], e[1][j], e[2][j]);
        }
    }
    __device__ __forceinline__ void cols(float* vp) const {              // (B^T d) B: all 6 columns of the three rows, 18 LDS writes
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) {
            float o[6];
            bt_lo(e[rr], o[0], o[1], o[2]);
            bt_hi(e[rr], o[3], o[4], o[5]);
#pragma unroll
            for (int c = 0; c < 6; ++c) vp[(rr * 6 + c) * (G::CK * 16)] = o[c];
        }
    }
};

}  // namespace grk
