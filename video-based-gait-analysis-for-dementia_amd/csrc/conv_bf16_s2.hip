// bf16 path: the 3x3 stride-2 layers with a band (or a ring of rows) of the input resident in LDS.  The flattened, padded LDS plane and the MFMA roles are
// those of the frame-resident chain kernels (conv_bf16_chain.hip: its header describes them); the tile geometry and the k-loop with its weight ring are the
// LDS-plane family's one definition (conv_bf16_plane.h).
//
// ---- ONE 3x3 STRIDE-2 convolution (fuse layers' down paths hrnet.py:213-241, transitions hrnet.py:348-387, the stem's second convolution hrnet.py:470-475) with a
// band of the input resident in LDS.  conv_bf16_nhwc runs these layers at 0.05-0.16 of the matrix peak and 2-3 x their HBM time: 112-pixel tiles of ~60
// MFMAs per wave behind a slot table, a DMA wait, an LDS transpose and two barriers, 1 500 ms-scale launches of them per step (1.5 ms of 11).
// Stride 2 breaks the flattened plane of the stride-1 kernels (tap (dy, dx) of output (Y, X) is input (2Y + dy - 1, 2X + dx - 1): not a constant slot offset)
// -- unless the input is DE-INTERLEAVED by row and column parity into four sub-planes sub(py, px)[Y'][X'] = in[2Y' + py][2X' + px]: then tap (dy, dx) reads
// sub(py, px) at (Y + oy, X + ox) with py = (dy != 1), oy = -(dy == 0) and likewise for x, and inside its sub-plane every tap IS a constant offset again.
// The LDS-DMA does the de-interleaving for free: its source address is per lane.  Each sub-plane is flattened with pitch Wo + 1 (column X' = -1 is the shared
// zero column, row Y' = y0 - 1 the zero / halo row), R + 1 rows; output column o = (Y - y0)(Wo + 1) + X.  Everything else -- CP input channels per pass,
// weight ring, MFMA roles, in-place tile through LDS -- is as in conv_bf16_wide_band (the k-loop IS the same one: plane_kloop with this geometry's tap
// offsets); the epilogue adds the layer's fused addends (nearest-upsampled terms of
// the fuse sum, hrnet.py:258-265) before the ReLU.
#include "kernels.h"
#include "device.h"
#include "conv_bf16_plane.h"

namespace grk {

namespace {

template <int CP, int CT, int WO, int R>
struct S2Geom : PlaneGeom<CP, CT, WO, R, R> {             // the plane geometry of the OUTPUT (pitch Wo + 1) for each of the four sub-planes
    typedef PlaneGeom<CP, CT, WO, R, R> B;
    using B::P; using B::SB; using B::NT;
    static constexpr int UPS = SB / 16, OSB = 2 * CT + 32;
    static constexpr int SUBROWS = R + 1;
    static constexpr int SUB = (SUBROWS * P > NT * 16 + P + 1 ? SUBROWS * P : NT * 16 + P + 1);      // slots per sub-plane: its rows, or what the farthest tap of the last column tile reaches
    static constexpr int FILL_UNITS = (4 * SUB * UPS + 63) / 64 * 64;
    static constexpr int NFILL = (FILL_UNITS / 64 + 7) / 8;
    static constexpr int LDS = (4 * SUB * SB + SB > FILL_UNITS * 16 ? 4 * SUB * SB + SB : FILL_UNITS * 16);
    static_assert(LDS <= 160 * 1024 && NT * 16 * OSB <= LDS, "stride-2 band geometry");
    // byte offset of tap (dy, dx) from the lane's base (sub-plane (0,0), row 0, column slot 0); replaces the stride-1 offsets of PlaneGeom
    static constexpr int toff(int tap) {
        const int dy = tap / 3, dx = tap % 3, py = dy != 1, px = dx != 1, oy = dy == 0 ? -1 : 0, ox = dx == 0 ? -1 : 0;
        return ((py * 2 + px) * SUB + (oy + 1) * P + (ox + 1)) * SB;
    }
};

template <int CP, int CT, int WO, int R>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(S2Geom<CP, CT, WO, R>::LDS <= 80 * 1024 ? 4 : 2))) void conv_bf16_s2_band(const ConvArgs a) {
    typedef S2Geom<CP, CT, WO, R> G;
    constexpr int P = G::P, SB = G::SB, CS = G::CS, PS = G::PS, UPS = G::UPS, UPP = G::UPP, OSB = G::OSB, WI = 2 * WO;
    extern __shared__ __align__(16) unsigned char plane[];
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wcb = wave % G::WCB, pg = wave / G::WCB;
    const int ncb = a.CoutPad / CT;
    const int cbo = blockIdx.x % ncb, nb = blockIdx.x / ncb, n = nb / G::NB, band = nb - n * G::NB;
    if (n >= a.N) return;
    const int y0 = band * R;
    const u16* inb = reinterpret_cast<const u16*>(a.in) + (size_t)n * WI * WI * a.in_ctot + a.in_coff;
    const u16* zeros = reinterpret_cast<const u16*>(a.zeros);

    auto fill = [&](int c0, int cw) {                          // input channels c0 .. c0 + cw - 1 of the band, de-interleaved -> the four sub-planes, by LDS-DMA
        int ln = lane;
        asm volatile("" : "+v"(ln));                           // (keeps hipcc from hoisting the unit -> pixel map out of the pass loop into registers, as in the wide kernel)
#pragma unroll
        for (int i = 0; i < G::NFILL; ++i) {
            const int ub = (i * 8 + wave) * 64;
            if (ub >= G::FILL_UNITS) break;                    // wave-uniform
            const int u = ub + ln, slot = u / UPS, part = u - slot * UPS, sub = slot / G::SUB, ss = slot - sub * G::SUB, rr = ss / P, xx = ss - rr * P;
            const int py = sub >> 1, px = sub & 1, row = 2 * (y0 - 1 + rr) + py, col = 2 * (xx - 1) + px;
            const bool data = sub < 4 && rr < G::SUBROWS && !(py == 0 && rr == 0) && row >= 0 && row < WI && col >= 0 && col < WI && part * 8 < cw;
            dma16_builtin(data ? inb + (size_t)(row * WI + col) * a.in_ctot + c0 + part * 8 : zeros, plane + ub * 16);
        }
    };

    const int o_first = pg * PS * 16 + l15;
    const unsigned char* bread = plane + o_first * SB + lq * 16;
    const int co = cbo * CT + wcb * CS * 16;
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
        if (pass) __syncthreads();
        fill(c0, cw);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const u16* wpass = wg + (size_t)(c0 / 32) * 9 * wtap;       // the pass's first k-step; behind the layer's last one the stream ends: its own first steps again
        plane_kloop<G>(acc, wr, bread, wpass, wpass, wtap, cw / 32, pass == npass - 1, wlb);
    }
    // ---- epilogue: + fused addends (nearest-upsampled by 2^shift), ReLU, bf16; through LDS as whole channel rows
    const int Ho = WO;
    unsigned valid = 0;
    int pix[PS];                                               // (Y << 8) | X of this lane's column of tile ps
#pragma unroll
    for (int ps = 0; ps < PS; ++ps) {
        const int o = o_first + ps * 16, yy = o / P, X = o - yy * P;
        pix[ps] = ((y0 + yy) << 8) | X;
        if (X < WO && yy < R && y0 + yy < Ho) valid |= 1u << ps;
    }
#pragma unroll
    for (int k = 0; k < kMaxAdd; ++k) {
        if (k >= a.n_add) break;
        const int sh = a.add_shift[k], hs = Ho >> sh, ws = WO >> sh;
        const u16* ab = reinterpret_cast<const u16*>(a.add[k]) + (size_t)n * hs * ws * a.add_ctot[k] + a.add_coff[k] + co + lq * 4;
        u32x2 r[PS][CS];
#pragma unroll
        for (int ps = 0; ps < PS; ++ps) {
            const bool ok = (valid >> ps) & 1u;
            const int Y = ok ? pix[ps] >> 8 : 0, X = ok ? pix[ps] & 255 : 0;
            const u16* ap = ab + ((size_t)(Y >> sh) * ws + (X >> sh)) * a.add_ctot[k];
#pragma unroll
            for (int cs = 0; cs < CS; ++cs) r[ps][cs] = ok ? *reinterpret_cast<const u32x2*>(ap + cs * 16) : u32x2{0u, 0u};
        }
#pragma unroll
        for (int ps = 0; ps < PS; ++ps)
#pragma unroll
            for (int cs = 0; cs < CS; ++cs) {
                acc[cs][ps][0] += bf_lo(r[ps][cs][0]); acc[cs][ps][1] += bf_hi(r[ps][cs][0]);
                acc[cs][ps][2] += bf_lo(r[ps][cs][1]); acc[cs][ps][3] += bf_hi(r[ps][cs][1]);
            }
    }
    __syncthreads();                                           // every wave has finished reading the sub-planes
    unsigned char* owrite = plane + o_first * OSB + (wcb * CS * 16 + lq * 4) * 2;
#pragma unroll
    for (int ps = 0; ps < PS; ++ps)
#pragma unroll
        for (int cs = 0; cs < CS; ++cs)
            if (valid & (1u << ps)) *reinterpret_cast<u32x2*>(owrite + ps * 16 * OSB + cs * 32) = pack4_relu_if(acc[cs][ps], a.relu);
    __syncthreads();
    u16* outb = reinterpret_cast<u16*>(a.out) + (size_t)n * Ho * WO * a.out_ctot + a.out_coff + cbo * CT;
    const int cstore = a.Cout - cbo * CT;
#pragma unroll
    for (int i = 0; i < G::NUO; ++i) {
        const int u = i * 512 + tid, px = u / UPP, part = u - px * UPP, yy = px / WO, X = px - yy * WO;
        if (u < R * WO * UPP && y0 + yy < Ho && part * 8 < cstore)
            *reinterpret_cast<u32x4*>(outb + ((size_t)(y0 + yy) * WO + X) * a.out_ctot + part * 8) = *reinterpret_cast<const u32x4*>(plane + (yy * P + X) * OSB + part * 16);
    }
}

// ---- The narrow 3x3 stride-2 layers of the fuse down paths (32 / 64 input channels) as a WALK OVER OUTPUT ROWS.  These launches are neither compute- nor
// byte-bound in the band kernel above or in conv_bf16_nhwc (0.05-0.15 of the matrix peak at 1.9 TB/s: fill -> barrier -> k-loop -> epilogue -> store, one after
// another per workgroup).  Here a workgroup owns a segment of a frame's output rows; per output row Y it needs input rows 2Y - 1 .. 2Y + 1, of which two are new:
// they arrive by LDS-DMA one step ahead, DE-INTERLEAVED by column parity (odd columns with a leading zero slot, then even columns: tap dx reads odd index x, even
// index x, odd index x + 1 -- 16 consecutive slots for 16 output pixels), 16-byte parts XOR-swizzled by slot bits so that every fragment read is conflict-free.  A
// wave owns one (16-pixel tile, 16-channel block) of the row with that block's weights in its registers for the whole launch (9 x Cin/32 A fragments), so a step is
// 9 or 18 MFMAs per wave, an epilogue straight from the accumulators (bias, fused addends, ReLU, 8-byte stores) and ONE barrier; the ring is 6 input rows (25 KB), so
// four workgroups share a CU and cover each other's memory round trips.  Results equal the band kernel's bit for bit (same k order, same epilogue order).
template <int CIN, int COUT, int WO>
struct S2RowsGeom {
    static constexpr int WI = 2 * WO, SB = 2 * CIN, UPS = SB / 16, KS = CIN / 32;
    static constexpr int MT = (WO + 15) / 16, NBK = COUT / 16, ITEMS = MT * NBK;
    static constexpr int PO = 16 * MT + 1, PE = 16 * MT, SLOTS = PO + PE;      // odd-column plane (index 0 = column -1), even-column plane
    static constexpr int ROWB = SLOTS * SB, RING = 6;
    static constexpr int UNITS = SLOTS * UPS, NDMA = (UNITS + 63) / 64;      // 16-byte units of a row; wave-instructions per row
    static constexpr int LDS = RING * ROWB + 64 * 16;                         // + what the last instruction of the last row writes past it (masked lanes write nothing)
    static_assert(ITEMS <= 8 && 2 * NDMA <= 16 && (CIN == 32 || CIN == 64) && COUT % 16 == 0 && LDS <= 64 * 1024, "stride-2 row geometry");
    static __device__ __forceinline__ int swz(int slot) { return CIN == 32 ? (((slot >> 2) & 1) << 1) : (((slot >> 1) & 3) << 1); }
};

template <int CIN, int COUT, int WO>
__global__ __launch_bounds__(512) void conv_bf16_s2_rows(const ConvArgs a, int segs) {
    typedef S2RowsGeom<CIN, COUT, WO> G;
    constexpr int WI = G::WI, SB = G::SB, KS = G::KS;
    extern __shared__ __align__(16) unsigned char ring[];
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = blockIdx.x / segs, seg = blockIdx.x - n * segs;
    if (n >= a.N) return;
    const int rows_per = (WO + segs - 1) / segs, y_lo = seg * rows_per, y_hi = min(WO, y_lo + rows_per);
    const u16* inb = reinterpret_cast<const u16*>(a.in) + (size_t)n * WI * WI * a.in_ctot + a.in_coff;
    u16* outb = reinterpret_cast<u16*>(a.out) + (size_t)n * WO * WO * a.out_ctot + a.out_coff;
    const bool works = wave < G::ITEMS;
    const int nb = wave % G::NBK, mt = wave / G::NBK, co = nb * 16;

    bf16x8 wf[KS][9];
    f32x4 bias = f32x4{0.f, 0.f, 0.f, 0.f};
    if (works) {
        const u16* wg = reinterpret_cast<const u16*>(a.w);
#pragma unroll
        for (int kc = 0; kc < KS; ++kc)
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) wf[kc][tap] = *reinterpret_cast<const bf16x8*>(wg + (((size_t)kc * 9 + tap) * a.CoutPad + co + l15) * 32 + 8 * lq);
        bias = *reinterpret_cast<const f32x4*>(a.bias + co + 4 * lq);
    }
    for (int u = tid; u < G::LDS / 16; u += 512) reinterpret_cast<u32x4*>(ring)[u] = u32x4{0u, 0u, 0u, 0u};
    // this wave's share of a step's two new rows: wave-instructions q = wave, wave + 8 of the 2 x NDMA (row q / NDMA, instruction q % NDMA); per lane the unit's
    // (validity, source offset inside an input row): unit d = (slot, stored part) -> column 2 i - 1 (odd plane, i = slot) or 2 j (even plane), part = stored ^ swz(slot)
    int dq_row[2], dq_k[2], dq_off[2];
    bool dq_on[2], dq_lane[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q = wave + 8 * i;
        dq_on[i] = q < 2 * G::NDMA;
        dq_row[i] = q / G::NDMA; dq_k[i] = q - dq_row[i] * G::NDMA;
        const int d = dq_k[i] * 64 + lane, slot = d / G::UPS, sp = d - slot * G::UPS;
        const int col = slot < G::PO ? 2 * slot - 1 : 2 * (slot - G::PO);
        dq_lane[i] = dq_on[i] && d < G::UNITS && col >= 0 && col < WI && (slot < G::PO ? slot <= WO : slot - G::PO < WO);
        dq_off[i] = col * a.in_ctot + (sp ^ G::swz(slot)) * 8;
    }
    // fragment offsets of this wave's tile inside a ring row: tap dx reads odd index x (dx = 0), even index x (1), odd index x + 1 (2), x = 16 mt + l15
    unsigned foff[3][KS];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
        const int x = 16 * mt + l15, slot = dx == 1 ? G::PO + x : x + (dx >> 1);
#pragma unroll
        for (int kc = 0; kc < KS; ++kc) foff[dx][kc] = (unsigned)(slot * SB + (((4 * kc + lq) ^ G::swz(slot)) * 16));
    }
    auto request = [&](int y, int rr0) {                       // input rows 2 y, 2 y + 1 -> ring rows rr0, rr0 + 1 (wrapped by the caller)
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (dq_on[i]) {
                const int row = 2 * y + dq_row[i];
                int rr = rr0 + dq_row[i];
                rr = rr >= G::RING ? rr - G::RING : rr;
                if (dq_lane[i] && row < WI) dma16_builtin(inb + (size_t)row * WI * a.in_ctot + dq_off[i], ring + rr * G::ROWB + dq_k[i] * 1024);
            }
    };
    lds_barrier();                                             // the ring is zero (the halo slots and the row above the image stay zero: no DMA ever writes them ... see below)
    // ring row of input row r: (r + 2) mod 6 by a wrapping counter; row 2 y_lo - 1 (or the zero row above the image) sits at `cur`
    int cur = 0;
    if (y_lo > 0 && wave == 0) {                               // the segment's first output row needs input row 2 y_lo - 1: one extra row, by wave 0
#pragma unroll
        for (int k = 0; k < G::NDMA; ++k) {
            const int d = k * 64 + lane, slot = d / G::UPS, sp = d - slot * G::UPS;
            const int col = slot < G::PO ? 2 * slot - 1 : 2 * (slot - G::PO);
            const bool ok = d < G::UNITS && col >= 0 && col < WI && (slot < G::PO ? slot <= WO : slot - G::PO < WO);
            if (ok) dma16_builtin(inb + ((size_t)(2 * y_lo - 1) * WI + col) * a.in_ctot + (sp ^ G::swz(slot)) * 8, ring + cur * G::ROWB + k * 1024);
        }
    }
    request(y_lo, cur + 1);
#pragma unroll 1
    for (int y = y_lo; y < y_hi; ++y) {
        // fused addends of this row (nearest-upsampled by 2^shift), requested before the wait below so that it covers them
        u32x2 av[kMaxAdd];
        const int x = 16 * mt + l15;
        const bool px_ok = works && x < WO;
#pragma unroll
        for (int k = 0; k < kMaxAdd; ++k) {
            av[k] = u32x2{0u, 0u};
            if (k < a.n_add && px_ok) {
                const int sh = a.add_shift[k], ws = WO >> sh;
                av[k] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const u16*>(a.add[k]) + ((size_t)n * (WO >> sh) * ws + (size_t)(y >> sh) * ws + (x >> sh)) * a.add_ctot[k] + a.add_coff[k] + co + 4 * lq);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's pieces of rows 2 y, 2 y + 1 (requested a step ago) have landed
        lds_barrier();                                         // ... and everybody's; every wave is done with row 2 y - 2 (the next request overwrites it)
        f32x4 af[kMaxAdd];                                     // the addends as floats HERE: hipcc's own wait for their loads must not land behind the next request
#pragma unroll
        for (int k = 0; k < kMaxAdd; ++k) af[k] = f32x4{bf_lo(av[k][0]), bf_hi(av[k][0]), bf_lo(av[k][1]), bf_hi(av[k][1])};
        __builtin_amdgcn_sched_barrier(0);
        int nxt = cur + 3;
        nxt = nxt >= G::RING ? nxt - G::RING : nxt;
        if (y + 1 < y_hi) request(y + 1, nxt);
        if (works) {
            f32x4 acc = bias;
            const unsigned char* r0 = ring + cur * G::ROWB;
            int c1 = cur + 1, c2 = cur + 2;
            c1 = c1 >= G::RING ? c1 - G::RING : c1; c2 = c2 >= G::RING ? c2 - G::RING : c2;
            const unsigned char* r1 = ring + c1 * G::ROWB;
            const unsigned char* r2 = ring + c2 * G::ROWB;
#pragma unroll
            for (int kc = 0; kc < KS; ++kc)
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const unsigned char* rb = tap < 3 ? r0 : tap < 6 ? r1 : r2;
                    const bf16x8 px = *reinterpret_cast<const bf16x8*>(rb + foff[tap % 3][kc]);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[kc][tap], px, acc, 0, 0, 0);
                }
#pragma unroll
            for (int k = 0; k < kMaxAdd; ++k)
                if (k < a.n_add) { acc[0] += af[k][0]; acc[1] += af[k][1]; acc[2] += af[k][2]; acc[3] += af[k][3]; }
            if (a.relu) { acc[0] = relu_bits(acc[0]); acc[1] = relu_bits(acc[1]); acc[2] = relu_bits(acc[2]); acc[3] = relu_bits(acc[3]); }
            if (px_ok) *reinterpret_cast<u32x2*>(outb + ((size_t)y * WO + x) * a.out_ctot + co + 4 * lq) = u32x2{pack2(acc[0], acc[1]), pack2(acc[2], acc[3])};
        }
        cur += 2;
        cur = cur >= G::RING ? cur - G::RING : cur;
    }
}
// (the three shapes the band kernel lost on; on its own shapes -- 64 -> 128, 32 -> 128, 32 -> 32 @28->14 -- the walk ties with it: 15.1 against 14.5 us, not instantiated)
#define GRK_S2R_SHAPES(X) X(32, 64, 28) X(32, 32, 28) X(64, 64, 14)
template <int CIN, int COUT, int WO>
hipError_t launch_s2_rows(const ConvArgs& a, hipStream_t s) {
    typedef S2RowsGeom<CIN, COUT, WO> G;
    int cus = 0;
    GRK_TRY(device_cu_count(&cus));
    // segments of output rows per frame: several workgroups per CU where the frame count allows it, but never fewer than 7 rows per workgroup (each one loads
    // its channel blocks' weights: 18-74 KB from L2)
    int segs = 1;
    if (a.N < 4 * cus) segs = 2;
    if (WO == 28 && a.N * 2 < 4 * cus) segs = 4;
    return launch_k(conv_bf16_s2_rows<CIN, COUT, WO>, dim3(a.N * segs), dim3(512), G::LDS, s, a, segs);
}

template <int CP, int CT, int WO, int R>
hipError_t set_s2_lds() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(conv_bf16_s2_band<CP, CT, WO, R>), hipFuncAttributeMaxDynamicSharedMemorySize, S2Geom<CP, CT, WO, R>::LDS);
}
template <int CP, int CT, int WO, int R>
hipError_t launch_s2(const ConvArgs& a, hipStream_t s) {
    typedef S2Geom<CP, CT, WO, R> G;
    return launch_k(conv_bf16_s2_band<CP, CT, WO, R>, dim3(a.N * G::NB * (a.CoutPad / CT)), dim3(512), G::LDS, s, a);
}
// (CP, CT, Wo, R) per layer shape: the band is as tall as the four sub-planes' LDS allows
// Measured at 256 frames against conv_bf16_nhwc (profiles/r05_s2_band_vs_generic.txt): the band kernel wins where a workgroup's MFMA share is large enough to
// carry its fill -> barrier -> store round trip -- 64 -> 128 @28->14 (20.6 / 23.1 us against 30.2 / 35.1), 32 -> 128 @28->14 (10.5 / 17.3), 32 -> 32 @28->14
// (7.8 / 9.8), the stem's 64 -> 64 @112->56 (216 / 237) -- ties on the 14->7 layers and loses on 256 -> 64 (four passes, each with an exposed fill:
// 174 / 144), 32 -> 32 and 32 -> 64 @56->28 (7-row bands 26.7 / 40.7 against 27.6 / 34.4; 3-row bands with two workgroups per CU 35.0 / 47.5),
// 64 -> 64 @28->14 (17.7 / 12.9), 128 -> 256 @14->7 (30.1 / 24.0): those stay on the generic kernel and are not instantiated.
#define GRK_S2_SHAPES(X) X(64, 64, 56, 3) X(64, 128, 14, 14) X(32, 128, 14, 14) X(32, 32, 14, 14)

}  // namespace

hipError_t conv_bf16_s2_init() {
#define GRK_S2_SET(cp, ct, wo, r) GRK_TRY((set_s2_lds<cp, ct, wo, r>()));
    GRK_S2_SHAPES(GRK_S2_SET)
#undef GRK_S2_SET
    return hipSuccess;
}

// Stride-2 band kernel: 3x3, stride 2, even input size, <= 3 fused addends; (input channels per pass, output-channel tile) by the layer's channel counts.
static int s2_cp(const ConvArgs& a) { return a.CinPad >= 64 ? 64 : 32; }
static int s2_ct(const ConvArgs& a) { return a.CoutPad >= 128 ? 128 : a.CoutPad; }
static bool s2_rows_shape(const ConvArgs& a) {                 // the row-walking kernel's shapes (every add view 4-channel aligned: checked by the caller)
    if (!GRNET_AB(BF16_S2_ROWS, 1)) return false;
#define GRK_S2R_HAS(ci_, co_, wo_) if (a.CinPad == ci_ && a.Cin == ci_ && a.Cout == co_ && a.Wo == wo_) return true;
    GRK_S2R_SHAPES(GRK_S2R_HAS)
#undef GRK_S2R_HAS
    return false;
}
bool conv_bf16_s2_eligible(const ConvArgs& a) {
    if (a.ks != 3 || a.stride != 2 || a.H != a.W || a.Ho != a.Wo || a.H != 2 * a.Ho || a.CinPad % 32 != 0 || a.n_add > kMaxAdd || a.relu_from != 0) return false;
    if (a.in_ctot % 8 != 0 || a.in_coff % 8 != 0 || a.out_ctot % 8 != 0 || a.out_coff % 8 != 0 || a.Cout % 32 != 0 || a.CoutPad != a.Cout) return false;
    for (int k = 0; k < a.n_add; ++k)
        if (a.add_ctot[k] % 4 != 0 || a.add_coff[k] % 4 != 0) return false;
    if (s2_rows_shape(a)) return true;
    const int cp = s2_cp(a), ct = s2_ct(a);
    if (a.CinPad != cp) return false;                          // one pass (layers with more input channels lose to the generic kernel: see GRK_S2_SHAPES)
#define GRK_S2_HAS(cp_, ct_, wo_, r_) if (cp == cp_ && ct == ct_ && a.Wo == wo_) return true;
    GRK_S2_SHAPES(GRK_S2_HAS)
#undef GRK_S2_HAS
    return false;
}
hipError_t launch_conv_bf16_s2(const ConvArgs& a, hipStream_t s) {
    if (!conv_bf16_s2_eligible(a) || a.N < 1) return hipErrorInvalidValue;
    if (s2_rows_shape(a)) {
#define GRK_S2R_GO(ci_, co_, wo_) if (a.CinPad == ci_ && a.Cout == co_ && a.Wo == wo_) return launch_s2_rows<ci_, co_, wo_>(a, s);
        GRK_S2R_SHAPES(GRK_S2R_GO)
#undef GRK_S2R_GO
    }
    const int cp = s2_cp(a), ct = s2_ct(a);
#define GRK_S2_GO(cp_, ct_, wo_, r_) if (cp == cp_ && ct == ct_ && a.Wo == wo_) return launch_s2<cp_, ct_, wo_, r_>(a, s);
    GRK_S2_SHAPES(GRK_S2_GO)
#undef GRK_S2_GO
    return hipErrorInvalidValue;
}

}  // namespace grk
