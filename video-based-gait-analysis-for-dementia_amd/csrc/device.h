// Device-side helpers shared by the kernels: vector types, bf16 packing, the LDS-only barrier, wave reductions, the 1-D transforms of Winograd F(4,3),
// wave priority and buffer resources, the LDS-DMA forms, and the timing-only hooks of the diagnostic build.  Included by the .hip files after kernels.h; the .cpp files do not include it.
#pragma once
#include "kernels.h"

// LDS-DMA operands of __builtin_amdgcn_global_load_lds
#define GRNET_GLOBAL_AS __attribute__((address_space(1)))
#define GRNET_LDS_AS __attribute__((address_space(3)))

namespace grk {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short s16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float bf2f(u16 h) { return __uint_as_float((unsigned)h << 16); }
// two floats -> two bf16 (round to nearest even) in ONE instruction: v_cvt_pk_bf16_f32.  The integer form ((u + 0x7fff + (u >> 16 & 1)) >> 16, five
// vector instructions per value) made the in-place epilogue of the chain kernels -- 4 values x CS x PS tiles per wave and convolution -- cost a third
// of a k-loop, and the epilogues of the 1x1 and narrow layers are dozens of such values per handful of MFMAs.
__device__ __forceinline__ unsigned pack2(float lo, float hi) { return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, bf16x2)); }
// relu on the bits: negative floats (and -0) are negative integers; one v_max_i32, where fmaxf(x, 0) costs a canonicalising v_max first
__device__ __forceinline__ float relu_bits(float x) { const int i = __float_as_int(x); return __int_as_float(i > 0 ? i : 0); }
__device__ __forceinline__ unsigned relu_pk(unsigned v) {      // max(x, 0) on two packed bf16: v_pk_max_i16
    const s16x2 a = __builtin_bit_cast(s16x2, v);
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(a, s16x2{0, 0}));
}
// an accumulator's four values -> ReLU -> four bf16 (8 bytes); the second form applies the ReLU where the layer has one (relu: wave-uniform)
__device__ __forceinline__ u32x2 pack4_relu(const f32x4 v) { return u32x2{pack2(relu_bits(v[0]), relu_bits(v[1])), pack2(relu_bits(v[2]), relu_bits(v[3]))}; }
__device__ __forceinline__ u32x2 pack4_relu_if(f32x4 v, int relu) {
    if (relu) { v[0] = relu_bits(v[0]); v[1] = relu_bits(v[1]); v[2] = relu_bits(v[2]); v[3] = relu_bits(v[3]); }
    return u32x2{pack2(v[0], v[1]), pack2(v[2], v[3])};
}
__device__ __forceinline__ float bf_lo(unsigned v) { return __uint_as_float(v << 16); }
__device__ __forceinline__ float bf_hi(unsigned v) { return __uint_as_float(v & 0xffff0000u); }
// q / d for 0 <= q < 2^20, 0 < d < 2^20 through one fp32 reciprocal multiply (exact: the +0.5 keeps the quotient of an exact multiple away from the
// rounding edge); an integer division by a run-time value costs ~40 VALU instructions, and a tile of a 32-channel layer has only ~1000 cycles of MFMAs
__device__ __forceinline__ int fdiv(int q, float inv_d) { return (int)(((float)q + 0.5f) * inv_d); }

// Workgroup barrier for LDS data only: every wave's LDS operations so far are done; vector-memory operations (DMAs, loads, stores) stay in flight.
// (__syncthreads() also waits for vmcnt(0): it would drain pending DMAs -- a pending DMA is a pending LDS write to its fence -- and loads requested up front.)
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// 64-lane xor butterfly: every lane ends with the result
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// 1-D input transforms of Winograd F(4,3).  B^T rows 0..2 / 3..5 (Lavin & Gray):  [4 0 -5 0 1 0] [0 -4 -4 1 1 0] [0 4 -4 -1 1 0] /
// [0 -2 -1 2 1 0] [0 2 -1 -2 1 0] [0 4 0 -5 0 1]
__device__ __forceinline__ void bt_lo(const float* d, float& r0, float& r1, float& r2) {
    const float t1 = fmaf(-4.f, d[2], d[4]), t2 = fmaf(-4.f, d[1], d[3]);
    r0 = fmaf(4.f, d[0], fmaf(-5.f, d[2], d[4]));
    r1 = t1 + t2;
    r2 = t1 - t2;
}
__device__ __forceinline__ void bt_hi(const float* d, float& r3, float& r4, float& r5) {
    const float u1 = d[4] - d[2], u2 = 2.f * (d[3] - d[1]);
    r3 = u1 + u2;
    r4 = u1 - u2;
    r5 = fmaf(4.f, d[1], fmaf(-5.f, d[3], d[5]));
}
// the 1-D output transform: A^T = [1 1 1 1 1 0] [0 1 -1 2 -2 0] [0 1 1 4 4 0] [0 1 -1 8 -8 1]; rows, then columns of A^T M A go through it.  ADD: + add
// behind each result (the column pass adds the bias there; written into the same expressions, the epilogues compile as they did with the sums spelled out)
template <bool ADD = false>
__device__ __forceinline__ void at_f43(const float* m, float& s0, float& s1, float& s2, float& s3, float add = 0.f) {
    const float p12 = m[1] + m[2], m12 = m[1] - m[2], p34 = m[3] + m[4], m34 = m[3] - m[4];
    auto out = [&](float v) { return ADD ? v + add : v; };
    s0 = out(m[0] + p12 + p34);
    s1 = out(fmaf(2.f, m34, m12));
    s2 = out(fmaf(4.f, p34, p12));
    s3 = out(fmaf(8.f, m34, m12) + m[5]);
}

// wave priority of a layer (ConvArgs::prio): 1 = on the critical chain, >= 2 = the pole of it
__device__ __forceinline__ void set_wave_prio(int prio) {
    if (prio == 1) __builtin_amdgcn_s_setprio(1);
    else if (prio >= 2) __builtin_amdgcn_s_setprio(3);
}
// raw buffer resource over `bytes` bytes from p: offsets past the end load zeros and store nothing
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* p, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, bytes, 0x00020000);
}

// ---- LDS-DMA: lane l's 16 bytes land at the wave's LDS base + 16 l; the source address is per lane.  Four forms.
// The builtin: the compiler knows of the DMA and counts it in its own waits.
__device__ __forceinline__ void dma16_builtin(const u16* src, unsigned char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const GRNET_GLOBAL_AS void*)src, (GRNET_LDS_AS void*)lds_wave_base, 16, 0, 0);
}
// Inline asm, NOT __builtin_amdgcn_global_load_lds: while an LDS-DMA hipcc knows of is in flight, every wait it puts in front of an LDS operand read is
// lgkmcnt(0) and the reads are not hoisted -- conv_bf16_nhwc's tap loop was `ds_read, s_waitcnt lgkmcnt(0), v_mfma` 63 times over, one exposed LDS round trip per
// MFMA.  The kernel waits for its pieces itself (s_waitcnt vmcnt(0) in front of every chunk's barrier), so the compiler does not have to know.  M0 = the wave's LDS
// byte address (one wait state between its write and the DMA); every lane is on (padding units fetch zeros).
__device__ __forceinline__ void dma16(const u16* src, u16* lds_wave_base) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(__builtin_amdgcn_readfirstlane((unsigned)(size_t)lds_wave_base)) : "memory");
}
// LDS-DMA pieces the compiler does not know of: lane l's 16 bytes land at lds + 16 l (M0 = LDS byte address of the piece).
// uniform base + 32-bit lane offset, only the lanes of `mask` (all lanes are on around it: the callers are in uniform control flow)
__device__ __forceinline__ void dma16_masked(unsigned off, const void* base, unsigned lds, unsigned long long mask) {
    asm volatile("s_mov_b32 m0, %2\n\ts_mov_b64 exec, %3\n\tglobal_load_lds_dwordx4 %0, %1\n\ts_mov_b64 exec, -1" ::"v"(off), "s"(base), "s"(lds), "s"(mask) : "memory");
}
// the same with all lanes: lane l's 16 bytes at base + off land at lds + 16 l.  One wait state between the M0 write and the DMA that reads it.
__device__ __forceinline__ void dma16_uniform(unsigned off, const void* base, unsigned lds) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(off), "s"(base), "s"(lds) : "memory");
}

// ---- Timing-only hooks of the diagnostic build (make ABLATION=1): ablation bits and phase clocks.  In the product build bit() is the constant
// false -- `if (!abl::bit(a.dbg, 2)) kloop(...)` is the bare call -- and Ticks is an empty type whose members do nothing.
// The __device__ counter arrays exist in the diagnostic build only (each file declares its own under #ifdef, so the product code object gains no
// globals): a kernel names one as GRK_ABL_COUNTERS(g_array) in its flush().
#ifdef GRNET_ABLATION
#define GRK_ABL_COUNTERS(sym) (sym)
#else
#define GRK_ABL_COUNTERS(sym) (static_cast<unsigned long long*>(nullptr))
#endif
namespace abl {
#ifdef GRNET_ABLATION
__device__ __forceinline__ int bit(int flags, int b) { return flags & b; }      // non-zero = set (the masked bits, so that `!abl::bit(f, b)` compiles as `!(f & b)` does)
// Shader-clock ticks of K phases of one thread's life: mark(k) adds the ticks since the previous mark (or the construction) to phase k, count(k) adds one,
// flush() adds the sums to K device counters from the threads of `who`.
template <int K>
struct Ticks {
    bool on;
    unsigned long long last, acc[K];
    __device__ __forceinline__ explicit Ticks(bool enabled) : on(enabled), last(__builtin_readcyclecounter()), acc{} {}
    __device__ __forceinline__ void mark(int k) {
        if (on) { const unsigned long long t = __builtin_readcyclecounter(); acc[k] += t - last; last = t; }
    }
    __device__ __forceinline__ void count(int k) { acc[k] += 1; }
    __device__ __forceinline__ void flush(unsigned long long* counters, bool who) const {
        if (on && who)
            for (int k = 0; k < K; ++k) atomicAdd(&counters[k], acc[k]);
    }
};
// host side of a report: everything on the stream has finished; the K device counters of `symbol` -> h, and zeroed for the next launch
template <int K>
void take_counters(const void* symbol, unsigned long long (&h)[K], hipStream_t s) {
    const unsigned long long z[K] = {};
    (void)hipStreamSynchronize(s);
    (void)hipMemcpyFromSymbol(h, symbol, sizeof(h));
    (void)hipMemcpyToSymbol(symbol, z, sizeof(z));
}
#else
__device__ __forceinline__ constexpr bool bit(int, int) { return false; }
template <int K>
struct Ticks {
    __device__ __forceinline__ explicit Ticks(bool) {}
    __device__ __forceinline__ void mark(int) {}
    __device__ __forceinline__ void count(int) {}
    __device__ __forceinline__ void flush(unsigned long long*, bool) const {}
};
#endif
}  // namespace abl

}  // namespace grk
