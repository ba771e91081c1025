// GRU gait-feature encoder (reference: BidirectionalModel.forward, use_pareFeat=True, eval;
// lib/models/layers/gait_feat_encoder.py:79-104; nn.GRU equations, gate order r,z,n, h0 = 0).
//   1. xin = x + cparam_mpl(cparams)           per-joint 3->128 locally connected (line 85)
//   2. gi  = xin . W_ih^T + b_ih               fp32 MFMA GEMM batched over all b*T rows, per direction
//   3. recurrence, one workgroup per (sequence, direction): W_hh is stored transposed [k][g] so the
//      900 gate rows are read coalesced from L2 each step; h lives in LDS
//   4. layer 1 on concat(fwd,bwd) of layer 0 (steps 2-3 again)
//   5. heads: speed/step MLPs on the final hidden states, phase MLP + tanh on the layer-1 outputs
#include "kernels.h"
#include "device.h"

#include <cstdlib>

namespace grk {

// C[M][N] = A[M][K] . B[N][K]^T + bias[N]   (row-major, K contiguous, K % 4 == 0, 16-byte aligned rows)
// 64x64 tile, K-chunk 32, 4 waves as 2x2, each 2x2 MFMA 16x16x4 tiles.  LDS row stride 34 floats:
// the 32 lanes of a half-wave (16 rows x 2 k) fall on 32 distinct banks (2*row + k).
constexpr int kGemmLd = 34;
// blockIdx.z = K slice (split-K for GEMMs with few rows: slice z covers [z*kc, (z+1)*kc) and writes its partial sums to C + z*zstride;
// gemm_splitk_reduce adds the slices in a fixed order and the bias).  kc is a multiple of 32; one slice = the plain GEMM.
__global__ __launch_bounds__(256) void gemm_nt_bias_f32(const float* __restrict__ A, const float* __restrict__ B,
                                                          const float* __restrict__ bias, float* __restrict__ C, int M, int N, int K,
                                                          int ldc, int kc, size_t zstride) {
    __shared__ __align__(16) float As[64 * kGemmLd];
    __shared__ __align__(16) float Bs[64 * kGemmLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l15 = lane & 15, lq = lane >> 4;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int lr = tid >> 3, lk = (tid & 7) * 4;
    const int kbeg = blockIdx.z * kc, kend = (kbeg + kc < K) ? kbeg + kc : K;
    C += (size_t)blockIdx.z * zstride;
    for (int k0 = kbeg; k0 < kend; k0 += 32) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = lr + 32 * h;
            f32x4 va = f32x4{0.f, 0.f, 0.f, 0.f}, vb = f32x4{0.f, 0.f, 0.f, 0.f};
            if (k0 + lk < kend) {
                if (m0 + r < M) va = *reinterpret_cast<const f32x4*>(A + (size_t)(m0 + r) * K + k0 + lk);
                if (n0 + r < N) vb = *reinterpret_cast<const f32x4*>(B + (size_t)(n0 + r) * K + k0 + lk);
            }
            f32x2* pa = reinterpret_cast<f32x2*>(As + r * kGemmLd + lk);
            f32x2* pb = reinterpret_cast<f32x2*>(Bs + r * kGemmLd + lk);
            pa[0] = f32x2{va[0], va[1]}; pa[1] = f32x2{va[2], va[3]};
            pb[0] = f32x2{vb[0], vb[1]}; pb[1] = f32x2{vb[2], vb[3]};
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = As[(wm * 32 + i * 16 + l15) * kGemmLd + kk * 4 + lq];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = Bs[(wn * 32 + j * 16 + l15) * kGemmLd + kk * 4 + lq];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn * 32 + j * 16 + l15;
            if (n >= N) continue;
            const float bv = bias ? bias[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm * 32 + i * 16 + lq * 4 + r;
                if (m < M) C[(size_t)m * ldc + n] = acc[i][j][r] + bv;
            }
        }
}

// C = bias + sum_z P[z]  (fixed order: deterministic)
__global__ __launch_bounds__(256) void gemm_splitk_reduce(const float* __restrict__ P, const float* __restrict__ bias, float* __restrict__ C, int M, int N,
                                                            int ldc, int splits) {
    const long total = (long)M * N;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int m = (int)(i / N), n = (int)(i - (long)m * N);
        float v = bias ? bias[n] : 0.f;
        for (int z = 0; z < splits; ++z) v += P[(size_t)z * total + i];
        C[(size_t)m * ldc + n] = v;
    }
}

thread_local float* g_gemm_ws = nullptr;       // split-K partial sums: scratch lent by the caller (the handle), see set_gemm_workspace
thread_local size_t g_gemm_ws_floats = 0;
void set_gemm_workspace(float* ws, size_t floats) { g_gemm_ws = ws; g_gemm_ws_floats = floats; }

thread_local TapSink* g_taps = nullptr;        // installed by the C entry points for ONE armed temporal call (grnet_temporal_taps)
hipError_t tap_copy(const char* name, const float* src, std::initializer_list<size_t> shape, hipStream_t s) {
    TapSink& t = *g_taps;
    size_t count = 1;
    std::string line = std::string("tap ") + name + " " + std::to_string(t.used);
    for (size_t d : shape) { count *= d; line += " " + std::to_string(d); }
    if (t.used + count > t.floats) return hipErrorInvalidValue;      // the entry point sized the buffer with *_tap_floats: never reached unless they disagree
    GRK_TRY(hipMemcpyAsync(t.buf + t.used, src, count * sizeof(float), hipMemcpyDeviceToDevice, s));
    t.used += count;
    t.layout += line + "\n";
    return hipSuccess;
}
size_t gru_tap_floats(int b, int T) {
    const size_t rows = (size_t)b * T;
    return rows * (2 * 3072 + 4 * 900 + 2 * 600 + 100 + 4) + (size_t)b * (1200 + 2 * 100 + 3);
}

hipError_t launch_gemm_nt_bias(const float* A, const float* B, const float* bias, float* C, int M, int N, int K, int ldc, hipStream_t s) {
    if (K % 4 != 0) return hipErrorInvalidValue;
    const int blocks = ((N + 63) / 64) * ((M + 63) / 64);
    // few rows (a clip of 16 frames is ONE row block): 47 workgroups would stream a 37 MB weight matrix; split K so that >= ~512 do
    int splits = 1;
    if (blocks < 128 && K >= 512) {                          // (at 188 blocks -- 8 clips x 32 frames -- splitting already costs more than it saves)
        splits = (512 + blocks - 1) / blocks;
        if (splits > 16) splits = 16;
        if (splits > K / 128) splits = K / 128;
    }
    if (g_taps) {                                             // the census of GEMM shapes an armed call ran, with the slice count the launch below takes
        int sp = splits;
        if (sp > 1) sp = (K + (((K + sp - 1) / sp + 31) / 32 * 32) - 1) / (((K + sp - 1) / sp + 31) / 32 * 32);
        g_taps->layout += "gemm " + std::to_string(M) + " " + std::to_string(N) + " " + std::to_string(K) + " " + std::to_string(sp) + "\n";
    }
    if (splits <= 1) {
        GRK_TRY(launch_k(gemm_nt_bias_f32, dim3((N + 63) / 64, (M + 63) / 64, 1), dim3(256), 0, s, A, B, bias, C, M, N, K, ldc, K, (size_t)0));
        return hipGetLastError();
    }
    const int kc = ((K + splits - 1) / splits + 31) / 32 * 32;
    splits = (K + kc - 1) / kc;
    float* part = nullptr;
    const size_t need = (size_t)splits * M * N;
    const bool lent = g_gemm_ws && need <= g_gemm_ws_floats;  // the handle's scratch: no allocation in the call (graph-capturable);
    if (lent) part = g_gemm_ws;                               // the launches of one stream run one after another, so one region serves them all
    else GRK_TRY(hipMallocAsync(reinterpret_cast<void**>(&part), need * sizeof(float), s));
    hipError_t e = launch_k(gemm_nt_bias_f32, dim3((N + 63) / 64, (M + 63) / 64, splits), dim3(256), 0, s, A, B, static_cast<const float*>(nullptr), part, M, N, K, N, kc,
                            (size_t)M * N);
    if (e == hipSuccess) {
        const long total = (long)M * N;
        e = launch_k(gemm_splitk_reduce, dim3((unsigned)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048)), dim3(256), 0, s, part, bias, C, M, N, ldc, splits);
    }
    if (!lent) hipFreeAsync(part, s);
    return e != hipSuccess ? e : hipGetLastError();
}

// xc[r, c*24+j] = sum_f cp[r,f] * wc[c,f,j];  xin = x + xc   (dropout is the identity in eval)
__global__ __launch_bounds__(256) void gru_prep_kernel(const float* __restrict__ x, const float* __restrict__ cp,
                                                         const float* __restrict__ wc, float* __restrict__ xc, float* __restrict__ xin,
                                                         long rows) {
    const long total = rows * 3072;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / 3072;
        const int e = (int)(i % 3072), c = e / 24, j = e % 24;
        const float v = cp[r * 3] * wc[(c * 3 + 0) * 24 + j] + cp[r * 3 + 1] * wc[(c * 3 + 1) * 24 + j] +
                        cp[r * 3 + 2] * wc[(c * 3 + 2) * 24 + j];
        xc[i] = v;
        xin[i] = x[i] + v;
    }
}

// One (sequence, direction) per workgroup of 1024 threads.  gi: (2, b*T, 900); w_hhT: [dir](300, 900).
constexpr int kH = 300;
__global__ __launch_bounds__(1024) void gru_recurrent_kernel(const float* __restrict__ gi, const float* __restrict__ w_hhT_f,
                                                               const float* __restrict__ w_hhT_b, const float* __restrict__ b_hh_f,
                                                               const float* __restrict__ b_hh_b, float* __restrict__ out,
                                                               float* __restrict__ hfin, int hfin_off, int b, int T) {
    __shared__ float h[kH];
    __shared__ float gh[3 * kH];
    const int seq = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    const float* wT = dir ? w_hhT_b : w_hhT_f;
    const float* bh = dir ? b_hh_b : b_hh_f;
    const float* gid = gi + (size_t)dir * b * T * 900;
    if (tid < kH) h[tid] = 0.f;
    __syncthreads();
    for (int step = 0; step < T; ++step) {
        const int t = dir ? T - 1 - step : step;
        if (tid < 3 * kH) {
            float acc = bh[tid];
#pragma unroll 10
            for (int k = 0; k < kH; ++k) acc += h[k] * wT[(size_t)k * 900 + tid];
            gh[tid] = acc;
        }
        __syncthreads();
        if (tid < kH) {
            const float* g = gid + ((size_t)seq * T + t) * 900;
            const float r = 1.f / (1.f + expf(-(g[tid] + gh[tid])));
            const float z = 1.f / (1.f + expf(-(g[kH + tid] + gh[kH + tid])));
            const float nn = tanhf(g[2 * kH + tid] + r * gh[2 * kH + tid]);
            const float hn = (1.f - z) * nn + z * h[tid];
            h[tid] = hn;
            out[((size_t)seq * T + t) * (2 * kH) + dir * kH + tid] = hn;
        }
        __syncthreads();
    }
    if (tid < kH) hfin[(size_t)seq * (4 * kH) + hfin_off + dir * kH + tid] = h[tid];
}


// ---------------------------------------------------------------------------------------------
// Recurrence with W_hh RESIDENT for the whole sequence (long clips: BASELINE configs[3] reassembles 10 000 frames before the GRU).
// The kernel above pulls the 1.08 MB of W_hh from L2 every step (~10 us per step).  Here the 900 x 300 matrix of one (sequence,
// direction) is split over kGruSlices workgroups: slice s owns the hidden units [s*38, s*38+38) = 114 gate rows, kept in REGISTERS
// for all T steps (lane l holds rows l and l+64, wave w the 38 columns [w*38, w*38+38): 76 weights per lane).  A step is
//   1. every workgroup collects the 300 values of h_{t-1}: its own slice from LDS, the others from the exchange buffer, where each
//      value travels as ONE 8-byte granule {value, step tag} written with a device-scope (sc1) store and polled with device-scope
//      loads -- no flag, no fence, placement-independent (guide: handoff-1to1);
//   2. per wave: its 38 h values are broadcast lane by lane (v_readlane -> scalar operand), 76 FMAs per lane, no cross-lane
//      reduction; the 8 column-slices are added through LDS in a fixed order (deterministic);
//   3. the 38 owners of a hidden unit apply the gate equations and publish h_t.
// Two granule buffers alternate by step parity: a workgroup can be at most one step ahead of its peers (it cannot finish step t+1
// without their h_t), so a buffer is never overwritten while somebody still reads it.  The buffer is zeroed before the launch and
// tags are step+1, so no stale tag can match.  The kGruSlices workgroups of a group are all resident for sure when the grid is
// <= one workgroup per CU (b <= 16 here); larger batches use the kernel above (they have sequences to run in parallel instead).
constexpr int kGruSlices = 8, kGruUnits = 38, kGruCols = 38;      // 8 x 38 = 304 >= 300
__global__ __launch_bounds__(512) void gru_recurrent_split_kernel(const float* __restrict__ gi, const float* __restrict__ w_hhT_f,
                                                                    const float* __restrict__ w_hhT_b, const float* __restrict__ b_hh_f,
                                                                    const float* __restrict__ b_hh_b, float* __restrict__ out,
                                                                    float* __restrict__ hfin, int hfin_off, int b, int T,
                                                                    unsigned long long* __restrict__ xbuf, unsigned* __restrict__ fault) {
    __shared__ float h[kGruSlices * kGruCols];                 // 304: columns >= 300 stay 0
    __shared__ float part[kGruSlices][128];
    // block id = slice*8 + (group % 8) + 64*(group / 8): the 8 slices of a group have ids congruent mod 8 -> one XCD (speed only)
    const int slot = blockIdx.x & 7, slice = (blockIdx.x >> 3) & 7, group = (blockIdx.x >> 6) * 8 + slot;
    if (group >= 2 * b) return;
    const int seq = group >> 1, dir = group & 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* wT = dir ? w_hhT_b : w_hhT_f;
    const float* bh = dir ? b_hh_b : b_hh_f;
    const float* gid = gi + (size_t)dir * b * T * 900;
    const int u0 = slice * kGruUnits, nu = min(kGruUnits, kH - u0);          // hidden units of this slice
    const int c0 = wave * kGruCols;                                           // columns of this wave
    // local row lr in [0, 114): gate lr / 38, unit u0 + lr % 38
    float W0[kGruCols], W1[kGruCols];
    {
        const int lr0 = lane, lr1 = lane + 64;
        const int g0 = lr0 / kGruUnits, j0 = lr0 - g0 * kGruUnits, g1 = lr1 / kGruUnits, j1 = lr1 - g1 * kGruUnits;
        const bool v0 = j0 < nu, v1 = lr1 < 3 * kGruUnits && j1 < nu;
#pragma unroll
        for (int k = 0; k < kGruCols; ++k) {
            const int c = c0 + k;
            W0[k] = (v0 && c < kH) ? wT[(size_t)c * 900 + g0 * kH + u0 + j0] : 0.f;
            W1[k] = (v1 && c < kH) ? wT[(size_t)c * 900 + g1 * kH + u0 + j1] : 0.f;
        }
    }
    float bias3[3] = {0.f, 0.f, 0.f};
    if (tid < nu) {
#pragma unroll
        for (int g = 0; g < 3; ++g) bias3[g] = bh[g * kH + u0 + tid];
    }
    if (tid < kGruSlices * kGruCols) h[tid] = 0.f;
    unsigned long long* xb = xbuf + (size_t)group * 2 * kH;                 // [parity][300] granules of this (sequence, direction)
    float h_own = 0.f;                                                      // h of the unit this thread owns (tid < nu)
    __syncthreads();
    for (int step = 0; step < T; ++step) {
        const int t = dir ? T - 1 - step : step;
        float g3[3] = {0.f, 0.f, 0.f};
        if (tid < nu) {                                                     // this step's input projections: in flight under the exchange
            const float* g = gid + ((size_t)seq * T + t) * 900 + u0 + tid;
            g3[0] = g[0]; g3[1] = g[kH]; g3[2] = g[2 * kH];
        }
        if (step > 0 && tid < kH && (tid < u0 || tid >= u0 + nu)) {          // collect h_{t-1} of the other slices
            const unsigned long long* src = xb + (size_t)((step - 1) & 1) * kH + tid;
            unsigned long long v;
            unsigned polls = 0;
            do {
                v = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } while ((unsigned)(v >> 32) != (unsigned)step && ++polls < (1u << 26));   // tag of step-1's result = (step-1)+1
            // the bound (tens of seconds) is never reached while the launcher's residency check holds; if it ever is, the result is
            // poisoned with NaN instead of hanging the GPU
            const bool arrived = (unsigned)(v >> 32) == (unsigned)step;
            if (!arrived && fault) *fault = 1u;                   // host-visible: the next temporal call reports it and falls back (grnet.cpp)
            h[tid] = arrived ? __uint_as_float((unsigned)v) : __builtin_nanf("");
        }
        __syncthreads();
        const float hv = (lane < kGruCols) ? h[c0 + lane] : 0.f;
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int k = 0; k < kGruCols; ++k) {
            const float hk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hv), k));
            a0 = fmaf(W0[k], hk, a0);
            a1 = fmaf(W1[k], hk, a1);
        }
        part[wave][lane] = a0;
        part[wave][lane + 64] = a1;
        __syncthreads();
        if (tid < nu) {
            float gh[3];
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                float acc = bias3[g];
#pragma unroll
                for (int w = 0; w < kGruSlices; ++w) acc += part[w][g * kGruUnits + tid];
                gh[g] = acc;
            }
            const float r = 1.f / (1.f + expf(-(g3[0] + gh[0])));
            const float z = 1.f / (1.f + expf(-(g3[1] + gh[1])));
            const float nn = tanhf(g3[2] + r * gh[2]);
            const float hn = (1.f - z) * nn + z * h_own;
            h_own = hn;
            h[u0 + tid] = hn;                                               // read again only after the next barrier
            out[((size_t)seq * T + t) * (2 * kH) + dir * kH + u0 + tid] = hn;
            const unsigned long long granule = ((unsigned long long)(unsigned)(step + 1) << 32) | (unsigned long long)__float_as_uint(hn);
            __hip_atomic_store(xb + (size_t)(step & 1) * kH + u0 + tid, granule, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // no barrier here: the next step's collect writes h[] entries of OTHER slices only, and its barrier orders h[own] and part[]
    }
    if (tid < nu) hfin[(size_t)seq * (4 * kH) + hfin_off + dir * kH + u0 + tid] = h_own;
}

// ---------------------------------------------------------------------------------------------
// Round 5: the same split (8 workgroups per (sequence, direction), W_hh in registers, granule hand-off), 1.0 instead of 1.8 us per step:
//  * the hand-off stays in the XCD's L2.  An agent-scope (sc1) store DROPS the line from the L2 (MI355X_MICROARCH, visibility table), so
//    every poll of the kernel above goes out to the fabric and queues behind the step's input-projection reads.  The 8 slices of a group
//    have block ids congruent mod 8 -- dealt to ONE XCD by the dispatcher as observed, which HIP does not promise: so every workgroup
//    publishes its HW_REG_XCC_ID at start (agent scope), reads its 7 peers' and, only if all 8 agree, stores its granules with WORKGROUP
//    scope (write-through L1 -> the shared L2, the line stays there) -- the polls remain sc1 loads (L1-bypassing, L2-served).  A group that
//    spans XCDs keeps the agent-scope stores.  The decision is the same in the 8 workgroups (same 8 values).
//  * ONE barrier per step and a third of the vector instructions: the kernel above gives a wave a COLUMN slice of all 114 rows (38
//    v_readlane + 76 FMAs, the 8 column-slices summed through LDS behind a second barrier by 38 threads, 24 LDS reads each).  Here a wave
//    owns ROWS: 5 hidden units x 3 gates = 15 rows, a row spread over the 4 lanes of a quad (lane = 4 * (3 * unit + gate) + cq); a lane
//    holds the 76 weights of its row for the columns {16 i + 4 cq + e}.  Per step and wave: 19 ds_read_b128 of h (the four quarters of a
//    quad read 64 contiguous bytes; all quads the same address -> broadcast) feeding 38 v_pk_fma_f32, two DPP adds across the quad, two
//    ds_bpermute to bring the z and n sums to the r lane, the gate equations in 5 lanes of EVERY wave at once.  h is double-buffered in LDS
//    by step parity (the gate lanes write h_t into the other buffer while slower waves still read h_{t-1}).
//  * the input projections of step t + 1 are requested at the start of step t, IN FRONT of the polls (behind them: +0.2 us per step).
//  * FAST: sigmoid as v_rcp(1 + v_exp(-x)), tanh as 2 sigmoid(2x) - 1 (1 ulp instructions; |error| < 3e-7 per gate) instead of expf /
//    division / tanhf: 0.4 us of the step's serial tail.
// Same arithmetic per element otherwise, except for the order of the 300-term sums (quarters, even/odd columns).
constexpr int kGruQuadCols = 76, kGruWaveUnits = 5;              // 4 x 76 = 304 columns; 8 waves x 5 = 40 >= 38 units
template <bool FAST>
__device__ __forceinline__ float gru_sigmoid(float x) {
    if (FAST) return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.442695040888963f * x));
    return 1.f / (1.f + expf(-x));
}
template <bool FAST>
__global__ __launch_bounds__(512) void gru_recurrent_rows_kernel(const float* __restrict__ gi, const float* __restrict__ w_hhT_f,
                                                                   const float* __restrict__ w_hhT_b, const float* __restrict__ b_hh_f,
                                                                   const float* __restrict__ b_hh_b, float* __restrict__ out,
                                                                   float* __restrict__ hfin, int hfin_off, int b, int T,
                                                                   unsigned long long* __restrict__ xbuf, int force_agent, unsigned* __restrict__ fault) {
    __shared__ __align__(16) float h[2][4 * kGruQuadCols];       // [parity][304]: columns >= 300 stay 0
    __shared__ int same_xcd;
    const int slot = blockIdx.x & 7, slice = (blockIdx.x >> 3) & 7, group = (blockIdx.x >> 6) * 8 + slot;
    if (group >= 2 * b) return;
    const int seq = group >> 1, dir = group & 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* wT = dir ? w_hhT_b : w_hhT_f;
    const float* bh = dir ? b_hh_b : b_hh_f;
    const float* gid = gi + (size_t)dir * b * T * 900;
    const int u0 = slice * kGruUnits, nu = min(kGruUnits, kH - u0);
    {   // placement: {1, XCC id} of every slice of this group, behind the granules of all groups
        unsigned long long* place = xbuf + (size_t)b * 2 * 2 * kH + (size_t)group * kGruSlices;
        if (tid < kGruSlices) {
            unsigned xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
            if (tid == slice) __hip_atomic_store(place + slice, (1ull << 32) | xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            unsigned long long v;
            unsigned polls = 0;
            do {
                v = __hip_atomic_load(place + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } while ((unsigned)(v >> 32) != 1u && ++polls < (1u << 26));
            const bool ok = (unsigned)(v >> 32) == 1u && (unsigned)v == xcc;
            const unsigned long long all = __ballot(ok);
            if (tid == 0) same_xcd = (all & 0xFFull) == 0xFFull && !force_agent;
        }
    }
    const int q = lane >> 2, cq = lane & 3, ul = q / 3, gate = q - ul * 3;
    const int j = wave * kGruWaveUnits + ul;                     // unit of this lane within the slice
    const bool row_ok = q < 3 * kGruWaveUnits && j < nu;
    const bool owner = row_ok && gate == 0 && cq == 0;           // applies the gate equations for unit u0 + j
    f32x2 W[kGruQuadCols / 2];
#pragma unroll
    for (int i = 0; i < kGruQuadCols / 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 16 * i + 4 * cq + e;
            W[2 * i + (e >> 1)][e & 1] = (row_ok && c < kH) ? wT[(size_t)c * 900 + gate * kH + u0 + j] : 0.f;
        }
    float bias3[3] = {0.f, 0.f, 0.f};
    if (owner) {
#pragma unroll
        for (int g = 0; g < 3; ++g) bias3[g] = bh[g * kH + u0 + j];
    }
    for (int i = tid; i < 2 * 4 * kGruQuadCols; i += 512) (&h[0][0])[i] = 0.f;
    unsigned long long* xb = xbuf + (size_t)group * 2 * kH;
    float h_own = 0.f;
    float g3[3] = {0.f, 0.f, 0.f};
    if (owner) {
        const float* g = gid + ((size_t)seq * T + (dir ? T - 1 : 0)) * 900 + u0 + j;
        g3[0] = g[0]; g3[1] = g[kH]; g3[2] = g[2 * kH];
    }
    __syncthreads();
    const bool local = same_xcd != 0;
    for (int step = 0; step < T; ++step) {
        const int t = dir ? T - 1 - step : step;
        const float* hb = h[step & 1];
        float* hn_buf = h[(step + 1) & 1];
        float gn[3] = {0.f, 0.f, 0.f};
        if (owner && step + 1 < T) {                                        // the NEXT step's input projections: a whole step to arrive
            const float* g = gid + ((size_t)seq * T + (dir ? t - 1 : t + 1)) * 900 + u0 + j;
            gn[0] = g[0]; gn[1] = g[kH]; gn[2] = g[2 * kH];
        }
        if (step > 0 && tid < kH && (tid < u0 || tid >= u0 + nu)) {          // collect h_{t-1} of the other slices
            const unsigned long long* src = xb + (size_t)((step - 1) & 1) * kH + tid;
            unsigned long long v;
            unsigned polls = 0;
            do {
                v = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } while ((unsigned)(v >> 32) != (unsigned)step && ++polls < (1u << 26));   // tag of step-1's result = (step-1)+1
            // the bound (tens of seconds) is never reached while the launcher's residency check holds; if it ever is, the result is
            // poisoned with NaN instead of hanging the GPU
            const bool arrived = (unsigned)(v >> 32) == (unsigned)step;
            if (!arrived && fault) *fault = 1u;                   // host-visible: the next temporal call reports it and falls back to agent-scope stores (grnet.cpp)
            h[step & 1][tid] = arrived ? __uint_as_float((unsigned)v) : __builtin_nanf("");
        }
        __syncthreads();
        f32x2 acc0 = {0.f, 0.f}, acc1 = {0.f, 0.f};
#pragma unroll
        for (int i = 0; i < kGruQuadCols / 4; ++i) {
            const f32x4 hv = *reinterpret_cast<const f32x4*>(hb + 16 * i + 4 * cq);
            acc0 = __builtin_elementwise_fma(W[2 * i], f32x2{hv[0], hv[1]}, acc0);
            acc1 = __builtin_elementwise_fma(W[2 * i + 1], f32x2{hv[2], hv[3]}, acc1);
        }
        float sum = (acc0[0] + acc1[0]) + (acc0[1] + acc1[1]);
        sum += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(sum), 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
        sum += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(sum), 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
        const float sz = __shfl(sum, lane + 4, 64), sn = __shfl(sum, lane + 8, 64);                            // the z and n rows of this unit
        if (owner) {
            const float r = gru_sigmoid<FAST>(g3[0] + (bias3[0] + sum));
            const float z = gru_sigmoid<FAST>(g3[1] + (bias3[1] + sz));
            const float pre = g3[2] + r * (bias3[2] + sn);
            const float nn = FAST ? 2.f * gru_sigmoid<true>(2.f * pre) - 1.f : tanhf(pre);
            const float hn = (1.f - z) * nn + z * h_own;
            h_own = hn;
            const unsigned long long granule = ((unsigned long long)(unsigned)(step + 1) << 32) | (unsigned long long)__float_as_uint(hn);
            unsigned long long* dst = xb + (size_t)(step & 1) * kH + u0 + j;
            if (local) __hip_atomic_store(dst, granule, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);     // first: seven workgroups wait for it
            else __hip_atomic_store(dst, granule, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            hn_buf[u0 + j] = hn;
            out[((size_t)seq * T + t) * (2 * kH) + dir * kH + u0 + j] = hn;
        }
#pragma unroll
        for (int g = 0; g < 3; ++g) g3[g] = gn[g];
        // no second barrier: this step's writes go to the OTHER h buffer; the buffer read here is written again only behind the next barrier
    }
    if (owner) hfin[(size_t)seq * (4 * kH) + hfin_off + dir * kH + u0 + j] = h_own;
}

// hidden (rows,100) -> LeakyReLU(0.05) -> Linear(100 -> nout) [-> tanh]
__global__ __launch_bounds__(64) void mlp_out_kernel(const float* __restrict__ hidden, const float* __restrict__ w2,
                                                       const float* __restrict__ b2, float* __restrict__ out, int nout, int ld_out,
                                                       int col_off, int do_tanh) {
    const long r = blockIdx.x;
    const int lane = threadIdx.x;
    float hv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int k = lane + 64 * i;
        float v = k < 100 ? hidden[r * 100 + k] : 0.f;
        hv[i] = v > 0.f ? v : 0.05f * v;
    }
    for (int o = 0; o < nout; ++o) {
        float acc = hv[0] * w2[o * 100 + lane] + (lane + 64 < 100 ? hv[1] * w2[o * 100 + lane + 64] : 0.f);
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s, 64);
        if (lane == 0) {
            acc += b2[o];
            out[r * ld_out + col_off + o] = do_tanh ? tanhf(acc) : acc;
        }
    }
}

hipError_t launch_gru(const float* x, const float* cparams, GruWeights w, GruWorkspace ws, float* y, float* phase, float* xc,
                      int b, int T, hipStream_t s) {
    const long rows = (long)b * T;
    hipError_t e;
    int blocks = (int)((rows * 3072 + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    GRK_TRY(launch_k(gru_prep_kernel, dim3(blocks), dim3(256), 0, s, x, cparams, w.cparam_w, xc, ws.xin, rows));
    const size_t urows = (size_t)rows, ub = (size_t)b;
    GRK_TRY(tap("gru.xc", xc, {urows, 3072}, s));
    GRK_TRY(tap("gru.xin", ws.xin, {urows, 3072}, s));
    const float* layer_in = ws.xin;
    int in_size = 3072;
    float* layer_out[2] = {ws.l0, ws.l1};
    for (int layer = 0; layer < 2; ++layer) {
        for (int d = 0; d < 2; ++d) {
            e = launch_gemm_nt_bias(layer_in, w.w_ih[layer][d], w.b_ih[layer][d], ws.gi + (size_t)d * rows * 900, (int)rows, 900, in_size, 900, s);
            if (e != hipSuccess) return e;
            static const char* const gi_name[2][2] = {{"gru.gi00", "gru.gi01"}, {"gru.gi10", "gru.gi11"}};
            GRK_TRY(tap(gi_name[layer][d], ws.gi + (size_t)d * rows * 900, {urows, 900}, s));
        }
        const int split_env = ws.mode & 15;                  // GRNET_OPT_GRU_MODE; 0 = one workgroup per (sequence, direction)
        // the 8 slices of a (sequence, direction) spin on each other: every workgroup of the grid must be resident at once, i.e. the
        // grid may not exceed one 512-thread workgroup per CU of THIS device (256 on MI355X; fewer on a partitioned or smaller part)
        const int split_grid = 64 * ((2 * b + 7) / 8);
        int cus = 0;
        GRK_TRY(device_cu_count(&cus));
        if (split_env && ws.xbuf && b <= 16 && T >= 8 && split_grid <= cus) {
            // W_hh resident in registers, split over 8 workgroups per (sequence, direction); the exchange buffer (granules + placement table) starts zeroed
            // 3 (default): rows per wave, one barrier per step, hand-off inside the XCD's L2 where the group's placement allows, v_exp / v_rcp gate functions;
            // 2: the same with expf / tanhf; 1: round 3's column slices, two barriers per step, agent-scope hand-off.  GRNET_OPT_GRU_MODE + 16: agent-scope
            // granule stores whatever the placement (the path a group spanning XCDs takes)
            const int force_agent = (ws.mode >> 4) & 1;
            GRK_TRY(hipMemsetAsync(ws.xbuf, 0, (size_t)b * kGruXbufU64PerSeq * sizeof(unsigned long long), s));
            if (split_env == 1)
                GRK_TRY(launch_k(gru_recurrent_split_kernel, dim3(split_grid), dim3(512), 0, s, (const float*)ws.gi, w.w_hh[layer][0], w.w_hh[layer][1],
                                 w.b_hh[layer][0], w.b_hh[layer][1], layer_out[layer], ws.hfin, layer * 600, b, T, ws.xbuf, ws.fault));
            else
                GRK_TRY(launch_k(split_env == 2 ? gru_recurrent_rows_kernel<false> : gru_recurrent_rows_kernel<true>, dim3(split_grid), dim3(512), 0, s, (const float*)ws.gi,
                                 w.w_hh[layer][0], w.w_hh[layer][1], w.b_hh[layer][0], w.b_hh[layer][1], layer_out[layer], ws.hfin, layer * 600, b, T, ws.xbuf, force_agent, ws.fault));
        } else {
            GRK_TRY(launch_k(gru_recurrent_kernel, dim3(b, 2), dim3(1024), 0, s, ws.gi, w.w_hh[layer][0], w.w_hh[layer][1],
                             w.b_hh[layer][0], w.b_hh[layer][1], layer_out[layer], ws.hfin, layer * 600, b, T));
        }
        GRK_TRY(tap(layer ? "gru.l1" : "gru.l0", layer_out[layer], {urows, 600}, s));
        layer_in = layer_out[layer];
        in_size = 600;
    }
    GRK_TRY(tap("gru.hfin", ws.hfin, {ub, 1200}, s));
    // heads: hidden activations reuse the gi workspace
    float* hid = ws.gi;
    if ((e = launch_gemm_nt_bias(ws.hfin, w.speed_w0, w.speed_b0, hid, b, 100, 1200, 100, s)) != hipSuccess) return e;
    GRK_TRY(tap("gru.hid_speed", hid, {ub, 100}, s));
    GRK_TRY(launch_k(mlp_out_kernel, dim3(b), dim3(64), 0, s, hid, w.speed_w2, w.speed_b2, y, 1, 3, 0, 0));
    float* hid2 = hid + (size_t)b * 100;
    if ((e = launch_gemm_nt_bias(ws.hfin, w.step_w0, w.step_b0, hid2, b, 100, 1200, 100, s)) != hipSuccess) return e;
    GRK_TRY(tap("gru.hid_step", hid2, {ub, 100}, s));
    GRK_TRY(launch_k(mlp_out_kernel, dim3(b), dim3(64), 0, s, hid2, w.step_w2, w.step_b2, y, 2, 3, 1, 0));
    GRK_TRY(tap("gru.avg", y, {ub, 3}, s));
    float* hid3 = hid2 + (size_t)b * 100;
    if ((e = launch_gemm_nt_bias(ws.l1, w.phase_w0, w.phase_b0, hid3, (int)rows, 100, 600, 100, s)) != hipSuccess) return e;
    GRK_TRY(tap("gru.hid_phase", hid3, {urows, 100}, s));
    GRK_TRY(launch_k(mlp_out_kernel, dim3((unsigned)rows), dim3(64), 0, s, hid3, w.phase_w2, w.phase_b2, phase, 4, 4, 0, 1));
    GRK_TRY(tap("gru.phase", phase, {urows, 4}, s));
    return hipGetLastError();
}

}  // namespace grk
