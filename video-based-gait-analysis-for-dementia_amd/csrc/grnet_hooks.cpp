// The single-op test and timing hooks: one convolution, one BasicBlock chain or one upsampling on tensors the caller supplies, through the
// launchers the forward uses, and the timers of tools/.  None of this runs in a forward.
#include "grnet_impl.h"

namespace {

// Device memory of one hook call: what alloc() hands out is freed when the hook returns, whichever way it returns -- on the way through
// its launches that is after the final hipStreamSynchronize.
struct HookBuffers {
    std::vector<void*> ptrs;
    HookBuffers() = default;
    HookBuffers(const HookBuffers&) = delete;
    HookBuffers& operator=(const HookBuffers&) = delete;
    ~HookBuffers() { for (void* p : ptrs) (void)hipFree(p); }
    template <class T = void>
    T* alloc(size_t bytes) {                                // nullptr: hipMalloc failed
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        return static_cast<T*>(p);
    }
};

// `reps` calls of launch() on stream s between two HIP events: the milliseconds between the events.  *err (a hipError_t or a GRNET_* code, 0 = fine)
// is the first failure: no call is made once it is set, the caller's earlier launches included.  < 0: the events could not be created, nothing ran.
template <class F, class E>
float timed_launches(hipStream_t s, int reps, F&& launch, E* err) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
        if (e0) (void)hipEventDestroy(e0);
        return -1.f;
    }
    (void)hipEventRecord(e0, s);
    for (int i = 0; i < reps && !*err; ++i) *err = launch();
    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return ms;
}

}  // namespace

// Test hook on a bf16 handle: (n,cin,h,w) f32 NCHW in / out, converted to and from NHWC bf16 around ONE conv launch.  Addend k (grnet_op_conv2d_adds) is an
// (n,add_ctot[k],ho>>add_shift[k],wo>>add_shift[k]) f32 tensor, stored as NHWC bf16 with all its channels (padded to a multiple of 8); the launch
// reads channels add_coff[k] .. + cout of it.
int grnet::op_conv2d_bf16(const float* in_dev, int n, int cin, int hgt, int wid, const float* w_host, const float* bias_host, int cout, int ks,
                          int stride, int relu, const float* add_dev, float* out_dev, int tile_hint, hipStream_t s) {
    const int zero = 0;
    return op_conv2d_bf16_adds(in_dev, n, cin, hgt, wid, w_host, bias_host, cout, ks, stride, relu, add_dev ? 1 : 0, &add_dev, &cout, &zero, &zero, out_dev,
                               tile_hint, s);
}
int grnet::op_conv2d_bf16_adds(const float* in_dev, int n, int cin, int hgt, int wid, const float* w_host, const float* bias_host, int cout, int ks, int stride,
                               int relu, int n_add, const float* const* adds_dev, const int* add_ctot, const int* add_coff, const int* add_shift, float* out_dev,
                               int tile_hint, hipStream_t s) {
    const float* add_dev = n_add ? adds_dev[0] : nullptr;
    HookBuffers mem;
    const int taps = ks * ks, pad = ks / 2, cin8 = (cin + 7) / 8 * 8, cin_pad = (cin + 31) / 32 * 32, cout_pad = (cout + 31) / 32 * 32;
    const int ho = (hgt + 2 * pad - ks) / stride + 1, wo = (wid + 2 * pad - ks) / stride + 1, cout8 = (cout + 7) / 8 * 8;
    std::vector<uint16_t> wp((size_t)taps * cout_pad * cin_pad, 0);
    std::vector<float> bp(cout_pad, 0.f);
    for (int co = 0; co < cout; ++co) {
        if (bias_host) bp[co] = bias_host[co];
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < taps; ++t)
                wp[(((size_t)(ci / 32) * taps + t) * cout_pad + co) * 32 + ci % 32] = f32_to_bf16(w_host[((size_t)co * cin + ci) * taps + t]);
    }
    if (tile_hint == 3001) {                               // conv_bf16_stem on this one convolution: fp32 NCHW in, (n,cout,112,112) f32 out
        if (!conv_stem_eligible(cin, cout, ks, stride, hgt, wid, add_dev ? 1 : 0)) return fail(GRNET_EINVAL, "shape not eligible for the bf16 stem kernel");
        std::vector<double> wf((size_t)cout * cin * 9);
        for (size_t i = 0; i < wf.size(); ++i) wf[i] = w_host[i];
        std::vector<unsigned short> sw(4 * 64 * 8);
        pack_stem_weights_bf16(wf.data(), sw.data());
        std::vector<float> bh(64, 0.f);
        if (bias_host) for (int c = 0; c < 64; ++c) bh[c] = bias_host[c];
        void *swd = mem.alloc(sw.size() * 2), *bhd = mem.alloc(256), *od = mem.alloc((size_t)n * ho * wo * 64 * 2);
        if (!swd || !bhd || !od) return fail(GRNET_ENOMEM, "hipMalloc failed");
        hipError_t e = hipMemcpy(swd, sw.data(), sw.size() * 2, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(bhd, bh.data(), 256, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = launch_conv_bf16_stem(in_dev, swd, static_cast<const float*>(bhd), od, 64, 0, n, relu, s);
        if (e == hipSuccess) e = launch_nhwc_bf16_to_nchw_f32(od, out_dev, n, 64, ho, wo, 64, 0, s);
        hipError_t e2 = hipStreamSynchronize(s);
        if (e != hipSuccess || e2 != hipSuccess) return fail(GRNET_EHIP, std::string("bf16 stem conv: ") + hipGetErrorString(e != hipSuccess ? e : e2));
        return 0;
    }
    if (n_add < 0 || n_add > kMaxAdd) return fail(GRNET_EINVAL, "at most " + std::to_string(kMaxAdd) + " addends");
    for (int k = 0; k < n_add; ++k)
        if (!adds_dev[k] || add_ctot[k] < 1 || add_coff[k] < 0 || add_coff[k] + cout > add_ctot[k] || add_shift[k] < 0 || add_shift[k] > 3 ||
            ho % (1 << add_shift[k]) != 0 || wo % (1 << add_shift[k]) != 0)
            return fail(GRNET_EINVAL, "bad addend " + std::to_string(k) + " (channels holding [coff, coff + cout), a map of (ho, wo) >> shift)");
    void* xadds[kMaxAdd] = {};
    int add_ct8[kMaxAdd] = {};
    for (int k = 0; k < n_add; ++k) add_ct8[k] = (add_ctot[k] + 7) / 8 * 8;
    const size_t in_b = (size_t)n * hgt * wid * cin8 * 2, out_b = (size_t)n * ho * wo * cout8 * 2;
    void *wd = mem.alloc(wp.size() * 2), *bd = mem.alloc(bp.size() * 4), *xin = mem.alloc(in_b), *xout = mem.alloc(out_b);
    bool alloc_ok = wd && bd && xin && xout;
    for (int k = 0; k < n_add && alloc_ok; ++k)
        alloc_ok = (xadds[k] = mem.alloc((size_t)n * (ho >> add_shift[k]) * (wo >> add_shift[k]) * add_ct8[k] * 2)) != nullptr;
    if (!alloc_ok) return fail(GRNET_ENOMEM, "hipMalloc failed");
    if (hipMemcpy(wd, wp.data(), wp.size() * 2, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(bd, bp.data(), bp.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail(GRNET_EHIP, "hipMemcpy of the test weights failed");
    hipError_t e = launch_nchw_f32_to_nhwc_bf16(in_dev, xin, n, cin, hgt, wid, cin8, s);
    for (int k = 0; k < n_add && e == hipSuccess; ++k)
        e = launch_nchw_f32_to_nhwc_bf16(adds_dev[k], xadds[k], n, add_ctot[k], ho >> add_shift[k], wo >> add_shift[k], add_ct8[k], s);
    ConvArgs a{};
    a.in = static_cast<const float*>(xin); a.in_ctot = cin8; a.in_coff = 0; a.N = n; a.Cin = cin8; a.H = hgt; a.W = wid;
    a.Cout = cout; a.Ho = ho; a.Wo = wo;
    a.out = static_cast<float*>(xout); a.out_ctot = cout8; a.out_coff = 0;
    a.w = static_cast<const float*>(wd); a.bias = static_cast<const float*>(bd); a.CinPad = cin_pad; a.CoutPad = cout_pad;
    a.ks = ks; a.stride = stride; a.relu = relu;
    a.n_add = n_add;
    for (int k = 0; k < n_add; ++k) {
        a.add[k] = static_cast<const float*>(xadds[k]); a.add_ctot[k] = add_ct8[k]; a.add_coff[k] = add_coff[k]; a.add_shift[k] = add_shift[k];
    }
    a.zeros = zeros;
    a.pw_stream = 1;
    if (const char* d = GRNET_AB_STR(CONV_DBG)) a.dbg = atoi(d);
    const bool wide = tile_hint == 3003, s2 = tile_hint == 3004;      // conv_bf16_wide_band / conv_bf16_s2_band on this one convolution
    if ((wide && !conv_bf16_wide_eligible(a)) || (s2 && !conv_bf16_s2_eligible(a)))
        return fail(GRNET_EINVAL, "shape not eligible for the band kernel");
    auto launch_one = [&]() { return wide ? launch_conv_bf16_wide(a, s) : s2 ? launch_conv_bf16_s2(a, s) : launch_conv_bf16(a, s, tile_hint); };
    if (e == hipSuccess) e = launch_one();
    if (const char* r = GRNET_AB_STR(CONV_REPS)) {       // timing loop for tools/bf16_micro.py
        const int reps = atoi(r);
        const float ms = timed_launches(s, reps, launch_one, &e);
        const double mb = (in_b + out_b * (add_dev ? 2 : 1)) / 1e6;
        fprintf(stderr, "[bf16_micro] cin %d cout %d k %d s %d hw %d n %d hint %d add %d: %.2f us/launch, %.0f MB algorithmic = %.2f TB/s\n", cin, cout, ks, stride,
                hgt, n, tile_hint, add_dev ? 1 : 0, ms * 1e3f / reps, mb, mb / (ms * 1e3 / reps));
    }
    if (e == hipSuccess) e = launch_nhwc_bf16_to_nchw_f32(xout, out_dev, n, cout, ho, wo, cout8, 0, s);
    hipError_t e2 = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(GRNET_EHIP, std::string("bf16 conv: ") + hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(GRNET_EHIP, std::string("bf16 conv kernel: ") + hipGetErrorString(e2));
    return 0;
}

// Test / timing hook on a bf16 handle: a chain of nconv 3x3 convolutions c -> c on (n,c,w,w) f32 NCHW in / out (converted to and from NHWC
// bf16 around ONE conv_bf16_chain launch).  w_host: nconv x (c,c,3,3), bias_host: nconv x (c).  reps > 0: also times `reps` back-to-back
// launches with HIP events (*us_out: us per launch).
int grnet::op_conv_chain_bf16(const float* in_dev, int n, int c, int wid, int nconv, const float* w_host, const float* bias_host, float* out_dev, int reps,
                              float* us_out, hipStream_t s) {
    if (dtype != 1) return fail(GRNET_ESTATE, "grnet_op_conv_chain needs a bf16 handle");
    if (!conv_bf16_chain_eligible(c, wid) || nconv < 2 || nconv > kMaxChain || (nconv & 1) || n < 1) return fail(GRNET_EINVAL, "shape not eligible for the chain kernel");
    const size_t wel = (size_t)9 * c * c;
    std::vector<uint16_t> wp(wel * nconv, 0);
    for (int i = 0; i < nconv; ++i)
        for (int co = 0; co < c; ++co)
            for (int ci = 0; ci < c; ++ci)
                for (int t = 0; t < 9; ++t)
                    wp[i * wel + (((size_t)(ci / 32) * 9 + t) * c + co) * 32 + ci % 32] = f32_to_bf16(w_host[i * wel + ((size_t)co * c + ci) * 9 + t]);
    const size_t act_b = (size_t)n * wid * wid * c * 2;
    HookBuffers mem;
    void *wd = mem.alloc(wp.size() * 2), *bd = mem.alloc((size_t)nconv * c * 4), *xin = mem.alloc(act_b), *xout = mem.alloc(act_b);
    if (!wd || !bd || !xin || !xout) return fail(GRNET_ENOMEM, "hipMalloc failed");
    hipError_t e = hipMemcpy(wd, wp.data(), wp.size() * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(bd, bias_host, (size_t)nconv * c * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_nchw_f32_to_nhwc_bf16(in_dev, xin, n, c, wid, wid, c, s);
    ChainArgs ca{};
    ca.in = xin; ca.in_ctot = c; ca.in_coff = 0; ca.out = xout; ca.out_ctot = c; ca.out_coff = 0; ca.N = n; ca.nconv = nconv;
    if (conv_bf16_chain_launches(c, wid, nconv) > 1)
        for (int k = 0; k + 1 < nconv / 2; ++k) {
            if (!(ca.mid[k] = mem.alloc(act_b))) return fail(GRNET_ENOMEM, "hipMalloc failed");
            ca.mid_ctot[k] = c; ca.mid_coff[k] = 0;
        }
    for (int i = 0; i < nconv; ++i) { ca.w[i] = static_cast<const uint16_t*>(wd) + i * wel; ca.bias[i] = static_cast<const float*>(bd) + (size_t)i * c; }
    if (e == hipSuccess) e = launch_conv_bf16_chain(ca, c, wid, s);
    if (e == hipSuccess && reps > 0 && us_out)
        *us_out = timed_launches(s, reps, [&] { return launch_conv_bf16_chain(ca, c, wid, s); }, &e) * 1e3f / reps;
    if (e == hipSuccess) e = launch_nhwc_bf16_to_nchw_f32(xout, out_dev, n, c, wid, wid, c, 0, s);
    hipError_t e2 = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(GRNET_EHIP, std::string("bf16 chain: ") + hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(GRNET_EHIP, std::string("bf16 chain kernel: ") + hipGetErrorString(e2));
    return 0;
}

extern "C" {

int grnet_time_conv(grnet_t* h, int pos, int n_frames, int reps, void* stream, float* us_out) {
    if (!h || !us_out || !h->finalized || pos < 0 || reps < 1 || n_frames < 1 || n_frames > h->max_frames) return GRNET_EINVAL;
    DeviceGuard guard(h->device);
    const Op* op = h->nth_conv_op(pos);
    if (!op) return GRNET_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = 0, nl = 0;
    auto once = [&]() { return op->kind == Op::FUSEUP ? h->launch_fuse_up_op(h->fuse_ups[op->conv_idx], n_frames, s) : h->launch_conv_op(h->convs[op->conv_idx], h->base(h->v_cat), n_frames, s, &nl); };
    for (int r = 0; r < 2 && !rc; ++r) rc = once();              // warm: weights and inputs in the caches, as between two steps
    const float ms = timed_launches(s, reps, once, &rc);
    if (ms < 0) return GRNET_EHIP;
    *us_out = ms * 1e3f / reps;
    return rc;
}

int grnet_time_convs(grnet_t* h, int n_frames, void* stream, float* ms_out) {
    if (!h || !ms_out || !h->finalized) return GRNET_EINVAL;
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    grnet_outputs_t o{};
    int rc = 0;
    // the frames pointer of the first conv is only read; reuse the concat buffer as a stand-in input
    const float ms = timed_launches(s, 1, [&] { return h->enqueue(h->base(h->v_cat), n_frames, o, s, true); }, &rc);
    if (ms < 0) return GRNET_EHIP;
    *ms_out = ms;
    return rc;
}

int grnet_op_conv2d_adds(grnet_t* h, const float* in_dev, int n, int cin, int hgt, int wid, const float* w_host, const float* bias_host, int cout, int ks,
                         int stride, int relu, int n_add, const float* const* adds_dev, const int* add_ctot, const int* add_coff, const int* add_shift,
                         float* out_dev, int tile_hint, void* stream) {
    if (!h || !in_dev || !w_host || !out_dev || n < 1 || (n_add && (!adds_dev || !add_ctot || !add_coff || !add_shift))) return GRNET_EINVAL;
    if (h->dtype != 1) return h->fail(GRNET_ESTATE, "grnet_op_conv2d_adds needs a bf16 handle");
    DeviceGuard guard(h->device);
    return h->op_conv2d_bf16_adds(in_dev, n, cin, hgt, wid, w_host, bias_host, cout, ks, stride, relu, n_add, adds_dev, add_ctot, add_coff, add_shift, out_dev,
                                  tile_hint, static_cast<hipStream_t>(stream));
}

int grnet_op_conv2d(grnet_t* h, const float* in_dev, int n, int cin, int hgt, int wid, const float* w_host, const float* bias_host,
                    int cout, int ks, int stride, int relu, const float* add_dev, float* out_dev, int tile_hint, void* stream) {
    if (!h || !in_dev || !w_host || !out_dev) return GRNET_EINVAL;
    DeviceGuard guard(h->device);
    if (h->dtype == 1) return h->op_conv2d_bf16(in_dev, n, cin, hgt, wid, w_host, bias_host, cout, ks, stride, relu, add_dev, out_dev, tile_hint,
                                                static_cast<hipStream_t>(stream));
    const int taps = ks * ks, TC = conv_pick_tc(cout);
    const int cin_pad = (cin + kConvCK - 1) / kConvCK * kConvCK, cout_pad = (cout + TC - 1) / TC * TC;
    std::vector<float> wp((size_t)taps * cin_pad * cout_pad, 0.f), bp(cout_pad, 0.f);
    for (int co = 0; co < cout; ++co) {
        if (bias_host) bp[co] = bias_host[co];
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < taps; ++t) wp[((size_t)t * cin_pad + ci) * cout_pad + co] = w_host[((size_t)co * cin + ci) * taps + t];
    }
    HookBuffers mem;
    float *wd = mem.alloc<float>(wp.size() * 4), *bd = mem.alloc<float>(bp.size() * 4);
    if (!wd || !bd) return h->fail(GRNET_ENOMEM, "hipMalloc failed");
    if (hipMemcpy(wd, wp.data(), wp.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(bd, bp.data(), bp.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return h->fail(GRNET_EHIP, "hipMemcpy of the test weights failed");
    const int pad = ks / 2;
    ConvArgs a{};
    a.in = in_dev; a.in_ctot = cin; a.in_coff = 0; a.N = n; a.Cin = cin; a.H = hgt; a.W = wid;
    a.Cout = cout; a.Ho = (hgt + 2 * pad - ks) / stride + 1; a.Wo = (wid + 2 * pad - ks) / stride + 1;
    a.out = out_dev; a.out_ctot = cout; a.out_coff = 0;
    a.w = wd; a.bias = bd; a.CinPad = cin_pad; a.CoutPad = cout_pad; a.ks = ks; a.stride = stride; a.relu = relu;
    if (add_dev) { a.n_add = 1; a.add[0] = add_dev; a.add_ctot[0] = cout; a.add_coff[0] = 0; a.add_shift[0] = 0; }
    a.zeros = h->zeros;
    if (const char* d = GRNET_AB_STR(CONV_DBG)) a.dbg = atoi(d);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* ud = nullptr;
    if (tile_hint == 2003) { tile_hint = 2001; a.dbg |= 32; }   // 2003: the 4-wave F(4x4,3x3) kernel also where the 8-wave one would run
    if (tile_hint == 2001) {                                   // the F(4x4,3x3) kernel on this one convolution
        if (!conv_wino4_eligible(cin, cout, ks, stride, hgt, wid, add_dev ? 1 : 0) || cin_pad % 8 != 0 || cout_pad % (cout % 64 == 0 ? 64 : 32) != 0)
            return h->fail(GRNET_EINVAL, "shape not eligible for the F(4x4,3x3) kernel");
        std::vector<double> wf((size_t)cout * cin * 9);
        for (size_t i = 0; i < wf.size(); ++i) wf[i] = w_host[i];
        std::vector<float> uw((size_t)36 * cin_pad * cout_pad);
        pack_wino4_weights(wf.data(), cout, cin, cin_pad, cout_pad, uw.data(), wid);
        if (!(ud = mem.alloc<float>(uw.size() * 4)) || hipMemcpy(ud, uw.data(), uw.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
            return h->fail(GRNET_ENOMEM, "Winograd test weights");
        a.w = ud;
    }
    if (tile_hint == 3002 && !conv_pw_eligible(cin, cout, ks, stride, hgt, wid, add_dev ? 1 : 0))   // the register-resident 1x1 kernel on this one convolution
        return h->fail(GRNET_EINVAL, "shape not eligible for the 1x1 kernel");
    if (tile_hint == 3001) {                                   // the flattened-K stem kernel on this one convolution
        if (!conv_stem_eligible(cin, cout, ks, stride, hgt, wid, add_dev ? 1 : 0))
            return h->fail(GRNET_EINVAL, "shape not eligible for the stem kernel");
        std::vector<double> wf((size_t)cout * cin * 9);
        for (size_t i = 0; i < wf.size(); ++i) wf[i] = w_host[i];
        std::vector<float> sw(7 * 4 * 64);
        pack_stem_weights(wf.data(), sw.data());
        if (!(ud = mem.alloc<float>(sw.size() * 4)) || hipMemcpy(ud, sw.data(), sw.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
            return h->fail(GRNET_ENOMEM, "stem test weights");
        a.w = ud;
    }
    int w4s_on = 0, w4s_ks = 0;
    if (tile_hint >= 2020 && tile_hint <= 2024) {              // the small-map F(4x4,3x3) kernel, 202k: k waves split the input channels (0: default)
        w4s_on = 1; w4s_ks = tile_hint - 2020;
        if (!conv_wino4s_eligible(cin, cout, ks, stride, hgt, wid, add_dev ? 1 : 0))
            return h->fail(GRNET_EINVAL, "shape not eligible for the small-map F(4x4,3x3) kernel");
        std::vector<double> wf((size_t)cout * cin * 9);
        for (size_t i = 0; i < wf.size(); ++i) wf[i] = w_host[i];
        std::vector<float> uw((size_t)36 * cin * cout);
        pack_wino4r_weights(wf.data(), cout, cin, uw.data());
        if (!(ud = mem.alloc<float>(uw.size() * 4)) || hipMemcpy(ud, uw.data(), uw.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
            return h->fail(GRNET_ENOMEM, "Winograd test weights");
        a.w = ud;
    }
    auto launch_one = [&]() {
        return w4s_on ? launch_conv_wino4s(a, s, w4s_ks) : tile_hint == 2001 ? launch_conv_wino4(a, s) : tile_hint == 3001 ? launch_conv_stem(a, s) : tile_hint == 3002 ? launch_conv_pw(a, s) : launch_conv(a, s, tile_hint);
    };
    hipError_t e = launch_one();
    if (const char* r = GRNET_AB_STR(CONV_REPS)) {           // timing loop for tools/conv_micro.py
        const int reps = atoi(r);
        const float ms = timed_launches(s, reps, launch_one, &e);
        fprintf(stderr, "[conv_micro] cin %d cout %d k %d s %d hw %d n %d hint %d dbg %d: %.2f us/launch\n", cin, cout, ks, stride, hgt, n,
                tile_hint, a.dbg, ms * 1e3f / reps);
    }
    hipError_t e2 = hipStreamSynchronize(s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("launch_conv: ") + hipGetErrorString(e));
    if (e2 != hipSuccess) return h->fail(GRNET_EHIP, std::string("conv kernel: ") + hipGetErrorString(e2));
    return 0;
}

int grnet_op_conv_chain(grnet_t* h, const float* in_dev, int n, int c, int wid, int nconv, const float* w_host, const float* bias_host, float* out_dev,
                        int reps, float* us_out, void* stream) {
    if (!h || !in_dev || !w_host || !bias_host || !out_dev) return GRNET_EINVAL;
    DeviceGuard guard(h->device);
    return h->op_conv_chain_bf16(in_dev, n, c, wid, nconv, w_host, bias_host, out_dev, reps, us_out, static_cast<hipStream_t>(stream));
}

int grnet_op_bilinear2x(grnet_t* h, const float* in_dev, int n, int c, int hgt, int wid, float* out_dev, void* stream) {
    if (!h || !in_dev || !out_dev) return GRNET_EINVAL;
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (h->dtype == 1) {                                       // bf16 handle: the bf16 NHWC kernel of the bf16 path (fp32 NCHW -> bf16 NHWC -> x2 -> fp32 NCHW)
        if (n < 1 || c < 8 || c % 8 != 0 || hgt < 1 || wid < 1) return h->fail(GRNET_EINVAL, "bilinear2x (bf16): channels must be a multiple of 8");
        const size_t nin = (size_t)n * hgt * wid * c;
        void* tmp = nullptr;
        hipError_t eb = hipMallocAsync(&tmp, nin * 2 * 5, s);
        if (eb != hipSuccess) return h->fail(GRNET_EHIP, std::string("bilinear2x (bf16) scratch: ") + hipGetErrorString(eb));
        void* up = static_cast<unsigned short*>(tmp) + nin;
        eb = launch_nchw_f32_to_nhwc_bf16(in_dev, tmp, n, c, hgt, wid, c, s);
        if (eb == hipSuccess) eb = launch_bilinear2x_bf16(tmp, up, n, c, hgt, wid, s);
        if (eb == hipSuccess) eb = launch_nhwc_bf16_to_nchw_f32(up, out_dev, n, c, 2 * hgt, 2 * wid, c, 0, s);
        (void)hipFreeAsync(tmp, s);
        if (eb != hipSuccess) return h->fail(GRNET_EHIP, std::string("bilinear2x (bf16): ") + hipGetErrorString(eb));
        return 0;
    }
    hipError_t e = launch_bilinear2x(in_dev, out_dev, n, c, hgt, wid, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("bilinear2x: ") + hipGetErrorString(e));
    return 0;
}

int grnet_op_attention_pool(grnet_t* h, const float* heat_dev, const float* feat_a_dev, const float* feat_b_dev, int n, float* plf_out_dev, float* csf_out_dev,
                            void* stream) {
    if (!h || !heat_dev || !feat_a_dev || !feat_b_dev || !plf_out_dev || !csf_out_dev || n < 1) return GRNET_EINVAL;
    if (!h->finalized) return h->fail(GRNET_ESTATE, "grnet_op_attention_pool before grnet_finalize_weights");      // the tail behind the merge reads the regressor's weights
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    constexpr int P = 56 * 56;
    HookBuffers mem;
    // the pooling workspace and the tail's other outputs (rot6d 144 | shape 10 | cam 3 | rotmat 216 | theta 85 per frame): scratch of this call
    float *ws = mem.alloc<float>(softmax_pool_ws_floats(n) * 4), *tail = mem.alloc<float>((size_t)n * (144 + 10 + 3 + 216 + 85) * 4);
    if (!ws || !tail) return h->fail(GRNET_ENOMEM, "hipMalloc failed");
    hipError_t e;
    if (h->dtype == 1) {                                       // bf16 handle: the maps as the plan keeps them (NHWC bf16, the 25 heat channels in 32), then the bf16 path's kernel
        const int hc = h->v_heat.ctot, cta = h->v_smpl_feats.ctot, ctb = h->v_csmap.ctot;
        if (hc < 32 || cta < 128 || ctb < 64) return h->fail(GRNET_ESTATE, "grnet_op_attention_pool: the plan's channel strides do not hold the maps");
        void *xh = mem.alloc((size_t)n * P * hc * 2), *xa = mem.alloc((size_t)n * P * cta * 2), *xb = mem.alloc((size_t)n * P * ctb * 2);
        if (!xh || !xa || !xb) return h->fail(GRNET_ENOMEM, "hipMalloc failed");
        e = launch_nchw_f32_to_nhwc_bf16(heat_dev, xh, n, 25, 56, 56, hc, s);
        if (e == hipSuccess) e = launch_nchw_f32_to_nhwc_bf16(feat_a_dev, xa, n, 128, 56, 56, cta, s);
        if (e == hipSuccess) e = launch_nchw_f32_to_nhwc_bf16(feat_b_dev, xb, n, 64, 56, 56, ctb, s);
        if (e == hipSuccess) e = launch_softmax_pool_bf16(xh, hc, xa, 128, cta, xb, 64, ctb, ws, n, P, s);
    } else {
        e = launch_softmax_pool(heat_dev, 25, feat_a_dev, 128, feat_b_dev, 64, plf_out_dev, csf_out_dev, ws, n, P, s);
    }
    float* t = tail;
    if (e == hipSuccess)
        e = launch_head_tail(ws, true, plf_out_dev, csf_out_dev, h->tailw, t, t + (size_t)n * 144, t + (size_t)n * 154, t + (size_t)n * 157, t + (size_t)n * 373, n, s);
    hipError_t e2 = hipStreamSynchronize(s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("attention pool: ") + hipGetErrorString(e));
    if (e2 != hipSuccess) return h->fail(GRNET_EHIP, std::string("attention pool kernels: ") + hipGetErrorString(e2));
    return 0;
}

}  // extern "C"
