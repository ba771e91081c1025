// The C ABI of include/grnet_hip.h on one MI355X, except the entry points that live beside what they drive (weights: grnet_weights.cpp, the
// single-op hooks: grnet_hooks.cpp): create and destroy, the arena queries, options and tuning text, the describe / info calls, the forward,
// the temporal modules, SMPL, the crop, pose smoothing and the debug tensors -- and what a handle owns for them (its device memory, the scratch
// and the taps of the temporal calls).  The handle itself is `struct grnet` (grnet_impl.h); its plan is grnet_plan.cpp, its launch path grnet_run.cpp.
#include "grnet_impl.h"

// s into the caller's (buf, size) with its terminating zero; false: it does not fit, nothing was written
static bool copy_text(const std::string& s, char* buf, int size) {
    if ((int)s.size() + 1 > size) return false;
    memcpy(buf, s.c_str(), s.size() + 1);
    return true;
}

// releases everything the handle owns (also the clean-up of a failed grnet_create)
grnet::~grnet() {
    for (auto& g : graphs) (void)hipGraphExecDestroy(g.second.exec);
    if (capture_stream) (void)hipStreamDestroy(capture_stream);
    for (int l = 1; l < kLanes; ++l) {
        if (side[l]) (void)hipStreamDestroy(side[l]);
        if (ev_join[l]) (void)hipEventDestroy(ev_join[l]);
    }
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    for (hipEvent_t e : op_events_flat) if (e) (void)hipEventDestroy(e);
    for (void* p : dev_allocs) (void)hipFree(p);
    jreg_clear();
    faces_clear();
    if (raster_ws) (void)hipFree(raster_ws);
    if (seg_stage) (void)hipHostFree(seg_stage);
    for (hipEvent_t e : seg_stage_done)
        if (e) (void)hipEventDestroy(e);
    if (temporal_ws) (void)hipFree(temporal_ws);
    if (bbox_ws) (void)hipFree(bbox_ws);
    if (metric_ws) (void)hipFree(metric_ws);
    if (gru_fault) (void)hipHostFree(gru_fault);
    if (arena) (void)hipFree(arena);
}

int grnet::dev_alloc(float** p, size_t floats) {
    void* q = nullptr;
    if (hipMalloc(&q, floats * sizeof(float)) != hipSuccess) return fail(GRNET_ENOMEM, "hipMalloc failed");
    dev_allocs.push_back(q);
    *p = static_cast<float*>(q);
    return 0;
}

void grnet::jreg_clear() {
    if (jreg_pack || jreg_ws) (void)hipDeviceSynchronize();         // a call that reads them may still be running
    if (jreg_pack) (void)hipFree(jreg_pack);
    if (jreg_ws) (void)hipFree(jreg_ws);
    jreg_pack = jreg_ws = nullptr;
    jreg_rows = 0;
}

// Convolution / fuse launch number pos of the schedule (the positions of grnet_describe_conv and its kin); nullptr: past the end
const Op* grnet::nth_conv_op(int pos) const {
    int seen = 0;
    for (const Op& op : ops_flat) {
        if (op.kind != Op::CONV && op.kind != Op::FUSEUP) continue;
        if (seen++ == pos) return &op;
    }
    return nullptr;
}

// ------------------------------------------------------------------ the temporal modules
int grnet::gru_fault_check() {
    if (!gru_fault) {
        void* q = nullptr;
        if (hipHostMalloc(&q, 64, hipHostMallocMapped) != hipSuccess) return fail(GRNET_ENOMEM, "hipHostMalloc of the GRU fault word failed");
        gru_fault = static_cast<unsigned*>(q);
        *gru_fault = 0u;
        void* d = nullptr;
        if (hipHostGetDevicePointer(&d, q, 0) != hipSuccess) return fail(GRNET_EHIP, "hipHostGetDevicePointer failed");
        gru_fault_dev = static_cast<unsigned*>(d);
    }
    if (*reinterpret_cast<volatile unsigned*>(gru_fault)) {
        *gru_fault = 0u;
        const bool was_agent = (gru_mode & 16) != 0;
        gru_mode = was_agent ? 0 : (gru_mode | 16);
        return fail(GRNET_ESTATE, std::string("a hand-off poll of the split GRU recurrence timed out in an earlier call on this handle: the outputs of that call are NaN-poisoned. ") +
                    (was_agent ? "The handle now runs the unsplit recurrence (GRNET_OPT_GRU_MODE 0)." : "The handle now publishes with agent-scope stores (GRNET_OPT_GRU_MODE + 16).") + " Repeat the call.");
    }
    return 0;
}

int grnet::taps_begin(size_t need, const char* what) {
    taps_armed = false;
    if (tap_sink.floats < need)
        return fail(GRNET_EINVAL, "the tap buffer holds " + std::to_string(tap_sink.floats) + " floats, " + what + " of this size copies " + std::to_string(need) +
                                      " floats: nothing was enqueued");
    tap_sink.used = 0;
    tap_sink.layout.clear();
    return 0;
}

int grnet::temporal_scratch(size_t floats, float** out) {
    if (floats > temporal_ws_floats) {
        if (temporal_ws) { (void)hipDeviceSynchronize(); (void)hipFree(temporal_ws); temporal_ws = nullptr; temporal_ws_floats = 0; }
        const size_t want = floats + floats / 4;                 // head-room: clips of slightly different length reuse the buffer
        void* q = nullptr;
        if (hipMalloc(&q, want * sizeof(float)) != hipSuccess) return fail(GRNET_ENOMEM, "temporal workspace (" + std::to_string(want * 4 >> 20) + " MiB)");
        temporal_ws = static_cast<float*>(q);
        temporal_ws_floats = want;
    }
    *out = temporal_ws;
    return 0;
}

// Scratch of one GRU call over rows = b * T frames, and its parts: xin | xc | gi | l0 | l1 | hfin | xbuf.  *xc is the scratch copy of x + xc for a
// caller that does not keep one.
size_t grnet::gru_ws_floats(size_t rows, int b) {
    return rows * 3072 * 2 + 2 * rows * 900 + 2 * rows * 600 + (size_t)b * 1200 + (size_t)b * 2 * kGruXbufU64PerSeq + 1024;
}
GruWorkspace grnet::gru_carve(float* p, size_t rows, int b, float** xc) const {
    GruWorkspace w;
    w.xin = p;
    *xc = p + rows * 3072;
    w.gi = p + rows * 3072 * 2;
    w.l0 = w.gi + 2 * rows * 900;
    w.l1 = w.l0 + rows * 600;
    w.hfin = w.l1 + rows * 600;
    w.xbuf = reinterpret_cast<unsigned long long*>(w.hfin + (((size_t)b * 1200 + 63) & ~(size_t)63));
    w.mode = gru_mode; w.fault = gru_fault_dev;
    return w;
}

// The attention block's softmax row over a clip lives in LDS: 0, or the error of a clip of n frames that exceeds the limit of the current device
// (`tail`: what the entry point adds to the message)
int grnet::clip_limit(int n, const char* tail) {
    if (n <= tsattn_max_frames()) return 0;
    return fail(GRNET_EINVAL, "a clip of " + std::to_string(n) + " frames exceeds the attention block's limit of " + std::to_string(tsattn_max_frames()) + " frames per clip" + tail);
}

// ================================================================================ C ABI
extern "C" {

const char* grnet_version(void) { return "grnet_hip 0.1 (gfx950, fp32 MFMA)"; }

int grnet_create(grnet_t** out_handle, int device_id, int dtype, int max_frames) { return grnet_create_ex(out_handle, device_id, dtype, max_frames, 0u); }

int grnet_create_ex(grnet_t** out_handle, int device_id, int dtype, int max_frames, unsigned flags) {
    if (!out_handle || max_frames < 1 || max_frames > 2048 || (dtype != 0 && dtype != 1) || (flags & ~(unsigned)GRNET_CREATE_COMPACT_ARENA)) return GRNET_EINVAL;
    *out_handle = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return GRNET_EHIP;
    DeviceGuard guard(device_id);                          // the caller's current device is restored on return
    std::unique_ptr<grnet> h(new grnet());
    h->device = device_id;
    h->max_frames = max_frames;
    h->dtype = dtype;
    h->compact = (flags & GRNET_CREATE_COMPACT_ARENA) != 0;
    if (const char* ml = getenv("GRNET_MULTI_LANE")) h->multi_lane = atoi(ml) != 0;   // profiling: per-kernel times without overlap
    if (const char* wn = getenv("GRNET_WINO")) h->wino_mode = atoi(wn) != 0;
    h->build_plan();
    int rc = h->allocate();
    if (rc) { fprintf(stderr, "grnet_create: %s\n", h->err.c_str()); return rc; }
    if (conv_init() != hipSuccess || conv_bf16_init() != hipSuccess || conv_bf16_chain_init() != hipSuccess || conv_bf16_roll_init() != hipSuccess) { fprintf(stderr, "grnet_create: conv_init failed\n"); return GRNET_EHIP; }
    *out_handle = h.release();
    return 0;
}

// The plan of (precision, max_frames) and its arena, on the host alone: no device, no HIP call.
static int arena_plan_on_host(int precision, int max_frames, unsigned flags, std::unique_ptr<grnet>& g) {
    if (max_frames < 1 || max_frames > 2048 || (precision != 0 && precision != 1) || (flags & ~(unsigned)GRNET_CREATE_COMPACT_ARENA)) return GRNET_EINVAL;
    g.reset(new grnet());
    g->max_frames = max_frames;
    g->dtype = precision;
    g->compact = (flags & GRNET_CREATE_COMPACT_ARENA) != 0;
    g->build_plan();
    return g->plan_arena(g->compact, g->arena_plan);
}

int grnet_arena_query(int precision, int max_frames, unsigned flags, int64_t* info) {
    if (!info) return GRNET_EINVAL;
    std::unique_ptr<grnet> g;
    if (int rc = arena_plan_on_host(precision, max_frames, flags, g)) return rc;
    g->arena_info(g->arena_plan, info);
    return 0;
}

int grnet_arena_layout(int precision, int max_frames, unsigned flags, char* buf, int size) {
    std::unique_ptr<grnet> g;
    if (int rc = arena_plan_on_host(precision, max_frames, flags, g)) return rc;
    const std::string out = g->arena_text(g->arena_plan);
    if (!buf) return (int)out.size() + 1;
    if (!copy_text(out, buf, size)) return GRNET_EINVAL;
    return (int)out.size();
}

int grnet_arena_info(grnet_t* h, int64_t* info) {
    if (!h || !info) return GRNET_EINVAL;
    h->arena_info(h->arena_plan, info);
    return 0;
}

int grnet_arena_fill(grnet_t* h, uint32_t pattern, void* stream) {
    if (!h) return GRNET_EINVAL;
    DeviceGuard guard(h->device);
    const size_t head = (size_t)grnet::kArenaHead;
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->arena + head), (int)pattern, h->arena_floats - head, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("hipMemsetD32Async: ") + hipGetErrorString(e));
    return 0;
}

int grnet_arena_assign(int n, const int64_t* sizes, int n_pairs, const int32_t* conflict_pairs, int64_t* offsets, int64_t* total) {
    if (n < 0 || n_pairs < 0 || (n && (!sizes || !offsets)) || (n_pairs && !conflict_pairs) || !total) return GRNET_EINVAL;
    std::vector<int64_t> sz(n), off;
    std::vector<std::vector<int>> adj(n);
    for (int i = 0; i < n; ++i) {
        if (sizes[i] < 0) return GRNET_EINVAL;
        sz[i] = sizes[i];
    }
    for (int k = 0; k < n_pairs; ++k) {
        const int a = conflict_pairs[2 * k], b = conflict_pairs[2 * k + 1];
        if (a < 0 || a >= n || b < 0 || b >= n) return GRNET_EINVAL;
        if (a == b) continue;
        adj[a].push_back(b);
        adj[b].push_back(a);
    }
    int64_t tot = 0;
    arena_first_fit(sz, adj, 256, off, &tot);
    for (int i = 0; i < n; ++i) offsets[i] = off[i];
    *total = tot;
    return 0;
}

int grnet_forward(grnet_t* h, const float* frames_dev, int n_frames, const grnet_outputs_t* out, void* stream) {
    if (!h) return GRNET_EINVAL;
    DeviceGuard guard(h->device);
    return h->forward(frames_dev, n_frames, out, static_cast<hipStream_t>(stream));
}

int grnet_gru_forward(grnet_t* h, const float* x, const float* cp, int b, int T, float* y, float* phase, float* xc, void* stream) {
    if (!h || !x || !cp || !y || !phase || b < 1 || T < 1) return GRNET_EINVAL;
    if (!h->gru_ready) return h->fail(GRNET_ESTATE, "GRU weights were not loaded (keys gru.* or pfeat_corrector.featnet.*)");
    DeviceGuard guard(h->device);
    if (int rc = h->gru_fault_check()) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t rows = (size_t)b * T;
    const bool taps = h->taps_armed;
    if (taps) if (int rc = h->taps_begin(gru_tap_floats(b, T), "a GRU call")) return rc;
    TapLease tap_lease(taps ? &h->tap_sink : nullptr);
    float* ws = nullptr;                                   // handle-owned scratch: no allocation once a size has been seen
    const size_t need = grnet::gru_ws_floats(rows, b);
    if (int rc = h->temporal_scratch(kGemmWsFloats + need, &ws)) return rc;
    GemmWorkspaceLease lease(ws, kGemmWsFloats);
    ws += kGemmWsFloats;
    float* xc_buf = nullptr;
    const GruWorkspace w = h->gru_carve(ws, rows, b, &xc_buf);
    if (xc) xc_buf = xc;
    hipError_t e = launch_gru(x, cp, h->gruw, w, y, phase, xc_buf, b, T, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("launch_gru: ") + hipGetErrorString(e));
    return 0;
}

int grnet_tsattn_forward(grnet_t* h, const float* x, const float* xs, int b, int n, float* y, void* stream) {
    if (!h || !x || !xs || !y || b < 1 || n < 1) return GRNET_EINVAL;
    DeviceGuard guard(h->device);                          // the limit below is the handle's device's
    if (int rc = h->clip_limit(n, " (its softmax row over the clip lives in LDS): split the sequence into clips")) return rc;
    if (!h->tsattn_ready)
        return h->fail(GRNET_ESTATE, "attention-block weights were not loaded (keys tsattn.* or pfeat_corrector.featTencoder.0.*)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool taps = h->taps_armed;
    if (taps) {
        size_t need = 0;
        if (tsattn_tap_floats(b, n, &need) != hipSuccess) { h->taps_armed = false; return h->fail(GRNET_EHIP, "device query for the tap layout failed"); }
        if (int rc = h->taps_begin(need, "an attention-block call")) return rc;
    }
    TapLease tap_lease(taps ? &h->tap_sink : nullptr);
    float* ws = nullptr;                                   // handle-owned scratch, like the GRU's
    if (int rc = h->temporal_scratch(kGemmWsFloats + tsattn_ws_floats(b, n), &ws)) return rc;
    GemmWorkspaceLease lease(ws, kGemmWsFloats);
    hipError_t e = launch_tsattn(x, xs, h->tsw, ws + kGemmWsFloats, y, b, n, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("launch_tsattn: ") + hipGetErrorString(e));
    return 0;
}

int grnet_temporal_taps(grnet_t* h, float* buf_dev, size_t floats) {
    if (!h) return GRNET_EINVAL;
    if (!buf_dev || floats == 0) { h->taps_armed = false; return 0; }
    h->tap_sink.buf = buf_dev;
    h->tap_sink.floats = floats;
    h->taps_armed = true;
    return 0;
}

int grnet_temporal_tap_layout(grnet_t* h, char* buf, int buf_size) {
    if (!h) return GRNET_EINVAL;
    const std::string& out = h->tap_sink.layout;
    if (!buf) return (int)out.size() + 1;
    if (!copy_text(out, buf, buf_size)) return h->fail(GRNET_EINVAL, "buffer too small: the layout is " + std::to_string(out.size() + 1) + " bytes");
    return (int)out.size();
}

int grnet_tsattn_plan(grnet_t* h, int n, int32_t* plan) {
    if (!h || !plan || n < 1) return GRNET_EINVAL;
    DeviceGuard guard(h->device);                          // the CU count and the LDS limit are the handle's device's
    if (int rc = h->clip_limit(n, "")) return rc;
    int p[4];
    if (tsattn_plan(n, p) != hipSuccess) return h->fail(GRNET_EHIP, "device query failed");
    for (int i = 0; i < 4; ++i) plan[i] = p[i];
    return 0;
}

int grnet_set_option(grnet_t* h, int option, int value) {
    if (!h) return GRNET_EINVAL;
    if (option == GRNET_OPT_USE_GRAPH) { h->use_graph = value != 0; return 0; }
    if (option == GRNET_OPT_CONV_TILE) {
        if (value != 0 && value != 7 && value != 14 && value != 1071 && value != 1072 && value != 1041 && value != 1042 && value != 1171 && value != 1141)
            return h->fail(GRNET_EINVAL, "conv tile must be 0, 7, 14 or a split-K code 1071/1072/1041/1042/1171/1141");
        h->conv_tile_hint = value;
        h->drop_graphs();
        return 0;
    }
    if (option == GRNET_OPT_WINOGRAD) { h->wino_mode = value != 0; h->drop_graphs(); return 0; }
    if (option == GRNET_OPT_BF16_CHAIN) { h->chain_mode = value & grnet::kChainModeAll; h->drop_graphs(); return 0; }
    if (option == GRNET_OPT_GRU_MODE) {
        if (value < 0 || (value & 15) > 3 || (value & ~31)) return h->fail(GRNET_EINVAL, "GRU mode is 0 .. 3, + 16 for agent-scope stores");
        h->gru_mode = value;
        return 0;
    }
    if (option == GRNET_OPT_BF16_MIN_FRAMES) {
        if (value < 0) return h->fail(GRNET_EINVAL, "the smallest call of the bf16 kernel groups is >= 1 frame (0: each group's own default)");
        h->bf16_min_frames = value;
        h->drop_graphs();
        return 0;
    }
    if (option == GRNET_OPT_MULTI_LANE) {
        h->multi_lane = value != 0;
        h->drop_graphs();
        return 0;
    }
    return h->fail(GRNET_EINVAL, "unknown option");
}

int grnet_tune(grnet_t* h, int n_frames, void* stream, int level) {
    if (!h) return GRNET_EINVAL;
    DeviceGuard guard(h->device);
    return h->tune(n_frames, static_cast<hipStream_t>(stream), level);
}

// Tuned table <-> text ("mode" line + one line per convolution: index hint), so a table measured once on a GPU
// can be stored next to the model and re-applied without re-measuring.
int grnet_get_tuning(grnet_t* h, int n_frames, char* buf, int buf_size) {
    if (!h || !buf || buf_size < 16) return GRNET_EINVAL;
    auto m = h->tuned_mode.find(n_frames);
    if (m == h->tuned_mode.end()) return h->fail(GRNET_ESTATE, "no tuning for this n_frames");
    std::string out = "mode " + std::to_string(m->second) + "\n";
    for (size_t i = 0; i < h->convs.size(); ++i) {
        auto it = h->convs[i].tuned.find(n_frames);
        out += std::to_string(i) + " " + std::to_string(it == h->convs[i].tuned.end() ? 0 : it->second) + "\n";
    }
    if (!copy_text(out, buf, buf_size)) return h->fail(GRNET_EINVAL, "buffer too small");
    return (int)out.size();
}

int grnet_set_tuning(grnet_t* h, int n_frames, const char* text) {
    if (!h || !text) return GRNET_EINVAL;
    int mode = 0, consumed = 0;
    if (sscanf(text, "mode %d\n%n", &mode, &consumed) != 1) return h->fail(GRNET_EINVAL, "bad tuning text");
    const char* p = text + consumed;
    int idx, hint, used;
    while (sscanf(p, "%d %d\n%n", &idx, &hint, &used) == 2) {
        if (idx < 0 || idx >= (int)h->convs.size()) return h->fail(GRNET_EINVAL, "tuning text does not match this plan");
        h->convs[idx].tuned[n_frames] = hint;
        p += used;
    }
    h->tuned_mode[n_frames] = mode;
    h->drop_graphs();
    return 0;
}

int grnet_num_kernel_launches(grnet_t* h) { return h ? h->launches_last : GRNET_EINVAL; }

int grnet_plan_counts(grnet_t* h, int64_t* counts) {
    if (!h || !counts) return GRNET_EINVAL;
    std::copy(h->handoff_counts, h->handoff_counts + GRNET_PLAN_COUNTS, counts);
    return 0;
}

int grnet_num_conv_launches(grnet_t* h) { return h ? (int)(h->convs.size() + h->fuse_ups.size()) : GRNET_EINVAL; }

double grnet_conv_flops_per_frame(grnet_t* h) {
    if (!h) return 0;
    double m = 0;
    for (auto& L : h->convs) m += L.macs_per_frame;
    for (auto& fp : h->fuse_ups) m += fp.macs_per_frame;            // the 1x1 fuse terms computed by hr_fuse_up_f32
    return 2.0 * m;
}

double grnet_conv_executed_flops_per_frame_n(grnet_t* h, int n_frames) {
    if (!h) return 0;
    double m = 0;
    for (auto& L : h->convs) m += L.macs_per_frame * h->executed_ratio(L, n_frames);
    for (auto& fp : h->fuse_ups) m += fp.macs_per_frame;
    return 2.0 * m;
}

double grnet_conv_executed_flops_per_frame(grnet_t* h) { return h ? grnet_conv_executed_flops_per_frame_n(h, h->last_n) : 0; }

int grnet_describe_conv(grnet_t* h, int pos, int32_t* info, char* name, int name_size) {
    if (!h || !info || !h->finalized || pos < 0) return GRNET_EINVAL;
    const Op* found = h->nth_conv_op(pos);
    if (!found) return GRNET_EINVAL;
    const Op& op = *found;
    if (op.kind == Op::FUSEUP) {                       // the grouped 1x1 up terms of one HR module: Cin = 0 marks the entry
        const FuseUpPlan& fp = h->fuse_ups[op.conv_idx];
        int cout = 0;
        int64_t rd = 0;
        for (int i = 0; i < fp.nb - 1; ++i) cout += kBranchCh[i];
        for (int j = 0; j < fp.nb; ++j) rd += (int64_t)kBranchCh[j] * fp.xs[j].h * fp.xs[j].w;       // every branch output is read once
        const int32_t v[12] = {0, cout, 1, 1, fp.xs[0].h, fp.xs[0].w, fp.xs[0].h, fp.xs[0].w, fp.nb, 1, op.lane, (int32_t)rd};
        memcpy(info, v, sizeof(v));
        if (name && name_size > 0) snprintf(name, name_size, "%sfuse_layers(up)", fp.prefix.c_str());
        return 0;
    }
    const ConvLayer& L = h->convs[op.conv_idx];
    int64_t add_elems = 0;
    for (const AddRef& r : L.adds) add_elems += (int64_t)L.cout * (L.out.h >> r.shift) * (L.out.w >> r.shift);
    const int32_t v[12] = {L.in.c + L.in2.c, L.cout, L.ks, L.stride, L.in.h, L.in.w, L.out.h, L.out.w, (int32_t)L.adds.size(), L.relu,
                           op.lane, (int32_t)add_elems};
    memcpy(info, v, sizeof(v));
    if (name && name_size > 0) snprintf(name, name_size, "%s", L.segs.empty() ? "" : L.segs[0].wkey.c_str());
    return 0;
}

double grnet_describe_conv_macs(grnet_t* h, int pos) {
    if (!h || pos < 0) return -1.0;
    const Op* op = h->nth_conv_op(pos);
    if (!op) return -1.0;
    return op->kind == Op::FUSEUP ? h->fuse_ups[op->conv_idx].macs_per_frame : h->convs[op->conv_idx].macs_per_frame;
}

int grnet_conv_kernel_info(grnet_t* h, int pos, int n_frames, char* name, int name_size, double* executed_macs_per_frame) {
    if (!h || !h->finalized || pos < 0 || n_frames < 1) return GRNET_EINVAL;
    const Op* op = h->nth_conv_op(pos);
    if (!op) return GRNET_EINVAL;
    if (op->kind == Op::FUSEUP) {
        if (name && name_size > 0) snprintf(name, name_size, h->dtype == 1 ? "hr_fuse_up_bf16<%d>" : "hr_fuse_up_f32<%d>", h->fuse_ups[op->conv_idx].nb);
        if (executed_macs_per_frame) *executed_macs_per_frame = h->fuse_ups[op->conv_idx].macs_per_frame;
        return 0;
    }
    const ConvLayer& L = h->convs[op->conv_idx];
    if (name && name_size > 0) snprintf(name, name_size, "%s", h->kernel_name(L, n_frames).c_str());
    if (executed_macs_per_frame) *executed_macs_per_frame = L.macs_per_frame * h->executed_ratio(L, n_frames);
    return 0;
}

int grnet_conv_launch_form(grnet_t* h, int pos, int n_frames, char* buf, int size, int* tuning_index) {
    if (!h || !h->finalized || pos < 0 || n_frames < 1 || !buf || size < 1) return GRNET_EINVAL;
    if (h->dtype != 0) return h->fail(GRNET_ESTATE, "grnet_conv_launch_form reports the launches of fp32 handles");
    const Op* op = h->nth_conv_op(pos);
    if (!op) return GRNET_EINVAL;
    DeviceGuard guard(h->device);                          // conv_wino4_form reads the CU count of the current device
    std::string text;
    if (op->kind == Op::FUSEUP) {
        text = "fuse_up";
        if (tuning_index) *tuning_index = -1;
    } else {
        if (int rc = h->launch_form(h->convs[op->conv_idx], n_frames, &text)) return rc;
        if (tuning_index) *tuning_index = op->conv_idx;
    }
    if (!copy_text(text, buf, size)) return h->fail(GRNET_EINVAL, "grnet_conv_launch_form: buffer too small");
    return 0;
}

int grnet_op_timeline(grnet_t* h, const float* frames_dev, int n_frames, void* stream, char* buf, int buf_size) {
    if (!h || !buf || buf_size < 1) return GRNET_EINVAL;
    DeviceGuard guard(h->device);
    std::string text;
    if (int rc = h->op_timeline(frames_dev, n_frames, static_cast<hipStream_t>(stream), text)) return rc;
    if (!copy_text(text, buf, buf_size)) return h->fail(GRNET_EINVAL, "grnet_op_timeline: buffer too small (" + std::to_string(text.size() + 1) + " bytes needed)");
    return (int)text.size();
}

int grnet_debug_tensor(grnet_t* h, const char* name, int n_frames, float* out_dev, int64_t* shape_out, void* stream) {
    if (!h || !name) return GRNET_EINVAL;
    if (n_frames < 1 || n_frames > h->last_n || n_frames > h->max_frames)         // the buffers hold last_n frames (the last buffer ends at the arena's end): never read past them
        return h->fail(GRNET_EINVAL, "debug tensor " + std::string(name) + ": n_frames " + std::to_string(n_frames) + " outside [1, frames of the last forward = " +
                                         std::to_string(h->last_n) + "]");
    DeviceGuard guard(h->device);
    for (auto& nv : h->named) {
        if (nv.first != name) continue;
        const View& v = nv.second;
        if (h->compact && (v.slot < 0 || !h->arena_plan.final_tenant[v.slot]))
            return h->fail(GRNET_ESTATE, "debug tensor " + std::string(name) + " cannot be read back from a compact arena: a later tensor of the forward is placed over it. "
                                             "Create the handle without GRNET_CREATE_COMPACT_ARENA to read every intermediate");
        if (!h->tap_written(v))
            return h->fail(GRNET_ESTATE, "debug tensor " + std::string(name) + " was not written by the last forward (" + std::to_string(h->last_n) +
                                             " frames): its producer ran inside a fused launch that keeps it on chip");
        if (shape_out) { shape_out[0] = v.c; shape_out[1] = v.h; shape_out[2] = v.w; }
        if (!out_dev) return 0;
        const size_t plane = (size_t)v.h * v.w;
        if (h->dtype == 1) {
            hipError_t eb = launch_nhwc_bf16_to_nchw_f32(h->base(v), out_dev, n_frames, v.c, v.h, v.w, v.ctot, v.coff, static_cast<hipStream_t>(stream));
            if (eb != hipSuccess) return h->fail(GRNET_EHIP, std::string("debug convert: ") + hipGetErrorString(eb));
            return 0;
        }
        hipError_t e = hipMemcpy2DAsync(out_dev, (size_t)v.c * plane * 4, h->base(v) + (size_t)v.coff * plane, (size_t)v.ctot * plane * 4,
                                        (size_t)v.c * plane * 4, n_frames, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream));
        if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("debug copy: ") + hipGetErrorString(e));
        return 0;
    }
    return h->fail(GRNET_EINVAL, std::string("unknown debug tensor ") + name);
}

int grnet_smpl_forward(grnet_t* h, const float* betas_dev, const float* rotmat_dev, const float* cam_dev, int n, float* verts_dev,
                       float* kp3d_dev, float* kp2d_dev, void* stream) {
    if (!h || !betas_dev || !rotmat_dev || !verts_dev || !kp3d_dev || n < 1) return GRNET_EINVAL;
    if (!h->smpl_loaded) return h->fail(GRNET_ESTATE, "SMPL tables were not loaded");
    if (n > h->max_frames) return h->fail(GRNET_EINVAL, "n exceeds max_frames (the skinning-matrix workspace is sized for it)");
    DeviceGuard guard(h->device);
    hipError_t e = launch_smpl(betas_dev, rotmat_dev, cam_dev, h->smpl, h->d_A, verts_dev, kp3d_dev, kp2d_dev, n,
                               static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("smpl: ") + hipGetErrorString(e));
    return 0;
}

int grnet_joint_regressor_rows(grnet_t* h) { return h ? h->jreg_rows : GRNET_EINVAL; }

int grnet_regress_joints(grnet_t* h, const float* verts_dev, int n, float* joints_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    if (!h->jreg_rows) return h->fail(GRNET_ESTATE, "grnet_regress_joints without a table (grnet_set_joint_regressor)");
    if (!verts_dev || !joints_dev) return h->fail(GRNET_EINVAL, "grnet_regress_joints: null pointer");
    if (reinterpret_cast<uintptr_t>(verts_dev) & 7) return h->fail(GRNET_EINVAL, "grnet_regress_joints: verts_dev must be 8-byte aligned");
    if (n < 1 || n > h->max_frames)
        return h->fail(GRNET_EINVAL, "grnet_regress_joints: n " + std::to_string(n) + " outside [1, max_frames=" + std::to_string(h->max_frames) + "]");
    DeviceGuard guard(h->device);
    hipError_t e = launch_joint_regress(verts_dev, h->jreg_pack, h->jreg_rows, h->jreg_ws, joints_dev, n, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("joint_regress: ") + hipGetErrorString(e));
    return 0;
}

int grnet_crop_normalise(grnet_t* h, const unsigned char* images_dev, int n, int height, int width, int one_image_for_all,
                         const float* bboxes_dev, float scale, int bgr, float* out_dev, void* stream) {
    if (!h || !images_dev || !bboxes_dev || !out_dev || n < 1 || height < 1 || width < 1 || !(scale > 0.f)) return GRNET_EINVAL;
    DeviceGuard guard(h->device);
    hipError_t e = launch_crop_normalise(images_dev, height, width, one_image_for_all ? 0 : 1, bboxes_dev, scale, bgr, out_dev, n,
                                         static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("crop_normalise: ") + hipGetErrorString(e));
    return 0;
}

int grnet_crop_normalise_cv(grnet_t* h, const unsigned char* images_dev, int n, int height, int width, int one_image_for_all,
                            const double* inv_affine_dev, int bgr, float* out_dev, void* stream) {
    if (!h || !images_dev || !inv_affine_dev || !out_dev || n < 1 || height < 1 || width < 1) return GRNET_EINVAL;
    DeviceGuard guard(h->device);
    hipError_t e = launch_crop_normalise_cv(images_dev, height, width, one_image_for_all ? 0 : 1, inv_affine_dev, 6, bgr, out_dev, n,
                                            static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("crop_normalise_cv: ") + hipGetErrorString(e));
    return 0;
}

int grnet_crop_normalise_cv_maps(grnet_t* h, const unsigned char* images_dev, int n, int height, int width, int one_image_for_all,
                                 const double* maps_dev, int bgr, float* out_dev, void* stream) {
    if (!h || !images_dev || !maps_dev || !out_dev || n < 1 || height < 1 || width < 1) return GRNET_EINVAL;
    DeviceGuard guard(h->device);
    hipError_t e = launch_crop_normalise_cv(images_dev, height, width, one_image_for_all ? 0 : 1, maps_dev, 10, bgr, out_dev, n,
                                            static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("crop_normalise_cv_maps: ") + hipGetErrorString(e));
    return 0;
}

const char* grnet_last_error(grnet_t* h) { return h ? h->err.c_str() : "null handle"; }

void grnet_destroy(grnet_t* h) {
    if (!h) return;
    DeviceGuard guard(h->device);
    delete h;                                              // ~grnet releases graphs, streams, events and device memory
}

// PareHead.forward + VPRegressor.forward from given pooled features -- lib/models/pare.py:271-303,52-91: the second head pass of the
// use_gait_feat branch (grnet.py:165,171) and the single-op parity hook of the tail.
int grnet_head_forward(grnet_t* h, const float* plf_dev, const float* csf_dev, int n, const grnet_outputs_t* out, void* stream) {
    if (!h || !plf_dev || !csf_dev || !out || n < 1) return GRNET_EINVAL;
    if (!h->finalized) return h->fail(GRNET_ESTATE, "grnet_head_forward before grnet_finalize_weights");
    if (n > h->max_frames) return h->fail(GRNET_EINVAL, "n exceeds max_frames");
    DeviceGuard guard(h->device);
    return h->head_from_feats(plf_dev, csf_dev, n, *out, static_cast<hipStream_t>(stream));
}

int grnet_gait_correct(grnet_t* h, const float* plf_dev, const float* csf_dev, const float* cam_dev, int cam_ld, const float* bbox_dev,
                       const float* cimg_dev, int b, int T, const grnet_outputs_t* out, const grnet_gait_outputs_t* gait, void* stream) {
    if (!h || !plf_dev || !csf_dev || !cam_dev || !bbox_dev || !cimg_dev || !out || b < 1 || T < 1 || cam_ld < 3) return GRNET_EINVAL;
    if (!h->finalized) return h->fail(GRNET_ESTATE, "grnet_gait_correct before grnet_finalize_weights");
    if (!h->gru_ready || !h->tsattn_ready || !h->featcorr_ready)
        return h->fail(GRNET_ESTATE, "pose-feature corrector weights were not loaded (keys pfeat_corrector.*)");
    if ((long)b * T > 65536) return h->fail(GRNET_EINVAL, "b*T exceeds 65536 frames");
    DeviceGuard guard(h->device);                          // the limit below is the handle's device's
    if (int rc = h->clip_limit(T, ": split the sequence into clips (b, T)")) return rc;
    grnet_gait_outputs_t g{};
    if (gait) g = *gait;
    return h->gait_correct(plf_dev, csf_dev, cam_dev, cam_ld, bbox_dev, cimg_dev, b, T, *out, g, static_cast<hipStream_t>(stream));
}

int grnet_op_rot6d_to_rotmat(grnet_t* h, const float* rot6d_dev, int m, float* rotmat_dev, void* stream) {
    if (!h || !rot6d_dev || !rotmat_dev || m < 1) return GRNET_EINVAL;
    DeviceGuard guard(h->device);
    hipError_t e = launch_rot6d_to_rotmat(rot6d_dev, rotmat_dev, m, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("rot6d_to_rotmat: ") + hipGetErrorString(e));
    return 0;
}

// The constants of the One-Euro recurrence as the reference's float32 numpy forms them (one_euro_filter.py:5-7,32 with t_e = 1): 2 pi, min_cutoff
// and beta rounded to float32 once, a_d = r_d / (r_d + 1) with r_d = f32(2 pi d_cutoff), and 1 - a_d.
static OneEuroCoef one_euro_coef(float min_cutoff, float beta, float d_cutoff) {
    const double two_pi = 6.283185307179586476925286766559;
    OneEuroCoef c;
    const volatile float r_d = (float)(two_pi * (double)d_cutoff);      // volatile: each step is rounded to float32 whatever the host's evaluation mode
    const volatile float r_d1 = r_d + 1.f;
    const volatile float a_d = r_d / r_d1;
    c.a_d = a_d;
    c.one_minus_a_d = 1.f - a_d;
    c.two_pi = (float)two_pi;
    c.min_cutoff = min_cutoff;
    c.beta = beta;
    return c;
}

int grnet_op_one_euro(grnet_t* h, const float* x_dev, int ld, int T, float min_cutoff, float beta, float d_cutoff, float* xhat_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    if (!x_dev || !xhat_dev) return h->fail(GRNET_EINVAL, "grnet_op_one_euro: null pointer");
    if (T < 1) return h->fail(GRNET_EINVAL, "grnet_op_one_euro: T " + std::to_string(T) + " < 1");
    if (ld < 72) return h->fail(GRNET_EINVAL, "grnet_op_one_euro: row stride " + std::to_string(ld) + " < 72");
    if (!std::isfinite(min_cutoff) || !std::isfinite(beta) || !std::isfinite(d_cutoff))
        return h->fail(GRNET_EINVAL, "grnet_op_one_euro: min_cutoff, beta and d_cutoff must be finite");
    DeviceGuard guard(h->device);
    hipError_t e = launch_one_euro(x_dev, ld, T, one_euro_coef(min_cutoff, beta, d_cutoff), xhat_dev, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("one_euro: ") + hipGetErrorString(e));
    return 0;
}

int grnet_op_aa_to_rotmat(grnet_t* h, const float* aa_dev, int m, float* rotmat_dev, void* stream) {
    if (!h || !aa_dev || !rotmat_dev || m < 1) return GRNET_EINVAL;
    DeviceGuard guard(h->device);
    hipError_t e = launch_aa_to_rotmat(aa_dev, rotmat_dev, m, nullptr, nullptr, 0, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("aa_to_rotmat: ") + hipGetErrorString(e));
    return 0;
}

// lib/utils/smooth_pose.py:28-116 for axis-angle poses: the filter over all T frames in one launch, then SMPL on the filtered pose with the
// betas of frame 0 (:97) in chunks of max_frames, each chunk's joints written in the caller's skeleton.
int grnet_smooth_pose(grnet_t* h, const float* pose_dev, int pose_ld, const float* betas_dev, int T, float min_cutoff, float beta, int joints_kind,
                      float* pose_hat_dev, float* verts_dev, float* joints_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    if (!pose_dev || !betas_dev || !pose_hat_dev || !joints_dev) return h->fail(GRNET_EINVAL, "grnet_smooth_pose: null pointer (only verts_dev may be NULL)");
    if (T < 1) return h->fail(GRNET_EINVAL, "grnet_smooth_pose: T " + std::to_string(T) + " < 1");
    if (pose_ld < 72) return h->fail(GRNET_EINVAL, "grnet_smooth_pose: pose row stride " + std::to_string(pose_ld) + " < 72");
    const int nj = smooth_joint_count(joints_kind);
    if (!nj) return h->fail(GRNET_EINVAL, "grnet_smooth_pose: unknown joints_kind " + std::to_string(joints_kind) + " (GRNET_JOINTS_SPIN49 / _SPIN2 / _KINECTV2)");
    if (!std::isfinite(min_cutoff) || !std::isfinite(beta)) return h->fail(GRNET_EINVAL, "grnet_smooth_pose: min_cutoff and beta must be finite");
    if (!h->smpl_loaded) return h->fail(GRNET_ESTATE, "grnet_smooth_pose: SMPL tables were not loaded");
    if (!h->d_A) return h->fail(GRNET_ESTATE, "grnet_smooth_pose before grnet_finalize_weights (the SMPL workspace is allocated there)");
    DeviceGuard guard(h->device);
    const size_t mf = (size_t)h->max_frames;
    if (!h->smooth_ws) {
        if (int rc = h->dev_alloc(&h->smooth_ws, mf * (216 + 10 + 87))) return rc;
    }
    float *rot = h->smooth_ws, *betas = rot + mf * 216, *kp = betas + mf * 10;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = launch_one_euro(pose_dev, pose_ld, T, one_euro_coef(min_cutoff, beta, 1.f), pose_hat_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("smooth_pose (filter): ") + hipGetErrorString(e));
    for (int f0 = 0; f0 < T; f0 += h->max_frames) {
        const int n = std::min(h->max_frames, T - f0);
        float* verts = verts_dev ? verts_dev + (size_t)f0 * 6890 * 3 : h->d_verts;
        e = launch_aa_to_rotmat(pose_hat_dev + (size_t)f0 * 72, rot, n * 24, betas_dev, betas, n, s);
        if (e == hipSuccess) e = launch_smpl(betas, rot, nullptr, h->smpl, h->d_A, verts, kp, nullptr, n, s);
        if (e == hipSuccess) e = launch_smpl_joints54(kp, verts, h->smpl, joints_kind, joints_dev + (size_t)f0 * nj * 3, n, s);
        if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("smooth_pose (SMPL): ") + hipGetErrorString(e));
    }
    return 0;
}

int grnet_op_rotmat_to_aa(grnet_t* h, const float* rotmat_dev, int m, float* aa_dev, void* stream) {
    if (!h || !rotmat_dev || !aa_dev || m < 1) return GRNET_EINVAL;
    DeviceGuard guard(h->device);
    hipError_t e = launch_rotmat_to_aa(rotmat_dev, aa_dev, m, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("rotmat_to_aa: ") + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
