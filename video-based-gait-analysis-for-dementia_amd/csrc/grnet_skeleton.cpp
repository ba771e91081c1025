// The 3D skeleton view of demo.py --skeleton_view behind the C ABI (demo.py:303-361, lib/utils/vis.py:571-587; kernels: skeleton_kernels.hip,
// rules: DESIGN 4.6): grnet_render_segments, the hooks that run its two stages alone, and grnet_spin_joints, which forms the 49 SPIN joints the
// view is defined on from what a forward leaves on the device.
#include "grnet_impl.h"

namespace {

// The record area of the render workspace as the skeleton view uses it: [xy | depth of the points | segment table | boxes]
constexpr size_t kSegXyBytes = (size_t)kSegGroupPoints * 2 * sizeof(int), kSegZBytes = (size_t)kSegGroupPoints * sizeof(float);
constexpr size_t kSegTableBytes = (size_t)kSegMaxSegments * sizeof(SegSegment);
constexpr size_t kSegRecordBytes = kSegXyBytes + kSegZBytes + kSegTableBytes + (size_t)kRasterSlots * 4 * sizeof(int);

struct SegCarve { RasterWork work; SegSegment* seg; };

SegCarve seg_carve(void* base, size_t depth_words) {
    SegCarve c{};
    c.work.depth = static_cast<unsigned long long*>(base);
    char* p = reinterpret_cast<char*>(c.work.depth + depth_words);
    c.work.xy = reinterpret_cast<int*>(p), p += kSegXyBytes;
    c.work.z = reinterpret_cast<float*>(p), p += kSegZBytes;
    c.seg = reinterpret_cast<SegSegment*>(p), p += kSegTableBytes;
    c.work.bbox = reinterpret_cast<int*>(p);
    return c;
}

bool all_finite(const double* v, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// "" or what is wrong with the view: R 9 floats or NULL, proj 16 and window 4 doubles
std::string view_error(const float* R, const double* proj, const double* window) {
    if (R)
        for (int i = 0; i < 9; ++i)
            if (!std::isfinite(R[i])) return "R has a non-finite entry";
    if (!all_finite(proj, 16)) return "proj has a non-finite entry";
    if (!all_finite(window, 4)) return "window has a non-finite entry";
    if (!(window[1] > window[0]) || !(window[3] > window[2])) return "the window (x0, x1, y0, y1) is empty";
    return "";
}

// The projection and the window mapping folded into three rows, in double (the rules: DESIGN 4.6, "Panel")
SegView seg_view(const float* R, const double* proj, const double* window, int H, int W) {
    SegView v{{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {}, {}, {}, 0.f, 0.f, H, W};
    if (R) memcpy(v.R, R, sizeof(v.R));
    const double S = std::min(H, W), sx = S / (window[1] - window[0]), sy = S / (window[3] - window[2]);
    for (int c = 0; c < 4; ++c) {
        v.X[c] = (float)(sx * proj[c]);
        v.Y[c] = (float)(sy * proj[4 + c]);
        v.Wh[c] = (float)proj[12 + c];
    }
    v.cx = (float)((W - S) / 2 - sx * window[0]);
    v.cy = (float)((H - S) / 2 - sy * window[2]);
    return v;
}

// "" or what is wrong with the segment table; out: the device's records, colours (S,3) uint8 in memory order or NULL (the hook: no colours)
std::string pack_segments(const int32_t* segments, const unsigned char* colours, const int32_t* widths, int S, int P, std::vector<SegSegment>& out, int* wmax) {
    out.resize(S);
    *wmax = 1;
    for (int s = 0; s < S; ++s) {
        const int a = segments[2 * s], b = segments[2 * s + 1], w = widths[s];
        if (a < 0 || a >= P || b < 0 || b >= P)
            return "segment " + std::to_string(s) + " names point " + std::to_string(a < 0 || a >= P ? a : b) + ", outside [0, " + std::to_string(P) + ")";
        if (w < 1 || w > kSegMaxWidth) return "widths[" + std::to_string(s) + "] = " + std::to_string(w) + " outside [1, " + std::to_string(kSegMaxWidth) + "]";
        const int c = colours ? colours[3 * s] | colours[3 * s + 1] << 8 | colours[3 * s + 2] << 16 : 0;
        out[s] = SegSegment{a, b, w, c};
        *wmax = std::max(*wmax, w);
    }
    return "";
}

std::string sizes_error(int P, int S, int H, int W) {
    if (P < 1 || P > kSegMaxPoints) return "P " + std::to_string(P) + " outside [1, " + std::to_string(kSegMaxPoints) + "]";
    if (S < 0 || S > kSegMaxSegments) return "S " + std::to_string(S) + " outside [0, " + std::to_string(kSegMaxSegments) + "]";
    if (!raster_dims_ok(H, W)) return "image " + std::to_string(H) + " x " + std::to_string(W) + " outside [1, " + std::to_string(kRasterMaxDim) + "]";
    return "";
}

const RasterView kIdentityView{{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, 0, 0};

RasterView raster_view(int H, int W) {
    RasterView v = kIdentityView;
    v.H = H, v.W = W;
    return v;
}

}  // namespace

// The next table of the pinned ring.  It waits only if the copy that read this slot kSegStageSlots calls ago has not finished yet.
int grnet::seg_stage_slot(void** slot, hipEvent_t* done) {
    if (!seg_stage) {
        void* p = nullptr;
        if (hipHostMalloc(&p, kSegStageSlots * kSegTableBytes, hipHostMallocDefault) != hipSuccess) return fail(GRNET_ENOMEM, "grnet_render_segments: hipHostMalloc of the table ring failed");
        for (hipEvent_t& e : seg_stage_done)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
                (void)hipHostFree(p);
                return fail(GRNET_EHIP, "grnet_render_segments: hipEventCreate failed");
            }
        seg_stage = p;
    }
    const unsigned k = seg_stage_next++ % kSegStageSlots;
    if (hipEventSynchronize(seg_stage_done[k]) != hipSuccess) return fail(GRNET_EHIP, "grnet_render_segments: hipEventSynchronize failed");   // at once for an event never recorded
    *slot = static_cast<char*>(seg_stage) + (size_t)k * kSegTableBytes;
    *done = seg_stage_done[k];
    return 0;
}

extern "C" {

int grnet_spin_joints(grnet_t* h, const float* kp29_dev, const float* verts_dev, int n, int joints_kind, float* joints_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    if (n < 0) return h->fail(GRNET_EINVAL, "grnet_spin_joints: n " + std::to_string(n) + " < 0");
    const int nj = smooth_joint_count(joints_kind);
    if (!nj) return h->fail(GRNET_EINVAL, "grnet_spin_joints: unknown joints_kind " + std::to_string(joints_kind) + " (GRNET_JOINTS_SPIN49 / _SPIN2 / _KINECTV2)");
    if (!h->smpl_loaded) return h->fail(GRNET_ESTATE, "grnet_spin_joints: SMPL tables were not loaded");
    if (n == 0) return 0;
    if (!kp29_dev || !verts_dev || !joints_dev) return h->fail(GRNET_EINVAL, "grnet_spin_joints: null pointer");
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int f0 = 0; f0 < n; f0 += h->max_frames) {
        const int m = std::min(h->max_frames, n - f0);
        const hipError_t e = launch_smpl_joints54(kp29_dev + (size_t)f0 * 87, verts_dev + (size_t)f0 * kSmplVerts * 3, h->smpl, joints_kind,
                                                  joints_dev + (size_t)f0 * nj * 3, m, s);
        if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("spin_joints: ") + hipGetErrorString(e));
    }
    return 0;
}

int grnet_render_segments(grnet_t* h, const float* points_dev, int n, int P, const int32_t* segments_host, int S, const unsigned char* colours_host,
                          const int32_t* widths_host, const int32_t* image_index_host, const float* R_host, const double* proj_host,
                          const double* window_host, unsigned char* images_dev, int F, int H, int W, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_render_segments: ";
    if (n < 0) return h->fail(GRNET_EINVAL, name + "n " + std::to_string(n) + " < 0");
    std::string why = sizes_error(P, S, H, W);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    if (F < 1) return h->fail(GRNET_EINVAL, name + "F " + std::to_string(F) + " < 1");
    if (n == 0) return 0;
    if (!points_dev || !segments_host || !colours_host || !widths_host || !image_index_host || !proj_host || !window_host || !images_dev)
        return h->fail(GRNET_EINVAL, name + "null pointer (only R_host may be NULL)");
    why = view_error(R_host, proj_host, window_host);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    std::vector<SegSegment> segs;
    int wmax = 1;
    why = pack_segments(segments_host, colours_host, widths_host, S, P, segs, &wmax);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    // the images in the order in which the call first names them; a skeleton's rank among those aimed at its image, in call order
    std::unordered_map<int, int> pos;
    std::vector<int> order, count, rank(n), where(n);
    for (int i = 0; i < n; ++i) {
        const int f = image_index_host[i];
        if (f < 0 || f >= F) return h->fail(GRNET_EINVAL, name + "image_index[" + std::to_string(i) + "] = " + std::to_string(f) + " outside [0, " + std::to_string(F) + ")");
        auto it = pos.find(f);
        if (it == pos.end()) {
            it = pos.emplace(f, (int)order.size()).first;
            order.push_back(f);
            count.push_back(0);
        }
        where[i] = it->second;
        rank[i] = count[it->second]++;
    }
    const long long most = *std::max_element(count.begin(), count.end());
    if (most * std::max(S, 1) > (1ll << 31))
        return h->fail(GRNET_EINVAL, name + std::to_string(most) + " skeletons aimed at one image: rank * S + segment no longer fits 31 bits");
    if (S == 0) return 0;
    DeviceGuard guard(h->device);
    if (int rc = h->raster_workspace("grnet_render_segments")) return rc;
    static_assert(kSegRecordBytes <= (size_t)kRasterSlots * ((size_t)kSmplVerts * 9 * 4 + 16), "the skeleton view's records fit the meshes' record area");
    const SegCarve ws = seg_carve(h->raster_ws, kRasterDepthWords);
    const SegView view = seg_view(R_host, proj_host, window_host, H, W);
    const RasterView rv = raster_view(H, W);
    const SegTables tables{ws.seg, S, P};
    const int slots = (int)std::min<size_t>(kRasterSlots, kRasterDepthWords / raster_depth_words(H, W));
    const int n_groups = ((int)order.size() + slots - 1) / slots;
    std::vector<std::vector<int>> members(n_groups);
    for (int i = 0; i < n; ++i) members[where[i] / slots].push_back(i);
    const int pass = kSegGroupPoints / P, pad = (wmax - 1) * (1 << kRasterSnapBits) / 2;      // skeletons whose points the record area holds at a time: >= 64
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the segment table goes through pinned memory, so the copy is enqueued like a kernel; every other table is a kernel argument
    void* stage = nullptr;
    hipEvent_t staged = nullptr;
    if (int rc = h->seg_stage_slot(&stage, &staged)) return rc;
    memcpy(stage, segs.data(), (size_t)S * sizeof(SegSegment));
    hipError_t e = hipMemcpyAsync(ws.seg, stage, (size_t)S * sizeof(SegSegment), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipEventRecord(staged, s);
    for (int g = 0; g < n_groups && e == hipSuccess; ++g) {
        SegGroup grp{};
        grp.n = std::min(slots, (int)order.size() - g * slots);
        for (int k = 0; k < grp.n; ++k) grp.image[k] = order[(size_t)g * slots + k];
        const std::vector<int>& mem = members[g];
        // skeletons [first, last) of the group in launches of up to kSegBatchSkeletons, their points at records 0 ... of the record area
        auto each_batch = [&](int first, int last, auto&& launch) {
            for (int b0 = first; b0 < last && e == hipSuccess; b0 += kSegBatchSkeletons) {
                SegBatch b{};
                b.n = std::min(kSegBatchSkeletons, last - b0);
                b.base = b0 - first;
                for (int k = 0; k < b.n; ++k) b.rec[k] = SegSkeleton{mem[b0 + k], where[mem[b0 + k]] - g * slots, rank[mem[b0 + k]], 0};
                e = launch(b);
            }
        };
        auto setup = [&](const SegBatch& b) { return launch_segments_setup(points_dev, view, tables, b, pad, ws.work, s); };
        auto cover = [&](const SegBatch& b) { return launch_segments_cover(view, tables, b, ws.work, s); };
        const int m = (int)mem.size();
        if (m <= pass) {
            // the usual case: all points of the group are set up first, the boxes grow from nothing, and clear and resolve touch only them
            e = hipMemsetAsync(ws.work.bbox, 0x80, (size_t)grp.n * 4 * sizeof(int), s);
            each_batch(0, m, setup);
            if (e == hipSuccess) e = launch_raster_lines_clear(rv, ws.work, grp.n, s);
            each_batch(0, m, cover);
        } else {
            // more points than the record area holds: they go through in passes, each overwriting the last one's, so the boxes start as the whole
            // viewport and the clear comes first
            e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ws.work.bbox), kRasterCoordLimit, (size_t)grp.n * 4, s);
            if (e == hipSuccess) e = launch_raster_lines_clear(rv, ws.work, grp.n, s);
            for (int first = 0; first < m && e == hipSuccess; first += pass) {
                each_batch(first, std::min(m, first + pass), setup);
                each_batch(first, std::min(m, first + pass), cover);
            }
        }
        if (e == hipSuccess) e = launch_segments_resolve(view, grp, tables, ws.work, images_dev, s);
    }
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("render_segments: ") + hipGetErrorString(e));
    return 0;
}

int grnet_op_segments_setup(grnet_t* h, const float* points_dev, int P, const float* R_host, const double* proj_host, const double* window_host, int H,
                            int W, int32_t* xy_dev, float* depth_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_op_segments_setup: ";
    std::string why = sizes_error(P, 0, H, W);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    if (!points_dev || !proj_host || !window_host || !xy_dev || !depth_dev) return h->fail(GRNET_EINVAL, name + "null pointer (only R_host may be NULL)");
    why = view_error(R_host, proj_host, window_host);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    DeviceGuard guard(h->device);
    DeviceBlock ws;                                         // the box
    if (hipMalloc(&ws.p, 4 * sizeof(int)) != hipSuccess) return h->fail(GRNET_ENOMEM, name + "hipMalloc failed");
    RasterWork work{};
    work.xy = xy_dev, work.z = depth_dev;
    work.bbox = static_cast<int*>(ws.p);
    SegBatch one{};
    one.n = 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(work.bbox, 0x80, 4 * sizeof(int), s);
    if (e == hipSuccess) e = launch_segments_setup(points_dev, seg_view(R_host, proj_host, window_host, H, W), SegTables{nullptr, 0, P}, one, 0, work, s);
    const hipError_t e2 = hipStreamSynchronize(s);          // the temporaries go when this returns
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("op_segments_setup: ") + hipGetErrorString(e));
    return 0;
}

int grnet_op_raster_segments(grnet_t* h, const int32_t* xy_dev, const float* depth_dev, int P, const int32_t* segments_host, int S,
                             const int32_t* widths_host, int H, int W, int32_t* winner_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_op_raster_segments: ";
    std::string why = sizes_error(P, S, H, W);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    if (!xy_dev || !depth_dev || !segments_host || !widths_host || !winner_dev) return h->fail(GRNET_EINVAL, name + "null pointer");
    std::vector<SegSegment> segs;
    int wmax = 1;
    why = pack_segments(segments_host, nullptr, widths_host, S, P, segs, &wmax);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    DeviceGuard guard(h->device);
    const size_t words = raster_depth_words(H, W), table = (size_t)std::max(S, 1) * sizeof(SegSegment);
    DeviceBlock ws;                                         // [depth | segment table | box]
    if (hipMalloc(&ws.p, words * 8 + table + 4 * sizeof(int)) != hipSuccess) return h->fail(GRNET_ENOMEM, name + "hipMalloc failed");
    RasterWork work{};
    work.depth = static_cast<unsigned long long*>(ws.p);
    SegSegment* seg_dev = reinterpret_cast<SegSegment*>(work.depth + words);
    work.bbox = reinterpret_cast<int*>(reinterpret_cast<char*>(seg_dev) + table);
    work.xy = const_cast<int*>(xy_dev);                     // the cover kernel only reads the point records
    work.z = const_cast<float*>(depth_dev);
    const int whole[4] = {kRasterCoordLimit, kRasterCoordLimit, kRasterCoordLimit, kRasterCoordLimit};    // (-X, -Y, X, Y): the whole viewport is cleared
    SegView view{};
    view.H = H, view.W = W;
    SegBatch one{};
    one.n = 1;
    const RasterView rv = raster_view(H, W);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemcpyAsync(work.bbox, whole, sizeof(whole), hipMemcpyHostToDevice, s);      // a hook: it synchronises below anyway
    if (e == hipSuccess && S) e = hipMemcpyAsync(seg_dev, segs.data(), (size_t)S * sizeof(SegSegment), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_raster_lines_clear(rv, work, 1, s);
    if (e == hipSuccess) e = launch_segments_cover(view, SegTables{seg_dev, S, P}, one, work, s);
    if (e == hipSuccess) e = launch_raster_winner(rv, work, winner_dev, s);
    const hipError_t e2 = hipStreamSynchronize(s);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("op_raster_segments: ") + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
