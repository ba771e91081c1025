// The mesh overlay of demo.py --mesh_render behind the C ABI (lib/utils/renderer.py:78-126; kernels: render_kernels.hip, rules: DESIGN 4.5):
// the face table of a handle, grnet_render_meshes / grnet_render_meshes_ex (filled, or the wireframe), and the hooks that run the stages alone
// on a small mesh.
#include "grnet_impl.h"

namespace {

// faces (F,3) host -> ONE device block [faces 3F | row offsets V+1 | faces at each vertex 3F], the vertex -> face rows in ascending face order.
// 0, or GRNET_EINVAL (an index outside [0, V)) / GRNET_ENOMEM / GRNET_EHIP with *why set; *block is the caller's to hipFree.
int build_raster_mesh(const int32_t* faces, int F, int V, RasterMesh* out, void** block, std::string* why) {
    std::vector<int> host((size_t)3 * F + V + 1 + (size_t)3 * F, 0);
    int* off = host.data() + (size_t)3 * F;
    int* idx = off + V + 1;
    for (size_t k = 0; k < (size_t)3 * F; ++k) {
        if (faces[k] < 0 || faces[k] >= V) {
            *why = "face " + std::to_string(k / 3) + " names vertex " + std::to_string(faces[k]) + ", outside [0, " + std::to_string(V) + ")";
            return GRNET_EINVAL;
        }
        host[k] = faces[k];
        ++off[faces[k] + 1];
    }
    for (int v = 0; v < V; ++v) off[v + 1] += off[v];
    std::vector<int> fill(off, off + V);
    for (int f = 0; f < F; ++f)
        for (int k = 0; k < 3; ++k) idx[fill[faces[3 * f + k]]++] = f;    // a face that names a vertex twice is listed twice: its normal is 0 anyway
    void* d = nullptr;
    if (hipMalloc(&d, host.size() * sizeof(int)) != hipSuccess) { *why = "hipMalloc failed"; return GRNET_ENOMEM; }
    if (hipMemcpy(d, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        *why = "hipMemcpy of the face table failed";
        return GRNET_EHIP;
    }
    const int* p = static_cast<const int*>(d);
    *out = RasterMesh{p, p + (size_t)3 * F, p + (size_t)3 * F + V + 1, V, F};
    *block = d;
    return 0;
}

// [depth words | q | normals | z | xy | bounding boxes] from an 8-byte aligned base
RasterWork raster_carve(void* base, size_t depth_words, int slots, int V) {
    RasterWork w;
    w.depth = static_cast<unsigned long long*>(base);
    w.q = reinterpret_cast<float*>(w.depth + depth_words);
    w.nrm = w.q + (size_t)slots * V * 3;
    w.z = w.nrm + (size_t)slots * V * 3;
    w.xy = reinterpret_cast<int*>(w.z + (size_t)slots * V);
    w.bbox = w.xy + (size_t)slots * V * 2;
    return w;
}

RasterView raster_view(const float* M_host, int H, int W) {
    RasterView v{{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, H, W};
    if (M_host) memcpy(v.M, M_host, sizeof(v.M));
    return v;
}

// grnet_op_raster (lines = false) and grnet_op_raster_lines: one validation, one synchronisation
int op_raster(grnet_t* h, const int32_t* xy_dev, const float* z_dev, int V, const int32_t* faces_host, int F, int H, int W, int32_t* winner_dev, bool lines,
              void* stream) {
    const std::string op = lines ? "op_raster_lines" : "op_raster", name = "grnet_" + op;
    if (!h) return GRNET_EINVAL;
    if (!xy_dev || !z_dev || !faces_host || !winner_dev) return h->fail(GRNET_EINVAL, name + ": null pointer");
    if (V < 1 || F < 1) return h->fail(GRNET_EINVAL, name + ": V and F must be >= 1");
    if (!raster_dims_ok(H, W)) return h->fail(GRNET_EINVAL, name + ": image outside [1, " + std::to_string(kRasterMaxDim) + "]");
    DeviceGuard guard(h->device);
    RasterMesh m{};
    DeviceBlock table, ws;
    std::string why;
    if (int rc = build_raster_mesh(faces_host, F, V, &m, &table.p, &why)) return h->fail(rc, name + ": " + why);
    const size_t words = raster_depth_words(H, W);
    if (hipMalloc(&ws.p, words * 8 + 16) != hipSuccess) return h->fail(GRNET_ENOMEM, name + ": hipMalloc failed");
    RasterWork work{};
    work.depth = static_cast<unsigned long long*>(ws.p);
    work.bbox = reinterpret_cast<int*>(work.depth + words);
    work.xy = const_cast<int*>(xy_dev);                     // the cover kernels only read the vertex records
    work.z = const_cast<float*>(z_dev);
    const int whole[4] = {kRasterCoordLimit, kRasterCoordLimit, kRasterCoordLimit, kRasterCoordLimit};    // (-X, -Y, X, Y): the whole viewport is cleared
    RasterChunk c{};
    c.n = 1;
    const RasterView view = raster_view(nullptr, H, W);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemcpyAsync(work.bbox, whole, sizeof(whole), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = lines ? launch_raster_lines_cover(c, view, m, work, s) : launch_raster_cover(c, view, m, work, s);
    if (e == hipSuccess) e = launch_raster_winner(view, work, winner_dev, s);
    const hipError_t e2 = hipStreamSynchronize(s);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return h->fail(GRNET_EHIP, op + ": " + hipGetErrorString(e));
    return 0;
}

}  // namespace

namespace grnet_detail {
size_t raster_record_bytes(int slots, int V) { return (size_t)slots * ((size_t)V * 9 * 4 + 16); }
bool raster_dims_ok(int H, int W) { return H >= 1 && H <= kRasterMaxDim && W >= 1 && W <= kRasterMaxDim; }
}  // namespace grnet_detail

int grnet::raster_workspace(const char* who) {
    if (!raster_ws && hipMalloc(&raster_ws, kRasterDepthWords * 8 + raster_record_bytes(kRasterSlots, kSmplVerts)) != hipSuccess)
        return fail(GRNET_ENOMEM, std::string(who) + ": hipMalloc of the workspace failed");
    return 0;
}

void grnet::faces_clear() {
    if (!rmesh_block) return;
    (void)hipDeviceSynchronize();                           // a render that reads the table may still be running
    (void)hipFree(rmesh_block);
    rmesh_block = nullptr;
    rmesh = RasterMesh{};
    faces_host.clear();
    faces_unmatched = -1;
}

extern "C" {

int grnet_load_faces(grnet_t* h, const int32_t* faces_host, int n_faces) {
    if (!h) return GRNET_EINVAL;
    if (!faces_host) return h->fail(GRNET_EINVAL, "grnet_load_faces: null pointer");
    if (n_faces < 1) return h->fail(GRNET_EINVAL, "grnet_load_faces: n_faces " + std::to_string(n_faces) + " < 1");
    DeviceGuard guard(h->device);
    RasterMesh m{};
    void* block = nullptr;
    std::string why;
    if (int rc = build_raster_mesh(faces_host, n_faces, kSmplVerts, &m, &block, &why)) return h->fail(rc, "grnet_load_faces: " + why);
    h->faces_clear();                                       // a failure above leaves the table loaded before in place
    h->rmesh = m;
    h->rmesh_block = block;
    h->faces_host.assign(faces_host, faces_host + (size_t)3 * n_faces);      // for the closed-surface rule of grnet_mesh_moments, counted at its first call
    h->faces_unmatched = -1;
    return 0;
}

int grnet_render_meshes(grnet_t* h, const float* verts_dev, int n, const float* cams_dev, const float* colours_host, const int32_t* image_index_host,
                        const float* M_host, unsigned char* images_dev, int F, int H, int W, void* stream) {
    return grnet_render_meshes_ex(h, verts_dev, n, cams_dev, colours_host, image_index_host, M_host, images_dev, F, H, W, 0u, stream);
}

int grnet_render_meshes_ex(grnet_t* h, const float* verts_dev, int n, const float* cams_dev, const float* colours_host, const int32_t* image_index_host,
                           const float* M_host, unsigned char* images_dev, int F, int H, int W, unsigned flags, void* stream) {
    if (!h) return GRNET_EINVAL;
    if (flags & ~(unsigned)GRNET_RENDER_WIREFRAME)
        return h->fail(GRNET_EINVAL, "grnet_render_meshes_ex: flags " + std::to_string(flags) + " has bits other than GRNET_RENDER_WIREFRAME (1)");
    const bool lines = flags & GRNET_RENDER_WIREFRAME;
    if (n < 0) return h->fail(GRNET_EINVAL, "grnet_render_meshes: n " + std::to_string(n) + " < 0");
    if (!raster_dims_ok(H, W))
        return h->fail(GRNET_EINVAL, "grnet_render_meshes: image " + std::to_string(H) + " x " + std::to_string(W) + " outside [1, " + std::to_string(kRasterMaxDim) + "]");
    if (F < 1) return h->fail(GRNET_EINVAL, "grnet_render_meshes: F " + std::to_string(F) + " < 1");
    if (!h->rmesh_block) return h->fail(GRNET_ESTATE, "grnet_render_meshes before grnet_load_faces");
    if (n == 0) return 0;
    if (!verts_dev || !cams_dev || !colours_host || !image_index_host || !images_dev) return h->fail(GRNET_EINVAL, "grnet_render_meshes: null pointer (only M_host may be NULL)");
    for (int i = 0; i < n; ++i)
        if (image_index_host[i] < 0 || image_index_host[i] >= F)
            return h->fail(GRNET_EINVAL, "grnet_render_meshes: image_index[" + std::to_string(i) + "] = " + std::to_string(image_index_host[i]) + " outside [0, " + std::to_string(F) + ")");
    DeviceGuard guard(h->device);
    if (int rc = h->raster_workspace("grnet_render_meshes")) return rc;
    const RasterWork work = raster_carve(h->raster_ws, kRasterDepthWords, kRasterSlots, kSmplVerts);
    const RasterView view = raster_view(M_host, H, W);
    const int slots = (int)std::min<size_t>(kRasterSlots, kRasterDepthWords / raster_depth_words(H, W));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // layer l holds the (l+1)-th mesh of every image in call order: at most one mesh per image, so the meshes of a layer are independent, and
    // the layers in stream order paint later meshes over earlier ones
    std::vector<int> layer(n);
    std::unordered_map<int, int> seen;
    int layers = 0;
    for (int i = 0; i < n; ++i) layers = std::max(layers, (layer[i] = seen[image_index_host[i]]++) + 1);
    RasterChunk c{};
    auto flush = [&]() -> hipError_t {
        if (!c.n) return hipSuccess;
        hipError_t e = launch_raster_setup(verts_dev, cams_dev, c, view, h->rmesh, work, s);
        if (e == hipSuccess) e = lines ? launch_raster_lines_cover(c, view, h->rmesh, work, s) : launch_raster_cover(c, view, h->rmesh, work, s);
        if (e == hipSuccess) e = lines ? launch_raster_lines_resolve(c, view, h->rmesh, work, images_dev, s) : launch_raster_resolve(c, view, h->rmesh, work, images_dev, s);
        c.n = 0;
        return e;
    };
    for (int l = 0; l < layers; ++l) {
        c.n = 0;
        for (int i = 0; i < n; ++i) {
            if (layer[i] != l) continue;
            c.mesh[c.n] = i;
            c.image[c.n] = image_index_host[i];
            for (int k = 0; k < 3; ++k) c.colour[c.n][k] = colours_host[3 * i + k];
            if (++c.n == slots) {
                if (hipError_t e = flush()) return h->fail(GRNET_EHIP, std::string("render_meshes: ") + hipGetErrorString(e));
            }
        }
        if (hipError_t e = flush()) return h->fail(GRNET_EHIP, std::string("render_meshes: ") + hipGetErrorString(e));
    }
    return 0;
}

int grnet_op_raster_setup(grnet_t* h, const float* verts_dev, int V, const int32_t* faces_host, int F, const float* cam_dev, const float* M_host,
                          int H, int W, int32_t* xy_dev, float* z_dev, float* normals_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    if (!verts_dev || !faces_host || !cam_dev || !xy_dev || !z_dev || !normals_dev) return h->fail(GRNET_EINVAL, "grnet_op_raster_setup: null pointer (only M_host may be NULL)");
    if (V < 1 || F < 1) return h->fail(GRNET_EINVAL, "grnet_op_raster_setup: V and F must be >= 1");
    if (!raster_dims_ok(H, W)) return h->fail(GRNET_EINVAL, "grnet_op_raster_setup: image outside [1, " + std::to_string(kRasterMaxDim) + "]");
    DeviceGuard guard(h->device);
    RasterMesh m{};
    DeviceBlock table, ws;
    std::string why;
    if (int rc = build_raster_mesh(faces_host, F, V, &m, &table.p, &why)) return h->fail(rc, "grnet_op_raster_setup: " + why);
    if (hipMalloc(&ws.p, raster_record_bytes(1, V)) != hipSuccess) return h->fail(GRNET_ENOMEM, "grnet_op_raster_setup: hipMalloc failed");
    const RasterWork work = raster_carve(ws.p, 0, 1, V);
    RasterChunk c{};
    c.n = 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = launch_raster_setup(verts_dev, cam_dev, c, raster_view(M_host, H, W), m, work, s);
    if (e == hipSuccess) e = hipMemcpyAsync(xy_dev, work.xy, (size_t)V * 2 * sizeof(int), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(z_dev, work.z, (size_t)V * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(normals_dev, work.nrm, (size_t)V * 3 * sizeof(float), hipMemcpyDeviceToDevice, s);
    const hipError_t e2 = hipStreamSynchronize(s);          // the temporaries go when this returns
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("op_raster_setup: ") + hipGetErrorString(e));
    return 0;
}

int grnet_op_raster(grnet_t* h, const int32_t* xy_dev, const float* z_dev, int V, const int32_t* faces_host, int F, int H, int W, int32_t* winner_dev,
                    void* stream) {
    return op_raster(h, xy_dev, z_dev, V, faces_host, F, H, W, winner_dev, false, stream);
}

int grnet_op_raster_lines(grnet_t* h, const int32_t* xy_dev, const float* z_dev, int V, const int32_t* faces_host, int F, int H, int W,
                          int32_t* winner_dev, void* stream) {
    return op_raster(h, xy_dev, z_dev, V, faces_host, F, H, W, winner_dev, true, stream);
}

}  // extern "C"
