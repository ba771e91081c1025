// Volume, centre of mass, central second moments and area of the mesh behind the C ABI (kernel: mesh_moments_kernels.hip, arithmetic and the
// closed-table rule: mesh_moments.h, rules: DESIGN 4.25): grnet_mesh_moments, its hook that names the form of the gather, and the host-only
// grnet_faces_closed.  None reads a weight or the arena; the face table is grnet_load_faces' (grnet_render.cpp).  Nothing synchronises.
#include "grnet_impl.h"
#include "mesh_moments.h"

namespace {

// rule 5 on the handle's table, counted at the first call after grnet_load_faces and kept
long long faces_unmatched(grnet_t* h) {
    if (h->faces_unmatched < 0) {
        std::vector<unsigned long long> keys(h->faces_host.size());
        h->faces_unmatched = mesh_unmatched_edges(h->faces_host.data(), (int)(h->faces_host.size() / 3), h->rmesh.n_verts, keys.data());
    }
    return h->faces_unmatched;
}

int mesh_moments(grnet_t* h, const std::string& name, const float* verts_dev, int n, double* rows_dev, double* sums_dev, int form, void* stream) {
    if (!verts_dev || !rows_dev) return h->fail(GRNET_EINVAL, name + "null pointer (verts_dev and rows_dev are needed; only sums_dev may be NULL)");
    if (n < 1) return h->fail(GRNET_EINVAL, name + "n " + std::to_string(n) + " < 1");
    if (form != kMeshFormDirect && form != kMeshFormStaged) return h->fail(GRNET_EINVAL, name + "form " + std::to_string(form) + " is neither 0 (direct) nor 1 (staged)");
    if (!h->rmesh_block) return h->fail(GRNET_ESTATE, name + "before grnet_load_faces");
    if (const long long bad = faces_unmatched(h)) {
        char why[192];
        mesh_table_text(MeshTableFault{kMeshTableOpen, 0, bad}, h->rmesh.n_verts, why, sizeof why);
        return h->fail(GRNET_EINVAL, name + why);
    }
    DeviceGuard guard(h->device);
    const hipError_t e = launch_mesh_moments(verts_dev, n, h->rmesh, form, rows_dev, sums_dev, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

}  // namespace

extern "C" {

int grnet_mesh_moments(grnet_t* h, const float* verts_dev, int n, double* rows_dev, double* sums_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    return mesh_moments(h, "grnet_mesh_moments: ", verts_dev, n, rows_dev, sums_dev, kMeshFormDefault, stream);
}

int grnet_op_mesh_moments(grnet_t* h, const float* verts_dev, int n, double* rows_dev, double* sums_dev, int form, void* stream) {
    if (!h) return GRNET_EINVAL;
    return mesh_moments(h, "grnet_op_mesh_moments: ", verts_dev, n, rows_dev, sums_dev, form, stream);
}

int grnet_faces_closed(grnet_t* h, int* unmatched_edges_host) {
    if (!h) return GRNET_EINVAL;
    if (!unmatched_edges_host) return h->fail(GRNET_EINVAL, "grnet_faces_closed: null pointer");
    if (!h->rmesh_block) return h->fail(GRNET_ESTATE, "grnet_faces_closed: before grnet_load_faces");
    *unmatched_edges_host = (int)std::min<long long>(faces_unmatched(h), 2147483647LL);
    return 0;
}

}  // extern "C"
