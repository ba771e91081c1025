// Pose metrics behind the C ABI (kernels: metric_kernels.hip, rules: DESIGN 4.8): grnet_pose_metrics and the hook that runs the Procrustes rotation
// alone.  Neither reads a weight or the arena; the scratch is metric_ws (grow_scratch).
#include "grnet_impl.h"

namespace {

// "" or what is wrong with `count` indices into J joints
std::string indices_error(const int32_t* idx, int count, int J, const char* what) {
    for (int i = 0; i < count; ++i)
        if (idx[i] < 0 || idx[i] >= J) return std::string(what) + "[" + std::to_string(i) + "] = " + std::to_string(idx[i]) + " outside [0, " + std::to_string(J) + ")";
    return "";
}

}  // namespace

extern "C" {

int grnet_pose_metrics(grnet_t* h, const float* pred_dev, const float* gt_dev, int J, const int32_t* frame_offsets_host, int n_seq,
                       const int32_t* select_host, int n_select, const int32_t* root_host, int n_root, const float* pred_verts_dev,
                       const float* gt_verts_dev, int V, double unit, double* per_frame_dev, double* per_seq_dev, double* total_dev, double* transform_dev,
                       void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_pose_metrics: ";
    const std::string top = std::to_string(kMetricMaxJoints);
    if (J < 1 || J > kMetricMaxJoints) return h->fail(GRNET_EINVAL, name + "J " + std::to_string(J) + " outside [1, " + top + "]");
    if (n_seq < 1) return h->fail(GRNET_EINVAL, name + "n_seq " + std::to_string(n_seq) + " < 1");
    if (!pred_dev || !gt_dev || !frame_offsets_host) return h->fail(GRNET_EINVAL, name + "null pointer (pred_dev, gt_dev and frame_offsets_host are needed)");
    if (select_host ? (n_select < 1 || n_select > kMetricMaxJoints) : n_select != 0)
        return h->fail(GRNET_EINVAL, name + "n_select " + std::to_string(n_select) + (select_host ? " outside [1, " + top + "]" : " without select_host"));
    if (root_host ? (n_root < 1 || n_root > kMetricMaxJoints) : n_root != 0)
        return h->fail(GRNET_EINVAL, name + "n_root " + std::to_string(n_root) + (root_host ? " outside [1, " + top + "]" : " without root_host"));
    if (!pred_verts_dev != !gt_verts_dev) return h->fail(GRNET_EINVAL, name + "pred_verts_dev and gt_verts_dev go together: one of them is null");
    const bool has_verts = pred_verts_dev != nullptr;
    if (has_verts && V < 1) return h->fail(GRNET_EINVAL, name + "V " + std::to_string(V) + " < 1");
    if (has_verts && 3LL * V > 0x7fffffffLL) return h->fail(GRNET_EINVAL, name + "V " + std::to_string(V) + ": 3 V no longer fits 31 bits");
    if (!std::isfinite(unit)) return h->fail(GRNET_EINVAL, name + "unit must be finite");
    std::string why = offsets_error(frame_offsets_host, n_seq, "frame_offsets", 0, 0);      // no 31-bit rule: the kernels index with size_t
    if (why.empty() && select_host) why = indices_error(select_host, n_select, J, "select");
    if (why.empty() && root_host) why = indices_error(root_host, n_root, J, "root");
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);

    MetricJoints mj{};
    mj.n_select = select_host ? n_select : J;
    mj.n_root = n_root;
    for (int i = 0; i < mj.n_select; ++i) mj.select[i] = (unsigned char)(select_host ? select_host[i] : i);
    for (int i = 0; i < n_root; ++i) mj.root[i] = (unsigned char)root_host[i];
    const int frames = frame_offsets_host[n_seq];
    const bool means = per_seq_dev || total_dev;
    if (!per_frame_dev && !means && !transform_dev) return 0;  // nothing was asked for
    const size_t b_rows = per_frame_dev ? 0 : align256((size_t)frames * 5 * sizeof(double));
    const size_t b_sum = means ? align256((size_t)n_seq * 5 * sizeof(double)) : 0, b_cnt = means ? align256((size_t)n_seq * 5 * sizeof(long long)) : 0;
    DeviceGuard guard(h->device);
    char* ws = nullptr;
    if (b_rows + b_sum + b_cnt)
        if (int rc = h->metric_scratch(b_rows + b_sum + b_cnt, &ws)) return rc;
    double* rows = per_frame_dev ? per_frame_dev : reinterpret_cast<double*>(ws);
    double* seq_sum = reinterpret_cast<double*>(ws + b_rows);
    long long* seq_cnt = reinterpret_cast<long long*>(ws + b_rows + b_sum);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = launch_metric_joints(pred_dev, gt_dev, J, frames, mj, unit, has_verts, rows, transform_dev, s);
    if (e == hipSuccess && has_verts) e = launch_metric_verts(pred_verts_dev, gt_verts_dev, V, frames, unit, rows, s);
    for (int q0 = 0; q0 < n_seq && e == hipSuccess; q0 += kMetricBatch) {
        MetricBatch b{};
        b.n = std::min(kMetricBatch, n_seq - q0);
        for (int q = 0; q <= b.n; ++q) b.off[q] = frame_offsets_host[q0 + q];
        e = launch_metric_accel(pred_dev, gt_dev, J, b, mj, unit, rows, s);
        if (e == hipSuccess && means) e = launch_metric_seq_means(rows, b, q0, has_verts, seq_sum, seq_cnt, per_seq_dev, s);
    }
    if (e == hipSuccess && total_dev) e = launch_metric_total(seq_sum, seq_cnt, n_seq, total_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("pose_metrics: ") + hipGetErrorString(e));
    return 0;
}

int grnet_op_procrustes(grnet_t* h, const double* K_dev, int k, double* R_dev, double* sigma_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    if (k < 1) return h->fail(GRNET_EINVAL, "grnet_op_procrustes: k " + std::to_string(k) + " < 1");
    if (!K_dev || !R_dev || !sigma_dev) return h->fail(GRNET_EINVAL, "grnet_op_procrustes: null pointer");
    DeviceGuard guard(h->device);
    const hipError_t e = launch_procrustes(K_dev, k, R_dev, sigma_dev, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("op_procrustes: ") + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
