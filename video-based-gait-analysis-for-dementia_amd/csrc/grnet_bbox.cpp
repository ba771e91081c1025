// Boxes from 2D joints behind the C ABI (batch_generation.py:39-93, get_bbox_from_joints2d; kernels: bbox_kernels.hip, rules: DESIGN 4.7):
// grnet_bbox_from_joints2d and the hook that runs the 1-medoid alone.  Neither reads a weight or the arena; their scratch is bbox_ws (grow_scratch).
#include "grnet_impl.h"

namespace {

constexpr int kMedoidMaxPoints = kBboxMaxFrames * kBboxMaxJoints;      // points of one sequence

// Column splits of a call: enough workgroups for four per CU (one 400-frame sequence is 40 row tiles), a split keeping at least one row tile's worth of columns
int choose_splits(const std::vector<int>& point_off) {
    long long tiles = 0;
    int most = 0;
    for (size_t q = 0; q + 1 < point_off.size(); ++q) {
        const int n = point_off[q + 1] - point_off[q];
        tiles += (n + kMedoidRows - 1) / kMedoidRows;
        most = std::max(most, n);
    }
    const long long want = (1024 + tiles - 1) / tiles;
    return (int)std::max<long long>(1, std::min<long long>(want, std::min(kMedoidMaxSplits, (most + kMedoidRows - 1) / kMedoidRows)));
}

// The launches of one call over sequences point_off[0 .. n_seq]: row sums, argmin and, with hgt, the boxes -- in batches of kMedoidBatch sequences
hipError_t run_medoid(const float* points, const std::vector<int>& point_off, int splits, double* partial, int* index, double* cost, float* centre,
                      const double* hgt, int K, double* bbox, hipStream_t s) {
    const int n_seq = (int)point_off.size() - 1;
    for (int q0 = 0; q0 < n_seq; q0 += kMedoidBatch) {
        MedoidBatch b{};
        b.n = std::min(kMedoidBatch, n_seq - q0);
        for (int q = 0; q <= b.n; ++q) b.off[q] = point_off[q0 + q];
        hipError_t e = launch_medoid_rowsum(points, b, splits, partial, s);
        if (e == hipSuccess) e = launch_medoid_argmin(points, b, q0, splits, partial, index, cost, centre, s);
        if (e == hipSuccess && hgt) e = launch_bbox_assemble(hgt, b, q0, K, centre, bbox, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

extern "C" {

int grnet_bbox_from_joints2d(grnet_t* h, const double* joints_dev, int K, const int32_t* frame_offsets_host, int n_seq, double threshold,
                             double* bbox_dev, int32_t* medoid_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_bbox_from_joints2d: ";
    if (K < 1 || K > kBboxMaxJoints) return h->fail(GRNET_EINVAL, name + "K " + std::to_string(K) + " outside [1, " + std::to_string(kBboxMaxJoints) + "]");
    if (n_seq < 1) return h->fail(GRNET_EINVAL, name + "n_seq " + std::to_string(n_seq) + " < 1");
    if (!joints_dev || !frame_offsets_host || !bbox_dev) return h->fail(GRNET_EINVAL, name + "null pointer (only medoid_dev may be NULL)");
    if (!std::isfinite(threshold)) return h->fail(GRNET_EINVAL, name + "threshold must be finite");
    const std::string why = offsets_error(frame_offsets_host, n_seq, "frame_offsets", kBboxMaxFrames, K);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why + " (a sequence has 1 .. " + std::to_string(kBboxMaxFrames) + " frames)");
    std::vector<int> point_off(n_seq + 1);
    for (int q = 0; q <= n_seq; ++q) point_off[q] = frame_offsets_host[q] * K;
    const int frames = frame_offsets_host[n_seq], splits = choose_splits(point_off);
    const size_t P = (size_t)frames * K;
    const size_t b_points = align256(P * 16), b_partial = align256(P * splits * sizeof(double)), b_hgt = align256((size_t)frames * sizeof(double));
    DeviceGuard guard(h->device);
    char* ws = nullptr;
    if (int rc = h->bbox_scratch(b_points + b_partial + b_hgt + (size_t)n_seq * 2 * sizeof(float), &ws)) return rc;
    float* points = reinterpret_cast<float*>(ws);
    double* partial = reinterpret_cast<double*>(ws + b_points);
    double* hgt = reinterpret_cast<double*>(ws + b_points + b_partial);
    float* centre = reinterpret_cast<float*>(ws + b_points + b_partial + b_hgt);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = launch_bbox_prepare(joints_dev, K, frames, threshold, points, hgt, s);
    if (e == hipSuccess) e = run_medoid(points, point_off, splits, partial, medoid_dev, nullptr, centre, hgt, K, bbox_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("bbox_from_joints2d: ") + hipGetErrorString(e));
    return 0;
}

int grnet_op_medoid(grnet_t* h, const float* points_dev, const int32_t* point_offsets_host, int n_seq, int splits, int32_t* index_dev, double* cost_dev,
                    void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_op_medoid: ";
    if (n_seq < 1) return h->fail(GRNET_EINVAL, name + "n_seq " + std::to_string(n_seq) + " < 1");
    if (splits < 0 || splits > kMedoidMaxSplits) return h->fail(GRNET_EINVAL, name + "splits " + std::to_string(splits) + " outside [0, " + std::to_string(kMedoidMaxSplits) + "]");
    if (!points_dev || !point_offsets_host || !index_dev || !cost_dev) return h->fail(GRNET_EINVAL, name + "null pointer");
    if (reinterpret_cast<uintptr_t>(points_dev) & 15) return h->fail(GRNET_EINVAL, name + "points_dev must be 16-byte aligned");
    const std::string why = offsets_error(point_offsets_host, n_seq, "point_offsets", kMedoidMaxPoints, 1);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    const std::vector<int> point_off(point_offsets_host, point_offsets_host + n_seq + 1);
    if (!splits) splits = choose_splits(point_off);
    DeviceGuard guard(h->device);
    char* ws = nullptr;
    if (int rc = h->bbox_scratch((size_t)point_off[n_seq] * splits * sizeof(double), &ws)) return rc;
    const hipError_t e = run_medoid(points_dev, point_off, splits, reinterpret_cast<double*>(ws), index_dev, cost_dev, nullptr, nullptr, 1, nullptr,
                                    static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("op_medoid: ") + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
