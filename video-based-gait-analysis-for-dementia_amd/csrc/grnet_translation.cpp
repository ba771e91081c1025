// The camera-space trajectory behind the C ABI (kernels: translation_kernels.hip, arithmetic: translation3.h, rules: DESIGN 4.9):
// grnet_fit_translation.  It reads no weight and no arena, and needs no scratch: both outputs are the caller's.
#include "grnet_impl.h"

extern "C" {

int grnet_fit_translation(grnet_t* h, const float* joints3d_dev, int K3, const float* joints2d_dev, int K2, int frames, const int32_t* frame_offsets_host,
                          int n_seq, const int32_t* pairs_host, int n_pairs, const double* camera_host, double conf_threshold, int min_joints, int root,
                          int fill, double* per_frame_dev, double* per_seq_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_fit_translation: ";
    auto num = [](long long v) { return std::to_string(v); };
    if (!joints3d_dev || !joints2d_dev || !frame_offsets_host || !pairs_host || !camera_host || !per_frame_dev || !per_seq_dev)
        return h->fail(GRNET_EINVAL, name + "null pointer (joints3d_dev, joints2d_dev, frame_offsets_host, pairs_host, camera_host, per_frame_dev and "
                                            "per_seq_dev are all needed)");
    if (K3 < 1 || K2 < 1) return h->fail(GRNET_EINVAL, name + "K3 " + num(K3) + " or K2 " + num(K2) + " < 1");
    if (n_pairs < 1 || n_pairs > kTransMaxPairs) return h->fail(GRNET_EINVAL, name + "n_pairs " + num(n_pairs) + " outside [1, " + num(kTransMaxPairs) + "]");
    for (int j = 0; j < n_pairs; ++j) {
        if (pairs_host[2 * j] < 0 || pairs_host[2 * j] >= K3)
            return h->fail(GRNET_EINVAL, name + "pairs[" + num(j) + "][0] = " + num(pairs_host[2 * j]) + " outside [0, K3 = " + num(K3) + ")");
        if (pairs_host[2 * j + 1] < 0 || pairs_host[2 * j + 1] >= K2)
            return h->fail(GRNET_EINVAL, name + "pairs[" + num(j) + "][1] = " + num(pairs_host[2 * j + 1]) + " outside [0, K2 = " + num(K2) + ")");
    }
    if (n_seq < 1) return h->fail(GRNET_EINVAL, name + "n_seq " + num(n_seq) + " < 1");
    if (frames < 1) return h->fail(GRNET_EINVAL, name + "frames " + num(frames) + " < 1");
    const std::string why = offsets_error(frame_offsets_host, n_seq, "frame_offsets", 0, 0);      // no 31-bit rule: the kernels index with size_t
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    if (frame_offsets_host[n_seq] != frames)
        return h->fail(GRNET_EINVAL, name + "the offsets end at " + num(frame_offsets_host[n_seq]) + ", not at the " + num(frames) + " frames");
    for (int q = 0; q < n_seq; ++q) {
        const double* cam = camera_host + 3 * (size_t)q;
        if (!std::isfinite(cam[0]) || cam[0] <= 0.) return h->fail(GRNET_EINVAL, name + "the focal length of sequence " + num(q) + " must be finite and positive");
        if (!std::isfinite(cam[1]) || !std::isfinite(cam[2])) return h->fail(GRNET_EINVAL, name + "the centre of sequence " + num(q) + " must be finite");
    }
    if (!std::isfinite(conf_threshold) || conf_threshold < 0.) return h->fail(GRNET_EINVAL, name + "conf_threshold must be finite and not negative");
    if (min_joints < 2) return h->fail(GRNET_EINVAL, name + "min_joints " + num(min_joints) + " < 2");
    if (root < 0 || root >= K3) return h->fail(GRNET_EINVAL, name + "root " + num(root) + " outside [0, K3 = " + num(K3) + ")");

    TransPairs pairs{};
    pairs.n = n_pairs;
    for (int j = 0; j < n_pairs; ++j) { pairs.p3[j] = pairs_host[2 * j]; pairs.p2[j] = pairs_host[2 * j + 1]; }
    DeviceGuard guard(h->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
    for (int q0 = 0; q0 < n_seq && e == hipSuccess; q0 += kTransBatch) {
        TransBatch b{};
        b.n = std::min(kTransBatch, n_seq - q0);
        for (int q = 0; q <= b.n; ++q) b.off[q] = frame_offsets_host[q0 + q];
        for (int q = 0; q < b.n; ++q)
            for (int c = 0; c < 3; ++c) b.cam[q][c] = camera_host[3 * (size_t)(q0 + q) + c];
        e = launch_translation_fit(joints3d_dev, joints2d_dev, K3, K2, pairs, b, conf_threshold, min_joints, per_frame_dev, s);
        if (e == hipSuccess) e = launch_translation_seq(joints3d_dev, K3, root, b, q0, fill != 0, per_frame_dev, per_seq_dev, s);
    }
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("fit_translation: ") + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
