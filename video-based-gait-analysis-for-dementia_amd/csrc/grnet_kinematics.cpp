// Joint-angle kinematics per gait cycle behind the C ABI (kernels: gait_kinematics_kernels.hip, arithmetic: gait_angles.h, rules: DESIGN 4.12):
// grnet_gait_kinematics and the hook that runs its cycle stage alone.  Neither reads a weight or the arena.  Their scratch and their table of
// offsets and weights are seq_call's (grnet_seq.cpp): the call returns without waiting for the device.
#include "grnet_impl.h"

namespace {

std::string strides_error(int min_stride, int max_stride) {
    if (min_stride < 1) return "min_stride " + std::to_string(min_stride) + " < 1";
    if (max_stride < min_stride) return "max_stride " + std::to_string(max_stride) + " < min_stride " + std::to_string(min_stride);
    if (max_stride > kKinMaxStride) return "max_stride " + std::to_string(max_stride) + " > " + std::to_string(kKinMaxStride);
    return "";
}

}  // namespace

extern "C" {

int grnet_gait_kinematics(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                          const int32_t* events_dev, double sigma, int min_stride, int max_stride, double* per_frame_dev, double* curves_dev,
                          double* per_seq_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_gait_kinematics: ";
    if (!joints3d_dev || !frame_offsets_host || !joints_host || !events_dev || !per_frame_dev || !curves_dev || !per_seq_dev)
        return h->fail(GRNET_EINVAL, name + "null pointer (joints3d_dev, frame_offsets_host, joints_host, events_dev, per_frame_dev, curves_dev and per_seq_dev are all needed)");
    KinTable tab{};
    std::string why = joint_table_take(joints_host, 16, J, tab.j);
    if (why.empty()) why = sigma_error(sigma, kTrackMaxSigma);
    if (why.empty()) why = strides_error(min_stride, max_stride);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    size_t mask_words = 0, b_words = 0, b_raw = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = seq_call(h, name, frame_offsets_host, n_seq, std::max(3LL * J, 13LL), sigma, s, &c, [&](int frames) {      // 13 angle columns a frame
            mask_words = gait_mask_words(frames, n_seq);
            b_words = gait_mask_bytes(kKinMaskSets, mask_words);
            b_raw = raw_bytes(sigma, 13, frames);
            return b_words + b_raw;
        }))
        return rc;
    const int frames = frame_offsets_host[n_seq];
    unsigned long long* words = reinterpret_cast<unsigned long long*>(c.behind);
    double* raw = b_raw ? reinterpret_cast<double*>(c.behind + b_words) : nullptr;
    hipError_t e = launch_kin_frames(joints3d_dev, J, frames, tab, raw, per_frame_dev, s);
    if (e == hipSuccess && raw) e = launch_seq_gauss_columns(c.off, n_seq, 13, c.weights, c.radius, frames, raw, per_frame_dev, 13, 0, s);
    if (e == hipSuccess) e = launch_kin_cycles(c.off, n_seq, events_dev, per_frame_dev, min_stride, max_stride, words, mask_words, curves_dev, per_seq_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

int grnet_op_gait_cycles(grnet_t* h, const double* angles_dev, const int32_t* events_dev, const int32_t* frame_offsets_host, int n_seq, int min_stride,
                         int max_stride, double* curves_dev, double* per_seq_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_op_gait_cycles: ";
    if (!angles_dev || !events_dev || !frame_offsets_host || !curves_dev || !per_seq_dev) return h->fail(GRNET_EINVAL, name + "null pointer");
    const std::string why = strides_error(min_stride, max_stride);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    size_t mask_words = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = seq_call(h, name, frame_offsets_host, n_seq, 13, 0., s, &c, [&](int frames) {
            mask_words = gait_mask_words(frames, n_seq);
            return gait_mask_bytes(kKinMaskSets, mask_words);
        }))
        return rc;
    const hipError_t e = launch_kin_cycles(c.off, n_seq, events_dev, angles_dev, min_stride, max_stride, reinterpret_cast<unsigned long long*>(c.behind), mask_words,
                                           curves_dev, per_seq_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
