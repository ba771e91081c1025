// Joint-angle kinematics per gait cycle behind the C ABI (kernels: gait_kinematics_kernels.hip, arithmetic: gait_angles.h, rules: DESIGN 4.12):
// grnet_gait_kinematics and the hook that runs its cycle stage alone.  Neither reads a weight or the arena.  Their scratch is the box calls'
// (bbox_scratch, grown on demand and kept); the sequences' offsets and the Gaussian's weights reach it as grnet_track_boxes' do, through a slot of
// the handle's pinned ring, so the copy is enqueued like a kernel and the call returns without waiting for the device.
#include "grnet_impl.h"

namespace {

size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

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
    if (J < 1) return h->fail(GRNET_EINVAL, name + "J " + std::to_string(J) + " < 1");
    KinTable tab{};
    for (int k = 0; k < 16; ++k) {
        if (joints_host[k] < 0 || joints_host[k] >= J)
            return h->fail(GRNET_EINVAL, name + "joint index " + std::to_string(joints_host[k]) + " (entry " + std::to_string(k) + ") outside [0, " + std::to_string(J) + ")");
        tab.j[k] = joints_host[k];
    }
    if (n_seq < 1 || n_seq > kTrackMaxSeqs) return h->fail(GRNET_EINVAL, name + "n_seq " + std::to_string(n_seq) + " outside [1, " + std::to_string(kTrackMaxSeqs) + "]");
    if (!std::isfinite(sigma) || sigma < 0. || sigma > kTrackMaxSigma) return h->fail(GRNET_EINVAL, name + "sigma must be 0 (no Gaussian) or within (0, " + std::to_string((int)kTrackMaxSigma) + "]");
    std::string why = strides_error(min_stride, max_stride);
    if (why.empty()) why = track_offsets_error(frame_offsets_host, n_seq, J * 3ll > 13 ? J * 3ll : 13);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    const int frames = frame_offsets_host[n_seq];
    const size_t mask_words = gait_mask_words(frames, n_seq);
    const size_t b_words = align256(kKinMaskSets * mask_words * sizeof(unsigned long long)), b_raw = sigma > 0. ? align256((size_t)frames * 13 * sizeof(double)) : 0;
    DeviceGuard guard(h->device);
    char* ws = nullptr;
    if (int rc = h->bbox_scratch(kTrackFront + b_words + b_raw, &ws)) return rc;
    unsigned long long* words = reinterpret_cast<unsigned long long*>(ws + kTrackFront);
    double* raw = b_raw ? reinterpret_cast<double*>(ws + kTrackFront + b_words) : nullptr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TrackTable t{};
    if (int rc = track_upload_table(h, name, frame_offsets_host, n_seq, sigma, ws, s, &t)) return rc;
    hipError_t e = launch_kin_frames(joints3d_dev, J, frames, tab, raw, per_frame_dev, s);
    if (e == hipSuccess && raw) e = launch_kin_smooth(t.off, n_seq, t.weights, t.radius, frames, raw, per_frame_dev, s);
    if (e == hipSuccess) e = launch_kin_cycles(t.off, n_seq, events_dev, per_frame_dev, min_stride, max_stride, words, mask_words, curves_dev, per_seq_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

int grnet_op_gait_cycles(grnet_t* h, const double* angles_dev, const int32_t* events_dev, const int32_t* frame_offsets_host, int n_seq, int min_stride,
                         int max_stride, double* curves_dev, double* per_seq_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_op_gait_cycles: ";
    if (!angles_dev || !events_dev || !frame_offsets_host || !curves_dev || !per_seq_dev) return h->fail(GRNET_EINVAL, name + "null pointer");
    if (n_seq < 1 || n_seq > kTrackMaxSeqs) return h->fail(GRNET_EINVAL, name + "n_seq " + std::to_string(n_seq) + " outside [1, " + std::to_string(kTrackMaxSeqs) + "]");
    std::string why = strides_error(min_stride, max_stride);
    if (why.empty()) why = track_offsets_error(frame_offsets_host, n_seq, 13);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    const int frames = frame_offsets_host[n_seq];
    const size_t mask_words = gait_mask_words(frames, n_seq);
    DeviceGuard guard(h->device);
    char* ws = nullptr;
    if (int rc = h->bbox_scratch(kTrackFront + align256(kKinMaskSets * mask_words * sizeof(unsigned long long)), &ws)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TrackTable t{};
    if (int rc = track_upload_table(h, name, frame_offsets_host, n_seq, 0., ws, s, &t)) return rc;
    const hipError_t e = launch_kin_cycles(t.off, n_seq, events_dev, angles_dev, min_stride, max_stride, reinterpret_cast<unsigned long long*>(ws + kTrackFront), mask_words,
                                           curves_dev, per_seq_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
