// Gait events and parameters from the 3D joints behind the C ABI (kernels: gait_kernels.hip, arithmetic: gait_events.h, rules: DESIGN 4.11):
// grnet_gait_parameters and the hook that runs its events rule alone.  Neither reads a weight or the arena.  Their scratch is the box calls'
// (bbox_scratch, grown on demand and kept); the sequences' offsets and the Gaussian's weights reach it as grnet_track_boxes' do, through a slot of
// the handle's pinned ring, so the copy is enqueued like a kernel and the call returns without waiting for the device.
#include "grnet_impl.h"

namespace {

size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

std::string events_error(int window, double min_excursion) {
    if (window < 1 || window > kGaitMaxWindow) return "window " + std::to_string(window) + " outside [1, " + std::to_string(kGaitMaxWindow) + "]";
    if (!std::isfinite(min_excursion) || min_excursion < 0.) return "min_excursion must be finite and not negative";
    return "";
}

}  // namespace

extern "C" {

int grnet_gait_parameters(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                          const double* trans_dev, double fps, double sigma, int window, double min_excursion, double* per_frame_dev, int32_t* events_dev,
                          double* per_seq_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_gait_parameters: ";
    if (!joints3d_dev || !frame_offsets_host || !joints_host || !per_frame_dev || !events_dev || !per_seq_dev)
        return h->fail(GRNET_EINVAL, name + "null pointer (joints3d_dev, frame_offsets_host, joints_host, per_frame_dev, events_dev and per_seq_dev are all needed)");
    if (J < 1) return h->fail(GRNET_EINVAL, name + "J " + std::to_string(J) + " < 1");
    GaitTable tab{};
    for (int k = 0; k < 8; ++k) {
        if (joints_host[k] < 0 || joints_host[k] >= J)
            return h->fail(GRNET_EINVAL, name + "joint index " + std::to_string(joints_host[k]) + " (entry " + std::to_string(k) + ") outside [0, " + std::to_string(J) + ")");
        tab.j[k] = joints_host[k];
    }
    if (n_seq < 1 || n_seq > kTrackMaxSeqs) return h->fail(GRNET_EINVAL, name + "n_seq " + std::to_string(n_seq) + " outside [1, " + std::to_string(kTrackMaxSeqs) + "]");
    if (!std::isfinite(fps) || !(fps > 0.)) return h->fail(GRNET_EINVAL, name + "fps must be positive and finite");
    if (!std::isfinite(sigma) || sigma < 0. || sigma > kTrackMaxSigma) return h->fail(GRNET_EINVAL, name + "sigma must be 0 (no Gaussian) or within (0, " + std::to_string((int)kTrackMaxSigma) + "]");
    std::string why = events_error(window, min_excursion);
    if (why.empty()) why = track_offsets_error(frame_offsets_host, n_seq, (long long)J * 3);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    const int frames = frame_offsets_host[n_seq];
    const size_t mask_words = gait_mask_words(frames, n_seq);
    const size_t b_words = align256(4 * mask_words * sizeof(unsigned long long)), b_raw = sigma > 0. ? align256((size_t)frames * 4 * sizeof(double)) : 0;
    DeviceGuard guard(h->device);
    char* ws = nullptr;
    if (int rc = h->bbox_scratch(kTrackFront + b_words + b_raw, &ws)) return rc;
    unsigned long long* words = reinterpret_cast<unsigned long long*>(ws + kTrackFront);
    double* raw = b_raw ? reinterpret_cast<double*>(ws + kTrackFront + b_words) : nullptr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TrackTable t{};
    if (int rc = track_upload_table(h, name, frame_offsets_host, n_seq, sigma, ws, s, &t)) return rc;
    hipError_t e = launch_gait_frames(joints3d_dev, J, frames, tab, raw, per_frame_dev, s);
    if (e == hipSuccess && raw) e = launch_gait_smooth(t.off, n_seq, t.weights, t.radius, frames, raw, per_frame_dev, s);
    if (e == hipSuccess)
        e = launch_gait_sequences(t.off, n_seq, J, tab.j[0], joints3d_dev, trans_dev, fps, window, min_excursion, words, mask_words, per_frame_dev, events_dev,
                                  per_seq_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

int grnet_op_gait_events(grnet_t* h, const double* signals_dev, const int32_t* frame_offsets_host, int n_seq, int window, double min_excursion,
                         int32_t* events_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_op_gait_events: ";
    if (!signals_dev || !frame_offsets_host || !events_dev) return h->fail(GRNET_EINVAL, name + "null pointer");
    if (n_seq < 1 || n_seq > kTrackMaxSeqs) return h->fail(GRNET_EINVAL, name + "n_seq " + std::to_string(n_seq) + " outside [1, " + std::to_string(kTrackMaxSeqs) + "]");
    std::string why = events_error(window, min_excursion);
    if (why.empty()) why = track_offsets_error(frame_offsets_host, n_seq, 4);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    DeviceGuard guard(h->device);
    char* ws = nullptr;
    if (int rc = h->bbox_scratch(kTrackFront, &ws)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TrackTable t{};
    if (int rc = track_upload_table(h, name, frame_offsets_host, n_seq, 0., ws, s, &t)) return rc;
    const hipError_t e = launch_gait_events(t.off, n_seq, signals_dev, window, min_excursion, events_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
