// Gait events and parameters from the 3D joints behind the C ABI (kernels: gait_kernels.hip, arithmetic: gait_events.h, rules: DESIGN 4.11):
// grnet_gait_parameters and the hook that runs its events rule alone.  Neither reads a weight or the arena.  Their scratch and their table of
// offsets and weights are seq_call's (grnet_seq.cpp): the call returns without waiting for the device.
#include "grnet_impl.h"

namespace {

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
    GaitTable tab{};
    std::string why = joint_table_take(joints_host, 8, J, tab.j);
    if (why.empty() && (!std::isfinite(fps) || !(fps > 0.))) why = "fps must be positive and finite";
    if (why.empty()) why = sigma_error(sigma, kTrackMaxSigma);
    if (why.empty()) why = events_error(window, min_excursion);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    size_t mask_words = 0, b_words = 0, b_raw = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = seq_call(h, name, frame_offsets_host, n_seq, 3LL * J, sigma, s, &c, [&](int frames) {
            mask_words = gait_mask_words(frames, n_seq);
            b_words = gait_mask_bytes(4, mask_words);
            b_raw = raw_bytes(sigma, 4, frames);
            return b_words + b_raw;
        }))
        return rc;
    const int frames = frame_offsets_host[n_seq];
    unsigned long long* words = reinterpret_cast<unsigned long long*>(c.behind);
    double* raw = b_raw ? reinterpret_cast<double*>(c.behind + b_words) : nullptr;
    hipError_t e = launch_gait_frames(joints3d_dev, J, frames, tab, raw, per_frame_dev, s);
    if (e == hipSuccess && raw) e = launch_seq_gauss_columns(c.off, n_seq, 4, c.weights, c.radius, frames, raw, per_frame_dev, 7, 0, s);
    if (e == hipSuccess)
        e = launch_gait_sequences(c.off, n_seq, J, tab.j[0], joints3d_dev, trans_dev, fps, window, min_excursion, words, mask_words, per_frame_dev, events_dev,
                                  per_seq_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

int grnet_op_gait_events(grnet_t* h, const double* signals_dev, const int32_t* frame_offsets_host, int n_seq, int window, double min_excursion,
                         int32_t* events_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_op_gait_events: ";
    if (!signals_dev || !frame_offsets_host || !events_dev) return h->fail(GRNET_EINVAL, name + "null pointer");
    const std::string why = events_error(window, min_excursion);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = seq_call(h, name, frame_offsets_host, n_seq, 4, 0., s, &c, seq_no_extra)) return rc;
    const hipError_t e = launch_gait_events(c.off, n_seq, signals_dev, window, min_excursion, events_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
