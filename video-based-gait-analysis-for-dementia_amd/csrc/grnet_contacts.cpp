// Foot contact phases and double support behind the C ABI (kernels: gait_contacts_kernels.hip, arithmetic: gait_contacts.h, rules: DESIGN 4.14):
// grnet_gait_contacts and the hook that runs its threshold, runs, phases and rows alone.  Neither reads a weight or the arena.  Their scratch and
// their table of offsets and weights are seq_call's (grnet_seq.cpp): the call returns without waiting for the device.
#include "grnet_impl.h"
#include "gait_contacts.h"

namespace {

// the masks, and behind them one float64 per word: the sums of the blocks of 64 intervals
size_t contact_mask_bytes(size_t mask_words) { return gait_mask_bytes(kContactMaskSets + 1, mask_words); }

}  // namespace

extern "C" {

int grnet_gait_contacts(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                        const int32_t* events_dev, double fps, double sigma, double fraction, double speed, int reach, int max_frames, int max_runs,
                        double* per_frame_dev, int32_t* phase_dev, double* runs_dev, double* per_seq_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_gait_contacts: ";
    if (!joints3d_dev || !frame_offsets_host || !joints_host || !events_dev || !per_frame_dev || !phase_dev || !runs_dev || !per_seq_dev)
        return h->fail(GRNET_EINVAL, name + "null pointer (joints3d_dev, frame_offsets_host, joints_host, events_dev, per_frame_dev, phase_dev, runs_dev and "
                                            "per_seq_dev are all needed)");
    GaitTable tab{};
    std::string why = joint_table_take(joints_host, 8, J, tab.j);
    const ContactRule rule{fps, fraction, speed, reach, max_frames, max_runs};
    if (why.empty()) why = rule_text(contact_rule_error(rule));      // gait_contacts.h's refusals, which the stand-alone checker runs too
    if (why.empty()) why = sigma_error(sigma, kTrackMaxSigma);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    size_t mask_words = 0, b_words = 0, b_raw = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = seq_call(h, name, frame_offsets_host, n_seq, std::max(3LL * J, (long long)kContactFrameCols), sigma, s, &c, [&](int frames) {
            mask_words = gait_mask_words(frames, n_seq);
            b_words = contact_mask_bytes(mask_words);
            b_raw = raw_bytes(sigma, 3, frames);
            return b_words + b_raw;
        }))
        return rc;
    const int frames = frame_offsets_host[n_seq];
    unsigned long long* words = reinterpret_cast<unsigned long long*>(c.behind);
    double* raw = b_raw ? reinterpret_cast<double*>(c.behind + b_words) : nullptr;
    hipError_t e = launch_contact_frames(c.off, n_seq, joints3d_dev, J, frames, tab, fps, raw, per_frame_dev, s);
    if (e == hipSuccess && raw) e = launch_seq_gauss_columns(c.off, n_seq, 3, c.weights, c.radius, frames, raw, per_frame_dev, kContactFrameCols, 1, s);
    if (e == hipSuccess)
        e = launch_contact_sequences(c.off, n_seq, rule, per_frame_dev, nullptr, raw != nullptr, events_dev, words, mask_words, phase_dev, runs_dev, per_seq_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

int grnet_op_gait_contact_runs(grnet_t* h, const double* speeds_dev, const int32_t* events_dev, const int32_t* frame_offsets_host, int n_seq, double fps,
                               double fraction, double speed, int reach, int max_frames, int max_runs, int32_t* phase_dev, double* runs_dev,
                               double* per_seq_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_op_gait_contact_runs: ";
    if (!speeds_dev || !events_dev || !frame_offsets_host || !phase_dev || !runs_dev || !per_seq_dev) return h->fail(GRNET_EINVAL, name + "null pointer");
    const ContactRule rule{fps, fraction, speed, reach, max_frames, max_runs};
    const std::string why = rule_text(contact_rule_error(rule));
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    size_t mask_words = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = seq_call(h, name, frame_offsets_host, n_seq, 1, 0., s, &c, [&](int frames) {
            mask_words = gait_mask_words(frames, n_seq);
            return contact_mask_bytes(mask_words);
        }))
        return rc;
    const hipError_t e = launch_contact_sequences(c.off, n_seq, rule, nullptr, speeds_dev, false, events_dev, reinterpret_cast<unsigned long long*>(c.behind),
                                                  mask_words, phase_dev, runs_dev, per_seq_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
