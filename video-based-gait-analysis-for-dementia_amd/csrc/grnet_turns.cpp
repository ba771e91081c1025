// Turns and straight-walking gait parameters behind the C ABI (kernels: gait_turns_kernels.hip, arithmetic: gait_turns.h, rules: DESIGN 4.13):
// grnet_gait_turns and the hook that runs its runs, phases and rows alone.  Neither reads a weight or the arena.  Their scratch and their table of
// offsets and weights are seq_call's (grnet_seq.cpp): the call returns without waiting for the device.
#include "grnet_impl.h"
#include "gait_turns.h"

namespace {

size_t turn_mask_bytes(size_t mask_words) { return gait_mask_bytes(kTurnMaskSets, mask_words); }

}  // namespace

extern "C" {

int grnet_gait_turns(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                     const int32_t* events_dev, const double* gait_rows_dev, double fps, double sigma, double edge_rate, double peak_rate, double min_angle,
                     int min_frames, int max_frames, int max_turns, double* per_frame_dev, int32_t* phase_dev, double* turns_dev, double* per_seq_dev,
                     void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_gait_turns: ";
    if (!joints3d_dev || !frame_offsets_host || !joints_host || !events_dev || !gait_rows_dev || !per_frame_dev || !phase_dev || !turns_dev || !per_seq_dev)
        return h->fail(GRNET_EINVAL, name + "null pointer (joints3d_dev, frame_offsets_host, joints_host, events_dev, gait_rows_dev, per_frame_dev, phase_dev, "
                                            "turns_dev and per_seq_dev are all needed)");
    GaitTable tab{};
    std::string why = joint_table_take(joints_host, 8, J, tab.j);
    const TurnRule rule{fps, edge_rate, peak_rate, min_angle, min_frames, max_frames, max_turns};
    if (why.empty()) why = rule_text(turn_rule_error(rule));      // gait_turns.h's refusals, which the stand-alone checker runs too
    if (why.empty()) why = sigma_error(sigma, kTrackMaxSigma);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    size_t mask_words = 0, b_words = 0, b_raw = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = seq_call(h, name, frame_offsets_host, n_seq, std::max(3LL * J, 7LL), sigma, s, &c, [&](int frames) {      // 7 gait columns a frame
            mask_words = gait_mask_words(frames, n_seq);
            b_words = turn_mask_bytes(mask_words);
            b_raw = raw_bytes(sigma, 1, frames);
            return b_words + b_raw;
        }))
        return rc;
    unsigned long long* words = reinterpret_cast<unsigned long long*>(c.behind);
    double* raw = b_raw ? reinterpret_cast<double*>(c.behind + b_words) : nullptr;
    hipError_t e = launch_turn_rates(c.off, n_seq, c.weights, raw ? c.radius : -1, J, tab, joints3d_dev, fps, raw, per_frame_dev, s);
    if (e == hipSuccess)
        e = launch_turn_sequences(c.off, n_seq, rule, per_frame_dev, events_dev, gait_rows_dev, words, mask_words, phase_dev, turns_dev, per_seq_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

int grnet_op_gait_turn_runs(grnet_t* h, const double* rates_dev, const int32_t* events_dev, const double* gait_rows_dev, const int32_t* frame_offsets_host,
                            int n_seq, double fps, double edge_rate, double peak_rate, double min_angle, int min_frames, int max_frames, int max_turns,
                            int32_t* phase_dev, double* turns_dev, double* per_seq_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_op_gait_turn_runs: ";
    if (!rates_dev || !events_dev || !gait_rows_dev || !frame_offsets_host || !phase_dev || !turns_dev || !per_seq_dev) return h->fail(GRNET_EINVAL, name + "null pointer");
    const TurnRule rule{fps, edge_rate, peak_rate, min_angle, min_frames, max_frames, max_turns};
    const std::string why = rule_text(turn_rule_error(rule));
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    size_t mask_words = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = seq_call(h, name, frame_offsets_host, n_seq, 7, 0., s, &c, [&](int frames) {
            mask_words = gait_mask_words(frames, n_seq);
            return turn_mask_bytes(mask_words);
        }))
        return rc;
    const hipError_t e = launch_turn_sequences(c.off, n_seq, rule, rates_dev, events_dev, gait_rows_dev, reinterpret_cast<unsigned long long*>(c.behind), mask_words,
                                               phase_dev, turns_dev, per_seq_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
