// Footprints, centre of mass and margin of stability behind the C ABI (kernels: gait_balance_kernels.hip, arithmetic: gait_balance.h, rules: DESIGN
// 4.22): grnet_gait_balance, grnet_gait_balance_com (the same call on a centre of mass the caller brings) and the hook that runs rules 2 to 8
// alone.  None reads a weight or the arena.  Their scratch and their table of
// offsets are seq_call's (grnet_seq.cpp): the call returns without waiting for the device.  The segment table travels as a kernel argument.
#include "grnet_impl.h"
#include "gait_balance.h"

namespace {

// what a call keeps behind its table: the masks, the list of marks, the pairs' rows, and (the whole call alone) [c, rL, rR]
struct BalanceScratch {
    size_t mask_words = 0, b_words = 0, b_list = 0, b_pairs = 0, b_rel = 0;
    size_t plan(int frames, int n_seq, bool with_rel) {
        mask_words = gait_mask_words(frames, n_seq);
        b_words = gait_mask_bytes(kBalanceMaskSets, mask_words);
        b_list = align256((size_t)frames * sizeof(int));
        b_pairs = align256((size_t)frames * kBalancePairCols * sizeof(double));
        b_rel = with_rel ? align256((size_t)frames * kBalanceRelCols * sizeof(double)) : 0;
        return b_words + b_list + b_pairs + b_rel;
    }
    unsigned long long* words(char* behind) const { return reinterpret_cast<unsigned long long*>(behind); }
    int* list(char* behind) const { return reinterpret_cast<int*>(behind + b_words); }
    double* pairs(char* behind) const { return reinterpret_cast<double*>(behind + b_words + b_list); }
    double* rel(char* behind) const { return reinterpret_cast<double*>(behind + b_words + b_list + b_pairs); }
};

}  // namespace

extern "C" {

int grnet_gait_balance(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                       const int32_t* events_dev, const int32_t* segments_host, const double* seg_weights_host, int n_seg, double fps, double gravity,
                       int window, int settle, int max_step, int max_steps, double* per_frame_dev, double* steps_dev, double* per_seq_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_gait_balance: ";
    if (!joints3d_dev || !frame_offsets_host || !joints_host || !events_dev || !segments_host || !seg_weights_host || !per_frame_dev || !steps_dev || !per_seq_dev)
        return h->fail(GRNET_EINVAL, name + "null pointer (joints3d_dev, frame_offsets_host, joints_host, events_dev, segments_host, seg_weights_host, "
                                            "per_frame_dev, steps_dev and per_seq_dev are all needed)");
    GaitTable tab{};
    std::string why = joint_table_take(joints_host, 8, J, tab.j);
    const BalanceRule rule{fps, gravity, window, settle, max_step, max_steps};
    BalanceSegments seg{};
    if (why.empty()) why = rule_text(balance_rule_error(rule));      // gait_balance.h's refusals, which the stand-alone checker runs too
    if (why.empty()) why = rule_text(balance_segments_error(segments_host, seg_weights_host, n_seg, J, &seg));
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    BalanceScratch at;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = seq_call(h, name, frame_offsets_host, n_seq, std::max(3LL * J, (long long)kBalancePairCols), 0., s, &c,
                          [&](int frames) { return at.plan(frames, n_seq, true); }))
        return rc;
    const int frames = frame_offsets_host[n_seq];
    hipError_t e = launch_balance_frames(joints3d_dev, J, frames, tab, seg, at.rel(c.behind), s);
    if (e == hipSuccess)
        e = launch_balance_steps(c.off, n_seq, rule, at.rel(c.behind), events_dev, at.words(c.behind), at.mask_words, at.list(c.behind), at.pairs(c.behind), steps_dev,
                                 per_seq_dev, s);
    if (e == hipSuccess) e = launch_balance_path(c.off, n_seq, frames, at.rel(c.behind), at.words(c.behind), at.mask_words, at.pairs(c.behind), per_frame_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

int grnet_gait_balance_com(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                           const int32_t* events_dev, const double* com_dev, double fps, double gravity, int window, int settle, int max_step, int max_steps,
                           double* per_frame_dev, double* steps_dev, double* per_seq_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_gait_balance_com: ";
    if (!joints3d_dev || !frame_offsets_host || !joints_host || !events_dev || !com_dev || !per_frame_dev || !steps_dev || !per_seq_dev)
        return h->fail(GRNET_EINVAL, name + "null pointer (joints3d_dev, frame_offsets_host, joints_host, events_dev, com_dev, per_frame_dev, steps_dev and "
                                            "per_seq_dev are all needed)");
    GaitTable tab{};
    std::string why = joint_table_take(joints_host, 8, J, tab.j);
    const BalanceRule rule{fps, gravity, window, settle, max_step, max_steps};
    if (why.empty()) why = rule_text(balance_rule_error(rule));
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    BalanceScratch at;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = seq_call(h, name, frame_offsets_host, n_seq, std::max(3LL * J, (long long)kBalancePairCols), 0., s, &c,
                          [&](int frames) { return at.plan(frames, n_seq, true); }))
        return rc;
    const int frames = frame_offsets_host[n_seq];
    hipError_t e = launch_balance_com_frames(joints3d_dev, J, frames, tab, com_dev, at.rel(c.behind), s);      // the caller's c; the steps and the path as grnet_gait_balance
    if (e == hipSuccess)
        e = launch_balance_steps(c.off, n_seq, rule, at.rel(c.behind), events_dev, at.words(c.behind), at.mask_words, at.list(c.behind), at.pairs(c.behind), steps_dev,
                                 per_seq_dev, s);
    if (e == hipSuccess) e = launch_balance_path(c.off, n_seq, frames, at.rel(c.behind), at.words(c.behind), at.mask_words, at.pairs(c.behind), per_frame_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

int grnet_op_gait_balance_steps(grnet_t* h, const double* rel_dev, const int32_t* events_dev, const int32_t* frame_offsets_host, int n_seq, double fps,
                                double gravity, int window, int settle, int max_step, int max_steps, double* per_frame_dev, double* steps_dev,
                                double* per_seq_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_op_gait_balance_steps: ";
    if (!rel_dev || !events_dev || !frame_offsets_host || !per_frame_dev || !steps_dev || !per_seq_dev) return h->fail(GRNET_EINVAL, name + "null pointer");
    const BalanceRule rule{fps, gravity, window, settle, max_step, max_steps};
    const std::string why = rule_text(balance_rule_error(rule));
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    BalanceScratch at;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = seq_call(h, name, frame_offsets_host, n_seq, kBalancePairCols, 0., s, &c, [&](int frames) { return at.plan(frames, n_seq, false); })) return rc;
    const int frames = frame_offsets_host[n_seq];
    hipError_t e = launch_balance_steps(c.off, n_seq, rule, rel_dev, events_dev, at.words(c.behind), at.mask_words, at.list(c.behind), at.pairs(c.behind), steps_dev,
                                        per_seq_dev, s);
    if (e == hipSuccess) e = launch_balance_path(c.off, n_seq, frames, rel_dev, at.words(c.behind), at.mask_words, at.pairs(c.behind), per_frame_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
