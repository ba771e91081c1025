// Local dynamic stability behind the C ABI (kernels: gait_stability_kernels.hip and gait_regularity's frame kernel, arithmetic: gait_stability.h,
// rules: DESIGN 4.18): grnet_gait_stability and the hook that runs its differences, neighbour search and divergence walk alone.  Neither reads a
// weight or the arena.  Their scratch and their table of offsets and weights are seq_call's (grnet_seq.cpp), behind grnet_impl.h's ent_seq_call with
// its refusal of a sequence too long: the call returns without waiting for the device.
#include "grnet_impl.h"
#include "gait_stability.h"

namespace {

// What the curve kernel keeps in the call's scratch: where a sequence has more frames than its LDS arrays hold (else nothing), per channel the
// differenced signal of every frame.
struct StabScratch {
    size_t b_y = 0;
    int longest = 0;
    size_t bytes() const { return b_y; }
    void size(const int32_t* off, int n_seq) {
        for (int q = 0; q < n_seq; ++q) longest = std::max(longest, off[q + 1] - off[q]);
        if (longest > kRegLdsFrames) b_y = align256(kRegChannels * (size_t)off[n_seq] * sizeof(double));
    }
};

hipError_t sequences(const SeqCall& c, char* at, const StabScratch& sc, int n_seq, int frames, const StabRule& rule, const double* rows, const int32_t* exclude,
                     int32_t* nn, int64_t* pairs, double* mant, hipStream_t s) {
    double* y_long = sc.b_y ? reinterpret_cast<double*>(at) : nullptr;
    return launch_stab_sequences(c.off, n_seq, sc.longest, rule, rows, exclude, frames, nn, y_long, reinterpret_cast<long long*>(pairs), mant, s);
}

}  // namespace

extern "C" {

int grnet_gait_stability(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                         const double* trans_dev, const int32_t* exclude_dev, double sigma, int derivative, int dim, int lag, int theiler, int horizon,
                         double* per_frame_dev, int32_t* nn_dev, int64_t* pairs_dev, double* mant_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_gait_stability: ";
    if (!joints3d_dev || !frame_offsets_host || !joints_host || !per_frame_dev || !nn_dev || !pairs_dev || !mant_dev)
        return h->fail(GRNET_EINVAL, name + "null pointer (joints3d_dev, frame_offsets_host, joints_host, per_frame_dev, nn_dev, pairs_dev and mant_dev are all needed)");
    GaitTable tab{};
    std::string why = joint_table_take(joints_host, 8, J, tab.j);
    const StabRule rule{derivative, dim, lag, theiler, horizon};
    if (why.empty()) why = rule_text(stab_rule_error(rule));     // gait_stability.h's refusals, which the stand-alone checker runs too
    if (why.empty()) why = sigma_error(sigma, kTrackMaxSigma);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    StabScratch sc;
    size_t b_raw = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = ent_seq_call(h, name, frame_offsets_host, n_seq, std::max(3LL * J, (long long)kRegChannels), sigma, s, &c, [&](int frames) {
            sc.size(frame_offsets_host, n_seq);
            b_raw = raw_bytes(sigma, kRegChannels, frames);
            return b_raw + sc.bytes();
        }))
        return rc;
    const int frames = frame_offsets_host[n_seq];
    double* raw = b_raw ? reinterpret_cast<double*>(c.behind) : nullptr;
    hipError_t e = launch_reg_frames(joints3d_dev, J, frames, tab, trans_dev, raw, per_frame_dev, s);
    if (e == hipSuccess && raw) e = launch_seq_gauss_columns(c.off, n_seq, kRegChannels, c.weights, c.radius, frames, raw, per_frame_dev, kRegChannels, 0, s);
    if (e == hipSuccess) e = sequences(c, c.behind + b_raw, sc, n_seq, frames, rule, per_frame_dev, exclude_dev, nn_dev, pairs_dev, mant_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

int grnet_op_gait_divergence(grnet_t* h, const double* signals_dev, const int32_t* exclude_dev, const int32_t* frame_offsets_host, int n_seq, int derivative,
                             int dim, int lag, int theiler, int horizon, int32_t* nn_dev, int64_t* pairs_dev, double* mant_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_op_gait_divergence: ";
    if (!signals_dev || !frame_offsets_host || !nn_dev || !pairs_dev || !mant_dev) return h->fail(GRNET_EINVAL, name + "null pointer");
    const StabRule rule{derivative, dim, lag, theiler, horizon};
    const std::string why = rule_text(stab_rule_error(rule));
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    StabScratch sc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = ent_seq_call(h, name, frame_offsets_host, n_seq, kRegChannels, 0., s, &c, [&](int) {
            sc.size(frame_offsets_host, n_seq);
            return sc.bytes();
        }))
        return rc;
    const hipError_t e = sequences(c, c.behind, sc, n_seq, frame_offsets_host[n_seq], rule, signals_dev, exclude_dev, nn_dev, pairs_dev, mant_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
