// Sample entropy at several scales behind the C ABI (kernels: gait_entropy_kernels.hip and gait_regularity's frame kernel, arithmetic:
// gait_entropy.h, rules: DESIGN 4.17): grnet_gait_entropy and the hook that runs its differences, spread and counts alone.  Neither reads a weight or
// the arena.  Their scratch and their table of offsets and weights are seq_call's (grnet_seq.cpp): the call returns without waiting for the device.
#include "grnet_impl.h"
#include "gait_entropy.h"

namespace {

// What the two sequence kernels keep in the call's scratch: per channel the differenced signal of every frame, and, where a sequence has more frames
// than the counting kernel's LDS array holds (else nothing), per channel and scale room for its coarse-grained signal.
struct EntScratch {
    size_t b_y = 0, b_z = 0;
    size_t bytes() const { return b_y + b_z; }
    void size(const int32_t* off, int n_seq, int scales) {
        const size_t frames = (size_t)off[n_seq];
        b_y = align256(kRegChannels * frames * sizeof(double));
        bool any = false;
        for (int q = 0; q < n_seq; ++q) any = any || off[q + 1] - off[q] > kRegLdsFrames;
        if (any) b_z = align256(kRegChannels * (size_t)scales * frames * sizeof(double));
    }
};

hipError_t sequences(const SeqCall& c, char* at, const EntScratch& sc, int n_seq, int frames, const EntRule& rule, const double* rows, const int32_t* exclude,
                     int64_t* counts, double* per_seq, hipStream_t s) {
    double* z_long = sc.b_z ? reinterpret_cast<double*>(at + sc.b_y) : nullptr;
    return launch_ent_sequences(c.off, n_seq, rule, rows, exclude, frames, reinterpret_cast<double*>(at), z_long, reinterpret_cast<long long*>(counts), per_seq, s);
}

}  // namespace

extern "C" {

int grnet_gait_entropy(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                       const double* trans_dev, const int32_t* exclude_dev, double sigma, int m, double fraction, int derivative, int scales,
                       double* per_frame_dev, int64_t* counts_dev, double* per_seq_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_gait_entropy: ";
    if (!joints3d_dev || !frame_offsets_host || !joints_host || !per_frame_dev || !counts_dev || !per_seq_dev)
        return h->fail(GRNET_EINVAL, name + "null pointer (joints3d_dev, frame_offsets_host, joints_host, per_frame_dev, counts_dev and per_seq_dev are all needed)");
    GaitTable tab{};
    std::string why = joint_table_take(joints_host, 8, J, tab.j);
    const EntRule rule{m, fraction, derivative, scales};
    if (why.empty()) why = rule_text(ent_rule_error(rule));      // gait_entropy.h's refusals, which the stand-alone checker runs too
    if (why.empty()) why = sigma_error(sigma, kTrackMaxSigma);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    EntScratch sc;
    size_t b_raw = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = ent_seq_call(h, name, frame_offsets_host, n_seq, std::max(3LL * J, (long long)kRegChannels), sigma, s, &c, [&](int frames) {
            sc.size(frame_offsets_host, n_seq, scales);
            b_raw = raw_bytes(sigma, kRegChannels, frames);
            return b_raw + sc.bytes();
        }))
        return rc;
    const int frames = frame_offsets_host[n_seq];
    double* raw = b_raw ? reinterpret_cast<double*>(c.behind) : nullptr;
    hipError_t e = launch_reg_frames(joints3d_dev, J, frames, tab, trans_dev, raw, per_frame_dev, s);
    if (e == hipSuccess && raw) e = launch_seq_gauss_columns(c.off, n_seq, kRegChannels, c.weights, c.radius, frames, raw, per_frame_dev, kRegChannels, 0, s);
    if (e == hipSuccess) e = sequences(c, c.behind + b_raw, sc, n_seq, frames, rule, per_frame_dev, exclude_dev, counts_dev, per_seq_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

int grnet_op_gait_sampen(grnet_t* h, const double* signals_dev, const int32_t* exclude_dev, const int32_t* frame_offsets_host, int n_seq, int m, double fraction,
                         int derivative, int scales, int64_t* counts_dev, double* per_seq_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_op_gait_sampen: ";
    if (!signals_dev || !frame_offsets_host || !counts_dev || !per_seq_dev) return h->fail(GRNET_EINVAL, name + "null pointer");
    const EntRule rule{m, fraction, derivative, scales};
    const std::string why = rule_text(ent_rule_error(rule));
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    EntScratch sc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = ent_seq_call(h, name, frame_offsets_host, n_seq, kRegChannels, 0., s, &c, [&](int) {
            sc.size(frame_offsets_host, n_seq, scales);
            return sc.bytes();
        }))
        return rc;
    const hipError_t e = sequences(c, c.behind, sc, n_seq, frame_offsets_host[n_seq], rule, signals_dev, exclude_dev, counts_dev, per_seq_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
