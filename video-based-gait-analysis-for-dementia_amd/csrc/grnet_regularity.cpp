// Gait regularity and symmetry behind the C ABI (kernels: gait_regularity_kernels.hip, arithmetic: gait_regularity.h, rules: DESIGN 4.15):
// grnet_gait_regularity and the hook that runs its validity, autocorrelation, peaks and rows alone.  Neither reads a weight or the arena.  Their
// scratch and their table of offsets and weights are seq_call's (grnet_seq.cpp): the call returns without waiting for the device.
#include "grnet_impl.h"
#include "gait_regularity.h"

namespace {

// What the sequence kernel keeps in the call's scratch where a sequence has more frames than its LDS arrays hold (else nothing): per channel the
// centred signal and the run numbers of every frame, and two sets of mask words (the validity and the counts before each word).
struct RegLong {
    size_t mask_words = 0, b_d = 0, b_key = 0, b_words = 0;
    size_t bytes() const { return b_d + b_key + b_words; }
    void size(const int32_t* off, int n_seq) {
        bool any = false;
        for (int q = 0; q < n_seq; ++q) any = any || off[q + 1] - off[q] > kRegLdsFrames;
        if (!any) return;
        const size_t frames = (size_t)off[n_seq];
        mask_words = gait_mask_words(off[n_seq], n_seq);
        b_d = align256(kRegChannels * frames * sizeof(double));
        b_key = align256(kRegChannels * frames * sizeof(int));
        b_words = gait_mask_bytes(kRegChannels * 2, mask_words);
    }
};

hipError_t sequences(const SeqCall& c, char* at, const RegLong& lg, int n_seq, int frames, const RegRule& rule, const double* rows, const int32_t* exclude, double* acf,
                     double* per_seq, hipStream_t s) {
    double* long_d = lg.bytes() ? reinterpret_cast<double*>(at) : nullptr;
    int* long_key = lg.bytes() ? reinterpret_cast<int*>(at + lg.b_d) : nullptr;
    unsigned long long* words = lg.bytes() ? reinterpret_cast<unsigned long long*>(at + lg.b_d + lg.b_key) : nullptr;
    return launch_reg_sequences(c.off, n_seq, rule, rows, exclude, frames, long_d, long_key, words, lg.mask_words, acf, per_seq, s);
}

}  // namespace

extern "C" {

int grnet_gait_regularity(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                          const double* trans_dev, const int32_t* exclude_dev, double fps, double sigma, int max_lag, int min_lag, double min_peak,
                          int min_pairs, double* per_frame_dev, double* acf_dev, double* per_seq_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_gait_regularity: ";
    if (!joints3d_dev || !frame_offsets_host || !joints_host || !per_frame_dev || !acf_dev || !per_seq_dev)
        return h->fail(GRNET_EINVAL, name + "null pointer (joints3d_dev, frame_offsets_host, joints_host, per_frame_dev, acf_dev and per_seq_dev are all needed)");
    GaitTable tab{};
    std::string why = joint_table_take(joints_host, 8, J, tab.j);
    const RegRule rule{fps, max_lag, min_lag, min_peak, min_pairs};
    if (why.empty()) why = rule_text(reg_rule_error(rule));      // gait_regularity.h's refusals, which the stand-alone checker runs too
    if (why.empty()) why = sigma_error(sigma, kTrackMaxSigma);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    RegLong lg;
    size_t b_raw = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = seq_call(h, name, frame_offsets_host, n_seq, std::max(3LL * J, (long long)kRegChannels), sigma, s, &c, [&](int frames) {
            lg.size(frame_offsets_host, n_seq);
            b_raw = raw_bytes(sigma, kRegChannels, frames);
            return b_raw + lg.bytes();
        }))
        return rc;
    const int frames = frame_offsets_host[n_seq];
    double* raw = b_raw ? reinterpret_cast<double*>(c.behind) : nullptr;
    hipError_t e = launch_reg_frames(joints3d_dev, J, frames, tab, trans_dev, raw, per_frame_dev, s);
    if (e == hipSuccess && raw) e = launch_seq_gauss_columns(c.off, n_seq, kRegChannels, c.weights, c.radius, frames, raw, per_frame_dev, kRegChannels, 0, s);
    if (e == hipSuccess) e = sequences(c, c.behind + b_raw, lg, n_seq, frames, rule, per_frame_dev, exclude_dev, acf_dev, per_seq_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

int grnet_op_gait_autocorr(grnet_t* h, const double* signals_dev, const int32_t* exclude_dev, const int32_t* frame_offsets_host, int n_seq, double fps,
                           int max_lag, int min_lag, double min_peak, int min_pairs, double* acf_dev, double* per_seq_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_op_gait_autocorr: ";
    if (!signals_dev || !frame_offsets_host || !acf_dev || !per_seq_dev) return h->fail(GRNET_EINVAL, name + "null pointer");
    const RegRule rule{fps, max_lag, min_lag, min_peak, min_pairs};
    const std::string why = rule_text(reg_rule_error(rule));
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    RegLong lg;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = seq_call(h, name, frame_offsets_host, n_seq, kRegChannels, 0., s, &c, [&](int) {
            lg.size(frame_offsets_host, n_seq);
            return lg.bytes();
        }))
        return rc;
    const hipError_t e = sequences(c, c.behind, lg, n_seq, frame_offsets_host[n_seq], rule, signals_dev, exclude_dev, acf_dev, per_seq_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
