// Harmonic ratios per stride behind the C ABI (kernels: gait_harmonics_kernels.hip and gait_regularity's frame kernel, arithmetic: gait_harmonics.h,
// rules: DESIGN 4.16): grnet_gait_harmonics and the hook that runs its strides, spectra and rows alone.  Neither reads a weight or the arena.  Their
// scratch and their table of offsets and weights are seq_call's (grnet_seq.cpp): the call returns without waiting for the device.
#include "grnet_impl.h"
#include "gait_harmonics.h"

namespace {

// What the sequence kernel keeps in the call's scratch: per channel a slot for every stride of an allowed length (har_slots), and, where a sequence
// has more frames than the LDS masks hold (else nothing), per channel the two heel-strike masks.
struct HarScratch {
    size_t mask_words = 0, b_slots = 0, b_words = 0;
    size_t bytes() const { return b_slots + b_words; }
    void size(const int32_t* off, int n_seq, int n_harmonics) {
        b_slots = align256(kRegChannels * har_slots(off[n_seq], n_seq) * (size_t)(n_harmonics + kHarSlotTail) * sizeof(double));
        bool any = false;
        for (int q = 0; q < n_seq; ++q) any = any || off[q + 1] - off[q] > 64 * kGaitLdsWords;
        if (!any) return;
        mask_words = gait_mask_words(off[n_seq], n_seq);
        b_words = gait_mask_bytes(kRegChannels * 2, mask_words);
    }
};

hipError_t sequences(const SeqCall& c, char* at, const HarScratch& sc, int n_seq, int frames, const HarRule& rule, const double* rows, const int32_t* events,
                     const int32_t* exclude, double* strides, double* spectrum, double* per_seq, hipStream_t s) {
    unsigned long long* words = sc.b_words ? reinterpret_cast<unsigned long long*>(at + sc.b_slots) : nullptr;
    return launch_har_sequences(c.off, n_seq, rule, rows, events, exclude, frames, words, sc.mask_words, reinterpret_cast<double*>(at), strides, spectrum, per_seq, s);
}

}  // namespace

extern "C" {

int grnet_gait_harmonics(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                         const double* trans_dev, const int32_t* events_dev, const int32_t* exclude_dev, double fps, double sigma, int n_harmonics,
                         int derivative, int min_stride, int max_stride, int max_strides, double* per_frame_dev, double* strides_dev,
                         double* spectrum_dev, double* per_seq_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_gait_harmonics: ";
    if (!joints3d_dev || !frame_offsets_host || !joints_host || !events_dev || !per_frame_dev || !strides_dev || !spectrum_dev || !per_seq_dev)
        return h->fail(GRNET_EINVAL, name + "null pointer (joints3d_dev, frame_offsets_host, joints_host, events_dev, per_frame_dev, strides_dev, spectrum_dev and "
                                            "per_seq_dev are all needed)");
    GaitTable tab{};
    std::string why = joint_table_take(joints_host, 8, J, tab.j);
    const HarRule rule{fps, n_harmonics, derivative, min_stride, max_stride, max_strides};
    if (why.empty()) why = rule_text(har_rule_error(rule));      // gait_harmonics.h's refusals, which the stand-alone checker runs too
    if (why.empty()) why = sigma_error(sigma, kTrackMaxSigma);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    HarScratch sc;
    size_t b_raw = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = seq_call(h, name, frame_offsets_host, n_seq, std::max(3LL * J, (long long)kRegChannels), sigma, s, &c, [&](int frames) {
            sc.size(frame_offsets_host, n_seq, n_harmonics);
            b_raw = raw_bytes(sigma, kRegChannels, frames);
            return b_raw + sc.bytes();
        }))
        return rc;
    const int frames = frame_offsets_host[n_seq];
    double* raw = b_raw ? reinterpret_cast<double*>(c.behind) : nullptr;
    hipError_t e = launch_reg_frames(joints3d_dev, J, frames, tab, trans_dev, raw, per_frame_dev, s);
    if (e == hipSuccess && raw) e = launch_seq_gauss_columns(c.off, n_seq, kRegChannels, c.weights, c.radius, frames, raw, per_frame_dev, kRegChannels, 0, s);
    if (e == hipSuccess) e = sequences(c, c.behind + b_raw, sc, n_seq, frames, rule, per_frame_dev, events_dev, exclude_dev, strides_dev, spectrum_dev, per_seq_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

int grnet_op_gait_stride_dft(grnet_t* h, const double* signals_dev, const int32_t* events_dev, const int32_t* exclude_dev,
                             const int32_t* frame_offsets_host, int n_seq, double fps, int n_harmonics, int derivative, int min_stride, int max_stride,
                             int max_strides, double* strides_dev, double* spectrum_dev, double* per_seq_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_op_gait_stride_dft: ";
    if (!signals_dev || !events_dev || !frame_offsets_host || !strides_dev || !spectrum_dev || !per_seq_dev) return h->fail(GRNET_EINVAL, name + "null pointer");
    const HarRule rule{fps, n_harmonics, derivative, min_stride, max_stride, max_strides};
    const std::string why = rule_text(har_rule_error(rule));
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    HarScratch sc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = seq_call(h, name, frame_offsets_host, n_seq, kRegChannels, 0., s, &c, [&](int) {
            sc.size(frame_offsets_host, n_seq, n_harmonics);
            return sc.bytes();
        }))
        return rc;
    const hipError_t e = sequences(c, c.behind, sc, n_seq, frame_offsets_host[n_seq], rule, signals_dev, events_dev, exclude_dev, strides_dev, spectrum_dev, per_seq_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
