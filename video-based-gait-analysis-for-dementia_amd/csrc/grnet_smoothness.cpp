// Movement smoothness behind the C ABI (kernels: gait_smoothness_kernels.hip and gait_regularity's frame kernel, arithmetic: gait_smoothness.h,
// rules: DESIGN 4.24): grnet_gait_smoothness, the hook that runs its segments and rows alone, and the host-only slot count.  None reads a weight or
// the arena.  Their scratch and their table of offsets and weights are seq_call's (grnet_seq.cpp): the call returns without waiting for the device.
#include "grnet_impl.h"
#include "gait_smoothness.h"

namespace {

// What the three launches keep in the call's scratch: the twiddle table (2 nfft float64), every slot's sequence and every sequence's first slot
struct SmoScratch {
    size_t b_tw = 0, b_seq = 0, b_base = 0;
    int slots = 0;
    size_t bytes() const { return b_tw + b_seq + b_base; }
    void size(const int32_t* off, int n_seq, const SmoRule& r) {
        std::vector<long long> at((size_t)n_seq + 1);
        smo_slot_offsets(off, n_seq, r.segment, r.hop, at.data());
        slots = (int)at[n_seq];                                // at most the call's frames
        b_tw = align256(2 * (size_t)r.nfft * sizeof(double));
        b_seq = align256((size_t)slots * sizeof(int));
        b_base = align256((size_t)n_seq * sizeof(int));
    }
};

hipError_t sequences(const SeqCall& c, char* at, const SmoScratch& sc, int n_seq, const SmoRule& rule, const double* rows, const int32_t* exclude, double* per_seg,
                     double* per_seq, hipStream_t s) {
    const int form = GRNET_AB(SMO_TWIDDLES, 0);                // 0, a constant in the product build: the call's table through L1 and L2; 1, 2 (diagnostic builds): the forms DESIGN 4.24 measures against it
    return launch_smo_sequences(c.off, n_seq, sc.slots, rule, smo_cut_bin(rule), form < 0 || form > 2 ? 0 : form, rows, exclude, reinterpret_cast<double*>(at),
                                reinterpret_cast<int*>(at + sc.b_tw), reinterpret_cast<int*>(at + sc.b_tw + sc.b_seq), per_seg, per_seq, s);
}

}  // namespace

extern "C" {

int grnet_gait_smoothness(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                          const double* trans_dev, const int32_t* exclude_dev, double fps, double sigma, int derivative, int segment, int hop, int nfft,
                          double f_cut, double amplitude, int min_segments, double* per_frame_dev, double* per_segment_dev, double* per_seq_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_gait_smoothness: ";
    if (!joints3d_dev || !frame_offsets_host || !joints_host || !per_frame_dev || !per_seq_dev)
        return h->fail(GRNET_EINVAL, name + "null pointer (joints3d_dev, frame_offsets_host, joints_host, per_frame_dev and per_seq_dev are all needed)");
    GaitTable tab{};
    std::string why = joint_table_take(joints_host, 8, J, tab.j);
    const SmoRule rule{fps, derivative, segment, hop, nfft, f_cut, amplitude, min_segments};
    if (why.empty()) why = rule_text(smo_rule_error(rule));      // gait_smoothness.h's refusals, which the stand-alone checker runs too
    if (why.empty()) why = sigma_error(sigma, kTrackMaxSigma);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    if (int rc = seq_call_check(h, name, frame_offsets_host, n_seq, std::max(3LL * J, (long long)kRegChannels))) return rc;
    SmoScratch sc;
    if (ent_long_sequence(frame_offsets_host, n_seq) < 0) {      // else ent_seq_call refuses below, in its own sentence
        sc.size(frame_offsets_host, n_seq, rule);
        if (sc.slots > 0 && !per_segment_dev) return h->fail(GRNET_EINVAL, name + "null pointer (per_segment_dev is needed where a sequence holds a slot)");
    }
    size_t b_raw = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = ent_seq_call(h, name, frame_offsets_host, n_seq, std::max(3LL * J, (long long)kRegChannels), sigma, s, &c, [&](int frames) {
            b_raw = raw_bytes(sigma, kRegChannels, frames);
            return b_raw + sc.bytes();
        }))
        return rc;
    const int frames = frame_offsets_host[n_seq];
    double* raw = b_raw ? reinterpret_cast<double*>(c.behind) : nullptr;
    hipError_t e = launch_reg_frames(joints3d_dev, J, frames, tab, trans_dev, raw, per_frame_dev, s);
    if (e == hipSuccess && raw) e = launch_seq_gauss_columns(c.off, n_seq, kRegChannels, c.weights, c.radius, frames, raw, per_frame_dev, kRegChannels, 0, s);
    if (e == hipSuccess) e = sequences(c, c.behind + b_raw, sc, n_seq, rule, per_frame_dev, exclude_dev, per_segment_dev, per_seq_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

int grnet_op_gait_sparc(grnet_t* h, const double* signals_dev, const int32_t* exclude_dev, const int32_t* frame_offsets_host, int n_seq, double fps,
                        int derivative, int segment, int hop, int nfft, double f_cut, double amplitude, int min_segments, double* per_segment_dev,
                        double* per_seq_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_op_gait_sparc: ";
    if (!signals_dev || !frame_offsets_host || !per_seq_dev) return h->fail(GRNET_EINVAL, name + "null pointer");
    const SmoRule rule{fps, derivative, segment, hop, nfft, f_cut, amplitude, min_segments};
    const std::string why = rule_text(smo_rule_error(rule));
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    if (int rc = seq_call_check(h, name, frame_offsets_host, n_seq, kRegChannels)) return rc;
    SmoScratch sc;
    if (ent_long_sequence(frame_offsets_host, n_seq) < 0) {
        sc.size(frame_offsets_host, n_seq, rule);
        if (sc.slots > 0 && !per_segment_dev) return h->fail(GRNET_EINVAL, name + "null pointer (per_segment_dev is needed where a sequence holds a slot)");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = ent_seq_call(h, name, frame_offsets_host, n_seq, kRegChannels, 0., s, &c, [&](int) { return sc.bytes(); })) return rc;
    const hipError_t e = sequences(c, c.behind, sc, n_seq, rule, signals_dev, exclude_dev, per_segment_dev, per_seq_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

int grnet_gait_smoothness_slots(const int32_t* frame_offsets_host, int n_seq, int segment, int hop, int64_t* slots_host) {
    if (!frame_offsets_host || !slots_host || n_seq < 1 || frame_offsets_host[0] != 0) return GRNET_EINVAL;
    if (segment < kSpecMinSegment || segment > kSpecMaxSegment || (segment & 1) || hop < segment / 8 || hop > segment) return GRNET_EINVAL;
    for (int q = 0; q < n_seq; ++q)
        if (frame_offsets_host[q + 1] <= frame_offsets_host[q]) return GRNET_EINVAL;
    slots_host[0] = 0;
    for (int q = 0; q < n_seq; ++q) slots_host[q + 1] = slots_host[q] + spec_run_segments(frame_offsets_host[q + 1] - frame_offsets_host[q], segment, hop);
    return 0;
}

}  // extern "C"
