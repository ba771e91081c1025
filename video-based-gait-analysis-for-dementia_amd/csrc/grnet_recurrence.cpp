// Recurrence quantification behind the C ABI (kernels: gait_recurrence_kernels.hip, gait_entropy's spread kernel and gait_regularity's frame kernel,
// arithmetic: gait_recurrence.h, rules: DESIGN 4.20): grnet_gait_recurrence and the hook that runs its differences, spread, pairs and rows alone.
// Neither reads a weight or the arena.  Their scratch and their table of offsets and weights are seq_call's (grnet_seq.cpp), behind grnet_impl.h's
// ent_seq_call with its refusal of a sequence too long: the call returns without waiting for the device.
#include "grnet_impl.h"
#include "gait_recurrence.h"

namespace {

// What the three sequence kernels keep in the call's scratch: per channel the differenced signal of every frame; n, mu, SD and r of every (sequence,
// channel); and the partial of every workgroup of the pairs kernel -- kRecPartCols int64 for each channel of each part, the parts counted sequence by
// sequence (rec_parts of each), NOT n_seq times kRecMaxParts: 8191 short sequences beside one long one have 8207 parts, 68 MB, not 1.1 GB.  The worst
// case is 8320 bytes times the sum of the parts, which is at most frames / 512 + n_seq.
struct RecScratch {
    size_t b_y = 0, b_spread = 0, b_parts = 0;
    int max_parts = 1;
    size_t bytes() const { return b_y + b_spread + b_parts; }
    void size(const int32_t* off, int n_seq, const RecRule& rule) {
        b_y = align256(kRegChannels * (size_t)off[n_seq] * sizeof(double));
        b_spread = align256((size_t)n_seq * kRegChannels * kEntSeqCols * sizeof(double));
        size_t parts = 0;
        for (int q = 0; q < n_seq; ++q) {
            const int p = rec_parts(rec_points(off[q + 1] - off[q], rule));
            parts += (size_t)p;
            max_parts = std::max(max_parts, p);
        }
        b_parts = align256(parts * kRegChannels * kRecPartCols * sizeof(long long));
    }
};

hipError_t sequences(const SeqCall& c, char* at, const RecScratch& sc, int n_seq, int frames, const RecRule& rule, const double* rows, const int32_t* exclude,
                     double* per_seq, int64_t* hist, int64_t* counts, hipStream_t s) {
    return launch_rec_sequences(c.off, n_seq, sc.max_parts, rule, rows, exclude, frames, reinterpret_cast<double*>(at), reinterpret_cast<double*>(at + sc.b_y),
                                reinterpret_cast<long long*>(at + sc.b_y + sc.b_spread), per_seq, reinterpret_cast<long long*>(hist),
                                reinterpret_cast<long long*>(counts), s);
}

}  // namespace

extern "C" {

int grnet_gait_recurrence(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                          const double* trans_dev, const int32_t* exclude_dev, double sigma, int derivative, int dim, int lag, int theiler, double radius,
                          double* per_frame_dev, double* per_seq_dev, int64_t* hist_dev, int64_t* counts_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_gait_recurrence: ";
    if (!joints3d_dev || !frame_offsets_host || !joints_host || !per_frame_dev || !per_seq_dev || !hist_dev || !counts_dev)
        return h->fail(GRNET_EINVAL, name + "null pointer (joints3d_dev, frame_offsets_host, joints_host, per_frame_dev, per_seq_dev, hist_dev and counts_dev are all needed)");
    GaitTable tab{};
    std::string why = joint_table_take(joints_host, 8, J, tab.j);
    const RecRule rule{derivative, dim, lag, theiler, radius};
    if (why.empty()) why = rule_text(rec_rule_error(rule));      // gait_recurrence.h's refusals, which the stand-alone checker runs too
    if (why.empty()) why = sigma_error(sigma, kTrackMaxSigma);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    RecScratch sc;
    size_t b_raw = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = ent_seq_call(h, name, frame_offsets_host, n_seq, std::max(3LL * J, (long long)kRegChannels), sigma, s, &c, [&](int frames) {
            sc.size(frame_offsets_host, n_seq, rule);
            b_raw = raw_bytes(sigma, kRegChannels, frames);
            return b_raw + sc.bytes();
        }))
        return rc;
    const int frames = frame_offsets_host[n_seq];
    double* raw = b_raw ? reinterpret_cast<double*>(c.behind) : nullptr;
    hipError_t e = launch_reg_frames(joints3d_dev, J, frames, tab, trans_dev, raw, per_frame_dev, s);
    if (e == hipSuccess && raw) e = launch_seq_gauss_columns(c.off, n_seq, kRegChannels, c.weights, c.radius, frames, raw, per_frame_dev, kRegChannels, 0, s);
    if (e == hipSuccess) e = sequences(c, c.behind + b_raw, sc, n_seq, frames, rule, per_frame_dev, exclude_dev, per_seq_dev, hist_dev, counts_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

int grnet_op_gait_recurrence_counts(grnet_t* h, const double* signals_dev, const int32_t* exclude_dev, const int32_t* frame_offsets_host, int n_seq,
                                    int derivative, int dim, int lag, int theiler, double radius, double* per_seq_dev, int64_t* hist_dev, int64_t* counts_dev,
                                    void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_op_gait_recurrence_counts: ";
    if (!signals_dev || !frame_offsets_host || !per_seq_dev || !hist_dev || !counts_dev) return h->fail(GRNET_EINVAL, name + "null pointer");
    const RecRule rule{derivative, dim, lag, theiler, radius};
    const std::string why = rule_text(rec_rule_error(rule));
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    RecScratch sc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = ent_seq_call(h, name, frame_offsets_host, n_seq, kRegChannels, 0., s, &c, [&](int) {
            sc.size(frame_offsets_host, n_seq, rule);
            return sc.bytes();
        }))
        return rc;
    const hipError_t e = sequences(c, c.behind, sc, n_seq, frame_offsets_host[n_seq], rule, signals_dev, exclude_dev, per_seq_dev, hist_dev, counts_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
