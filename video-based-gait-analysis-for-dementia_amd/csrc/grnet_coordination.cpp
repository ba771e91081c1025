// Arm swing and inter-limb coordination behind the C ABI (kernels: gait_coordination_kernels.hip, arithmetic: gait_coordination.h, rules: DESIGN
// 4.21): grnet_gait_coordination and the hook that runs its segments, densities and rows alone.  Neither reads a weight or the arena.  Their scratch
// and their table of offsets and weights are seq_call's (grnet_seq.cpp): the call returns without waiting for the device.
#include "grnet_impl.h"
#include "gait_coordination.h"

namespace {

// What the density kernel keeps in the call's scratch, per workgroup of a sequence -- spec_bin_blocks of them -- and frame: the four differenced
// columns where a sequence has more frames than the kernel's LDS array holds, the segment starts and their four means each where one can hold more
// segments than its LDS lists do; else nothing.
struct CoordScratch {
    size_t b_y = 0, b_start = 0, b_mu = 0;
    size_t bytes() const { return b_y + b_start + b_mu; }
    void size(const int32_t* off, int n_seq, const SpecRule& r) {
        const size_t spans = (size_t)spec_bin_blocks(r.nfft) * (size_t)off[n_seq];
        bool long_y = false, long_seg = false;
        for (int q = 0; q < n_seq; ++q) {
            const int T = off[q + 1] - off[q];
            long_y = long_y || T > kCoordLdsFrames;
            long_seg = long_seg || spec_run_segments(T, r.segment, r.hop) > kCoordLdsSegments;
        }
        if (long_y) b_y = align256(spans * kCoordChannels * sizeof(double));
        if (long_seg) {
            b_start = align256(spans * sizeof(int));
            b_mu = align256(spans * kCoordChannels * sizeof(double));
        }
    }
};

hipError_t sequences(const SeqCall& c, char* at, const CoordScratch& sc, int n_seq, int frames, const SpecRule& rule, const double* rows, const int32_t* exclude, double* au,
                     double* cr, double* limbs, double* pairs, hipStream_t s) {
    double* y_long = sc.b_y ? reinterpret_cast<double*>(at) : nullptr;
    int* start_long = sc.b_start ? reinterpret_cast<int*>(at + sc.b_y) : nullptr;
    double* mu_long = sc.b_mu ? reinterpret_cast<double*>(at + sc.b_y + sc.b_start) : nullptr;
    return launch_coord_sequences(c.off, n_seq, rule, rows, exclude, frames, y_long, start_long, mu_long, au, cr, limbs, pairs, s);
}

}  // namespace

extern "C" {

int grnet_gait_coordination(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                            const int32_t* exclude_dev, double fps, double sigma, int derivative, int segment, int hop, int nfft, double f_lo, double f_hi,
                            int min_segments, double* per_frame_dev, double* auto_dev, double* cross_dev, double* limbs_dev, double* pairs_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_gait_coordination: ";
    if (!joints3d_dev || !frame_offsets_host || !joints_host || !per_frame_dev || !auto_dev || !cross_dev || !limbs_dev || !pairs_dev)
        return h->fail(GRNET_EINVAL, name + "null pointer (joints3d_dev, frame_offsets_host, joints_host, per_frame_dev, auto_dev, cross_dev, limbs_dev and pairs_dev are all needed)");
    KinTable tab{};
    std::string why = joint_table_take(joints_host, 16, J, tab.j);
    const SpecRule rule{fps, derivative, segment, hop, nfft, f_lo, f_hi, min_segments};
    if (why.empty()) why = rule_text(coord_rule_error(rule));    // gait_coordination.h's refusals, which the stand-alone checker runs too
    if (why.empty()) why = sigma_error(sigma, kTrackMaxSigma);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    CoordScratch sc;
    size_t b_raw = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = ent_seq_call(h, name, frame_offsets_host, n_seq, std::max(3LL * J, (long long)kCoordChannels), sigma, s, &c, [&](int frames) {
            sc.size(frame_offsets_host, n_seq, rule);
            b_raw = raw_bytes(sigma, kCoordChannels, frames);
            return b_raw + sc.bytes();
        }))
        return rc;
    const int frames = frame_offsets_host[n_seq];
    double* raw = b_raw ? reinterpret_cast<double*>(c.behind) : nullptr;
    hipError_t e = launch_coord_frames(joints3d_dev, J, frames, tab, raw, per_frame_dev, s);
    if (e == hipSuccess && raw) e = launch_seq_gauss_columns(c.off, n_seq, kCoordChannels, c.weights, c.radius, frames, raw, per_frame_dev, kCoordChannels, 0, s);
    if (e == hipSuccess) e = sequences(c, c.behind + b_raw, sc, n_seq, frames, rule, per_frame_dev, exclude_dev, auto_dev, cross_dev, limbs_dev, pairs_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

int grnet_op_gait_cross_welch(grnet_t* h, const double* signals_dev, const int32_t* exclude_dev, const int32_t* frame_offsets_host, int n_seq, double fps,
                              int derivative, int segment, int hop, int nfft, double f_lo, double f_hi, int min_segments, double* auto_dev, double* cross_dev,
                              double* limbs_dev, double* pairs_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_op_gait_cross_welch: ";
    if (!signals_dev || !frame_offsets_host || !auto_dev || !cross_dev || !limbs_dev || !pairs_dev) return h->fail(GRNET_EINVAL, name + "null pointer");
    const SpecRule rule{fps, derivative, segment, hop, nfft, f_lo, f_hi, min_segments};
    const std::string why = rule_text(coord_rule_error(rule));
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    CoordScratch sc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = ent_seq_call(h, name, frame_offsets_host, n_seq, kCoordChannels, 0., s, &c, [&](int) {
            sc.size(frame_offsets_host, n_seq, rule);
            return sc.bytes();
        }))
        return rc;
    const hipError_t e = sequences(c, c.behind, sc, n_seq, frame_offsets_host[n_seq], rule, signals_dev, exclude_dev, auto_dev, cross_dev, limbs_dev, pairs_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
