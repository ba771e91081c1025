// Per-frame boxes from 2D joints behind the C ABI (lib/utils/smooth_bbox.py, lib/dataset/inference.py:57-66; kernels: track_kernels.hip, arithmetic:
// track_boxes.h, rules: DESIGN 4.10): grnet_track_boxes and the hooks that run its median and its Gaussian alone.  None reads a weight or the arena.
// Their scratch and their table of offsets and weights are seq_call's (grnet_seq.cpp): the call returns without waiting for the device.
#include "grnet_impl.h"

namespace {

std::string filter_error(int kernel_size, double sigma, int pad) {
    if (kernel_size < 1 || kernel_size > kTrackMaxKernel || kernel_size % 2 == 0)
        return "kernel_size " + std::to_string(kernel_size) + " must be odd and within [1, " + std::to_string(kTrackMaxKernel) + "]";
    const std::string why = sigma_error(sigma, kTrackMaxSigma);
    if (!why.empty()) return why;
    if (pad != GRNET_TRACK_PAD_ZERO && pad != GRNET_TRACK_PAD_EDGE) return "unknown pad " + std::to_string(pad) + " (GRNET_TRACK_PAD_ZERO / _EDGE)";
    return "";
}

int op_filter(grnet_t* h, const std::string& name, const double* x_dev, const int32_t* offsets_host, int n_seq, int kernel_size, double sigma, int pad,
              double* out_dev, void* stream) {
    if (!x_dev || !offsets_host || !out_dev) return h->fail(GRNET_EINVAL, name + "null pointer");
    if (x_dev == out_dev) return h->fail(GRNET_EINVAL, name + "out_dev must not be x_dev");
    const std::string why = filter_error(kernel_size, sigma, pad);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = seq_call(h, name, offsets_host, n_seq, 1, sigma, s, &c, seq_no_extra)) return rc;
    const hipError_t e = launch_track_filter(c.off, n_seq, x_dev, c.weights, c.radius, kernel_size, pad, out_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

}  // namespace

extern "C" {

int grnet_track_boxes(grnet_t* h, const double* joints_dev, int K, const int32_t* frame_offsets_host, int n_seq, double vis_thresh, int kernel_size,
                      double sigma, int pad, double* boxes_dev, int32_t* status_dev, int32_t* range_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_track_boxes: ";
    if (K < 1 || K > kTrackMaxJoints) return h->fail(GRNET_EINVAL, name + "K " + std::to_string(K) + " outside [1, " + std::to_string(kTrackMaxJoints) + "]");
    if (!joints_dev || !frame_offsets_host || !boxes_dev || !status_dev || !range_dev)
        return h->fail(GRNET_EINVAL, name + "null pointer (joints_dev, frame_offsets_host, boxes_dev, status_dev and range_dev are all needed)");
    if (!std::isfinite(vis_thresh)) return h->fail(GRNET_EINVAL, name + "vis_thresh must be finite");
    const std::string why = filter_error(kernel_size, sigma, pad);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    size_t b_words = 0, b_params = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = seq_call(h, name, frame_offsets_host, n_seq, 3LL * K, sigma, s, &c, [&](int frames) {
            b_words = align256((size_t)((frames + 255) / 256) * 4 * sizeof(unsigned long long));
            b_params = align256((size_t)frames * 3 * sizeof(double));
            return b_words + b_params + align256((size_t)frames * 6 * sizeof(double));
        }))
        return rc;
    const int frames = frame_offsets_host[n_seq];
    unsigned long long* words = reinterpret_cast<unsigned long long*>(c.behind);
    double* params = reinterpret_cast<double*>(c.behind + b_words);
    double* work = reinterpret_cast<double*>(c.behind + b_words + b_params);
    hipError_t e = launch_track_frames(joints_dev, K, frames, vis_thresh, params, words, s);
    if (e == hipSuccess) e = launch_track_sequences(c.off, n_seq, c.weights, c.radius, kernel_size, pad, params, words, work, boxes_dev, status_dev, range_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

int grnet_op_median1d(grnet_t* h, const double* x_dev, const int32_t* offsets_host, int n_seq, int kernel_size, int pad, double* out_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    return op_filter(h, "grnet_op_median1d: ", x_dev, offsets_host, n_seq, kernel_size, 0., pad, out_dev, stream);
}

int grnet_op_gauss1d(grnet_t* h, const double* x_dev, const int32_t* offsets_host, int n_seq, double sigma, double* out_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    if (sigma == 0.) return h->fail(GRNET_EINVAL, "grnet_op_gauss1d: sigma must be within (0, " + std::to_string((int)kTrackMaxSigma) + "]");
    return op_filter(h, "grnet_op_gauss1d: ", x_dev, offsets_host, n_seq, 1, sigma, GRNET_TRACK_PAD_ZERO, out_dev, stream);
}

}  // extern "C"
