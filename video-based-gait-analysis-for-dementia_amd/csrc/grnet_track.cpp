// Per-frame boxes from 2D joints behind the C ABI (lib/utils/smooth_bbox.py, lib/dataset/inference.py:57-66; kernels: track_kernels.hip, arithmetic:
// track_boxes.h, rules: DESIGN 4.10): grnet_track_boxes and the hooks that run its median and its Gaussian alone.  None reads a weight or the arena.
// Their scratch is the box calls' (bbox_scratch, grown on demand and kept); the sequences' offsets and the Gaussian's weights reach it through a
// slot of the handle's pinned ring, so the copy is enqueued like a kernel and the call returns without waiting for the device.
#include "grnet_impl.h"

// The table of a call -- the Gaussian's weights, then the sequences' offsets -- and the offsets' rules: declared in grnet_impl.h, shared with grnet_gait.cpp
std::string track_offsets_error(const int32_t* off, int n_seq, long long unit) {
    if (off[0] != 0) return "offsets[0] = " + std::to_string(off[0]) + ", not 0";
    for (int q = 0; q < n_seq; ++q)
        if (off[q + 1] <= off[q])
            return "sequence " + std::to_string(q) + " is empty or its offsets do not increase (" + std::to_string(off[q]) + ", " + std::to_string(off[q + 1]) + ")";
    if ((long long)off[n_seq] * unit > 0x7fffffffLL) return std::to_string((long long)off[n_seq] * unit) + " values in one call no longer fit 31 bits";
    return "";
}

namespace {

constexpr size_t kTrackTableBytes = (size_t)kSegMaxSegments * sizeof(SegSegment);      // one slot of the pinned ring
static_assert(kTrackFront <= kTrackTableBytes, "the weights and the offsets fit one slot of the pinned ring");

size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

std::string filter_error(int kernel_size, double sigma, int pad) {
    if (kernel_size < 1 || kernel_size > kTrackMaxKernel || kernel_size % 2 == 0)
        return "kernel_size " + std::to_string(kernel_size) + " must be odd and within [1, " + std::to_string(kTrackMaxKernel) + "]";
    if (!std::isfinite(sigma) || sigma < 0. || sigma > kTrackMaxSigma) return "sigma must be 0 (no Gaussian) or within (0, " + std::to_string((int)kTrackMaxSigma) + "]";
    if (pad != GRNET_TRACK_PAD_ZERO && pad != GRNET_TRACK_PAD_EDGE) return "unknown pad " + std::to_string(pad) + " (GRNET_TRACK_PAD_ZERO / _EDGE)";
    return "";
}

// scipy.ndimage's _gaussian_kernel1d: exp(-0.5 / sigma^2 * x^2) over x = -r .. r divided by the sum, r = int(4 sigma + 0.5); w[i] for x = -i and +i.
// The sum runs from the outside in (the small terms first).  Returns r, or -1 for sigma == 0 (no Gaussian).
int gauss_weights(double sigma, double* w) {
    if (sigma == 0.) return -1;
    const int r = (int)(4. * sigma + 0.5);
    const double c = -0.5 / (sigma * sigma);
    for (int i = 0; i <= r; ++i) w[i] = std::exp(c * (double)(i * i));
    double sum = 0.;
    for (int i = r; i >= 1; --i) sum += 2. * w[i];
    sum += w[0];
    for (int i = 0; i <= r; ++i) w[i] /= sum;
    return r;
}

}  // namespace

// The call's table -- weights and offsets -- into the first kTrackFront bytes of the scratch `ws`, through the pinned ring
int track_upload_table(grnet* h, const std::string& name, const int32_t* off, int n_seq, double sigma, char* ws, hipStream_t s, TrackTable* t) {
    void* stage = nullptr;
    hipEvent_t staged = nullptr;
    if (int rc = h->seg_stage_slot(&stage, &staged)) return rc;
    t->radius = gauss_weights(sigma, static_cast<double*>(stage));
    memcpy(static_cast<char*>(stage) + kTrackOffsetsAt, off, (size_t)(n_seq + 1) * sizeof(int32_t));
    hipError_t e = hipMemcpyAsync(ws, stage, kTrackOffsetsAt + (size_t)(n_seq + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipEventRecord(staged, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    t->off = reinterpret_cast<const int*>(ws + kTrackOffsetsAt);
    t->weights = reinterpret_cast<const double*>(ws);
    return 0;
}

namespace {

int op_filter(grnet_t* h, const std::string& name, const double* x_dev, const int32_t* offsets_host, int n_seq, int kernel_size, double sigma, int pad,
              double* out_dev, void* stream) {
    if (n_seq < 1 || n_seq > kTrackMaxSeqs) return h->fail(GRNET_EINVAL, name + "n_seq " + std::to_string(n_seq) + " outside [1, " + std::to_string(kTrackMaxSeqs) + "]");
    if (!x_dev || !offsets_host || !out_dev) return h->fail(GRNET_EINVAL, name + "null pointer");
    if (x_dev == out_dev) return h->fail(GRNET_EINVAL, name + "out_dev must not be x_dev");
    std::string why = filter_error(kernel_size, sigma, pad);
    if (why.empty()) why = track_offsets_error(offsets_host, n_seq, 1);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    DeviceGuard guard(h->device);
    char* ws = nullptr;
    if (int rc = h->bbox_scratch(kTrackFront, &ws)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TrackTable t{};
    if (int rc = track_upload_table(h, name, offsets_host, n_seq, sigma, ws, s, &t)) return rc;
    const hipError_t e = launch_track_filter(t.off, n_seq, x_dev, t.weights, t.radius, kernel_size, pad, out_dev, s);
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
    if (n_seq < 1 || n_seq > kTrackMaxSeqs) return h->fail(GRNET_EINVAL, name + "n_seq " + std::to_string(n_seq) + " outside [1, " + std::to_string(kTrackMaxSeqs) + "]");
    if (!joints_dev || !frame_offsets_host || !boxes_dev || !status_dev || !range_dev)
        return h->fail(GRNET_EINVAL, name + "null pointer (joints_dev, frame_offsets_host, boxes_dev, status_dev and range_dev are all needed)");
    if (!std::isfinite(vis_thresh)) return h->fail(GRNET_EINVAL, name + "vis_thresh must be finite");
    std::string why = filter_error(kernel_size, sigma, pad);
    if (why.empty()) why = track_offsets_error(frame_offsets_host, n_seq, (long long)K * 3);
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    const int frames = frame_offsets_host[n_seq];
    const size_t b_words = align256((size_t)((frames + 255) / 256) * 4 * sizeof(unsigned long long)), b_params = align256((size_t)frames * 3 * sizeof(double)),
                 b_work = align256((size_t)frames * 6 * sizeof(double));
    DeviceGuard guard(h->device);
    char* ws = nullptr;
    if (int rc = h->bbox_scratch(kTrackFront + b_words + b_params + b_work, &ws)) return rc;
    unsigned long long* words = reinterpret_cast<unsigned long long*>(ws + kTrackFront);
    double* params = reinterpret_cast<double*>(ws + kTrackFront + b_words);
    double* work = reinterpret_cast<double*>(ws + kTrackFront + b_words + b_params);
    hipStream_t s = static_cast<hipStream_t>(stream);
    TrackTable t{};
    if (int rc = track_upload_table(h, name, frame_offsets_host, n_seq, sigma, ws, s, &t)) return rc;
    hipError_t e = launch_track_frames(joints_dev, K, frames, vis_thresh, params, words, s);
    if (e == hipSuccess) e = launch_track_sequences(t.off, n_seq, t.weights, t.radius, kernel_size, pad, params, words, work, boxes_dev, status_dev, range_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, std::string("track_boxes: ") + hipGetErrorString(e));
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
