// What the calls over sequences lying back to back share on the host (their argument rules: seq_args.h): the grower of the two scratch buffers the
// handle keeps for them, and seq_call's two halves -- the entry of the calls whose kernels read the sequences' offsets and the Gaussian's weights
// from a table on the device (grnet_track.cpp, grnet_gait.cpp, grnet_kinematics.cpp).  The table reaches the device through a slot of the handle's
// pinned ring, so the copy is enqueued like a kernel and the call returns without waiting for the device.
#include "grnet_impl.h"

namespace {

constexpr size_t kSeqSlotBytes = (size_t)kSegMaxSegments * sizeof(SegSegment);      // one slot of the pinned ring
static_assert(kSeqFront <= kSeqSlotBytes, "the weights and the offsets fit one slot of the pinned ring");

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

// A scratch buffer of the handle (bbox_ws, metric_ws), grown on demand and kept: a call of a size seen before allocates nothing.  Growing
// synchronises the device, so no call still in flight loses the buffer it reads.
int grnet::grow_scratch(void*& ws, size_t& have, size_t bytes, const char* what, char** out) {
    if (bytes > have) {
        if (ws) { (void)hipDeviceSynchronize(); (void)hipFree(ws); ws = nullptr; have = 0; }
        const size_t want = bytes + bytes / 4;
        if (hipMalloc(&ws, want) != hipSuccess) { ws = nullptr; return fail(GRNET_ENOMEM, std::string(what) + " (" + std::to_string(want >> 20) + " MiB)"); }
        have = want;
    }
    *out = static_cast<char*>(ws);
    return 0;
}

// seq_call, first half: what the call refuses about n_seq and the offsets.  One table holds at most kTrackMaxSeqs + 1 offsets.
int seq_call_check(grnet* h,const std::string& name, const int32_t* off, int n_seq, long long unit) {
    if (n_seq < 1 || n_seq > kTrackMaxSeqs) return h->fail(GRNET_EINVAL, name + "n_seq " + std::to_string(n_seq) + " outside [1, " + std::to_string(kTrackMaxSeqs) + "]");
    const std::string why = offsets_error(off, n_seq, "frame_offsets", 0, unit);
    return why.empty() ? 0 : h->fail(GRNET_EINVAL, name + why);
}

// seq_call, second half: the guard, the scratch, and the table -- weights and offsets -- into the first kSeqFront bytes of the scratch through the
// next slot of the pinned ring; the slot's event is recorded behind the copy, so the slot is written again only once the copy has read it
int seq_call_upload(grnet* h,const std::string& name, const int32_t* off, int n_seq, double sigma, size_t extra, hipStream_t s, SeqCall* c) {
    c->guard.emplace(h->device);
    char* ws = nullptr;
    if (int rc = h->bbox_scratch(kSeqFront + extra, &ws)) return rc;
    void* stage = nullptr;
    hipEvent_t staged = nullptr;
    if (int rc = h->seg_stage_slot(&stage, &staged)) return rc;
    c->radius = gauss_weights(sigma, static_cast<double*>(stage));
    memcpy(static_cast<char*>(stage) + kSeqOffsetsAt, off, (size_t)(n_seq + 1) * sizeof(int32_t));
    hipError_t e = hipMemcpyAsync(ws, stage, kSeqOffsetsAt + (size_t)(n_seq + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipEventRecord(staged, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    c->weights = reinterpret_cast<const double*>(ws);
    c->off = reinterpret_cast<const int*>(ws + kSeqOffsetsAt);
    c->behind = ws + kSeqFront;
    return 0;
}
