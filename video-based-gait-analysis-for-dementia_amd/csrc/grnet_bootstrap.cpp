// The gait call's per-step and per-stride tables and bootstrap intervals of a per-step table behind the C ABI (kernels: gait_bootstrap_kernels.hip,
// arithmetic and generator: gait_bootstrap.h, rules: DESIGN 4.23): grnet_gait_step_tables and grnet_bootstrap_table.  Neither reads a weight or the
// arena, and neither waits for the device.  The tables' scratch and offsets are seq_call's (grnet_seq.cpp).  The bootstrap has no frames and so no
// offsets: its rule travels as a kernel argument, its samples and replicates lie in LDS and registers, and it needs no scratch at all.
#include "grnet_impl.h"
#include "gait_bootstrap.h"

extern "C" {

int grnet_gait_step_tables(grnet_t* h, const int32_t* events_dev, const double* per_frame_dev, const int32_t* frame_offsets_host, int n_seq, double fps,
                           int max_rows, const int32_t* phase_dev, int straight_only, double* steps_dev, double* strides_dev, int32_t* counts_dev, void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_gait_step_tables: ";
    if (!events_dev || !per_frame_dev || !frame_offsets_host || !steps_dev || !strides_dev || !counts_dev)
        return h->fail(GRNET_EINVAL, name + "null pointer (events_dev, per_frame_dev, frame_offsets_host, steps_dev, strides_dev and counts_dev are all needed)");
    if (!std::isfinite(fps) || !(fps > 0.)) return h->fail(GRNET_EINVAL, name + "fps must be positive and finite");
    if (max_rows < 1 || max_rows > kBootMaxRows) return h->fail(GRNET_EINVAL, name + "max_rows " + std::to_string(max_rows) + " outside [1, " + std::to_string(kBootMaxRows) + "]");
    if (straight_only && !phase_dev) return h->fail(GRNET_EINVAL, name + "straight_only needs phase_dev");
    size_t mask_words = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeqCall c;
    if (int rc = seq_call(h, name, frame_offsets_host, n_seq, kGaitFrameCols, 0., s, &c, [&](int frames) {
            mask_words = gait_mask_words(frames, n_seq);
            return gait_mask_bytes(kStepMaskSets, mask_words);
        }))
        return rc;
    const hipError_t e = launch_step_tables(c.off, n_seq, events_dev, straight_only ? phase_dev : nullptr, per_frame_dev, fps, max_rows,
                                            reinterpret_cast<unsigned long long*>(c.behind), mask_words, steps_dev, strides_dev, counts_dev, s);
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

int grnet_bootstrap_table(grnet_t* h, const double* table_dev, const int32_t* counts_dev, int n_seq, int max_rows, int C, const int32_t* cols_host, int n_cols,
                          int B, int block, uint64_t seed, int stream_id, const int32_t* quantiles_host, int n_q, double* out_dev, double* replicates_dev,
                          void* stream) {
    if (!h) return GRNET_EINVAL;
    const std::string name = "grnet_bootstrap_table: ";
    if (!table_dev || !counts_dev || !cols_host || !out_dev || (n_q > 0 && !quantiles_host))
        return h->fail(GRNET_EINVAL, name + "null pointer (table_dev, counts_dev, cols_host, out_dev and, with n_q > 0, quantiles_host are all needed)");
    if (n_seq < 1 || n_seq > kTrackMaxSeqs) return h->fail(GRNET_EINVAL, name + "n_seq " + std::to_string(n_seq) + " outside [1, " + std::to_string(kTrackMaxSeqs) + "]");
    BootRule rule{};
    rule.max_rows = max_rows; rule.C = C; rule.n_cols = n_cols; rule.B = B; rule.block = block; rule.stream = stream_id; rule.n_q = n_q; rule.seed = seed;
    for (int k = 0; k < n_cols && k < kBootMaxCols; ++k) rule.cols[k] = cols_host[k];
    for (int k = 0; k < n_q && k < kBootMaxQuantiles; ++k) rule.q[k] = quantiles_host[k];
    const std::string why = rule_text(boot_rule_error(rule));     // gait_bootstrap.h's refusals, which the stand-alone checker runs too
    if (!why.empty()) return h->fail(GRNET_EINVAL, name + why);
    DeviceGuard guard(h->device);
    const hipError_t e = launch_bootstrap(table_dev, counts_dev, n_seq, rule, out_dev, replicates_dev, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return h->fail(GRNET_EHIP, name + hipGetErrorString(e));
    return 0;
}

}  // extern "C"
