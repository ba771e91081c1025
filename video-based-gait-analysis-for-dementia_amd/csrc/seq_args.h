// The argument rules of the calls that take sequences lying back to back (boxes, metrics, trajectory, per-frame boxes, the five gait calls and their
// hooks): one statement each, in plain C++17 without a HIP header, so that a stand-alone program can run them (tests/helpers/seq_args_check.cpp).
#pragma once
#include <cstdint>
#include <string>

namespace seq_args {

constexpr size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }      // scratch is carved in 256-byte steps

// "" or what is wrong with the n_seq + 1 offsets `off` (n_seq >= 1) of sequences lying back to back; `what` names the array in the message.
//   off[0] is 0 and the offsets strictly increase: every sequence has at least one entry;
//   longest > 0: no sequence has more entries than that;
//   unit > 0: the kernels of the call index its off[n_seq] * unit values with an int, so that product -- tested in 64 bits -- must not exceed
//   2^31 - 1.  A call whose kernels index with size_t passes 0 and has no such rule (grnet_pose_metrics, grnet_fit_translation).
inline std::string offsets_error(const int32_t* off, int n_seq, const char* what, long long longest, long long unit) {
    if (off[0] != 0) return std::string(what) + "[0] = " + std::to_string(off[0]) + ", not 0";
    for (int q = 0; q < n_seq; ++q) {
        const long long len = (long long)off[q + 1] - off[q];
        if (len < 1) return "sequence " + std::to_string(q) + " is empty or its offsets do not increase (" + std::to_string(off[q]) + ", " + std::to_string(off[q + 1]) + ")";
        if (longest > 0 && len > longest) return "sequence " + std::to_string(q) + " has " + std::to_string(len) + " entries, more than " + std::to_string(longest);
    }
    if (unit > 0 && off[n_seq] > 0x7fffffffLL / unit)          // off[n_seq] * unit > 2^31 - 1, without a product that could leave 64 bits
        return std::to_string(off[n_seq]) + " entries of " + std::to_string(unit) + " values in one call no longer fit 31 bits";
    return "";
}

// "" or what is wrong with the width of a call's Gaussian, in frames: 0 means none, `most` is the widest whose weights fit the call's table
inline std::string sigma_error(double sigma, double most) {
    if (sigma >= 0. && sigma <= most) return "";                // false for a NaN
    return "sigma must be 0 (no Gaussian) or within (0, " + std::to_string((int)most) + "]";
}

// "" or which entry of a call's table of `count` joint indices lies outside its J joints (grnet_gait_parameters, grnet_gait_kinematics)
inline std::string joint_table_error(const int32_t* idx, int count, int J) {
    for (int k = 0; k < count; ++k)
        if (idx[k] < 0 || idx[k] >= J) return "joint index " + std::to_string(idx[k]) + " (entry " + std::to_string(k) + ") outside [0, " + std::to_string(J) + ")";
    return "";
}

// The opening of the five gait calls: "" and `table` = the call's `count` joint indices, or why not -- J < 1, else joint_table_error's words
inline std::string joint_table_take(const int32_t* idx, int count, int J, int* table) {
    if (J < 1) return "J " + std::to_string(J) + " < 1";
    std::string why = joint_table_error(idx, count, J);
    if (why.empty())
        for (int k = 0; k < count; ++k) table[k] = idx[k];
    return why;
}

// bytes of the (cols, frames) float64 columns that a call's frame kernel leaves for the Gaussian: none without one
inline size_t raw_bytes(double sigma, size_t cols, size_t frames) { return sigma > 0. ? align256(cols * frames * sizeof(double)) : 0; }

// a *_rule_error of the gait headers answers with a literal or null
inline std::string rule_text(const char* why) { return why ? why : ""; }

}  // namespace seq_args
