// csrc/seq_args.h on the host: a stand-alone program (its own main, no HIP) for tests/test_seq_args_host_cpu.py, built with AddressSanitizer and
// UBSan.  The cases a GPU test would need gigabytes to reach: offsets at the 31-bit edge, the longest sequence at its edge, 8192 sequences.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "seq_args.h"

using namespace seq_args;

static int failures = 0;

static void expect(bool ok, const char* what, const std::string& got) {
    if (ok) return;
    ++failures;
    std::printf("FAILED: %s (got \"%s\")\n", what, got.c_str());
}

static bool has(const std::string& text, const char* word) { return text.find(word) != std::string::npos; }

static std::string offsets(std::vector<int32_t> off, long long longest, long long unit, const char* what = "frame_offsets") {
    return offsets_error(off.data(), (int)off.size() - 1, what, longest, unit);
}

int main() {
    std::string why = offsets({1, 8}, 0, 1);
    expect(has(why, "not 0") && has(why, "frame_offsets[0] = 1"), "off[0] != 0 is refused and the array is named", why);
    why = offsets({1, 8}, 0, 1, "point_offsets");
    expect(has(why, "point_offsets[0] = 1"), "the message uses the name it is given", why);
    why = offsets({0, 4, 4}, 0, 1);
    expect(has(why, "empty") && has(why, "sequence 1"), "an empty sequence is refused", why);
    why = offsets({0, 5, 3}, 0, 1);
    expect(has(why, "increase") && has(why, "(5, 3)"), "decreasing offsets are refused", why);
    expect(offsets({0, 8}, 0, 0).empty() && offsets({0, 3, 8}, 0, 75).empty(), "good offsets pass", "");

    // the longest sequence: exactly `longest` passes, one more does not; 0 means no such rule
    expect(offsets({0, 4096}, 4096, 25).empty() && offsets({0, 3, 4099}, 4096, 25).empty(), "a sequence of exactly the longest length passes", "");
    why = offsets({0, 4097}, 4096, 25);
    expect(has(why, "more than") && has(why, "4096") && has(why, "4097 entries"), "longest + 1 is refused and the limit is named", why);
    why = offsets({0, 3, 4100}, 4096, 25);
    expect(has(why, "more than") && has(why, "sequence 1"), "the second sequence's length is checked too", why);
    expect(offsets({0, 4097}, 0, 25).empty(), "longest 0: no such rule", "");

    // the 31-bit rule: off[n] * unit <= 2^31 - 1, without signed overflow (UBSan is the witness)
    const int32_t top = std::numeric_limits<int32_t>::max();   // 2^31 - 1, a prime: only unit 1 meets it exactly
    expect(offsets({0, top}, 0, 1).empty(), "off[n] * unit == 2^31 - 1 passes (unit 1)", "");
    expect(offsets({0, 1, 16777215}, 0, 128).empty(), "2^31 - 128 passes (unit 128)", "");
    expect(offsets({0, 3, 2147483647 / 75}, 0, 75).empty(), "the largest multiple of 75 below 2^31 passes", "");
    why = offsets({0, 5, 16777216}, 0, 128);
    expect(has(why, "31 bits"), "off[n] * unit == 2^31 is refused", why);
    why = offsets({0, 2147483647 / 75 + 1}, 0, 75);
    expect(has(why, "31 bits"), "one entry more than fits with unit 75 is refused", why);
    why = offsets({0, top}, 0, 75);
    expect(has(why, "31 bits"), "{0, 2^31 - 1} with unit 75 is refused", why);
    why = offsets({0, top}, 0, 3LL * top);
    expect(has(why, "31 bits"), "a unit of 3 (2^31 - 1), whose product leaves 64 bits, is refused", why);
    expect(offsets({0, top}, 0, 0).empty(), "the same offsets with unit 0 pass: no such rule", "");
    expect(offsets({0, top}, top, 1).empty(), "the longest length and the 31-bit edge together", "");

    // sizes
    expect(offsets({0, 1}, 1, 1).empty(), "n_seq = 1, one entry", "");
    std::vector<int32_t> many(8193);
    for (int q = 0; q <= 8192; ++q) many[q] = q;
    expect(offsets(many, 1, 262143).empty(), "n_seq = 8192, offsets 0 .. 8192", "");
    many[8000] = many[7999];
    why = offsets(many, 1, 1);
    expect(has(why, "sequence 7999") && has(why, "empty"), "the empty one of 8192 sequences is found", why);
    expect(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512, "align256 of 0, 1, 256, 257", "");

    // sigma: 0 (no Gaussian) or within (0, most]
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (double bad : {-1., nan, inf, -inf, 16.5}) {
        why = sigma_error(bad, 16.);
        expect(has(why, "sigma must be 0 (no Gaussian) or within (0, 16]"), "a sigma outside [0, 16] is refused in these words", why);
    }
    expect(sigma_error(0., 16.).empty() && sigma_error(16., 16.).empty() && sigma_error(1e-300, 16.).empty(), "sigma 0, 16 and a tiny one pass", "");

    // the joint table of gait and kinematics
    const int32_t table[4] = {0, 24, 25, -1};
    expect(joint_table_error(table, 2, 25).empty(), "indices inside [0, J) pass", "");
    why = joint_table_error(table, 3, 25);
    expect(has(why, "joint index 25 (entry 2) outside [0, 25)"), "an index of J is refused, with its entry", why);
    why = joint_table_error(table + 3, 1, 25);
    expect(has(why, "joint index -1 (entry 0)"), "a negative index is refused", why);

    // the opening of the gait calls: J < 1 first, then the table's words; the table is copied only where it is good
    int taken[4] = {7, 7, 7, 7};
    expect(joint_table_take(table, 2, 25, taken).empty() && taken[0] == 0 && taken[1] == 24 && taken[2] == 7, "a good table is copied, `count` entries of it", "");
    why = joint_table_take(table, 3, 25, taken);
    expect(why == joint_table_error(table, 3, 25) && taken[1] == 24 && taken[2] == 7, "a bad table is refused in joint_table_error's words and not copied", why);
    why = joint_table_take(table, 3, 0, taken);
    expect(why == "J 0 < 1", "J = 0 is refused before the table is read", why);
    why = joint_table_take(nullptr, 3, -2, taken);
    expect(why == "J -2 < 1" && taken[0] == 0, "a negative J too, and no index is read", why);

    // the raw columns: none without a Gaussian (0, negative or NaN sigma: the entry refuses the last two before it asks), else whole 256-byte steps
    expect(raw_bytes(0., 13, 400) == 0 && raw_bytes(-1., 13, 400) == 0 && raw_bytes(nan, 13, 400) == 0, "no Gaussian, no raw columns", "");
    expect(raw_bytes(2., 1, 1) == 256 && raw_bytes(2., 4, 8) == 256 && raw_bytes(16., 3, 11) == 512, "cols * frames doubles, rounded up to 256 bytes", "");
    expect(raw_bytes(0.5, 13, 2147483647u / 75) == align256((size_t)13 * (2147483647u / 75) * 8), "13 columns of the most frames a call of J = 25 takes", "");

    // the rule checks of the gait headers answer with a literal or null
    expect(rule_text(nullptr).empty() && rule_text("max_lag outside [8, 255]") == "max_lag outside [8, 255]", "null is no refusal, a literal is its own text", "");

    if (failures) {
        std::printf("%d failed\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
