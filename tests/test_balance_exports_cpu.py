"""The C ABI of the balance call: the two exports with their arities, the refusal without a handle, the methods and the constants,
the header declarations, that csrc/gait_balance.h stays free of HIP, of the library and of libm and includes gait_turns.h alone, the Makefile's
lines, and that the kernels use no atomics."""
import os

from .conftest import PKG_NAME, ROOT


def test_exports(pkg):
    lib = pkg._lib.load()
    for name, arity in (("grnet_gait_balance", 20), ("grnet_op_gait_balance_steps", 15)):
        assert name in pkg._lib.EXPORTS and hasattr(lib, name)
        assert len(pkg._lib.EXPORTS[name][1]) == arity
    # without a handle every call is refused, whatever else is wrong with it
    assert lib.grnet_gait_balance(None, None, 25, None, 1, None, None, None, None, 14, 20.0, 9.81, 4, 1, 30, 256, None, None, None, None) == pkg._lib.EINVAL
    assert lib.grnet_op_gait_balance_steps(None, None, None, None, 1, 20.0, 9.81, 4, 1, 30, 256, None, None, None, None) == pkg._lib.EINVAL
    assert all(hasattr(pkg.GRNet, m) for m in ("gait_balance", "op_gait_balance_steps"))
    pipe = pkg.pipeline
    table = pipe.BALANCE_SEGMENTS_KINECTV2
    assert table is pkg._lib.BALANCE_SEGMENTS_KINECTV2 and len(table) == 14 and all(len(row) == 4 for row in table)
    assert abs(sum(row[2] for row in table) - 1.0) < 1e-12      # Winter's fractions of the whole body
    assert table[0] == (0, 20, 0.497, 0.5) and table[1] == (20, 3, 0.081, 1.0) and table[-1] == (18, 19, 0.0145, 0.5)
    assert [row[:2] for row in table[2:]] == [(4, 5), (8, 9), (5, 6), (9, 10), (6, 7), (10, 11), (12, 13), (16, 17), (13, 14), (17, 18), (14, 15), (18, 19)]
    assert [row[2:] for row in table[2::2]] == [row[2:] for row in table[3::2]] == [(0.028, 0.436), (0.016, 0.430), (0.006, 0.506), (0.100, 0.433), (0.0465, 0.433),
                                                                                    (0.0145, 0.5)]
    assert pipe.BALANCE_FRAME_COLUMNS == ("com_x", "com_y", "com_z", "path_x", "path_y", "path_z", "stance_side", "chain")
    assert pipe.BALANCE_STEP_COLUMNS == ("t1", "t2", "landing_side", "chain", "footprint_x", "footprint_y", "footprint_z", "stride_length", "step_length", "step_width",
                                         "com_speed", "mos_ap", "mos_ml", "vertical_excursion", "lateral_excursion")
    assert len(pipe.BALANCE_COLUMNS) == 24 and pipe.BALANCE_COLUMNS[:4] == ("strikes", "steps", "chains", "strides") and pipe.BALANCE_COLUMNS[13] == "ground_speed"
    assert pipe.BALANCE_COLUMNS[16:20] == ("mos_ml_mean", "mos_ml_sd", "mos_ml_left", "mos_ml_right")
    assert all(callable(getattr(pipe, f)) for f in ("gait_balance", "gait_balance_steps"))
    header = open(os.path.join(ROOT, "include", "grnet_hip.h")).read()
    assert "int grnet_gait_balance(" in header and "int grnet_op_gait_balance_steps(" in header and "const double* seg_weights_host" in header
    assert "LEVEL, FIXED CAMERA" in header and "creeps forward at heel rise" in header
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_balance.h")).read()
    assert [ln.strip() for ln in src.splitlines() if ln.lstrip().startswith("#include")] == ['#include "gait_turns.h"']
    assert "hip_runtime" not in src and "__global__" not in src and "namespace grk" in src and "GRK_TRANS_HD" in src and "__builtin_sqrt" in src
    assert all(word not in src for word in ("<cmath>", "<math.h>", "std::", " sqrt(", " fabs(", "cos(", "sin(", "log(", "atan"))      # no libm
    for name in ("balance_com", "balance_marks_before", "balance_mark_count", "balance_pair", "balance_chain", "balance_stride", "balance_path", "balance_row",
                 "balance_rule_error", "balance_segments_error", "window outside [1, 16]", "settle outside [0, 4]", "max_steps outside [1, 1024]", "n_seg outside [1, 16]"):
        assert name in src, name
    make = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    assert "$(BUILD)/gait_balance_kernels.hip.o: CXXFLAGS += -ffp-contract=off" in make and "grnet_balance.cpp" in make and "gait_balance_kernels.hip " in make
    assert make.count("gait_balance.h") >= 3                    # the flag's comment and both dependency lists
    deps = [ln for ln in make.splitlines() if ln.startswith("$(BUILD)/%.")]
    assert len(deps) == 2 and all("gait_balance.h" in ln for ln in deps)
    kernels = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_balance_kernels.hip")).read()
    assert "atomic" not in kernels.replace("No atomics", "") and all(k in kernels for k in ("balance_frames_kernel", "balance_steps_kernel", "balance_path_kernel"))
    limits = open(os.path.join(ROOT, PKG_NAME, "csrc", "kernels.h")).read()
    assert "constexpr int kBalanceLdsStrikes = 1024;" in limits
