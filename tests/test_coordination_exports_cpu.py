"""The C ABI of the coordination call: the two exports with their arities, the refusal without a handle, the methods and the constants,
the header declarations, that csrc/gait_coordination.h stays free of HIP, of the library and of libm and includes gait_spectrum.h and gait_angles.h
alone, and the Makefile's lines."""
import os

from .conftest import PKG_NAME, ROOT


def test_exports(pkg):
    lib = pkg._lib.load()
    for name, arity in (("grnet_gait_coordination", 22), ("grnet_op_gait_cross_welch", 18)):
        assert name in pkg._lib.EXPORTS and hasattr(lib, name)
        assert len(pkg._lib.EXPORTS[name][1]) == arity
    # without a handle every call is refused, whatever else is wrong with it
    assert lib.grnet_gait_coordination(None, None, 25, None, 1, None, None, 20.0, 0.0, 0, 64, 32, 256, 0.5, 3.0, 4, None, None, None, None, None, None) == pkg._lib.EINVAL
    assert lib.grnet_op_gait_cross_welch(None, None, None, None, 1, 20.0, 0, 64, 32, 256, 0.5, 3.0, 4, None, None, None, None, None) == pkg._lib.EINVAL
    assert all(hasattr(pkg.GRNet, m) for m in ("gait_coordination", "op_gait_cross_welch"))
    pipe = pkg.pipeline
    assert pipe.COORDINATION_CHANNELS == ("arm_left", "arm_right", "leg_left", "leg_right")
    assert pipe.COORDINATION_PAIRS == ((0, 1), (2, 3), (0, 3), (1, 2), (0, 2), (1, 3)) and pipe.COORDINATION_EXPECTED_PHASE == (180.0, 180.0, 0.0, 0.0, 180.0, 180.0)
    assert pipe.COORDINATION_PAIR_NAMES == tuple(f"{pipe.COORDINATION_CHANNELS[a]}__{pipe.COORDINATION_CHANNELS[b]}" for a, b in pipe.COORDINATION_PAIRS)
    assert pipe.COORDINATION_LIMB_COLUMNS is pipe.SPECTRUM_COLUMNS
    assert pipe.COORDINATION_PAIR_COLUMNS == ("used", "peak_bin", "peak_hz", "cross_amplitude", "coherence_peak", "phase_peak", "phase_deviation", "lag_seconds",
                                              "coherence_band", "coherence_bins")
    assert pipe.COORDINATION_ROWS == ("amplitude", "arm_asymmetry", "leg_asymmetry", "arm_leg_ratio", "phase_deviation_mean")
    assert [pipe.KINEMATICS_CHANNELS[c] for c in pipe.COORDINATION_KINEMATICS_COLUMNS] == ["shoulder_flexion_left", "shoulder_flexion_right", "hip_flexion_left", "hip_flexion_right"]
    assert all(callable(getattr(pipe, f)) for f in ("gait_coordination", "gait_cross_welch", "coordination_rows"))
    header = open(os.path.join(ROOT, "include", "grnet_hip.h")).read()
    assert "int grnet_gait_coordination(" in header and "int grnet_op_gait_cross_welch(" in header and "double* cross_dev" in header
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_coordination.h")).read()
    assert [ln.strip() for ln in src.splitlines() if ln.lstrip().startswith("#include")] == ['#include "gait_spectrum.h"', '#include "gait_angles.h"']
    assert "hip_runtime" not in src and "__global__" not in src and "namespace grk" in src and "GRK_TRANS_HD" in src
    assert all(word not in src for word in ("<cmath>", "<math.h>", "std::", "cos(", "sin(", "log(", " atan2(", "atan("))      # no libm: the arctangent is gait_atan2
    for name in ("coord_frame", "coord_valid", "coord_bin", "coord_pair_row", "coord_rule_error", "coord_pair_a", "coord_antiphase", "spec_rule_error", "gait_atan2", "ent_diff",
                 "spec_band", "min_segments outside [2, 2^20]"):
        assert name in src, name
    make = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    assert "$(BUILD)/gait_coordination_kernels.hip.o: CXXFLAGS += -ffp-contract=off" in make and "grnet_coordination.cpp" in make and "gait_coordination_kernels.hip " in make
    assert make.count("gait_coordination.h") >= 3               # the flag's comment and both dependency lists
    deps = [ln for ln in make.splitlines() if ln.startswith("$(BUILD)/%.")]
    assert len(deps) == 2 and all("gait_coordination.h" in ln for ln in deps)
    kernels = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_coordination_kernels.hip")).read()
    assert "atomic" not in kernels.replace("No atomics", "") and all(k in kernels for k in ("coord_frames_kernel", "coord_csd_kernel", "coord_row_kernel"))
    limits = open(os.path.join(ROOT, PKG_NAME, "csrc", "kernels.h")).read()
    assert "constexpr int kCoordLdsFrames = 1024;" in limits and "constexpr int kCoordLdsSegments = 128;" in limits
