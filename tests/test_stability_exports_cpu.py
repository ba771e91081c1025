"""The C ABI of the stability call: the two exports with their arities, the refusal without a handle, the methods and the constants,
the header declarations, that csrc/gait_stability.h stays free of HIP and includes gait_entropy.h alone, and the Makefile's lines."""
import os

from .conftest import PKG_NAME, ROOT


def test_exports(pkg):
    lib = pkg._lib.load()
    for name, arity in (("grnet_gait_stability", 19), ("grnet_op_gait_divergence", 14)):
        assert name in pkg._lib.EXPORTS and hasattr(lib, name)
        assert len(pkg._lib.EXPORTS[name][1]) == arity
    # without a handle every call is refused, whatever else is wrong with it
    assert lib.grnet_gait_stability(None, None, 25, None, 1, None, None, None, 0.0, 1, 5, 2, 20, 20, None, None, None, None, None) == pkg._lib.EINVAL
    assert lib.grnet_op_gait_divergence(None, None, None, None, 1, 1, 5, 2, 20, 20, None, None, None, None) == pkg._lib.EINVAL
    assert all(hasattr(pkg.GRNet, m) for m in ("gait_stability", "op_gait_divergence"))
    pipe = pkg.pipeline
    assert pipe.STABILITY_PAIRS == ("n", "exponent") and pipe.STABILITY_MAX_FRAMES == 32768 == pipe.ENTROPY_MAX_FRAMES
    assert pipe.STABILITY_CHANNELS is pipe.REGULARITY_CHANNELS and all(callable(getattr(pipe, f)) for f in ("gait_stability", "gait_divergence", "stability_rows"))
    header = open(os.path.join(ROOT, "include", "grnet_hip.h")).read()
    assert "int grnet_gait_stability(" in header and "int grnet_op_gait_divergence(" in header and "int32_t* nn_dev" in header and "int64_t* pairs_dev" in header
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_stability.h")).read()
    assert [ln.strip() for ln in src.splitlines() if ln.lstrip().startswith("#include")] == ['#include "gait_entropy.h"']
    assert "hip_runtime" not in src and "__global__" not in src and "namespace grk" in src and "GRK_TRANS_HD" in src
    for name in ("stab_frexp", "stab_points", "stab_dist2", "stab_scan", "stab_walk", "struct StabRule", "stab_rule_error"):
        assert name in src, name
    kernels = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_stability_kernels.hip")).read()
    assert "stab_nn_kernel" in kernels and "stab_curve_kernel" in kernels and "atomic" not in kernels.replace("No atomics", "")
    make = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    assert "$(BUILD)/gait_stability_kernels.hip.o: CXXFLAGS += -ffp-contract=off" in make and "grnet_stability.cpp" in make and "gait_stability_kernels.hip " in make
    assert make.count("gait_stability.h") >= 3                 # the comment and both header dependency lists
