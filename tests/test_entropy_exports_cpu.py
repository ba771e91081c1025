"""The C ABI of the entropy call: the two exports with their arities, the refusal without a handle, the methods and the column names,
the header declarations, and that csrc/gait_entropy.h stays free of HIP and includes gait_regularity.h alone."""
import os

from .conftest import PKG_NAME, ROOT


def test_exports(pkg):
    lib = pkg._lib.load()
    for name, arity in (("grnet_gait_entropy", 17), ("grnet_op_gait_sampen", 12)):
        assert name in pkg._lib.EXPORTS and hasattr(lib, name)
        assert len(pkg._lib.EXPORTS[name][1]) == arity
    # without a handle every call is refused, whatever else is wrong with it
    assert lib.grnet_gait_entropy(None, None, 25, None, 1, None, None, None, 0.0, 2, 0.2, 2, 3, None, None, None, None) == pkg._lib.EINVAL
    assert lib.grnet_op_gait_sampen(None, None, None, None, 1, 2, 0.2, 2, 3, None, None, None) == pkg._lib.EINVAL
    assert all(hasattr(pkg.GRNet, m) for m in ("gait_entropy", "op_gait_sampen"))
    pipe = pkg.pipeline
    assert pipe.ENTROPY_COLUMNS == ("n", "mean", "sd", "r") and pipe.ENTROPY_COUNTS == ("templates", "B", "A") and pipe.ENTROPY_MAX_FRAMES == 32768
    assert pipe.ENTROPY_CHANNELS is pipe.REGULARITY_CHANNELS and all(callable(getattr(pipe, f)) for f in ("gait_entropy", "gait_sampen", "entropy_rows"))
    header = open(os.path.join(ROOT, "include", "grnet_hip.h")).read()
    assert "int grnet_gait_entropy(" in header and "int grnet_op_gait_sampen(" in header and "int64_t* counts_dev" in header
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_entropy.h")).read()
    assert [ln.strip() for ln in src.splitlines() if ln.lstrip().startswith("#include")] == ['#include "gait_regularity.h"']
    assert "hip_runtime" not in src and "__global__" not in src and "namespace grk" in src and "GRK_TRANS_HD" in src
    for name in ("ent_diff", "ent_spread", "ent_coarse", "ent_template_valid", "ent_pair", "struct EntRule", "ent_rule_error"):
        assert name in src, name
    make = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    assert "$(BUILD)/gait_entropy_kernels.hip.o: CXXFLAGS += -ffp-contract=off" in make and "grnet_entropy.cpp" in make and make.count("gait_entropy.h") >= 2
