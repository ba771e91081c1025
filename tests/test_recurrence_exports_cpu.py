"""The C ABI of the recurrence call: the two exports with their arities, the refusal without a handle, the methods and the constants,
the header declarations, that csrc/gait_recurrence.h stays free of HIP and includes gait_stability.h alone, the kernels' names and that their only
atomics are the integer adds on LDS, and the Makefile's lines."""
import os
import re

from .conftest import PKG_NAME, ROOT


def test_exports(pkg):
    lib = pkg._lib.load()
    for name, arity in (("grnet_gait_recurrence", 19), ("grnet_op_gait_recurrence_counts", 14)):
        assert name in pkg._lib.EXPORTS and hasattr(lib, name)
        assert len(pkg._lib.EXPORTS[name][1]) == arity
    # without a handle every call is refused, whatever else is wrong with it
    assert lib.grnet_gait_recurrence(None, None, 25, None, 1, None, None, None, 0.0, 1, 5, 2, 8, 0.8, None, None, None, None, None) == pkg._lib.EINVAL
    assert lib.grnet_op_gait_recurrence_counts(None, None, None, None, 1, 1, 5, 2, 8, 0.8, None, None, None, None) == pkg._lib.EINVAL
    assert all(hasattr(pkg.GRNet, m) for m in ("gait_recurrence", "op_gait_recurrence_counts"))
    pipe = pkg.pipeline
    assert pipe.RECURRENCE_COLUMNS == ("n", "mean", "sd", "r", "eps2") and pipe.RECURRENCE_MAX_FRAMES == 32768 == pipe.ENTROPY_MAX_FRAMES and pipe.RECURRENCE_BINS == 255
    assert pipe.RECURRENCE_COUNTS == ("points", "comparable", "recurrent", "long_lines", "long_points", "longest")
    assert pipe.RECURRENCE_CHANNELS is pipe.REGULARITY_CHANNELS and all(callable(getattr(pipe, f)) for f in ("gait_recurrence", "gait_recurrence_counts", "recurrence_rows"))
    header = open(os.path.join(ROOT, "include", "grnet_hip.h")).read()
    assert "int grnet_gait_recurrence(" in header and "int grnet_op_gait_recurrence_counts(" in header and "int64_t* hist_dev" in header
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_recurrence.h")).read()
    assert [ln.strip() for ln in src.splitlines() if ln.lstrip().startswith("#include")] == ['#include "gait_stability.h"']
    assert "hip_runtime" not in src and "__global__" not in src and "atomic" not in src and "namespace grk" in src and "GRK_TRANS_HD" in src
    for name in ("struct RecRule", "rec_rule_error", "rec_eps2", "rec_pair", "rec_offset_walk", "rec_parts", "kRecBins = 255", "kRecMaxParts = 16", "static_assert"):
        assert name in src, name
    kernels = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_recurrence_kernels.hip")).read()
    assert "rec_pairs_kernel" in kernels and "rec_rows_kernel" in kernels and "launch_ent_spread" in kernels
    code = "\n".join(ln.split("//")[0] for ln in kernels.splitlines())
    assert re.findall(r"\batomic\w*", code) == ["atomicAdd"] and "atomicAdd(h + bin, 1u)" in code      # one integer add on LDS, no global and no floating-point atomic
    make = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    assert "$(BUILD)/gait_recurrence_kernels.hip.o: CXXFLAGS += -ffp-contract=off" in make and "grnet_recurrence.cpp" in make and "gait_recurrence_kernels.hip " in make
    assert make.count("gait_recurrence.h") >= 3                # the comment and both header dependency lists
    docs = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "grnet_gait_recurrence" in docs and "grnet_op_gait_recurrence_counts" in docs and "line_points / recurrent" in docs
