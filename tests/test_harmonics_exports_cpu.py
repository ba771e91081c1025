"""The C ABI of the harmonics call: the two exports with their arities, the refusal without a handle, the methods and the column names,
and that csrc/gait_harmonics.h stays free of HIP."""
import os

from .conftest import PKG_NAME, ROOT


def test_exports(pkg):
    lib = pkg._lib.load()
    for name, arity in (("grnet_gait_harmonics", 21), ("grnet_op_gait_stride_dft", 16)):
        assert name in pkg._lib.EXPORTS and hasattr(lib, name)
        assert len(pkg._lib.EXPORTS[name][1]) == arity
    # without a handle every call is refused, whatever else is wrong with it
    assert lib.grnet_gait_harmonics(None, None, 25, None, 1, None, None, None, None, 20.0, 0.0, 20, 2, 8, 60, 128, None, None, None, None, None) == pkg._lib.EINVAL
    assert lib.grnet_op_gait_stride_dft(None, None, None, None, None, 1, 20.0, 20, 2, 8, 60, 128, None, None, None, None) == pkg._lib.EINVAL
    assert all(hasattr(pkg.GRNet, m) for m in ("gait_harmonics", "op_gait_stride_dft"))
    pipe = pkg.pipeline
    cols, stride_cols = pipe.HARMONICS_COLUMNS, pipe.HARMONICS_STRIDE_COLUMNS
    assert len(cols) == 12 and len(set(cols)) == 12 and len(stride_cols) == 6 and len(set(stride_cols)) == 6
    assert pipe.HARMONICS_CHANNELS is pipe.REGULARITY_CHANNELS and all(callable(getattr(pipe, f)) for f in ("gait_harmonics", "gait_stride_dft"))
    header = open(os.path.join(ROOT, "include", "grnet_hip.h")).read()
    assert "int grnet_gait_harmonics(" in header and "int grnet_op_gait_stride_dft(" in header
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_harmonics.h")).read()
    assert [ln.strip() for ln in src.splitlines() if ln.lstrip().startswith("#include")] == ['#include "gait_regularity.h"']
    assert "hip_runtime" not in src and "__global__" not in src and "namespace grk" in src and "GRK_TRANS_HD" in src
    make = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    assert "$(BUILD)/gait_harmonics_kernels.hip.o: CXXFLAGS += -ffp-contract=off" in make
