"""The C ABI of the regularity call: the two exports with their arities, the refusal without a handle, the methods and the column names,
and that csrc/gait_regularity.h stays free of HIP."""
import os

from .conftest import PKG_NAME, ROOT


def test_exports(pkg):
    lib = pkg._lib.load()
    for name, arity in (("grnet_gait_regularity", 18), ("grnet_op_gait_autocorr", 13)):
        assert name in pkg._lib.EXPORTS and hasattr(lib, name)
        assert len(pkg._lib.EXPORTS[name][1]) == arity
    # without a handle every call is refused, whatever else is wrong with it
    assert lib.grnet_gait_regularity(None, None, 25, None, 1, None, None, None, 20.0, 0.0, 60, 4, 0.25, 20, None, None, None, None) == pkg._lib.EINVAL
    assert lib.grnet_op_gait_autocorr(None, None, None, None, 1, 20.0, 60, 4, 0.25, 20, None, None, None) == pkg._lib.EINVAL
    assert all(hasattr(pkg.GRNet, m) for m in ("gait_regularity", "op_gait_autocorr"))
    cols, channels = pkg.pipeline.REGULARITY_COLUMNS, pkg.pipeline.REGULARITY_CHANNELS
    assert len(cols) == 10 and len(set(cols)) == 10 and channels == ("sep", "lift", "sway", "bob")
    header = open(os.path.join(ROOT, "include", "grnet_hip.h")).read()
    assert "int grnet_gait_regularity(" in header and "int grnet_op_gait_autocorr(" in header
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_regularity.h")).read()
    assert [ln.strip() for ln in src.splitlines() if ln.lstrip().startswith("#include")] == ['#include "gait_turns.h"']
    assert "hip_runtime" not in src and "__global__" not in src
