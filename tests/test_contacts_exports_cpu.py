"""The C ABI of the contacts call: the two exports with their arities, the refusal without a handle, the methods and the column names,
and that csrc/gait_contacts.h stays free of HIP."""
import os

from .conftest import PKG_NAME, ROOT


def test_exports(pkg):
    lib = pkg._lib.load()
    for name, arity in (("grnet_gait_contacts", 19), ("grnet_op_gait_contact_runs", 15)):
        assert name in pkg._lib.EXPORTS and hasattr(lib, name)
        assert len(pkg._lib.EXPORTS[name][1]) == arity
    # without a handle every call is refused, whatever else is wrong with it
    assert lib.grnet_gait_contacts(None, None, 25, None, 1, None, None, 20.0, 0.0, 0.25, 0.0, 2, 20, 128, None, None, None, None, None) == pkg._lib.EINVAL
    assert lib.grnet_op_gait_contact_runs(None, None, None, None, 1, 20.0, 0.25, 0.0, 2, 20, 128, None, None, None, None) == pkg._lib.EINVAL
    assert all(hasattr(pkg.GRNet, m) for m in ("gait_contacts", "op_gait_contact_runs"))
    cols, run_cols = pkg.pipeline.CONTACT_COLUMNS, pkg.pipeline.CONTACT_RUN_COLUMNS
    assert len(cols) == 20 and len(set(cols)) == 20 and len(run_cols) == 6 and len(set(run_cols)) == 6
    header = open(os.path.join(ROOT, "include", "grnet_hip.h")).read()
    assert "int grnet_gait_contacts(" in header and "int grnet_op_gait_contact_runs(" in header
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_contacts.h")).read()
    assert [ln.strip() for ln in src.splitlines() if ln.lstrip().startswith("#include")] == ['#include "gait_turns.h"']
    assert "hip_runtime" not in src and "__global__" not in src
