"""The C ABI of the mesh moments: the new exports with their arities, the refusal without a handle, the methods and the column names, the
header declarations, and that csrc/mesh_moments.h stays free of HIP and of libm."""
import os
import re

from .conftest import PKG_NAME, ROOT

ENTRIES = (("grnet_mesh_moments", 6), ("grnet_faces_closed", 2), ("grnet_gait_balance_com", 18), ("grnet_op_mesh_moments", 7))


def test_exports(pkg):
    lib = pkg._lib.load()
    for name, arity in ENTRIES:
        assert name in pkg._lib.EXPORTS and hasattr(lib, name)
        assert len(pkg._lib.EXPORTS[name][1]) == arity
    # without a handle every call is refused, whatever else is wrong with it
    assert lib.grnet_mesh_moments(None, None, 1, None, None, None) == pkg._lib.EINVAL
    assert lib.grnet_op_mesh_moments(None, None, 1, None, None, 0, None) == pkg._lib.EINVAL
    assert lib.grnet_faces_closed(None, None) == pkg._lib.EINVAL
    assert lib.grnet_gait_balance_com(None, None, 25, None, 1, None, None, None, 20.0, 9.81, 4, 1, 30, 256, None, None, None, None) == pkg._lib.EINVAL
    assert all(hasattr(pkg.GRNet, m) for m in ("mesh_moments", "faces_closed", "gait_balance"))
    pipe = pkg.pipeline
    assert len(pipe.MESH_MOMENT_COLUMNS) == 11 and len(pipe.BODY_COLUMNS) == 15 and pipe.MESH_COLUMNS == 1024
    assert all(callable(getattr(pipe, f)) for f in ("mesh_moments", "faces_closed", "body_rows", "gait_balance"))


def test_the_signatures_match_the_header(pkg):
    """Every parameter of the declarations in include/grnet_hip.h against the ctypes list of _lib.py: a pointer is a pointer, an int an int, a double a double."""
    import ctypes as C
    header = open(os.path.join(ROOT, "include", "grnet_hip.h")).read()
    for name, arity in ENTRIES:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        kinds = ["p" if "*" in p else ("d" if p.startswith("double") else "i") for p in params]
        assert len(kinds) == arity, (name, params)
        have = pkg._lib.EXPORTS[name][1]
        want = {"d": (C.c_double,), "i": (C.c_int,)}
        for k, t, p in zip(kinds, have, params):
            if k == "p":
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, p, t)
            else:
                assert t in want[k], (name, p, t)
        assert pkg._lib.EXPORTS[name][0] is C.c_int


def test_the_sources():
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "mesh_moments.h")).read()
    assert [ln.strip() for ln in src.splitlines() if ln.lstrip().startswith("#include")] == ["#include <cstdio>"]
    assert "hip_runtime" not in src and "__global__" not in src and "namespace grk" in src and "GRK_MESH_HD" in src
    assert all(word not in src for word in ("<cmath>", "<math.h>", "std::sqrt", " sqrt(", " fabs(", "fma("))      # no libm: the root is the compiler's builtin
    for name in ("mesh_face_terms", "mesh_face", "mesh_origin", "mesh_column", "mesh_tree", "mesh_row", "mesh_unmatched_edges", "mesh_table_text"):
        assert name in src, name
    make = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    assert "$(BUILD)/mesh_moments_kernels.hip.o: CXXFLAGS += -ffp-contract=off" in make and "grnet_body.cpp" in make and make.count("mesh_moments.h") >= 2
    kernels = open(os.path.join(ROOT, PKG_NAME, "csrc", "mesh_moments_kernels.hip")).read()
    assert "atomic" not in kernels.replace("No atomics", "") and "mesh_moments_kernel" in kernels and "__shfl_xor" in kernels
    impl = open(os.path.join(ROOT, PKG_NAME, "csrc", "grnet_impl.h")).read()
    assert "grnet_body.cpp" in impl
    balance = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_balance_kernels.hip")).read()
    assert "balance_com_frames_kernel" in balance
