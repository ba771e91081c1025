"""The C ABI of the step tables and the bootstrap: the two exports with their arities, the refusal without a handle, the methods and
the constants, the header declarations, that csrc/gait_bootstrap.h stays free of HIP, of the library and of libm and includes gait_turns.h alone,
the Makefile's lines, and that the kernels use no atomics."""
import os

from .conftest import PKG_NAME, ROOT


def test_exports(pkg):
    lib = pkg._lib.load()
    for name, arity in (("grnet_gait_step_tables", 13), ("grnet_bootstrap_table", 17)):
        assert name in pkg._lib.EXPORTS and hasattr(lib, name)
        assert len(pkg._lib.EXPORTS[name][1]) == arity
    # without a handle every call is refused, whatever else is wrong with it
    assert lib.grnet_gait_step_tables(None, None, None, None, 1, 20.0, 256, None, 0, None, None, None, None) == pkg._lib.EINVAL
    assert lib.grnet_bootstrap_table(None, None, None, 1, 256, 6, None, 3, 2000, 1, 0, 0, None, 3, None, None, None) == pkg._lib.EINVAL
    assert all(hasattr(pkg.GRNet, m) for m in ("gait_step_tables", "bootstrap_table"))
    pipe = pkg.pipeline
    assert pipe.STEP_TABLE_COLUMNS == ("t_prev", "t", "landing_foot", "step_time", "step_length", "step_width")
    assert pipe.STRIDE_TABLE_COLUMNS == ("t0", "t1", "foot", "stride_time") and pipe.BOOTSTRAP_STATISTICS == ("mean", "sd", "cv")
    assert all(callable(getattr(pipe, f)) for f in ("gait_step_tables", "bootstrap_table", "bootstrap_indices", "bootstrap_u", "bootstrap_index", "bootstrap_mix",
                                                    "bootstrap_select"))
    header = open(os.path.join(ROOT, "include", "grnet_hip.h")).read()
    assert "int grnet_gait_step_tables(" in header and "int grnet_bootstrap_table(" in header and "uint64_t seed" in header
    assert "0x9E3779B97F4A7C15" in header and "UNDER-COVERS" in header and "TWO SEQUENCES WITH EQUAL n GET EQUAL INDICES" in header
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_bootstrap.h")).read()
    assert [ln.strip() for ln in src.splitlines() if ln.lstrip().startswith("#include")] == ['#include "gait_turns.h"']
    assert "hip_runtime" not in src and "__global__" not in src and "namespace grk" in src and "GRK_TRANS_HD" in src and "__builtin_sqrt" in src
    assert all(word not in src for word in ("<cmath>", "<math.h>", "std::", " sqrt(", " fabs(", "cos(", "sin(", "log(", "atan", "atomic"))      # no libm
    for name in ("boot_step_rows", "boot_stride_rows", "boot_mix", "boot_stream_key", "boot_replicate_key", "boot_u", "boot_index", "boot_statistics", "boot_before",
                 "boot_quantile_rank", "boot_select", "boot_rule_error", "0x9E3779B97F4A7C15ull", "0xBF58476D1CE4E5B9ull", "0x94D049BB133111EBull",
                 "max_rows outside [1, 1024]", "B outside [1, 4096]", "block outside [1, 1024]", "stream outside [0, 65535]", "n_cols outside [1, 8]", "C outside [1, 16]"):
        assert name in src, name
    make = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    assert "$(BUILD)/gait_bootstrap_kernels.hip.o: CXXFLAGS += -ffp-contract=off" in make and "grnet_bootstrap.cpp" in make and "gait_bootstrap_kernels.hip " in make
    assert make.count("gait_bootstrap.h") >= 3                  # the flag's comment and both dependency lists
    deps = [ln for ln in make.splitlines() if ln.startswith("$(BUILD)/%.")]
    assert len(deps) == 2 and all("gait_bootstrap.h" in ln for ln in deps)
    kernels = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_bootstrap_kernels.hip")).read()
    assert "atomic" not in kernels.replace("No atomics", "").replace("no atomics", "") and all(k in kernels for k in ("step_tables_kernel", "bootstrap_kernel"))
    assert "asm" not in kernels and "__ballot" in kernels
    limits = open(os.path.join(ROOT, PKG_NAME, "csrc", "kernels.h")).read()
    assert "constexpr int kBootThreads = 1024;" in limits and "constexpr int kBootRounds = 5;" in limits and "constexpr int kStepMaskSets = 3;" in limits
    host = open(os.path.join(ROOT, PKG_NAME, "csrc", "grnet_bootstrap.cpp")).read()
    assert "seq_call(" in host and "hipDeviceSynchronize" not in host and "hipStreamSynchronize" not in host and "hipMalloc" not in host
