"""The C ABI of the spectrum call: the two exports with their arities, the refusal without a handle, the methods and the column names,
the header declarations, and that csrc/gait_spectrum.h stays free of HIP and of the library and includes gait_harmonics.h and gait_entropy.h alone."""
import os

from .conftest import PKG_NAME, ROOT


def test_exports(pkg):
    lib = pkg._lib.load()
    for name, arity in (("grnet_gait_spectrum", 21), ("grnet_op_gait_welch", 16)):
        assert name in pkg._lib.EXPORTS and hasattr(lib, name)
        assert len(pkg._lib.EXPORTS[name][1]) == arity
    # without a handle every call is refused, whatever else is wrong with it
    assert lib.grnet_gait_spectrum(None, None, 25, None, 1, None, None, None, 20.0, 0.0, 2, 64, 32, 256, 0.5, 3.0, 2, None, None, None, None) == pkg._lib.EINVAL
    assert lib.grnet_op_gait_welch(None, None, None, None, 1, 20.0, 2, 64, 32, 256, 0.5, 3.0, 2, None, None, None) == pkg._lib.EINVAL
    assert all(hasattr(pkg.GRNet, m) for m in ("gait_spectrum", "op_gait_welch"))
    pipe = pkg.pipeline
    assert pipe.SPECTRUM_COLUMNS == ("n", "candidates", "used", "band_power", "total_power", "peak_bin", "peak_hz", "peak_height", "peak_width_hz", "dominance", "centroid_hz",
                                     "edge_hz", "cadence") and pipe.SPECTRUM_MAX_FRAMES == 32768
    assert pipe.SPECTRUM_CHANNELS is pipe.REGULARITY_CHANNELS and all(callable(getattr(pipe, f)) for f in ("gait_spectrum", "gait_welch", "spectrum_rows"))
    header = open(os.path.join(ROOT, "include", "grnet_hip.h")).read()
    assert "int grnet_gait_spectrum(" in header and "int grnet_op_gait_welch(" in header and "double* psd_dev" in header
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_spectrum.h")).read()
    assert [ln.strip() for ln in src.splitlines() if ln.lstrip().startswith("#include")] == ['#include "gait_harmonics.h"', '#include "gait_entropy.h"']
    assert "hip_runtime" not in src and "__global__" not in src and "namespace grk" in src and "GRK_TRANS_HD" in src
    assert all(word not in src for word in ("<cmath>", "<math.h>", "std::", "cos(", "sin(", "log("))      # no libm: the twiddles are har_twiddle's
    for name in ("spec_runs", "spec_mean", "spec_hann", "spec_window_power", "spec_bin", "spec_density", "spec_band", "spec_row", "struct SpecRule", "spec_rule_error",
                 "har_twiddle", "ent_diff"):
        assert name in src, name
    make = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    assert "$(BUILD)/gait_spectrum_kernels.hip.o: CXXFLAGS += -ffp-contract=off" in make and "grnet_spectrum.cpp" in make and make.count("gait_spectrum.h") >= 2
    kernels = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_spectrum_kernels.hip")).read()
    assert "atomic" not in kernels.replace("No atomics", "") and "spec_psd_kernel" in kernels and "spec_row_kernel" in kernels
