"""The C ABI of the smoothness call: the three exports with their arities, the refusal without a handle, the host-only slot count, the
methods and the column names, the header declarations, and that csrc/gait_smoothness.h stays free of HIP and of libm and includes gait_spectrum.h alone."""
import ctypes as C
import os

from .conftest import PKG_NAME, ROOT


def test_exports(pkg):
    lib = pkg._lib.load()
    for name, arity in (("grnet_gait_smoothness", 21), ("grnet_op_gait_sparc", 16), ("grnet_gait_smoothness_slots", 5)):
        assert name in pkg._lib.EXPORTS and hasattr(lib, name)
        assert len(pkg._lib.EXPORTS[name][1]) == arity
    # without a handle every call is refused, whatever else is wrong with it
    assert lib.grnet_gait_smoothness(None, None, 25, None, 1, None, None, None, 20.0, 0.0, 1, 64, 32, 1024, 10.0, 0.05, 2, None, None, None, None) == pkg._lib.EINVAL
    assert lib.grnet_op_gait_sparc(None, None, None, None, 1, 20.0, 1, 64, 32, 1024, 10.0, 0.05, 2, None, None, None) == pkg._lib.EINVAL
    assert all(hasattr(pkg.GRNet, m) for m in ("gait_smoothness", "op_gait_sparc", "smoothness_slots"))
    pipe = pkg.pipeline
    assert pipe.SMOOTHNESS_SEGMENT_COLUMNS == ("start", "sparc", "k_first", "k_last", "peak_bin", "peak_magnitude", "dj", "v_peak")
    assert pipe.SMOOTHNESS_COLUMNS == ("n", "candidates", "used", "defined", "sparc_mean", "sparc_sd", "sparc_min", "sparc_max", "last_hz_mean", "dj_defined")
    assert pipe.SMOOTHNESS_CHANNELS is pipe.REGULARITY_CHANNELS and pipe.SMOOTHNESS_MAX_FRAMES == 32768
    assert all(callable(getattr(pipe, f)) for f in ("gait_smoothness", "gait_sparc", "smoothness_rows", "smoothness_slots"))


def test_the_slot_count_on_the_host(pkg):
    lib = pkg._lib.load()
    lengths = [130, 1, 19, 20, 64, 65, 400, 63, 96, 95]
    off = (C.c_int32 * (len(lengths) + 1))(0, *[sum(lengths[:k + 1]) for k in range(len(lengths))])
    for segment, hop in ((64, 32), (64, 8), (8, 1), (16, 16), (256, 32)):
        slots = (C.c_int64 * (len(lengths) + 1))()
        assert lib.grnet_gait_smoothness_slots(off, len(lengths), segment, hop, slots) == 0
        want = [0]
        for T in lengths:
            want.append(want[-1] + len(range(0, T - segment + 1, hop)))      # every start at which a whole segment fits
        assert list(slots) == want == pkg.pipeline.smoothness_slots(lengths, segment, hop).tolist() == pkg.GRNet.smoothness_slots(lengths, segment, hop).tolist()
    slots = (C.c_int64 * 3)(-7, -7, -7)
    for bad in ((None, 2, 64, 32, slots), (off, 2, 64, 32, None), (off, 0, 64, 32, slots), (off, 2, 63, 32, slots), (off, 2, 6, 3, slots), (off, 2, 258, 64, slots),
                (off, 2, 64, 7, slots), (off, 2, 64, 65, slots), ((C.c_int32 * 3)(1, 5, 9), 2, 64, 32, slots), ((C.c_int32 * 3)(0, 5, 5), 2, 64, 32, slots)):
        assert lib.grnet_gait_smoothness_slots(*bad) == pkg._lib.EINVAL, bad[1:4]
    assert list(slots) == [-7, -7, -7]


def test_the_sources():
    header = open(os.path.join(ROOT, "include", "grnet_hip.h")).read()
    assert all(f"int {name}(" in header for name in ("grnet_gait_smoothness", "grnet_op_gait_sparc", "grnet_gait_smoothness_slots")) and "double* per_segment_dev" in header
    assert "UNVALIDATED ON THE MODEL'S OUTPUT" in header and "NYQUIST" in header
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_smoothness.h")).read()
    assert [ln.strip() for ln in src.splitlines() if ln.lstrip().startswith("#include")] == ['#include "gait_spectrum.h"']
    assert "hip_runtime" not in src and "__global__" not in src and "namespace grk" in src and "GRK_TRANS_HD" in src
    assert all(word not in src for word in ("<cmath>", "<math.h>", "std::", " cos(", " sin(", "log(", " sqrt(", " fabs("))      # no libm: the twiddles are har_twiddle's
    for name in ("smo_rule_error", "smo_cut_bin", "smo_magnitude", "smo_peak_merge", "smo_arc_term", "smo_arc", "smo_segment", "smo_jerk", "smo_row", "struct SmoRule",
                 "spec_rule_error", "spec_freq", "spec_run_segments"):
        assert name in src, name
    make = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    assert "$(BUILD)/gait_smoothness_kernels.hip.o: CXXFLAGS += -ffp-contract=off" in make and "grnet_smoothness.cpp" in make and make.count("gait_smoothness.h") >= 2
    kernels = open(os.path.join(ROOT, PKG_NAME, "csrc", "gait_smoothness_kernels.hip")).read()
    assert "atomic" not in kernels.replace("No atomics", "") and all(k in kernels for k in ("smo_starts_kernel", "smo_segment_kernel", "smo_row_kernel"))
