"""The references of the device --smooth step, checked without a GPU: the strict float32 restatement of the One-Euro filter IS the
reference (bit for bit on the reference-made golden), the fma-contracted form is not -- so the GPU tests' array_equal tells a correctly
compiled kernel from a contracted one -- and the built library carries the new entry points."""
import ctypes
import os
import re

import numpy as np

from .conftest import ROOT
from .helpers import smooth_checks as sc


def _golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "one_euro.npz"))      # produced by the reference's OneEuroFilter
    return g["seq"], g["hat"]


def test_strict_f32_restatement_is_the_reference_bit_for_bit():
    seq, hat = _golden()
    got = sc.one_euro_strict_f32(seq, 0.004, 0.7)
    assert got.dtype == np.float32 and got.shape == hat.shape == (40, 24, 3)
    assert np.array_equal(got, hat), int((got != hat).sum())


def test_fma_contraction_is_not_the_reference():
    """What hipcc's default (-ffp-contract=fast in device code) would compute: hundreds of elements off by an ulp after 40 frames."""
    seq, hat = _golden()
    got = sc.one_euro_fma(seq, 0.004, 0.7)
    differ = int((got != hat).sum())
    print(f"fma-contracted filter: {differ} of {hat.size} elements differ, max {np.abs(got - hat).max():.2e}")
    assert not np.array_equal(got, hat)
    assert differ > hat.size // 10                            # not a stray tie: a property a test can rely on
    assert np.allclose(got, hat, rtol=1e-5, atol=1e-6)        # and still the same filter


def test_host_filter_is_close_but_not_bit_exact(pkg):
    """pipeline.one_euro_filter stays the host statement (a_d formed in double): inside its own 1e-6 bar, not bit-identical -- the
    reason the device path is compared with the strict restatement and the host path only to that bar."""
    seq, hat = _golden()
    got = pkg.pipeline.one_euro_filter(seq, min_cutoff=0.004, beta=0.7)
    assert np.allclose(got, hat, rtol=1e-6, atol=1e-7)
    assert sc.one_euro_strict_f32(seq[:1]).shape == (1, 24, 3) and np.array_equal(sc.one_euro_strict_f32(seq[:1]), seq[:1])


def test_rodrigues_f64_agrees_with_the_host_statement(pkg):
    g = np.random.Generator(np.random.Philox(key=[5, 5]))
    aa = (g.standard_normal((200, 3)) * 1.5).astype(np.float32)
    R = sc.rodrigues_f64(aa)
    # the 1e-8 inside the norm leaves the axis a hair off unit length (|d|^2 - 1 ~ 2e-8 / |aa|): a rotation to 1e-6 for |aa| of order 1
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6
    assert np.abs(pkg.pipeline.rodrigues(aa) - R).max() < 2e-6


def test_library_exports_the_smooth_entry_points(pkg):
    new = ("grnet_op_one_euro", "grnet_op_aa_to_rotmat", "grnet_smooth_pose")
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "grnet_hip.h")).read()
    for name in new:
        assert hasattr(lib, name), name
        assert name in pkg._lib.EXPORTS, name
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert len(pkg._lib.EXPORTS["grnet_smooth_pose"][1]) == 12
    assert (pkg._lib.JOINTS_SPIN49, pkg._lib.JOINTS_SPIN2, pkg._lib.JOINTS_KINECTV2) == (0, 1, 2)
    for name, value in (("SPIN49", 0), ("SPIN2", 1), ("KINECTV2", 2)):
        assert re.search(r"#define\s+GRNET_JOINTS_" + name + r"\s+" + str(value) + r"\b", hdr), name


def test_filter_block_constant_is_stated_once(pkg):
    """The GPU tests pick their sequence lengths around the filter's staging block: the kernel header states it, kernels.h defines it."""
    csrc = os.path.join(os.path.dirname(pkg.__file__), "csrc")
    m = re.search(r"constexpr int kOneEuroBlock = (\d+);", open(os.path.join(csrc, "kernels.h")).read())
    assert m and int(m.group(1)) == 32
    assert "kOneEuroBlock = 32" in open(os.path.join(csrc, "smooth_kernels.hip")).read()
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"smooth_kernels\.hip\.o:\s*CXXFLAGS\s*\+=\s*-ffp-contract=off", mk)
