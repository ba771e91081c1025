"""The wide-line part of csrc/raster_lines.h, as the skeleton view's kernel runs it, checked on the host: tests/helpers/raster_wide_check.cpp is a
stand-alone program (its own main, no HIP, nothing of the library but that header) built with AddressSanitizer and UBSan and run directly.  It
proves, over 20 000 seeded random segments of widths 1 .. 16 and a few exact ones at every width, that the lowest minor index from one division
with the width's offset in the numerator, stepped by one major step and by 64, is the rule's formula evaluated in 128-bit arithmetic at every
step, and that width 1 is line_minor."""
import os
import shutil
import subprocess

from .conftest import PKG_NAME, ROOT


def test_wide_stepping_equals_the_formula(tmp_path):
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "raster_wide_check.cpp")
    exe = str(tmp_path / "raster_wide_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok" and lines[0].startswith("segments: 20288,") and lines[0].endswith("failures: 0"), r.stdout


def test_header_still_has_no_include():
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "raster_lines.h")).read()
    assert not [ln for ln in src.splitlines() if ln.startswith("#include")]
    assert "line_minor_wide" in src and "#if defined(__HIPCC__)" in src
