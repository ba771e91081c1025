"""csrc/seq_args.h, the argument rules of the calls that take sequences lying back to back -- the offsets' validator, align256, the sigma rule, the joint
table's and the opening the five gait calls share -- through tests/helpers/seq_args_check.cpp: a stand-alone program (its own main, no HIP) built with AddressSanitizer and UBSan and
run directly.  It reaches what a GPU test would need gigabytes for: offsets at the 31-bit edge, the longest sequence at its edge, 8192 sequences."""
import os
import shutil
import subprocess

from .conftest import PKG_NAME, ROOT


def test_header_on_the_host_under_sanitizers(tmp_path):
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "seq_args_check.cpp")
    exe = str(tmp_path / "seq_args_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-4000:] + r.stderr[-4000:]

