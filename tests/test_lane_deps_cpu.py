"""csrc/lane_deps.h, the reduction of the lane schedule's cross-lane waits, checked on the host: tests/helpers/lane_deps_check.cpp is a stand-alone
program (its own main, no HIP, nothing of the library but that header) built with AddressSanitizer and UBSan and run directly.  It proves, over 200
seeded random op lists and one HR module's fuse pattern, that the kept waits order exactly what all cross-lane edges order, that none of them is
implied by the others, and that an event is recorded exactly where a kept wait names it."""
import os
import shutil
import subprocess

from .conftest import PKG_NAME, ROOT


def test_wait_reduction_keeps_the_happens_before_order(tmp_path):
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "lane_deps_check.cpp")
    exe = str(tmp_path / "lane_deps_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           src, "-o", exe], timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok" and lines[0].startswith("random: 200 cases") and lines[1].startswith("hr: "), r.stdout


def test_header_has_no_hip_dependency():
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "lane_deps.h")).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
