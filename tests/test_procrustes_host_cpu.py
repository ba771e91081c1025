"""csrc/procrustes3.h, the float64 rotation of the Procrustes alignment as the metric kernels run it, checked on the host:
tests/helpers/procrustes_check.cpp is a stand-alone program (its own main, no HIP, nothing of the library but that header) built with
AddressSanitizer and UBSan and run directly.  Over 40 000 seeded matrices -- dense, rank 1, rank 2, repeated singular values, scales from 1e-30 to
1e+30, condition numbers up to 1e16, either sign of the determinant -- and twenty exact ones it checks the certificate that trusts no SVD:
R^T R = I to 1e-12, det R > 0, R K symmetric to 1e-12 |K| with eigenvalues l1 >= l2 >= |l3|, l2 + l3 >= 0; and R = I for K = 0."""
import os
import shutil
import subprocess

from .conftest import PKG_NAME, ROOT


def test_certificate_over_seeded_and_exact_matrices(tmp_path):
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "procrustes_check.cpp")
    exe = str(tmp_path / "procrustes_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok" and lines[0] == "matrices: 40020, exact: 20, failures: 0", r.stdout


def test_header_has_no_include():
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "procrustes3.h")).read()
    assert not [ln for ln in src.splitlines() if ln.lstrip().startswith("#include")]
    assert "#if defined(__HIPCC__)" in src
