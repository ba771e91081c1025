"""csrc/gait_harmonics.h, the arithmetic the kernels run, on the host through tests/helpers/gait_harmonics_check.cpp: a stand-alone
program (its own main, no HIP) built with AddressSanitizer and UBSan and run directly on files this test writes -- one per sequence of the device
tests' calls -- against pipeline.gait_harmonics and pipeline.gait_stride_dft with sigma = 0.  Every bit equal."""
import os
import shutil
import subprocess

import numpy as np

from .conftest import PKG_NAME, ROOT
from .helpers import gait_checks as gc
from .helpers import harmonic_checks as hc
from .helpers import regularity_checks as rc

FPS = hc.FPS


def test_header_on_the_host_under_sanitizers(pkg, tmp_path):
    pipe = pkg.pipeline
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.isfile(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler (g++, clang++ or ROCm's clang++): the repository cannot be built here either"
    src = os.path.join(ROOT, "tests", "helpers", "gait_harmonics_check.cpp")
    exe = str(tmp_path / "gait_harmonics_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, PKG_NAME, "csrc"), src, "-o", exe], timeout=300)
    files = []
    for J, rule, with_trans in ((25, dict(hc.RULE, fps=FPS), True), (49, dict(fps=FPS, n_harmonics=32, derivative=1, min_stride=6, max_stride=255, max_strides=512), False),
                                (25, dict(fps=FPS, n_harmonics=2, derivative=0, min_stride=20, max_stride=24, max_strides=3), True)):
        table = gc.KINECTV2 if J == 25 else gc.OTHER49
        joints, trans, lengths, names = rc.build_call(J, table)
        trans = trans.copy()
        trans[[5, 200]] = np.nan
        events = pipe.gait_parameters(joints, lengths, trans, fps=FPS, joints=table)["events"]
        ex = np.zeros(sum(lengths), np.int32)
        ex[[3, 70, 71, 300, 301]] = 1
        a = 0
        for name, n in zip(names, lengths):
            tr = trans[a:a + n] if with_trans else None
            e = ex[a:a + n] if J == 25 else None
            host = pipe.gait_harmonics(joints[a:a + n], events[a:a + n], trans=tr, exclude=e, joints=table, **rule)
            files.append(hc.write_case(str(tmp_path / f"J{J}_{rule['n_harmonics']}_{name}.bin"), joints[a:a + n], table, tr, None, events[a:a + n], e, rule, host))
            a += n
    x, ev, ex, lengths, names = hc.hand_events_call()
    for rule in (dict(hc.RULE, fps=FPS, min_stride=6, max_stride=255, max_strides=8), dict(fps=FPS, n_harmonics=32, derivative=0, min_stride=6, max_stride=255, max_strides=128)):
        a = 0
        for name, n in zip(names, lengths):
            host = pipe.gait_stride_dft(x[a:a + n], ev[a:a + n], exclude=ex[a:a + n], **rule)
            files.append(hc.write_case(str(tmp_path / f"hand{rule['n_harmonics']}_{name}.bin"), None, gc.KINECTV2, None, x[a:a + n], ev[a:a + n], ex[a:a + n], rule, host))
            a += n
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-4000:] + r.stderr[-4000:]
