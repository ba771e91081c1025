"""Time and accuracy of the camera-space translation (grnet_fit_translation, csrc/translation_kernels.hip) on one MI355X: one call at
400 frames (one sequence) and at 10 000 frames in 25 sequences of 400, 13 pairs (pipeline.BODY25_FROM_KINECTV2) of 25 + 25 joints, fill on, one frame
in ten without a usable detection, inputs on the device.

  device   the C ABI call with both outputs, warm (code loaded): HIP events around REPS back-to-back calls, the median of WINDOWS such windows; us
  host     pipeline.fit_translation after downloading the inputs (numpy float64 with a Python loop per frame): seconds, one run
  ratios   the device's result against the exact checker tests/helpers/translation_checks.py: the worst error of t, of the reprojection error, of the
           sequences' means and of the path lengths in units of their bars, the largest cond_2(A), and device against host in units of two bars

    python tools/translation_time.py [out.txt]            # profiles/translation_times.txt
"""
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from tests.helpers import translation_checks as tc  # noqa: E402

REPS, WINDOWS, T = 20, 7, 400
HD = (1920, 1080)


def device_us(torch, call, reps=REPS):
    call(); call()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) / reps * 1e3)
    return statistics.median(per_call), min(per_call), max(per_call)


def main():
    import torch
    pkg = importlib.import_module("video-based-gait-analysis-for-dementia_amd")
    assert torch.cuda.is_available(), "translation_time.py measures on the GPU: there is no CPU figure for the device call"
    m = pkg.GRNet(max_frames=1)                               # no weights: the fit needs none
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pairs = np.ascontiguousarray(pkg.pipeline.BODY25_FROM_KINECTV2, dtype=np.int32)
    f = float(np.hypot(*HD))
    lines = [f"# grnet_fit_translation on one MI355X: 13 pairs of 25 + 25 joints, sequences of {T} frames, fill on, one frame in ten unfitted, both outputs, inputs on the",
             f"# device; us per call: HIP events around {REPS} back-to-back warm calls, median (min .. max) of {WINDOWS} windows.  host: pipeline.fit_translation after",
             "# downloading the inputs, seconds.  The ratios are the device's worst errors in units of the bars of DESIGN 4.9 against the exact checker (t: cond_2(A) 2^-52),",
             "# vs_host in units of two bars.",
             "# frames sequences device_us_median device_us_min device_us_max host_s t_ratio reproj_ratio mean_ratio path_ratio largest_cond vs_host_ratio failures"]
    for n in (T, 10000):
        lengths = [T] * (n // T)
        cams = [(f, 960.0, 540.0)] * len(lengths)
        j3, j2, _, kw = tc.make_case((13, 25, 25, n, lengths, cams, HD, (2.0, 8.0)), 40)
        j2[::10, :, 2] = 0.0
        d3, d2 = torch.from_numpy(j3).cuda(), torch.from_numpy(j2).cuda()
        off = np.zeros(len(lengths) + 1, np.int32)
        off[1:] = np.cumsum(lengths)
        cam = np.ascontiguousarray(cams, dtype=np.float64)
        per_frame = torch.empty(n, 6, dtype=torch.float64, device="cuda")
        per_seq = torch.empty(len(lengths), 4, dtype=torch.float64, device="cuda")

        def call():
            rc = m._lib.grnet_fit_translation(m._h, d3.data_ptr(), 25, d2.data_ptr(), 25, n, off.ctypes.data_as(C.POINTER(C.c_int32)), len(lengths),
                                              pairs.ctypes.data_as(C.POINTER(C.c_int32)), 13, cam.ctypes.data_as(C.POINTER(C.c_double)), 0.1, 4, 0, 1,
                                              per_frame.data_ptr(), per_seq.data_ptr(), stream)
            assert rc == 0, m._lib.grnet_last_error(m._h)
        med, lo, hi = device_us(torch, call)
        out = {"per_frame": per_frame.cpu().numpy(), "per_sequence": per_seq.cpu().numpy()}
        t0 = time.perf_counter()
        host = pkg.pipeline.fit_translation(j3, j2, pairs, **kw)
        host_s = time.perf_counter() - t0
        fails, worst = tc.compare(out, j3, j2, pairs, other=host, **kw)
        lines.append(f"{n} {len(lengths)} {med:.1f} {lo:.1f} {hi:.1f} {host_s:.3f} {worst['t']:.3g} {worst['reproj']:.3g} {worst['mean']:.3g} {worst['path']:.3g} "
                     f"{worst['cond']:.3g} {worst['other']:.3g} {len(fails)}")
        print(lines[-1], flush=True)
        for line in fails[:5]:
            print("  " + line, flush=True)
    m.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
