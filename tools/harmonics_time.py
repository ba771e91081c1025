"""Time of the harmonic ratios per stride (grnet_gait_harmonics, csrc/gait_harmonics_kernels.hip) on one MI355X: one call at 400 frames (one
sequence) and at 10 000 frames in 25 sequences of 400, 25 joints, the walker of tests/helpers/regularity_checks.py at other periods, yaws and phases,
joints, translations and events on the device, the default rule (20 harmonics, the second derivative, strides of 8 .. 60 frames, 128 stored); without
smoothing (sigma 0, two launches) and with sigma 2 (three).  The events are pipeline.gait_parameters' of the same joints.

  device   the C ABI call with its four outputs, warm (code loaded): HIP events around REPS back-to-back calls, the median of WINDOWS such windows; us
  dft      grnet_op_gait_stride_dft alone on the call's own signals (the sequence kernel and the upload, without the frame kernel): the same measure
  host     pipeline.gait_harmonics after downloading the joints (numpy float64 with Python loops per sequence, channel, stride and harmonic): seconds
  equal    whether the device's outputs equal the host statement's bit for bit (sigma 0), or, with the Gaussian, what pipeline.gait_stride_dft makes
           of the device's own signals

    python tools/harmonics_time.py [out.txt]        # profiles/gait_harmonics_times.txt
"""
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from regularity_time import FPS, REPS, WINDOWS, T, device_us  # noqa: E402
from tests.helpers import gait_checks as gc  # noqa: E402
from tests.helpers import regularity_checks as rc  # noqa: E402

RULE = (20, 2, 8, 60, 128)                                      # n_harmonics, derivative, min_stride, max_stride, max_strides


def main():
    import torch
    pkg = importlib.import_module("video-based-gait-analysis-for-dementia_amd")
    assert torch.cuda.is_available(), "harmonics_time.py measures on the GPU: there is no CPU figure for the device call"
    m = pkg.GRNet(max_frames=1)                               # no weights: the call needs none
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = [f"# grnet_gait_harmonics on one MI355X: 25 joints, sequences of {T} frames of the walker of tests/helpers/regularity_checks.py (its four periods by turns, every",
             f"# other one asymmetric), the default rule (20 harmonics, derivative 2), four outputs, inputs on the device; us per call: HIP events around {REPS} back-to-back warm",
             f"# calls, median (min .. max) of {WINDOWS} windows.  dft_us: grnet_op_gait_stride_dft alone on the call's signals, median.  host: pipeline.gait_harmonics after",
             "# downloading the joints, seconds.  equal: every output bit against the host statement (sigma 0) or against pipeline.gait_stride_dft on the device's own signals",
             "# (sigma 2).  grnet_gait_regularity takes 71 us (sigma 0) and 79 us (sigma 2) at 400 frames (profiles/gait_regularity_times.txt).",
             "# frames sequences sigma launches device_us_median device_us_min device_us_max dft_us host_s strides_used mean_hr_sep equal"]
    table = (C.c_int32 * 8)(*gc.KINECTV2)
    for n in (T, 10000):
        lengths = [T] * (n // T)
        made = [rc.walker(T, rc.PERIODS[q % 4], 0.3 * (q % 2), 0.37 * q, 0.6137 * q) for q in range(len(lengths))]
        joints, trans = np.concatenate([j for j, _ in made]), np.concatenate([t for _, t in made])
        events = pkg.pipeline.gait_parameters(joints, lengths, trans, fps=FPS)["events"].astype(np.int32)
        dev_j, dev_t, dev_e = torch.from_numpy(joints).cuda(), torch.from_numpy(trans).cuda(), torch.from_numpy(events).cuda()
        off = np.zeros(len(lengths) + 1, np.int32)
        off[1:] = np.cumsum(lengths)
        offp = off.ctypes.data_as(C.POINTER(C.c_int32))
        per_frame = torch.empty(n, 4, dtype=torch.float64, device="cuda")
        strides = torch.empty(len(lengths), 4, RULE[4], 6, dtype=torch.float64, device="cuda")
        spectrum = torch.empty(len(lengths), 4, RULE[0], 2, dtype=torch.float64, device="cuda")
        per_seq = torch.empty(len(lengths), 4, 12, dtype=torch.float64, device="cuda")
        for sigma in (0.0, 2.0):
            def call():
                rc_ = m._lib.grnet_gait_harmonics(m._h, dev_j.data_ptr(), 25, offp, len(lengths), table, dev_t.data_ptr(), dev_e.data_ptr(), None, FPS, sigma, *RULE,
                                                  per_frame.data_ptr(), strides.data_ptr(), spectrum.data_ptr(), per_seq.data_ptr(), stream)
                assert rc_ == 0, m._lib.grnet_last_error(m._h)
            med, lo, hi = device_us(torch, call)
            out = {"per_frame": per_frame.cpu().numpy(), "strides": strides.cpu().numpy(), "spectrum": spectrum.cpu().numpy(), "per_sequence": per_seq.cpu().numpy()}
            signals = per_frame.clone()

            def hook():
                rc_ = m._lib.grnet_op_gait_stride_dft(m._h, signals.data_ptr(), dev_e.data_ptr(), None, offp, len(lengths), FPS, *RULE, strides.data_ptr(), spectrum.data_ptr(),
                                                      per_seq.data_ptr(), stream)
                assert rc_ == 0, m._lib.grnet_last_error(m._h)
            dft_us = device_us(torch, hook)[0]
            t0 = time.perf_counter()
            host = pkg.pipeline.gait_harmonics(joints, events, lengths, trans, fps=FPS, sigma=sigma)
            host_s = time.perf_counter() - t0
            if sigma > 0:
                host = dict(pkg.pipeline.gait_stride_dft(out["per_frame"], events, lengths, fps=FPS), per_frame=out["per_frame"])
            equal = all(rc.same_bits(out[k], host[k]) for k in out)
            lines.append(f"{n} {len(lengths)} {sigma:g} {3 if sigma > 0 else 2} {med:.1f} {lo:.1f} {hi:.1f} {dft_us:.1f} {host_s:.3f} {int(out['per_sequence'][:, 0, 1].sum())} "
                         f"{np.nanmean(out['per_sequence'][:, 0, 2]):.4f} {bool(equal)}")
            print(lines[-1], flush=True)
    m.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
