"""Time of gait regularity and symmetry from the autocorrelation (grnet_gait_regularity, csrc/gait_regularity_kernels.hip) on one MI355X:
one call at 400 frames (one sequence) and at 10 000 frames in 25 sequences of 400, 25 joints, the walker of tests/helpers/regularity_checks.py at
other periods, yaws and phases, joints and translations on the device, the default rule (61 lags); without smoothing (sigma 0, two launches) and with
sigma 2 (three).

  device   the C ABI call with its three outputs, warm (code loaded): HIP events around REPS back-to-back calls, the median of WINDOWS such windows; us
  acf      grnet_op_gait_autocorr alone on the call's own signals (the sequence kernel and the upload, without the frame kernel): the same measure
  host     pipeline.gait_regularity after downloading the joints (numpy float64 with Python loops per sequence, channel and lag): seconds, one run
  equal    whether the device's outputs equal the host statement's bit for bit (sigma 0), or, with the Gaussian, what pipeline.gait_autocorr makes of
           the device's own signals

    python tools/regularity_time.py [out.txt]        # profiles/gait_regularity_times.txt
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
from tests.helpers import gait_checks as gc  # noqa: E402
from tests.helpers import regularity_checks as rc  # noqa: E402

REPS, WINDOWS, T, FPS = 20, 7, 400, 20.0
RULE = (60, 4, 0.25, 20)                                        # max_lag, min_lag, min_peak, min_pairs


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
    assert torch.cuda.is_available(), "regularity_time.py measures on the GPU: there is no CPU figure for the device call"
    m = pkg.GRNet(max_frames=1)                               # no weights: the call needs none
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = [f"# grnet_gait_regularity on one MI355X: 25 joints, sequences of {T} frames of the walker of tests/helpers/regularity_checks.py (its four periods by turns, every",
             f"# other one asymmetric), the default rule (61 lags), three outputs, inputs on the device; us per call: HIP events around {REPS} back-to-back warm calls, median",
             f"# (min .. max) of {WINDOWS} windows.  acf_us: grnet_op_gait_autocorr alone on the call's signals, median.  host: pipeline.gait_regularity after downloading the",
             "# joints, seconds.  equal: every output bit against the host statement (sigma 0) or against pipeline.gait_autocorr on the device's own signals (sigma 2).",
             "# frames sequences sigma launches device_us_median device_us_min device_us_max acf_us host_s stride_lags_found mean_cadence equal"]
    table = (C.c_int32 * 8)(*gc.KINECTV2)
    for n in (T, 10000):
        lengths = [T] * (n // T)
        made = [rc.walker(T, rc.PERIODS[q % 4], 0.3 * (q % 2), 0.37 * q, 0.6137 * q) for q in range(len(lengths))]
        joints, trans = np.concatenate([j for j, _ in made]), np.concatenate([t for _, t in made])
        dev_j, dev_t = torch.from_numpy(joints).cuda(), torch.from_numpy(trans).cuda()
        off = np.zeros(len(lengths) + 1, np.int32)
        off[1:] = np.cumsum(lengths)
        offp = off.ctypes.data_as(C.POINTER(C.c_int32))
        per_frame = torch.empty(n, 4, dtype=torch.float64, device="cuda")
        acf = torch.empty(len(lengths), 4, RULE[0] + 1, dtype=torch.float64, device="cuda")
        per_seq = torch.empty(len(lengths), 4, 10, dtype=torch.float64, device="cuda")
        for sigma in (0.0, 2.0):
            def call():
                rc_ = m._lib.grnet_gait_regularity(m._h, dev_j.data_ptr(), 25, offp, len(lengths), table, dev_t.data_ptr(), None, FPS, sigma, *RULE, per_frame.data_ptr(),
                                                   acf.data_ptr(), per_seq.data_ptr(), stream)
                assert rc_ == 0, m._lib.grnet_last_error(m._h)
            med, lo, hi = device_us(torch, call)
            out = {"per_frame": per_frame.cpu().numpy(), "acf": acf.cpu().numpy(), "per_sequence": per_seq.cpu().numpy()}
            signals = per_frame.clone()

            def hook():
                rc_ = m._lib.grnet_op_gait_autocorr(m._h, signals.data_ptr(), None, offp, len(lengths), FPS, *RULE, acf.data_ptr(), per_seq.data_ptr(), stream)
                assert rc_ == 0, m._lib.grnet_last_error(m._h)
            acf_us = device_us(torch, hook)[0]
            t0 = time.perf_counter()
            host = pkg.pipeline.gait_regularity(joints, lengths, trans, fps=FPS, sigma=sigma)
            host_s = time.perf_counter() - t0
            if sigma > 0:
                host = dict(pkg.pipeline.gait_autocorr(out["per_frame"], lengths, fps=FPS), per_frame=out["per_frame"])
            equal = all(rc.same_bits(out[k], host[k]) for k in out)
            lines.append(f"{n} {len(lengths)} {sigma:g} {3 if sigma > 0 else 2} {med:.1f} {lo:.1f} {hi:.1f} {acf_us:.1f} {host_s:.3f} {int((out['per_sequence'][:, :, 5] >= 0).sum())} "
                         f"{np.nanmean(out['per_sequence'][:, 0, 9]):.2f} {bool(equal)}")
            print(lines[-1], flush=True)
    m.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
