"""Time of the per-frame boxes from 2D joints (grnet_track_boxes, csrc/track_kernels.hip) on one MI355X: one call at 400 frames (one
sequence) and at 10 000 frames in 25 sequences of 400, 25 joints, about one frame in five without a detection (in runs, with dead frames at both
ends), joints on the device; stages 1 and 2 alone (kernel_size 1, sigma 0) and the whole chain with the reference's median of 11 and sigma 3, edge
padding.

  device   the C ABI call with its three outputs, warm (code loaded): HIP events around REPS back-to-back calls, the median of WINDOWS such windows; us
  host     pipeline.track_boxes after downloading the joints (numpy float64 with a Python loop per frame): seconds, one run
  equal    whether the device's status and range equal the host statement's, and its boxes too -- bit for bit without the Gaussian, within twice the
           Gaussian's bar of tests/helpers/track_checks.py with it

    python tools/track_time.py [out.txt]            # profiles/track_boxes_times.txt
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
from tests.helpers import track_checks as tk  # noqa: E402
from tools.make_goldens_bbox import BODY  # noqa: E402

REPS, WINDOWS, T = 20, 7, 400


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


def walk(g, frames):
    """A body of 25 joints drifting across the frame with jitter; dead frames in runs of 1 to 9, and 5 at either end."""
    t = np.arange(frames, dtype=np.float64)
    kp = np.empty((frames, 25, 3))
    kp[:, :, 0] = (400.0 + 1100.0 * t / frames)[:, None] + BODY[None, :, 0] * 620.0 + g.normal(0.0, 4.0, (frames, 25))
    kp[:, :, 1] = (540.0 + 12.0 * np.sin(t * 0.55))[:, None] + BODY[None, :, 1] * 620.0 + g.normal(0.0, 4.0, (frames, 25))
    kp[:, :, 2] = g.uniform(0.31, 1.0, (frames, 25))
    kp[:5, :, 2] = kp[-5:, :, 2] = 0.1
    i = 10
    while i < frames - 10:
        run = int(g.integers(1, 10))
        kp[i:i + run, :, 2] = 0.1
        i += run + int(g.integers(10, 60))
    return kp


def main():
    import torch
    pkg = importlib.import_module("video-based-gait-analysis-for-dementia_amd")
    assert torch.cuda.is_available(), "track_time.py measures on the GPU: there is no CPU figure for the device call"
    m = pkg.GRNet(max_frames=1)                               # no weights: the boxes need none
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = [f"# grnet_track_boxes on one MI355X: 25 joints, sequences of {T} frames, about one frame in five without a detection, three outputs, joints on the device;",
             f"# us per call: HIP events around {REPS} back-to-back warm calls, median (min .. max) of {WINDOWS} windows.  host: pipeline.track_boxes after downloading",
             "# the joints, seconds.  equal: status, range and boxes against the host statement (bit for bit without the Gaussian; gauss_ratio: the worst difference in",
             "# units of twice the Gaussian's bar, (2 r + 8) 2^-53 max|x|).",
             "# frames sequences kernel_size sigma pad device_us_median device_us_min device_us_max host_s interpolated_frames equal gauss_ratio"]
    g = np.random.Generator(np.random.Philox(key=[410, 7]))
    for n in (T, 10000):
        lengths = [T] * (n // T)
        kp = np.concatenate([walk(g, T) for _ in lengths])
        dev = torch.from_numpy(kp).cuda()
        off = np.zeros(len(lengths) + 1, np.int32)
        off[1:] = np.cumsum(lengths)
        boxes = torch.empty(n, 4, dtype=torch.float64, device="cuda")
        status = torch.empty(n, dtype=torch.int32, device="cuda")
        rng = torch.empty(len(lengths), 2, dtype=torch.int32, device="cuda")
        for kernel, sigma, pad in ((1, 0.0, "zero"), (11, 3.0, "edge")):
            def call():
                rc = m._lib.grnet_track_boxes(m._h, dev.data_ptr(), 25, off.ctypes.data_as(C.POINTER(C.c_int32)), len(lengths), tk.VIS_THRESH, kernel, sigma,
                                              pkg._lib.TRACK_PAD[pad], boxes.data_ptr(), status.data_ptr(), rng.data_ptr(), stream)
                assert rc == 0, m._lib.grnet_last_error(m._h)
            med, lo, hi = device_us(torch, call)
            out = {"boxes": boxes.cpu().numpy(), "status": status.cpu().numpy(), "range": rng.cpu().numpy()}
            t0 = time.perf_counter()
            host = pkg.pipeline.track_boxes(kp, lengths=lengths, vis_thresh=tk.VIS_THRESH, kernel_size=kernel, sigma=sigma, pad=pad, return_params=True)
            host_s = time.perf_counter() - t0
            equal = np.array_equal(out["status"], host["status"]) and np.array_equal(out["range"], host["range"])
            ratio = 0.0
            if sigma == 0:
                equal = equal and np.array_equal(out["boxes"].view(np.int64), host["boxes"].view(np.int64))
            else:
                before = pkg.pipeline.track_boxes(kp, lengths=lengths, vis_thresh=tk.VIS_THRESH, kernel_size=kernel, pad=pad, return_params=True)["params"]
                for q in range(len(lengths)):
                    a, b = off[q] + host["range"][q, 0], off[q] + host["range"][q, 1]
                    for c in (0, 1):
                        ratio = max(ratio, np.abs(out["boxes"][a:b, c] - host["boxes"][a:b, c]).max() / (2 * tk.gauss_bar(before[a:b, c], sigma)))
                    rel = 2 * tk.gauss_bar(before[a:b, 2], sigma) / host["params"][a:b, 2] + 2 * tk.U
                    ratio = max(ratio, (np.abs(out["boxes"][a:b, 2] - host["boxes"][a:b, 2]) / (rel * host["boxes"][a:b, 2])).max())
                equal = equal and ratio <= 1.0
            lines.append(f"{n} {len(lengths)} {kernel} {sigma:g} {pad} {med:.1f} {lo:.1f} {hi:.1f} {host_s:.3f} {int((out['status'] == 1).sum())} {bool(equal)} {ratio:.3g}")
            print(lines[-1], flush=True)
    m.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
