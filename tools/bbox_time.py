"""Time of the box from 2D joints (grnet_bbox_from_joints2d, csrc/bbox_kernels.hip) on one MI355X against the host statement on the
same machine: one 400-frame sequence, and 100 of them in one call (a database window of 50 videos with two candidate skeletons each).

  device   the C ABI call on joints already on the device, warm (scratch grown, code loaded): HIP events around REPS back-to-back calls, the
           median of WINDOWS such windows; us per call
  host     pipeline.bbox_from_joints2d (numpy float64, row blocks) per 400-frame sequence: the median of 3 runs after a warm one
  sklearn  where it imports: what the reference runs per sequence, euclidean_distances over the float32 points and the float64 argmin of the
           row sums (the stand-in for kmedoids.fasterpam, which only reads the matrix): the median of 3 runs after a warm one

    python tools/bbox_time.py [out.txt]            # profiles/bbox_from_joints2d_times.txt
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
REPS, WINDOWS, T = 20, 7, 400


def device_us(torch, call):
    call(); call()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            call()
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) / REPS * 1e3)
    return statistics.median(per_call), min(per_call), max(per_call)


def host_s(fn):
    fn()
    runs = []
    for _ in range(3):
        t = time.perf_counter()
        fn()
        runs.append(time.perf_counter() - t)
    return statistics.median(runs)


def main():
    import torch
    import make_goldens_bbox as mg
    pkg = importlib.import_module("video-based-gait-analysis-for-dementia_amd")
    assert torch.cuda.is_available(), "bbox_time.py measures on the GPU: there is no CPU figure for the device call"
    m = pkg.GRNet(max_frames=1)                               # no weights: the box needs none
    seqs = [mg.make_case(T, 100 + q, 620.0, None) for q in range(100)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = [f"# grnet_bbox_from_joints2d on one MI355X, sequences of {T} frames x 25 joints ({T * 25} points, {(T * 25) ** 2 / 1e6:.0f} M pairs each), joints on the device;",
             f"# us per call: HIP events around {REPS} back-to-back warm calls, median (min .. max) of {WINDOWS} windows.  host / sklearn: seconds per sequence on the same",
             "# machine's CPU, median of 3 runs after a warm one.",
             "# sequences device_us_median device_us_min device_us_max device_us_per_sequence last_box_equals_host_statement"]
    for n_seq in (1, 100):
        joints = torch.from_numpy(np.concatenate(seqs[:n_seq], 0)).cuda()
        off = (C.c_int32 * (n_seq + 1))(*[q * T for q in range(n_seq + 1)])
        box = torch.empty(n_seq, 4, dtype=torch.float64, device="cuda")

        def call():
            rc = m._lib.grnet_bbox_from_joints2d(m._h, joints.data_ptr(), 25, off, n_seq, 0.1, box.data_ptr(), None, stream)
            assert rc == 0, m._lib.grnet_last_error(m._h)
        med, lo, hi = device_us(torch, call)
        want = pkg.pipeline.bbox_from_joints2d(seqs[n_seq - 1])[0]
        same = bool(np.array_equal(box[n_seq - 1].cpu().numpy(), want))
        lines.append(f"{n_seq} {med:.1f} {lo:.1f} {hi:.1f} {med / n_seq:.2f} {same}")
        print(lines[-1], flush=True)
    m.close()
    host = host_s(lambda: pkg.pipeline.bbox_from_joints2d(seqs[0]))
    lines.append(f"host_statement_s_per_sequence {host:.3f}")
    print(lines[-1], flush=True)
    try:
        from sklearn.metrics.pairwise import euclidean_distances
        from tests.helpers import bbox_checks as bc
        points = bc.prepare(seqs[0])[0]
        sk = host_s(lambda: int(np.argmin(euclidean_distances(points).sum(axis=1, dtype=np.float64))))
        lines.append(f"sklearn_path_s_per_sequence {sk:.3f}")
    except ImportError:
        lines.append("sklearn_path_s_per_sequence not measured: sklearn does not import here")
    print(lines[-1], flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
