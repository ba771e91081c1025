"""Time of the pose metrics (grnet_pose_metrics, csrc/metric_kernels.hip) on one MI355X: 16, 400 and 10 000 frames of 25 kinectv2 joints
(root 0, sequences of 400 frames), alone and with V = 6890 vertices, inputs on the device.

  device   the C ABI call with every output, warm (scratch grown, code loaded): HIP events around REPS back-to-back calls, the median of WINDOWS
           such windows; us per call
  torch    the same statement in torch float64 on that GPU (batched torch.linalg.svd, norms and means; one sequence's worth of accelerations per
           sequence), timed the same way
  host     pipeline.pose_metrics after downloading the inputs (numpy float64): seconds, the median of 3 runs after a warm one (one run where the
           call takes more than 2 s)

The vertex stage moves 165 360 bytes per frame; its byte floor is that over the measured HBM copy rate of 6.29 TB/s.  Back-to-back calls on the
same 400 frames re-read 66 MB, which stay in the 256 MiB Infinity Cache; the `rotating` row walks 8 copies of the vertices (529 MB), so every call's
input comes from HBM, and 10 000 frames (1.65 GB) never fit.

    python tools/pose_metrics_time.py [out.txt]            # profiles/pose_metrics_times.txt
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
REPS, WINDOWS, T, V = 20, 7, 400, 6890
HBM_BYTES_PER_S = 6.29e12
FRAME_BYTES = 2 * V * 3 * 4


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


def host_s(fn):
    t = time.perf_counter()
    fn()
    warm = time.perf_counter() - t
    if warm > 2.0:
        return warm
    runs = []
    for _ in range(3):
        t = time.perf_counter()
        fn()
        runs.append(time.perf_counter() - t)
    return statistics.median(runs)


def torch_statement(torch, pred, gt, lengths, pv, gv):
    """DESIGN 4.8 in torch float64 on the device: root 0, all joints, unit 1000."""
    p, g = pred.double(), gt.double()
    P, G = p - p[:, :1], g - g[:, :1]
    mpjpe = (P - G).norm(dim=2).mean(dim=1)
    mu1, mu2 = P.mean(dim=1, keepdim=True), G.mean(dim=1, keepdim=True)
    X1, X2 = P - mu1, G - mu2
    var1 = (X1 * X1).sum(dim=(1, 2))
    K = X1.transpose(1, 2) @ X2
    U, S, Vh = torch.linalg.svd(K)
    Z = torch.eye(3, dtype=torch.float64, device=p.device).repeat(p.shape[0], 1, 1)
    Z[:, 2, 2] = torch.sign(torch.linalg.det(U @ Vh))
    R = Vh.transpose(1, 2) @ Z @ U.transpose(1, 2)
    s = (R @ K).diagonal(dim1=1, dim2=2).sum(dim=1) / var1
    t = mu2 - s[:, None, None] * (mu1 @ R.transpose(1, 2))
    pa = (s[:, None, None] * (P @ R.transpose(1, 2)) + t - G).norm(dim=2).mean(dim=1)
    cols = [mpjpe, pa]
    if pv is not None:
        cols.append((pv.double() - gv.double()).norm(dim=2).mean(dim=1))
    L = lengths[0]                                             # every sequence of a timed call has the same length
    Ps, Es = P.reshape(len(lengths), L, -1, 3), (P - G).reshape(len(lengths), L, -1, 3)
    accel = (Ps[:, :-2] - 2 * Ps[:, 1:-1] + Ps[:, 2:]).norm(dim=3).mean(dim=2)
    err = (Es[:, :-2] - 2 * Es[:, 1:-1] + Es[:, 2:]).norm(dim=3).mean(dim=2)
    per_seq = torch.stack([c.reshape(len(lengths), L).mean(dim=1) for c in cols] + [accel.mean(dim=1), err.mean(dim=1)], 1)
    return per_seq * 1000.0, torch.stack([c.mean() for c in cols] + [accel.mean(), err.mean()]) * 1000.0


def main():
    import torch
    pkg = importlib.import_module("video-based-gait-analysis-for-dementia_amd")
    assert torch.cuda.is_available(), "pose_metrics_time.py measures on the GPU: there is no CPU figure for the device call"
    m = pkg.GRNet(max_frames=1)                               # no weights: the metrics need none
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32p = C.POINTER(C.c_int32)
    root = (C.c_int32 * 1)(0)
    lines = [f"# grnet_pose_metrics on one MI355X: 25 joints, root 0, sequences of {T} frames (16 frames: one sequence of 16), every output, inputs on the device;",
             f"# us per call: HIP events around {REPS} back-to-back warm calls, median (min .. max) of {WINDOWS} windows.  torch: the same statement in torch float64 on",
             "# that GPU (batched torch.linalg.svd).  host: pipeline.pose_metrics after downloading the inputs, seconds.  floor: 165 360 bytes per frame over 6.29 TB/s.",
             "# frames vertices device_us_median device_us_min device_us_max torch_us_median host_s byte_floor_us multiple_of_floor total_equals_host_statement_to_1e-10"]
    g = torch.Generator(device="cuda").manual_seed(5)
    for n in (16, 400, 10000):
        lengths = [n] if n < T else [T] * (n // T)
        off = np.zeros(len(lengths) + 1, np.int32)
        off[1:] = np.cumsum(lengths)
        pred = torch.randn(n, 25, 3, device="cuda", generator=g) * 0.4
        gt = pred + torch.randn(n, 25, 3, device="cuda", generator=g) * 0.03
        for with_verts in (False, True):
            pv = torch.randn(n, V, 3, device="cuda", generator=g) * 0.5 if with_verts else None
            gv = pv + torch.randn(n, V, 3, device="cuda", generator=g) * 0.02 if with_verts else None
            per_frame = torch.empty(n, 5, dtype=torch.float64, device="cuda")
            per_seq = torch.empty(len(lengths), 5, dtype=torch.float64, device="cuda")
            total = torch.empty(5, dtype=torch.float64, device="cuda")

            def call(pv=pv, gv=gv):
                rc = m._lib.grnet_pose_metrics(m._h, pred.data_ptr(), gt.data_ptr(), 25, off.ctypes.data_as(i32p), len(lengths), None, 0, root, 1,
                                               pv.data_ptr() if pv is not None else None, gv.data_ptr() if gv is not None else None, V if pv is not None else 0,
                                               1000.0, per_frame.data_ptr(), per_seq.data_ptr(), total.data_ptr(), None, stream)
                assert rc == 0, m._lib.grnet_last_error(m._h)
            med, lo, hi = device_us(torch, call)
            got = total.cpu().numpy()
            tmed = device_us(torch, lambda: torch_statement(torch, pred, gt, lengths, pv, gv), reps=5 if n > T else REPS)[0]
            host = host_s(lambda: pkg.pipeline.pose_metrics(pred.cpu().numpy(), gt.cpu().numpy(), lengths=lengths, root=[0],
                                                            pred_verts=pv.cpu().numpy() if with_verts else None, gt_verts=gv.cpu().numpy() if with_verts else None))
            want = pkg.pipeline.pose_metrics(pred.cpu().numpy(), gt.cpu().numpy(), lengths=lengths, root=[0])["total"]
            keep = ~np.isnan(want)
            same = bool(np.array_equal(np.isnan(got[[0, 1, 3, 4]]), np.isnan(want[[0, 1, 3, 4]])) and np.allclose(got[keep], want[keep], rtol=1e-10, atol=0))
            floor = n * FRAME_BYTES / HBM_BYTES_PER_S * 1e6 if with_verts else float("nan")
            lines.append(f"{n} {V if with_verts else 0} {med:.1f} {lo:.1f} {hi:.1f} {tmed:.1f} {host:.4f} {floor:.2f} {med / floor if with_verts else float('nan'):.2f} {same}")
            print(lines[-1], flush=True)
            if with_verts and n == T:                          # every call's vertices from HBM: 8 copies, 529 MB, walked in turn
                copies = [(pv.clone(), gv.clone()) for _ in range(8)]
                turn = [0]

                def rotating():
                    a, b = copies[turn[0] % 8]
                    turn[0] += 1
                    call(a, b)
                med, lo, hi = device_us(torch, rotating)
                lines.append(f"{n} {V} {med:.1f} {lo:.1f} {hi:.1f} nan nan {floor:.2f} {med / floor:.2f} rotating_over_8_copies_of_the_vertices")
                print(lines[-1], flush=True)
                del copies
            del pv, gv
    m.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
