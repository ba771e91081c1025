"""Time of the --smooth step (row f3): the device path (GRNet.smooth_pose = grnet_smooth_pose: One-Euro filter, Rodrigues, SMPL, 49 joints)
against the host path (pipeline.smooth_pose: Python filter loop, numpy Rodrigues, upload, grnet_smpl_forward in chunks, download, host einsum
for the extra joints), which this commit leaves exactly as its parent had it, at T = 64, 400 and 10 000 frames on a max_frames = 400 handle.

    device_events_ms   HIP events around one GRNet.smooth_pose call on a device-resident theta (T,85), vertices staying on the device
    device_wall_ms     host clock from the device-resident theta to host-resident verts, pose, joints3d (the call + three downloads)
    host_wall_ms       host clock around pipeline.smooth_pose on the host-resident pose / betas the parent's run_tracklet had downloaded
                       (its own uploads and downloads included; the download of the first pass's results that it needed is NOT charged to it)
    filter_ns_per_frame  HIP events around grnet_op_one_euro alone, per frame
Medians of REPS runs after a warm one (3 runs at 10 000 frames for the wall clocks).  The speed condition: device_wall_ms < host_wall_ms at
every size.

    python tools/smooth_time.py [profiles/smooth_times.txt]
"""
import ctypes as C
import importlib
import os
import statistics
import sys
import time

REPS = 10
SIZES = (64, 400, 10000)


def main():
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    pkg = importlib.import_module("video-based-gait-analysis-for-dementia_amd")
    pipe = pkg.pipeline
    assert torch.cuda.is_available(), "smooth_time.py measures on the GPU; there is no CPU figure to report"
    tables = pkg.synth.make_smpl_tables()
    m = pkg.build_synthetic_model(max_frames=400, with_gru=False, compact_arena=True)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = ["# --smooth on one MI355X, fp32 handle, max_frames 400, synthetic SMPL tables, random-walk pose (0.03 per step); ms, medians (tools/smooth_time.py)",
             "# device_events: GRNet.smooth_pose on a device theta, verts left on the device; device_wall: theta on the device -> verts, pose, joints3d on the host;",
             "# host_wall: pipeline.smooth_pose (unchanged from the parent commit) on host pose / betas, its transfers included; ratio = host_wall / device_wall",
             "# T device_events_ms device_wall_ms host_wall_ms ratio filter_us filter_ns_per_frame max_abs_pose_diff rel_verts_diff"]
    for T in SIZES:
        g = np.random.Generator(np.random.Philox(key=[T, 1]))
        pose = (g.uniform(-1, 1, (1, 72)) + np.cumsum(g.standard_normal((T, 72)) * 0.03, axis=0)).astype(np.float32)
        betas = (g.standard_normal((T, 10)) * 0.5).astype(np.float32)
        cam = np.ones((T, 3), np.float32)
        theta = torch.from_numpy(np.concatenate([cam, pose, betas], 1)).cuda()
        reps = REPS if T <= 400 else 3

        def device(download):
            out = m.smooth_pose(theta, theta[:, 75:])
            return tuple(t.cpu().numpy() for t in out) if download else out

        def host():
            return pipe.smooth_pose(m, pose, betas, smpl_tables=tables)

        def wall(fn):
            fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            return statistics.median(ts)

        def events(fn):
            fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(REPS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                keep = fn()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
                del keep
            return statistics.median(ts)

        xhat = torch.empty(T, 72, device="cuda")

        def filt():
            rc = m._lib.grnet_op_one_euro(m._h, theta.data_ptr() + 12, 85, T, 0.004, 0.7, 1.0, xhat.data_ptr(), stream)
            assert rc == 0, rc

        dv, dp, dj = device(True)
        hv, hp, hj = host()
        pose_diff = float(np.abs(dp - hp).max())
        verts_diff = float(np.abs(dv - hv).max() / np.abs(hv).max())
        del dv, hv
        ev, dw, hw, fl = events(lambda: device(False)), wall(lambda: device(True)), wall(host), events(filt)
        lines.append(f"{T} {ev:.3f} {dw:.2f} {hw:.2f} {hw / dw:.2f} {fl * 1e3:.1f} {fl * 1e6 / T:.1f} {pose_diff:.2e} {verts_diff:.2e}")
        print(lines[-1], flush=True)
    m.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
