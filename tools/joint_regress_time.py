"""Time of grnet_regress_joints (csrc/joint_regress.hip) against what the reference executes, torch.matmul(J[None].expand(n,-1,-1), verts), and
the byte floor (n * 82 680 + table bytes) / 6.3 TB/s, on the vertices a real forward leaves: n = 16 and 400, 17-row dense and 17-row
sparse-32 tables, all 17 rows computed.  HIP events around 20 back-to-back calls after two warm ones (the convention of grnet_time_conv).
"warm": the 20 calls read the same vertices, which at 400 frames (33 MB) stay in the 256 MB Infinity Cache; "cold": they walk 10 copies
(331 MB at 400 frames), so each call's vertices come from HBM -- the figure the HBM byte floor is fair to.

    python tools/joint_regress_time.py [out.txt]                  # writes everything profiles/joint_regress_times.txt holds but the trace lines
    rocprofv3 --kernel-trace --output-format csv -d DIR -o jr -- python tools/joint_regress_time.py
    python tools/joint_regress_time.py --trace DIR/jr_kernel_trace.csv [out.txt]     # appends the per-kernel summary of that run to out.txt
"""
import csv
import ctypes as C
import importlib
import os
import sys

REPS, HBM, COPIES = 20, 6.3e12, 10


def trace_summary(path):
    """Median / min duration per (kernel, grid) of the two joint_regress kernels in a rocprofv3 kernel trace of this tool.  Dispatches are
    back to back there, so a kernel's start is its predecessor's end: each figure includes the dispatch gap."""
    rows = {}
    for r in csv.DictReader(open(path)):
        if "joint_regress" in r["Kernel_Name"]:
            name = "sum" if "sum_kernel" in r["Kernel_Name"] else "regress"
            key = (name, int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Grid_Size_Y"]))
            rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    lines = ["# kernel trace (rocprofv3 --kernel-trace of this tool; back-to-back dispatches, each figure includes the dispatch gap)",
             "# kernel workgroups_x workgroups_y dispatches median_us min_us"]
    for (name, gx, gy), d in sorted(rows.items()):
        d.sort()
        lines.append(f"trace {name} {gx} {gy} {len(d)} {d[len(d) // 2]:.1f} {d[0]:.1f}")
    return lines


def timed(torch, fn):
    fn(0); fn(1)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(REPS):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


def measure():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    pkg = importlib.import_module("video-based-gait-analysis-for-dementia_amd")
    lines = ["# grnet_regress_joints on one MI355X, fp32 handle, vertices of a real 400-frame forward, all 17 rows computed; us per call, HIP events",
             f"# around {REPS} back-to-back calls after two warm ones.  warm: every call reads the same vertices (Infinity-Cache resident at 400 frames);",
             f"# cold: the calls walk {COPIES} copies of them.  byte floor = (n * 82 680 + 17 * 6890 * 4) bytes / 6.3 TB/s of HBM.",
             "# n table op_warm_us op_cold_us torch_matmul_warm_us torch_matmul_cold_us byte_floor_us max_abs_diff_vs_matmul"]
    m = pkg.build_synthetic_model(max_frames=400, with_gru=False)
    frames = torch.from_numpy(pkg.synth.make_frames(16)).cuda().repeat(25, 1, 1, 1)
    frames += 0.05 * torch.randn(400, 1, 1, 1, generator=torch.Generator().manual_seed(pkg.synth.FRAME_SEED)).cuda()
    verts_all = m(frames)[-1]["verts"].reshape(400, 6890, 3).clone()
    del frames
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for label, nnz in (("dense17", None), ("sparse32x17", 32)):
        W = pkg.synth.make_joint_regressor(17, nnz=nnz, seed=77)
        m.set_joint_regressor(W, select=None)
        Jd = torch.from_numpy(W).cuda()
        for n in (16, 400):
            copies = [verts_all[:n].clone() for _ in range(COPIES)]
            out = torch.empty(n, 17, 3, device="cuda")
            ref = [None]

            def op(i, cold=False):
                rc = m._lib.grnet_regress_joints(m._h, copies[i % COPIES if cold else 0].data_ptr(), n, out.data_ptr(), stream)
                assert rc == 0, rc

            def mm(i, cold=False):
                ref[0] = torch.matmul(Jd[None].expand(n, -1, -1), copies[i % COPIES if cold else 0])
            us, us_cold = timed(torch, op), timed(torch, lambda i: op(i, True))
            us_mm, us_mm_cold = timed(torch, mm), timed(torch, lambda i: mm(i, True))
            floor = (n * 82680 + W.size * 4) / HBM * 1e6
            diff = float((out - ref[0]).abs().max())
            lines.append(f"{n} {label} {us:.1f} {us_cold:.1f} {us_mm:.1f} {us_mm_cold:.1f} {floor:.2f} {diff:.2e}")
            print(lines[-1], flush=True)
    m.close()
    return lines


def main():
    args = sys.argv[1:]
    if args and args[0] == "--trace":
        lines, out, mode = trace_summary(args[1]), args[2:], "a"
        print("\n".join(lines))
    else:
        lines, out, mode = measure(), args, "w"
    if out:
        with open(out[0], mode) as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
