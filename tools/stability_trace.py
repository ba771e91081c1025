"""How long each of the two sequence kernels of the local dynamic stability takes (csrc/gait_stability_kernels.hip), from a kernel trace:
stability_time.py measures the whole call, this says which kernel the time is in.

  python tools/stability_trace.py                               # the workload: GRNet.op_gait_divergence with the default rule, CALLS times on one
                                                                # sequence of 400 standard-normal frames, then LONG_CALLS times on one of 32 768
  python tools/stability_trace.py --summarize TRACE.csv [out.txt]   # profiles/gait_stability_kernel_trace.txt from the trace's kernel rows

    rocprofv3 --kernel-trace --output-format csv -d DIR -o stab -- python tools/stability_trace.py
    python tools/stability_trace.py --summarize DIR/stab_kernel_trace.csv profiles/gait_stability_kernel_trace.txt
"""
import csv
import importlib
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

CALLS, LONG_CALLS, SHORT, LONG = 20, 3, 400, 32768
KERNELS = ("stab_nn_kernel", "stab_curve_kernel")


def workload():
    import numpy as np
    import torch
    pkg = importlib.import_module("video-based-gait-analysis-for-dementia_amd")
    assert torch.cuda.is_available(), "stability_trace.py runs the kernels: it needs the GPU"
    m = pkg.GRNet(max_frames=1)                               # no weights: the call needs none
    rng = np.random.default_rng(SHORT)
    for frames, calls in ((SHORT, CALLS), (LONG, LONG_CALLS)):
        x = torch.from_numpy(rng.standard_normal((frames, 4))).cuda()
        for _ in range(calls):
            m.op_gait_divergence(x)
        torch.cuda.synchronize()
    m.close()


def summarize(trace, out=None):
    took = {k: [] for k in KERNELS}
    with open(trace) as fh:
        for row in csv.DictReader(fh):
            for k in KERNELS:
                if k in row["Kernel_Name"]:
                    took[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    lines = ["# The two sequence kernels of grnet_op_gait_divergence (DESIGN 4.18) in ONE kernel trace on one MI355X (tools/stability_trace.py under rocprofv3",
             f"# --kernel-trace: the default rule, {CALLS} calls on one sequence of {SHORT} standard-normal frames, then {LONG_CALLS} on one of {LONG}): the duration of every launch",
             "# from its start and end timestamps, in us; ns_per_point: the median over the sequence's eligible points (E = frames - 28), the candidates a lane of",
             "# the search scans and the references the walk follows.  One run; a record, not a bar.  The first launch of a kernel includes loading its code.",
             "# kernel frames launches median_us min_us max_us ns_per_point"]
    for k in KERNELS:
        assert len(took[k]) == CALLS + LONG_CALLS, f"{k}: {len(took[k])} launches in {trace}, not {CALLS + LONG_CALLS}"
        for frames, part in ((SHORT, took[k][:CALLS]), (LONG, took[k][CALLS:])):
            med = statistics.median(part)
            lines.append(f"{k} {frames} {len(part)} {med:.1f} {min(part):.1f} {max(part):.1f} {med * 1e3 / (frames - 28):.0f}")
    print("\n".join(lines))
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(*sys.argv[2:4])
    else:
        workload()
