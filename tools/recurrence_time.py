"""Time of the recurrence quantification of the gait signals (grnet_gait_recurrence, csrc/gait_recurrence_kernels.hip) on one MI355X:
one call at 400 frames (one sequence) and at 10 000 frames in 25 sequences of 400, 25 joints, the walker of tests/helpers/regularity_checks.py at
other periods, yaws and phases with 5 mm of seeded noise on every joint coordinate, joints and translations on the device, the default rule
(derivative 1, dim 5, lag 2, theiler 8, radius 0.8), without smoothing (four launches).  grnet_gait_stability is measured on the same joints in the
same run: the call this one is compared with.

  device      the C ABI call with its four outputs, warm (code loaded): HIP events around REPS back-to-back calls, the median (min .. max) of WINDOWS
              such windows; us
  counts      grnet_op_gait_recurrence_counts alone on the call's own signals (the three sequence kernels and the upload, without the frame kernel):
              the same measure
  stability   grnet_gait_stability with its default rule on the same joints: the same measure
  host        pipeline.gait_recurrence after downloading the joints (numpy float64, a diagonal at a time): seconds, one run
  equal       whether the device's counts and hist equal the host statement's in every integer and its per_sequence and per_frame in every bit
  longest     the hook alone on ONE sequence of 32 768 standard-normal frames, the most a call takes: 16 parts a channel, four rounds of offsets a
              lane; median of WINDOWS windows of 3 calls; not compared with the statement, which would take an hour there, but held to rule 6's
              invariant

    python tools/recurrence_time.py [out.txt]        # profiles/gait_recurrence_times.txt
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
from tests.helpers import entropy_checks as ec  # noqa: E402
from tests.helpers import gait_checks as gc  # noqa: E402
from tests.helpers import recurrence_checks as kc  # noqa: E402
from tests.helpers import regularity_checks as rc  # noqa: E402

REPS, WINDOWS, T = 20, 7, 400
RULE = (1, 5, 2, 8, 0.8)                                        # derivative, dim, lag, theiler, radius
STAB_RULE = (1, 5, 2, 20, 20)                                   # derivative, dim, lag, theiler, horizon
LONGEST = 32768


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
    assert torch.cuda.is_available(), "recurrence_time.py measures on the GPU: there is no CPU figure for the device call"
    m = pkg.GRNet(max_frames=1)                               # no weights: the call needs none
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    K = STAB_RULE[4]
    lines = [f"# grnet_gait_recurrence on one MI355X: 25 joints, sequences of {T} frames of the walker of tests/helpers/regularity_checks.py (its four periods by turns, every",
             f"# other one asymmetric) with 5 mm of Gaussian noise on every joint coordinate (seed {ec.SEED}), derivative {RULE[0]}, dim {RULE[1]}, lag {RULE[2]}, theiler {RULE[3]},",
             f"# radius {RULE[4]}, sigma 0 (four launches), four outputs, inputs on the device; us per call: HIP events around {REPS} back-to-back warm calls, median (min .. max)",
             f"# of {WINDOWS} windows.  counts_us: grnet_op_gait_recurrence_counts alone on the call's signals, median.  stability_us: grnet_gait_stability (derivative 1, dim 5,",
             "# lag 2, theiler 20, horizon 20, sigma 0) on the same joints in the same run, median (min .. max).  host: pipeline.gait_recurrence after downloading the joints,",
             "# seconds.  equal: every integer of counts and hist and every bit of per_sequence and per_frame against the host statement.  pairs: the D2 computed per call, all",
             "# channels.  ONE RUN; a record, not a bar.",
             "# frames sequences device_us_median device_us_min device_us_max counts_us stability_us_median stability_us_min stability_us_max host_s pairs "
             "mean_rate_sep mean_determinism_sep equal"]
    table = (C.c_int32 * 8)(*gc.KINECTV2)
    for n in (T, 10000):
        lengths = [T] * (n // T)
        made = [rc.walker(T, rc.PERIODS[q % 4], 0.3 * (q % 2), 0.37 * q, 0.6137 * q) for q in range(len(lengths))]
        joints, trans = np.concatenate([j for j, _ in made]), np.concatenate([t for _, t in made])
        joints = (joints + ec.NOISE * np.random.default_rng(ec.SEED).standard_normal(joints.shape)).astype(np.float32)
        dev_j, dev_t = torch.from_numpy(joints).cuda(), torch.from_numpy(trans).cuda()
        off = np.zeros(len(lengths) + 1, np.int32)
        off[1:] = np.cumsum(lengths)
        offp = off.ctypes.data_as(C.POINTER(C.c_int32))
        per_frame = torch.empty(n, 4, dtype=torch.float64, device="cuda")
        nn = torch.empty(n, 4, dtype=torch.int32, device="cuda")
        pairs = torch.empty(len(lengths), 4, K + 1, 2, dtype=torch.int64, device="cuda")
        mant = torch.empty(len(lengths), 4, K + 1, dtype=torch.float64, device="cuda")
        per_seq = torch.empty(len(lengths), 4, 5, dtype=torch.float64, device="cuda")
        hist = torch.empty(len(lengths), 4, 255, dtype=torch.int64, device="cuda")
        counts = torch.empty(len(lengths), 4, 6, dtype=torch.int64, device="cuda")

        def stability():
            rc_ = m._lib.grnet_gait_stability(m._h, dev_j.data_ptr(), 25, offp, len(lengths), table, dev_t.data_ptr(), None, 0.0, *STAB_RULE, per_frame.data_ptr(), nn.data_ptr(),
                                              pairs.data_ptr(), mant.data_ptr(), stream)
            assert rc_ == 0, m._lib.grnet_last_error(m._h)

        def call():
            rc_ = m._lib.grnet_gait_recurrence(m._h, dev_j.data_ptr(), 25, offp, len(lengths), table, dev_t.data_ptr(), None, 0.0, *RULE, per_frame.data_ptr(), per_seq.data_ptr(),
                                               hist.data_ptr(), counts.data_ptr(), stream)
            assert rc_ == 0, m._lib.grnet_last_error(m._h)
        stab = device_us(torch, stability)
        med, lo, hi = device_us(torch, call)
        out = {"per_frame": per_frame.cpu().numpy(), "per_sequence": per_seq.cpu().numpy(), "hist": hist.cpu().numpy(), "counts": counts.cpu().numpy()}
        signals = per_frame.clone()

        def hook():
            rc_ = m._lib.grnet_op_gait_recurrence_counts(m._h, signals.data_ptr(), None, offp, len(lengths), *RULE, per_seq.data_ptr(), hist.data_ptr(), counts.data_ptr(), stream)
            assert rc_ == 0, m._lib.grnet_last_error(m._h)
        hook_us = device_us(torch, hook)[0]
        t0 = time.perf_counter()
        host = pkg.pipeline.gait_recurrence(joints, lengths, trans, **kc.rule_of(*RULE))
        host_s = time.perf_counter() - t0
        equal = kc.same_ints(out["counts"], host["counts"]) and kc.same_ints(out["hist"], host["hist"]) and all(kc.same_bits(out[k], host[k]) for k in ("per_frame", "per_sequence"))
        M = T - (RULE[1] - 1) * RULE[2]
        lines.append(f"{n} {len(lengths)} {med:.1f} {lo:.1f} {hi:.1f} {hook_us:.1f} {stab[0]:.1f} {stab[1]:.1f} {stab[2]:.1f} {host_s:.3f} {4 * (M * (M - 1) // 2) * len(lengths)} "
                     f"{np.nanmean(host['recurrence_rate'][:, 0]):.4f} {np.nanmean(host['determinism'][:, 0]):.4f} {bool(equal)}")
        print(lines[-1], flush=True)
    x = torch.from_numpy(np.random.default_rng(LONGEST).standard_normal((LONGEST, 4))).cuda()
    off = np.array([0, LONGEST], np.int32)
    offp = off.ctypes.data_as(C.POINTER(C.c_int32))
    per_seq = torch.empty(1, 4, 5, dtype=torch.float64, device="cuda")
    hist = torch.empty(1, 4, 255, dtype=torch.int64, device="cuda")
    counts = torch.empty(1, 4, 6, dtype=torch.int64, device="cuda")

    def longest():
        rc_ = m._lib.grnet_op_gait_recurrence_counts(m._h, x.data_ptr(), None, offp, 1, *RULE, per_seq.data_ptr(), hist.data_ptr(), counts.data_ptr(), stream)
        assert rc_ == 0, m._lib.grnet_last_error(m._h)
    med, lo, hi = device_us(torch, longest, reps=3)
    M = LONGEST - (RULE[1] - 1) * RULE[2]
    got = counts.cpu().numpy()
    lines.append(f"# longest: grnet_op_gait_recurrence_counts on one sequence of {LONGEST} standard-normal frames, the same rule: {med:.0f} us ({lo:.0f} .. {hi:.0f}), "
                 f"{4 * (M * (M - 1) // 2)} pairs, {int(got[0, 0, 1])} comparable and {int(got[0, 0, 2])} recurrent on the first channel, invariant "
                 f"{kc.invariant(hist.cpu().numpy(), got)}; not compared with the statement")
    print(lines[-1], flush=True)
    m.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
