"""Time of arm swing and inter-limb coordination (grnet_gait_coordination, csrc/gait_coordination_kernels.hip) on one MI355X: one call at
400 frames (one sequence) and at 10 000 frames in 25 sequences of 400, 25 joints, the articulated walker of tests/helpers/kinematics_checks.py
(arm_right = 0.6) at other yaws and phases with 5 mm of seeded noise on every joint coordinate, joints on the device, the default rule (derivative 0,
segments of 64 frames 32 apart, 256 points, the band 0.5 to 3 Hz, at least 4 segments), without smoothing (three launches).  grnet_gait_spectrum is
measured on the same joints in the same run: the call whose twiddle gather this one pays once for four channels and ten spectra.  Then the hook alone
on ONE sequence of 32 768 frames of noise, the longest a call takes, at the defaults.

  device      the C ABI call with its five outputs, warm (code loaded): HIP events around REPS back-to-back calls, the median (min .. max) of WINDOWS
              such windows; us
  hook        grnet_op_gait_cross_welch alone on the call's own signals (the two sequence kernels and the upload, without the frame kernel): the same
  spectrum    grnet_gait_spectrum with its default rule on the same joints (its own 8-joint table, no translation): the same measure
  host        pipeline.gait_coordination after downloading the joints (numpy float64): seconds, one run
  equal       whether the device's per_frame, auto, cross, limbs and pairs equal the host statement's in every bit

    python tools/coordination_time.py [out.txt]        # profiles/gait_coordination_times.txt
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
from tests.helpers import coordination_checks as cc  # noqa: E402
from tests.helpers import gait_checks as gc  # noqa: E402
from tests.helpers import kinematics_checks as kc  # noqa: E402

REPS, WINDOWS, T, LONGEST = 20, 7, 400, 32768
RULE = (20.0, 0, 64, 32, 256, 0.5, 3.0, 4)                      # fps, derivative, segment, hop, nfft, f_lo, f_hi, min_segments
SPEC_RULE = (20.0, 2, 64, 32, 256, 0.5, 3.0, 2)
KEYS = ("auto", "cross", "limbs", "pairs")


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


def outputs(torch, n_seq, nfft):
    bins = nfft // 2 + 1
    return {"auto": torch.empty(n_seq, 4, bins, dtype=torch.float64, device="cuda"), "cross": torch.empty(n_seq, 6, bins, 2, dtype=torch.float64, device="cuda"),
            "limbs": torch.empty(n_seq, 4, 13, dtype=torch.float64, device="cuda"), "pairs": torch.empty(n_seq, 6, 10, dtype=torch.float64, device="cuda")}


def main():
    import torch
    pkg = importlib.import_module("video-based-gait-analysis-for-dementia_amd")
    assert torch.cuda.is_available(), "coordination_time.py measures on the GPU: there is no CPU figure for the device call"
    m = pkg.GRNet(max_frames=1)                               # no weights: the call needs none
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = [f"# grnet_gait_coordination on one MI355X: 25 joints, sequences of {T} frames of the articulated walker of tests/helpers/kinematics_checks.py (arm_right 0.6, other",
             f"# yaws and phases) with 5 mm of Gaussian noise on every joint coordinate (seed {cc.SEED}), derivative {RULE[1]}, segments of {RULE[2]} frames {RULE[3]} apart, {RULE[4]} points,",
             f"# at least {RULE[7]} segments, sigma 0 (three launches), five outputs, inputs on the device; us per call: HIP events around {REPS} back-to-back warm calls, median (min ..",
             f"# max) of {WINDOWS} windows.  hook_us: grnet_op_gait_cross_welch alone on the call's signals, median.  spectrum_us: grnet_gait_spectrum (derivative 2, the same",
             "# segments, sigma 0, no translation) on the same joints in the same run, median (min .. max).  host: pipeline.gait_coordination after downloading the joints,",
             "# seconds.  equal: every bit of per_frame, auto, cross, limbs and pairs against the host statement.  segments: the segments transformed per call (each for four",
             "# channels).",
             "# frames sequences device_us_median device_us_min device_us_max hook_us spectrum_us_median spectrum_us_min spectrum_us_max host_s segments mean_coherence_arms equal"]
    table16, table8 = (C.c_int32 * 16)(*kc.KINECTV2), (C.c_int32 * 8)(*gc.KINECTV2)
    for n in (T, 10000):
        lengths = [T] * (n // T)
        joints = np.concatenate([kc.walker(T, 0.3 * (q % 5) - 0.5, 21.7, -3.02 + 0.37 * q, arm_right=0.6)[0] for q in range(len(lengths))])
        joints = (joints.astype(np.float64) + cc.NOISE * np.random.default_rng(cc.SEED).standard_normal(joints.shape)).astype(np.float32)
        dev_j = torch.from_numpy(joints).cuda()
        off = np.zeros(len(lengths) + 1, np.int32)
        off[1:] = np.cumsum(lengths)
        offp = off.ctypes.data_as(C.POINTER(C.c_int32))
        per_frame = torch.empty(n, 4, dtype=torch.float64, device="cuda")
        reg_frame = torch.empty(n, 4, dtype=torch.float64, device="cuda")
        psd = torch.empty(len(lengths), 4, SPEC_RULE[4] // 2 + 1, dtype=torch.float64, device="cuda")
        per_seq = torch.empty(len(lengths), 4, 13, dtype=torch.float64, device="cuda")
        out = outputs(torch, len(lengths), RULE[4])

        def spectrum():
            rc_ = m._lib.grnet_gait_spectrum(m._h, dev_j.data_ptr(), 25, offp, len(lengths), table8, None, None, SPEC_RULE[0], 0.0, *SPEC_RULE[1:], reg_frame.data_ptr(),
                                             psd.data_ptr(), per_seq.data_ptr(), stream)
            assert rc_ == 0, m._lib.grnet_last_error(m._h)

        def call():
            rc_ = m._lib.grnet_gait_coordination(m._h, dev_j.data_ptr(), 25, offp, len(lengths), table16, None, RULE[0], 0.0, *RULE[1:], per_frame.data_ptr(),
                                                 *(out[k].data_ptr() for k in KEYS), stream)
            assert rc_ == 0, m._lib.grnet_last_error(m._h)
        spec = device_us(torch, spectrum)
        med, lo, hi = device_us(torch, call)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        got["per_frame"] = per_frame.cpu().numpy()
        signals = per_frame.clone()

        def hook():
            rc_ = m._lib.grnet_op_gait_cross_welch(m._h, signals.data_ptr(), None, offp, len(lengths), *RULE, *(out[k].data_ptr() for k in KEYS), stream)
            assert rc_ == 0, m._lib.grnet_last_error(m._h)
        hook_us = device_us(torch, hook)[0]
        t0 = time.perf_counter()
        host = pkg.pipeline.gait_coordination(joints, lengths, joints=kc.KINECTV2, **cc.RULE)
        host_s = time.perf_counter() - t0
        equal = all(cc.same_bits(got[k], host[k]) for k in KEYS + ("per_frame",))
        lines.append(f"{n} {len(lengths)} {med:.1f} {lo:.1f} {hi:.1f} {hook_us:.1f} {spec[0]:.1f} {spec[1]:.1f} {spec[2]:.1f} {host_s:.3f} {int(host['limbs'][:, 0, 2].sum())} "
                     f"{np.nanmean(host['pairs'][:, 0, 4]):.4f} {bool(equal)}")
        print(lines[-1], flush=True)
    lines += [f"# grnet_op_gait_cross_welch on ONE sequence of {LONGEST} frames of seeded standard-normal noise on the four channels, the longest a call takes: us per call as",
              "# above; workgroups: the grid of the density kernel, one wave each; mean_coherence_band: of the six pairs of unrelated signals, about 1 / segments.",
              "# frames segment hop nfft hook_us_median hook_us_min hook_us_max workgroups host_s segments mean_coherence_band equal"]
    x = np.random.default_rng(LONGEST).standard_normal((LONGEST, 4))
    signals = torch.from_numpy(x).cuda()
    off = np.array([0, LONGEST], np.int32)
    offp = off.ctypes.data_as(C.POINTER(C.c_int32))
    out = outputs(torch, 1, RULE[4])

    def long_hook():
        rc_ = m._lib.grnet_op_gait_cross_welch(m._h, signals.data_ptr(), None, offp, 1, *RULE, *(out[k].data_ptr() for k in KEYS), stream)
        assert rc_ == 0, m._lib.grnet_last_error(m._h)
    med, lo, hi = device_us(torch, long_hook, reps=5)
    t0 = time.perf_counter()
    host = pkg.pipeline.gait_cross_welch(x, **cc.RULE)
    host_s = time.perf_counter() - t0
    equal = all(cc.same_bits(out[k].cpu().numpy(), host[k]) for k in KEYS)
    lines.append(f"{LONGEST} {RULE[2]} {RULE[3]} {RULE[4]} {med:.1f} {lo:.1f} {hi:.1f} {(RULE[4] // 2 + 1 + 63) // 64} {host_s:.3f} {int(host['limbs'][0, 0, 2])} "
                 f"{host['pairs'][0, :, 8].mean():.5f} {bool(equal)}")
    print(lines[-1], flush=True)
    m.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
