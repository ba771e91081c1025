"""Time of the Welch spectrum of the gait signals (grnet_gait_spectrum, csrc/gait_spectrum_kernels.hip) on one MI355X: one call at 400
frames (one sequence) and at 10 000 frames in 25 sequences of 400, 25 joints, the walker of tests/helpers/regularity_checks.py at other periods, yaws
and phases with 5 mm of seeded noise on every joint coordinate, joints and translations on the device, the default rule (derivative 2, segments of
64 frames 32 apart, 256 points, the band 0.5 to 3 Hz), without smoothing (three launches).  grnet_gait_entropy is measured on the same inputs in the
same run: the call this one is compared with.  Then the hook alone on ONE sequence of 32 768 frames of noise, the longest a call takes, at the
defaults and at segments of 256 frames 32 apart with 1024 points.

  device      the C ABI call with its three outputs, warm (code loaded): HIP events around REPS back-to-back calls, the median (min .. max) of WINDOWS
              such windows; us
  welch       grnet_op_gait_welch alone on the call's own signals (the two sequence kernels and the upload, without the frame kernel): the same measure
  entropy     grnet_gait_entropy with its default rule (3 scales) on the same joints: the same measure
  host        pipeline.gait_spectrum after downloading the joints (numpy float64): seconds, one run
  equal       whether the device's psd, per_sequence and per_frame equal the host statement's in every bit

    python tools/spectrum_time.py [out.txt]        # profiles/gait_spectrum_times.txt
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
from tests.helpers import regularity_checks as rc  # noqa: E402
from tests.helpers import spectrum_checks as sc  # noqa: E402

REPS, WINDOWS, T, LONGEST = 20, 7, 400, 32768
RULE = (20.0, 2, 64, 32, 256, 0.5, 3.0, 2)                      # fps, derivative, segment, hop, nfft, f_lo, f_hi, min_segments
WIDE = (20.0, 2, 256, 32, 1024, 0.5, 3.0, 2)
ENT_RULE = (0.0, 2, 0.2, 2, 3)                                  # sigma, m, fraction, derivative, scales


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
    assert torch.cuda.is_available(), "spectrum_time.py measures on the GPU: there is no CPU figure for the device call"
    m = pkg.GRNet(max_frames=1)                               # no weights: the call needs none
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = [f"# grnet_gait_spectrum on one MI355X: 25 joints, sequences of {T} frames of the walker of tests/helpers/regularity_checks.py (its four periods by turns, every",
             f"# other one asymmetric) with 5 mm of Gaussian noise on every joint coordinate (seed {ec.SEED}), derivative {RULE[1]}, segments of {RULE[2]} frames {RULE[3]} apart,",
             f"# {RULE[4]} points, sigma 0 (three launches), three outputs, inputs on the device; us per call: HIP events around {REPS} back-to-back warm calls, median (min .. max) of",
             f"# {WINDOWS} windows.  welch_us: grnet_op_gait_welch alone on the call's signals, median.  entropy_us: grnet_gait_entropy (m 2, 3 scales, sigma 0) on the same joints in",
             "# the same run, median (min .. max).  host: pipeline.gait_spectrum after downloading the joints, seconds.  equal: every bit of psd, per_sequence and per_frame against",
             "# the host statement.  segments: the segments transformed per call, all channels.",
             "# frames sequences device_us_median device_us_min device_us_max welch_us entropy_us_median entropy_us_min entropy_us_max host_s segments mean_peak_hz_sep equal"]
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
        counts = torch.empty(len(lengths), 4, ENT_RULE[4], 3, dtype=torch.int64, device="cuda")
        ent_seq = torch.empty(len(lengths), 4, 4, dtype=torch.float64, device="cuda")
        psd = torch.empty(len(lengths), 4, RULE[4] // 2 + 1, dtype=torch.float64, device="cuda")
        per_seq = torch.empty(len(lengths), 4, 13, dtype=torch.float64, device="cuda")

        def entropy():
            rc_ = m._lib.grnet_gait_entropy(m._h, dev_j.data_ptr(), 25, offp, len(lengths), table, dev_t.data_ptr(), None, *ENT_RULE, per_frame.data_ptr(), counts.data_ptr(),
                                            ent_seq.data_ptr(), stream)
            assert rc_ == 0, m._lib.grnet_last_error(m._h)

        def call():
            rc_ = m._lib.grnet_gait_spectrum(m._h, dev_j.data_ptr(), 25, offp, len(lengths), table, dev_t.data_ptr(), None, RULE[0], 0.0, *RULE[1:], per_frame.data_ptr(),
                                             psd.data_ptr(), per_seq.data_ptr(), stream)
            assert rc_ == 0, m._lib.grnet_last_error(m._h)
        ent = device_us(torch, entropy)
        med, lo, hi = device_us(torch, call)
        out = {"per_frame": per_frame.cpu().numpy(), "psd": psd.cpu().numpy(), "per_sequence": per_seq.cpu().numpy()}
        signals = per_frame.clone()

        def hook():
            rc_ = m._lib.grnet_op_gait_welch(m._h, signals.data_ptr(), None, offp, len(lengths), *RULE, psd.data_ptr(), per_seq.data_ptr(), stream)
            assert rc_ == 0, m._lib.grnet_last_error(m._h)
        hook_us = device_us(torch, hook)[0]
        t0 = time.perf_counter()
        host = pkg.pipeline.gait_spectrum(joints, lengths, trans, **sc.RULE)
        host_s = time.perf_counter() - t0
        equal = all(sc.same_bits(out[k], host[k]) for k in ("per_frame", "psd", "per_sequence"))
        lines.append(f"{n} {len(lengths)} {med:.1f} {lo:.1f} {hi:.1f} {hook_us:.1f} {ent[0]:.1f} {ent[1]:.1f} {ent[2]:.1f} {host_s:.3f} {int(host['per_sequence'][:, :, 2].sum())} "
                     f"{np.nanmean(host['per_sequence'][:, 0, 6]):.4f} {bool(equal)}")
        print(lines[-1], flush=True)
    lines += [f"# grnet_op_gait_welch on ONE sequence of {LONGEST} frames of seeded standard-normal noise on the four channels, the longest a call takes: us per call as above;",
              "# workgroups: the grid of the density kernel, one wave each.",
              "# frames segment hop nfft welch_us_median welch_us_min welch_us_max workgroups host_s equal"]
    x = np.random.default_rng(LONGEST).standard_normal((LONGEST, 4))
    signals = torch.from_numpy(x).cuda()
    off = np.array([0, LONGEST], np.int32)
    offp = off.ctypes.data_as(C.POINTER(C.c_int32))
    for rule in (RULE, WIDE):
        psd = torch.empty(1, 4, rule[4] // 2 + 1, dtype=torch.float64, device="cuda")
        per_seq = torch.empty(1, 4, 13, dtype=torch.float64, device="cuda")

        def long_hook():
            rc_ = m._lib.grnet_op_gait_welch(m._h, signals.data_ptr(), None, offp, 1, *rule, psd.data_ptr(), per_seq.data_ptr(), stream)
            assert rc_ == 0, m._lib.grnet_last_error(m._h)
        med, lo, hi = device_us(torch, long_hook, reps=5)
        t0 = time.perf_counter()
        host = pkg.pipeline.gait_welch(x, fps=rule[0], derivative=rule[1], segment=rule[2], hop=rule[3], nfft=rule[4], f_lo=rule[5], f_hi=rule[6], min_segments=rule[7])
        host_s = time.perf_counter() - t0
        equal = sc.same_bits(psd.cpu().numpy(), host["psd"]) and sc.same_bits(per_seq.cpu().numpy(), host["per_sequence"])
        lines.append(f"{LONGEST} {rule[2]} {rule[3]} {rule[4]} {med:.1f} {lo:.1f} {hi:.1f} {4 * ((rule[4] // 2 + 1 + 63) // 64)} {host_s:.3f} {bool(equal)}")
        print(lines[-1], flush=True)
    m.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
