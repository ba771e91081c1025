#!/usr/bin/env python3
"""batch_generation.py of the MI355X-native path: 3D-joint generation over a folder of videos with
precomputed bounding boxes, writing the reference's joblib "json" database
{'vid_name': (F,), 'bbox': (F,4) f32, 'joints3D': (F,25,3) f32 kinectv2} every 50 videos
(reference: batch_generation.py:180-287 prepare_data, :289-371 run_grnet_on_frame, argparse :373-387).

The boxes come from --bbox_path (a joblib file, as the reference's prepare_data wants it) or are made here from a folder of OpenPose .mat
files (--openpose_folder: the reference's load_openpose_anno, batch_generation.py:39-178, with the K-medoids centre on the GPU).

--gt_path FILE (opt-in) compares the joints with ground truth in this script's own output schema and reports MPJPE, PA-MPJPE, acceleration and
acceleration error per video in millimetres (GRNet.pose_metrics on the device; the reference has no evaluation code).

--trajectory (opt-in, with --openpose_folder and --vid_folder) fits the camera-space translation of every frame to the OpenPose 2D joints the
boxes were made from (GRNet.fit_translation on the device, DESIGN 4.9: SPIN's weighted least squares, the reference's estimate_translation_np) and
adds 'trans', 'trans_status' and 'reproj' to the database; the camera is an assumption, see --focal_length.

--bbox_track (opt-in, with --openpose_folder) makes one box PER FRAME for the chosen person of each video instead of the one fixed box, as the
reference's Inference(joints2d=...) does (lib/utils/smooth_bbox.py; GRNet.track_boxes on the device): the gaps without a detection
are interpolated, the frames before the first and after the last detection are dropped, --bbox_smooth adds the median and the Gaussian, and the
database gains 'bbox_status'.

--gait (opt-in, with --vid_folder) reads heel strikes, toe-offs and the gait parameters of every video off its 3D joints -- cadence, step and stride
time with their variability, step length and width, stance share, walking speed (GRNet.gait_parameters on the device, DESIGN 4.11: the
coordinate-based events of Zeni, Richards and Higginson 2008) -- writes them to <outpath>_gait.json and adds 'gait_events' to the database; with
--trajectory the speed along the fitted trajectory as well.

--gait_kinematics (opt-in, with --gait) adds the other half of what a gait lab reads off a walk: hip, knee, ankle, shoulder and elbow angles and the
trunk's inclination, cut at the heel strikes --gait found, put on 0 to 100 % of the gait cycle and averaged over the strides, with each joint's range
of motion and its left / right symmetry (GRNet.gait_kinematics on the device) -- in <outpath>_kinematics.json.  The numbers are
reported, never judged; the trunk's inclination assumes a level camera.

--gait_turns (opt-in, with --gait) finds where the subject turns round -- runs of the pelvis' yaw rate in the camera's horizontal plane that are fast,
long and wide enough (GRNet.gait_turns on the device; the thresholds follow El-Gohary et al. 2014 and are unvalidated on the model's
output) -- and makes the step and stride columns of --gait again over the intervals that are wholly straight walking: <outpath>_turns.json, and
'gait_phase' in the database.  Reported, never judged; the heading assumes a level camera.

--gait_contacts (opt-in, with --gait) finds when both feet are on the ground -- low runs of the speed of the vector from one ankle to the other, which
does not depend on the root and stands still while both feet do, their edges placed between frames, each run led by the foot whose heel strike --gait
found beside it (GRNet.gait_contacts on the device; the thresholds are unvalidated on the model's output, and smoothing shortens the
runs) -- and from them double-support, single-support, swing and stance time: <outpath>_contacts.json, and 'gait_support' in the database.
Reported, never judged.

--gait_regularity (opt-in, needs no --gait) reads step and stride regularity, their ratio -- a symmetry figure -- and a cadence off the autocorrelation of
four body signals (the ankles' separation along the facing and along the trunk, the trunk's lean, the pelvis' height), with no events at all
(GRNet.gait_regularity on the device; Moe-Nilssen and Helbostad 2004 on trunk accelerations; the defaults are unvalidated on the model's
output): <outpath>_regularity.json.  The line prints its cadence beside --gait's: where the two disagree, the event rule failed on that video or the
walk is not periodic.  With --gait_turns only straight walking counts.  Reported, never judged.

--gait_harmonics (opt-in, with --gait) cuts the same four body signals at the heel strikes --gait found and reports the harmonic ratio of every
stride -- the sum of the odd harmonics of its DFT over the sum of the even ones, or the inverse for the pelvis' height, which repeats every step --
and its bounded form in percent (GRNet.gait_harmonics on the device; Smidt et al. 1971, Menz et al. 2003 and Bellanca et al. 2013 on
trunk accelerations; the defaults are unvalidated on the model's output): <outpath>_harmonics.json.  With --gait_turns only straight strides count.
Reported, never judged.

--gait_entropy (opt-in, needs no --gait) reports how predictable the same four body signals are from one moment to the next: their sample entropy
(Richman and Moorman 2000), at several scales (Costa et al. 2002) and summed to a complexity index, as the cognitive-impairment gait studies report
it on a trunk accelerometer (Lamoth et al. 2011).  The device counts the matching pairs of templates (GRNet.gait_entropy); the
logarithm is pipeline.entropy_rows'.  <outpath>_entropy.json.  These signals are joint positions of a pose model, 400 frames at 20 fps are at the
short end of what the measure tolerates (Yentes et al. 2013), differencing twice amplifies joint noise, and the defaults are unvalidated on the model's
output.  With --gait_turns only straight walking counts.  Reported, never judged.

--gait_stability (opt-in, needs no --gait) reports the local dynamic stability of the same four body signals: the rate at which neighbouring states
of the delay-embedded signal diverge over the next frames, the short-term largest Lyapunov exponent of Rosenstein, Collins and De Luca (1993) that
the gait literature reports beside variability, harmonic ratio and entropy (Dingwell and Cusumano 2000, Lamoth et al. 2011, Bruijn et al. 2013).
The device finds every state's nearest neighbour and multiplies up the distances k frames later as a mantissa with an integer exponent
(GRNet.gait_stability); the logarithm and the slope are pipeline.stability_rows'.  <outpath>_stability.json.  The papers use a trunk
sensor and 100 and more strides; these are joint positions of a pose model, 400 frames at 20 fps hold some 15 strides, on a walker with 5 mm of joint
noise the divergence curve saturates within about 5 frames, so that the slope mostly measures the noise, and the defaults are unvalidated on the
model's output.  With --gait_turns only straight walking counts.  Reported, never judged.

--gait_spectrum (opt-in, needs no --gait) reports the frequency domain of the same four body signals: their Welch power spectral density (Welch
1967) and, in the band 0.5 to 3 Hz, the dominant frequency, the height and the width of that peak, how the power is spread and a third cadence
beside the events' and the autocorrelation's, as the gait accelerometry studies read them off a trunk sensor (Weiss et al. 2011, Sejdic et al.
2014).  The device averages the windowed, zero-padded transforms of the segments (GRNet.gait_spectrum); the logarithm of the
spectral entropy is pipeline.spectrum_rows'.  <outpath>_spectrum.json.  These signals are joint positions of a pose model; at 20 fps and 64-frame
segments the Hann window alone makes the peak about 0.45 Hz wide at half height, so the width has a floor set by the segment and not by the
walker, and the defaults are unvalidated on the model's output.  With --gait_turns a turn splits the walk into straight runs.  Reported, never
judged.

--gait_smoothness (opt-in, needs no --gait) reports the movement smoothness of the same four body signals, per segment of ongoing walking: the
spectral arc length (SPARC) of the speed profile's zero-padded magnitude spectrum and the log dimensionless jerk (LDLJ) of Balasubramanian et al.
2015, as Beck et al. 2018 apply them to gait.  The device makes every segment's magnitudes, band and arc length and the dimensionless jerk
(GRNet.gait_smoothness); the logarithm is pipeline.smoothness_rows'.  <outpath>_smoothness.json.  These signals are joint positions of
a pose model at 20 fps, where the cut-off of 10 Hz is the Nyquist frequency; a segment's rectangular window alone gives a noiseless sinusoid SPARC
about -4 at 64 frames, with 5 mm of joint noise a good part of the number is the noise, and the defaults are unvalidated on the model's output.
With --gait_turns a turn splits the walk into straight runs.  Reported, never judged.

--gait_recurrence (opt-in, needs no --gait) reports the recurrence quantification of the same four body signals: every pair of states of the
delay-embedded signal against one radius, and the diagonal lines of recurrent pairs by their length -- recurrence rate, determinism, mean and longest
line, divergence and the entropy of the line lengths (Webber and Zbilut 1994, Marwan et al. 2007), which the gait studies report beside harmonic
ratio, entropy and the Lyapunov exponents (Labini et al. 2012, Riva et al. 2013).  The device counts the pairs and the lines (GRNet.gait_recurrence,
DESIGN 4.20); the line threshold and the logarithm are pipeline.recurrence_rows'.  <outpath>_recurrence.json.  The papers use a trunk sensor and
minutes of walking; these are joint positions of a pose model over some 15 strides, the radius is this project's rule (a fraction of the signal's SD,
not of the phase-space diameter), and the defaults are unvalidated on the model's output.  With --gait_turns only straight walking counts.
Reported, never judged.

--gait_coordination (opt-in, needs no --gait) reports arm swing and inter-limb coordination, the first measure here that compares two signals: the
shoulder and the hip flexion of both sides (--gait_kinematics's angles, read without events), their auto and cross spectra by Welch's segments
(Carter, Knapp and Nuttall 1973), and at the stride frequency the swing amplitude of every limb, the left / right asymmetry of arms and legs, and for
the six pairs of limbs the coherence, the phase and its deviation from the expected 0 or 180 degrees (Wagenaar and van Emmerik 2000, Plotnik et al.
2007, Mirelman et al. 2016).  The device makes the spectra and the rows (GRNet.gait_coordination); the amplitudes and asymmetries are
pipeline.coordination_rows'.  <outpath>_coordination.json.  These are joint-position angles of a pose model over some 15 strides: with K segments
the coherence of two unrelated signals is about 1 / K (0.09 at the 11 segments of 400 frames), not 0, and the defaults are unvalidated on the
model's output.  With --gait_turns a turn splits the walk into straight runs.  Reported, never judged.

--gait_balance (opt-in, with --gait) reports where the feet land on the floor and where the body's mass is relative to them, without a camera
model: a foot on the ground stands still in the world, so the vector between the ankles just after a heel strike is a footprint-to-footprint
vector, and the centre of mass (Winter's segment masses laid on the kinectv2 joints, a layout of this project's that is unvalidated) relative to
the planted ankle gives its velocity over the ground.  Per video the footprints chained strike after strike, stride length, step length and step
width against the line of progression (as a walkway defines them, Webster et al. 2005), the speed over the ground, and Hof's margin of stability
at foot placement, forward and sideways (Hof, Gagey and Halbertsma 2005; Mehdizadeh et al. 2020 report it from video in dementia)
(GRNet.gait_balance on the device): <outpath>_balance.json, and 'footprints_phase' in the database.  THE FLOOR IS THE x-z PLANE OF A
LEVEL, FIXED CAMERA; the stance ankle creeps forward at heel rise; a margin of a few centimetres carries about two of noise per step at 5 mm of
joint noise.  Reported, never judged.

--gait_bootstrap (opt-in, with --gait) puts an interval on the step and stride numbers: the samples behind them (one row per step and per stride,
GRNet.gait_step_tables) are resampled with replacement --bootstrap_replicates times (Efron 1979; --bootstrap_block 2 keeps a left and a right step
together, the circular block bootstrap of Politis and Romano 1992), and the --bootstrap_level percentile interval of every mean, SD and CV is read
off the replicates (GRNet.bootstrap_table on the device).  With --gait_turns the same over straight walking alone, with
--gait_balance over its step table.  <outpath>_bootstrap.json; the database gains nothing.  A PERCENTILE INTERVAL FROM SOME 15 STRIDES UNDER-COVERS
(about 0.91 where 0.95 is asked), and the steps of one walk are serially correlated, which a block length addresses only partly.  Reported, never
judged.

--gait_body (opt-in, needs no --gait) reports what the joints cannot: the volume, the centre of mass, the central second moments per unit volume and
the surface area of the SMPL mesh of every frame, exact sums over the 13 776 triangles of the closed surface (the divergence theorem; Mirtich 1996,
Eberly 2002).  The vertices are read where the forward left them, on the rank that ran it (GRNet.mesh_moments); eleven doubles per frame
ride the window's one all-gather.  Per video the mean volume, its CV, the mass at --body_density (985 kg/m^3), the radii of gyration, and how far the
mesh's centre of mass lies from the one --gait_balance uses (Winter's segment masses on the kinectv2 joints): <outpath>_body.json, 'body_com' and
'body_volume' in the database.  --balance_com mesh hands that centre to --gait_balance in place of the table's.  UNIFORM DENSITY IS AN ASSUMPTION
(lungs and bone are not uniform, 985 kg/m^3 is a whole-body textbook figure); THE MESH IS A STATISTICAL BODY SHAPE, NOT THE SUBJECT'S; the model
predicts betas PER FRAME, so the volume's CV across a video measures the model's consistency, not the subject.  Reported, never judged.

Video decoding (ffmpeg) is out of scope: --vid_folder holds one sub-folder of extracted frames per video.
Image frames are cropped + normalised on the GPU (grnet_crop_normalise); .npy frames are ready crops.

Multi-GPU (torch.distributed.run, one process per GPU): the videos of one database window (<= 50 videos) are cut into
work items of <= --chunk consecutive frames (a short clip stays whole), the items are dealt to the ranks by load, every
rank runs its items in calls of >= the size at which the kernels are efficient, and the per-frame joints of the WHOLE
window are reassembled with ONE RCCL all-gather before rank 0 appends them to the database -- not one collective and one
host synchronisation per video.
"""
import argparse
import importlib
import os
import os.path as osp
import sys
import time

import numpy as np

ROOT = osp.dirname(osp.abspath(__file__))
sys.path.insert(0, ROOT)
PKG = "video-based-gait-analysis-for-dementia_amd"
MIN_FDIFF = 10            # batch_generation.py:35
IMG_W, IMG_H = 1920, 1080  # batch_generation.py:25-26: the frame the OpenPose joints are scaled to
BBOX_SCALE = 1.1          # batch_generation.py:296 (Inference(scale=1.1))


def vid_sort_key(x):
    try:                                                      # "SxxxCxxxPxxxRxxxAxxx" names (batch_generation.py:195)
        return (0, int(x[1:4] + x[6:9] + x[11:14] + x[16:19]))
    except ValueError:
        return (1, x)


def flush_windows(n_videos, max_vid):
    """Index ranges [a, b) of videos that end up in the same database file: the reference flushes at the top of iteration idx
    when idx % 50 == 0, idx > 0 and more than 10 videos remain (batch_generation.py:226), and once more at the end."""
    cuts = [0] + [i for i in range(1, n_videos) if i % max_vid == 0 and (n_videos - i) > 10] + [n_videos]
    return [(a, b) for a, b in zip(cuts, cuts[1:]) if b > a]


def boxes_from_openpose(openpose_folder, bbox_out=None, on_host=False, model_factory=None, return_joints=False, track=None):
    """load_openpose_anno (batch_generation.py:95-178): {vid_name: (T,4) float64 boxes} from a folder of OpenPose .mat files, by
    pipeline.openpose_boxes -- on the GPU through a GRNet handle without weights (model_factory(local_rank) -> an object with
    bbox_from_joints2d: the seam of the CPU tests), or on the host (on_host).  The call is deterministic, so under several ranks every
    rank computes the same boxes; rank 0 writes them to bbox_out with joblib.dump, and the bad files' names to bbox_out + '.bad'.
    return_joints: (boxes, {vid_name: the (T,25,3) pixel joints of the candidate whose box won}) -- what --trajectory fits to.
    track: {'kernel_size', 'sigma', 'pad'} -- --bbox_track: per-frame boxes of the frames [start, end) of each video (pipeline.openpose_boxes
    with track=; model.track_boxes, or pipeline.track_boxes with on_host), and a further last value, the tracks {vid_name: {'range', 'frames',
    'status'}} that prepare_data wants.  A video without any detection is dropped with one line (and keeps a None there); a frame inside a track whose smoothed scale is
    not positive (status 3: the zero padding of scipy's median near the ends of a track) stops the script."""
    pkg = importlib.import_module(PKG)
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    model = None
    if not on_host:
        model = model_factory(local_rank) if model_factory is not None else pkg.GRNet(max_frames=1, device_id=local_rank)
    found = pkg.pipeline.openpose_boxes(openpose_folder, model=model, img_w=IMG_W, img_h=IMG_H, return_joints=True, **({} if track is None else {"track": track}))
    boxes, bad, joints2d = found[:3]
    if model is not None and hasattr(model, "close"):
        model.close()
    tracks = None
    if track is not None:
        tracks = found[3]
        for key in sorted(tracks):
            if tracks[key] is None:
                if int(os.environ.get("RANK", "0")) == 0:
                    print(f"Track: skip video {key}, no frame of its 2D joints has a detection.")
                del boxes[key], joints2d[key]                   # tracks[key] stays None: prepare_data has nothing more to say about it
            elif (tracks[key]["status"] == pkg.pipeline.TRACK_BAD_SCALE).any():
                start = tracks[key]["range"][0]
                at = [int(i) + start for i in np.flatnonzero(tracks[key]["status"] == pkg.pipeline.TRACK_BAD_SCALE)]
                sys.exit(f"batch_generation.py: video {key}: the smoothed box scale of {len(at)} frame(s) (the first: {at[0]}) is not positive -- near the ends of a "
                         "track more than half of the median's window is zero padding (scipy's, the reference's own result); try --bbox_pad edge")
    if bbox_out and int(os.environ.get("RANK", "0")) == 0:
        import joblib
        joblib.dump(boxes, bbox_out)
        joblib.dump(bad, bbox_out + ".bad")
        print(f"Save {len(boxes)} boxes to {bbox_out} ({len(bad)} files without usable 2D joints: {bbox_out}.bad).")
    if track is not None:
        return (boxes, joints2d, tracks) if return_joints else (boxes, tracks)
    return (boxes, joints2d) if return_joints else boxes


def align_track(bboxes, status, start, end, T, n_files):
    """--bbox_track where a video has n_files extracted frames and its 2D joints T (within MIN_FDIFF): the fixed-box rule -- repeat box 0 -- would
    throw the track away.  Fewer files: the track is truncated to the frames that exist.  More files, and the track reaches the last frame of
    the 2D joints: the last box is held over the further frames (status 1).  Returns (bboxes, status, stop): the frames [start, stop)."""
    stop = end
    if n_files < end:
        stop = max(n_files, start)
        bboxes, status = bboxes[:stop - start], status[:stop - start]
    elif n_files > T and end == T:
        stop = n_files
        bboxes = np.concatenate([bboxes, np.repeat(bboxes[-1:], n_files - T, axis=0)], 0)
        status = np.concatenate([status, np.ones(n_files - T, status.dtype)], 0)
    return bboxes, status, stop


def load_ground_truth(gt_path):
    """{vid_name: (T,25,3) kinectv2 joints} from a joblib database in this script's own output schema: 'vid_name' (F,) and 'joints3D' (F,25,3),
    the frames of a video in order."""
    import joblib
    db = joblib.load(gt_path)
    names, joints = np.asarray(db["vid_name"]), np.asarray(db["joints3D"])
    if joints.ndim != 3 or joints.shape[1:] != (25, 3) or names.shape[0] != joints.shape[0]:
        raise ValueError(f"{gt_path}: 'vid_name' (F,) and 'joints3D' (F,25,3) expected, got {names.shape} and {joints.shape}")
    rows = {}
    for i, name in enumerate(names):
        rows.setdefault(str(name), []).append(i)
    return {name: joints[idx] for name, idx in rows.items()}


METRIC_NAMES = ("mpjpe", "pa_mpjpe", "pve", "accel", "accel_err")     # the columns of pose_metrics; no vertices here, so pve is not reported


class WindowMetrics:
    """--gt_path: one pose_metrics call per database window on rank 0, one sequence per video, on the joints the gather left on the device
    (model.pose_metrics; on_host, or a model without the method: pipeline.pose_metrics after a download).  root: kinectv2 joint 0; select: the
    kinectv2 joints that spin2 fills (kps_tables.json, entries >= 0) -- convert_kps leaves the others at zero.  Millimetres."""

    def __init__(self, gt, pipe, model, on_host):
        self.gt, self.pipe = gt, pipe
        self.device_call = None if on_host or not hasattr(model, "pose_metrics") else model.pose_metrics
        table = pipe._kps_tables()["from_spin2"]["kinectv2"]
        self.select = [k for k, i in enumerate(table) if i >= 0]
        self.videos = {}
        self.sums, self.counts = np.zeros(5), np.zeros(5, np.int64)

    def add_window(self, keys, per_video):
        """keys[vi], per_video[vi] (T,75): the videos of one window; a video the ground truth lacks, or of another length, is skipped."""
        import torch
        pred, truth, lengths, names = [], [], [], []
        for vi, key in enumerate(keys):
            kp = per_video[vi]
            frames = int(kp.shape[0])
            if key not in self.gt:
                print(f"Metrics: skip video {key}, the ground truth has no such video.")
            elif self.gt[key].shape[0] != frames:
                print(f"Metrics: skip video {key}, {frames} frames here and {self.gt[key].shape[0]} in the ground truth.")
            else:
                pred.append(kp.reshape(frames, 25, 3))
                truth.append(self.gt[key])
                lengths.append(frames)
                names.append(key)
        if not names:
            return
        pred, truth = torch.cat(pred, 0), np.concatenate(truth, 0)
        kw = dict(lengths=lengths, root=[0], select=self.select, unit=1000.0)
        if self.device_call is not None:
            per_seq = self.device_call(pred, truth, **kw)["per_sequence"].cpu().numpy()
        else:
            per_seq = self.pipe.pose_metrics(pred.cpu().numpy(), truth, **kw)["per_sequence"]
        for name, T, row in zip(names, lengths, per_seq):
            count = np.array([T, T, 0, max(T - 2, 0), max(T - 2, 0)], np.int64)
            self.videos[name] = {"frames": T, **{m: (float(row[c]) if count[c] else None) for c, m in enumerate(METRIC_NAMES) if m != "pve"}}
            self.sums += np.where(count > 0, row * count, 0.0)
            self.counts += count

    def write(self, path):
        import json
        total = {"frames": int(self.counts[0]), **{m: (float(self.sums[c] / self.counts[c]) if self.counts[c] else None)
                                                   for c, m in enumerate(METRIC_NAMES) if m != "pve"}}
        with open(path, "w") as f:
            json.dump({**self.videos, "total": total}, f, indent=1, allow_nan=False)
        shown = ", ".join(f"{m} {total[m]:.2f}" for m in total if m != "frames" and total[m] is not None)
        print(f"Save metrics of {len(self.videos)} videos ({total['frames']} frames; mm: {shown}) to {path}.")
        return path


class WindowTrajectory:
    """--trajectory: one fit_translation call per database window on rank 0, one sequence per video, on the kinectv2 joints the gather left on the
    device and the window's OpenPose joints, uploaded once (model.fit_translation; on_host, or a model without the method:
    pipeline.fit_translation after a download).  The pairs are pipeline.BODY25_FROM_KINECTV2, the centre the middle of the IMG_W x IMG_H frame, the
    focal length an assumption (--focal_length).  A video whose frame count differs from its OpenPose length has no detections to pair with its
    frames -- its boxes were repeated for the same reason -- and gets NaN rows with status 1."""

    def __init__(self, joints2d, pipe, model, on_host, focal_length=None):
        self.joints2d, self.pipe = joints2d, pipe
        self.device_call = None if on_host or not hasattr(model, "fit_translation") else model.fit_translation
        self.focal_length = float(focal_length) if focal_length else float(np.hypot(IMG_W, IMG_H))
        self.centre = (IMG_W / 2.0, IMG_H / 2.0)

    def add_window(self, keys, per_video):
        """keys[vi], per_video[vi] (T,75) -> per video (trans (T,3) float32, trans_status (T,) uint8, reproj (T,) float32)."""
        import torch
        rows = [None] * len(keys)
        j3, j2, lengths, which = [], [], [], []
        for vi, key in enumerate(keys):
            frames = int(per_video[vi].shape[0])
            found = self.joints2d.get(key)
            if found is None or found.shape[0] != frames:
                print(f"Trajectory: skip video {key}, {frames} frames here and {'no' if found is None else found.shape[0]} frames of 2D joints.")
                rows[vi] = (np.full((frames, 3), np.nan, np.float32), np.full(frames, self.pipe.TRANS_TOO_FEW, np.uint8), np.full(frames, np.nan, np.float32))
                continue
            j3.append(per_video[vi].reshape(frames, 25, 3))
            j2.append(np.asarray(found, np.float32))
            lengths.append(frames)
            which.append(vi)
        if not which:
            return rows
        j3, j2 = torch.cat(j3, 0), np.concatenate(j2, 0)
        kw = dict(lengths=lengths, focal_length=self.focal_length, centre=self.centre)
        if self.device_call is not None:
            out = {k: v.cpu().numpy() for k, v in self.device_call(j3, j2, self.pipe.BODY25_FROM_KINECTV2, **kw).items()}
        else:
            out = self.pipe.fit_translation(j3.cpu().numpy(), j2, self.pipe.BODY25_FROM_KINECTV2, **kw)
        a = 0
        for vi, T, seq in zip(which, lengths, out["per_sequence"]):
            r = out["per_frame"][a:a + T]
            rows[vi] = (r[:, :3].astype(np.float32), r[:, 5].astype(np.uint8), r[:, 3].astype(np.float32))
            mean = "none" if np.isnan(seq[2]) else f"{seq[2]:.2f} px"
            print(f"Trajectory: video {keys[vi]}, {int(seq[0])} frames fitted, {int(seq[1])} filled, mean reprojection error {mean}, path length {seq[3]:.3f} m.")
            a += T
        return rows


class WindowGait:
    """--gait: one gait_parameters call per database window on rank 0, one sequence per video, on the kinectv2 joints the gather left on the device
    (model.gait_parameters; on_host, or a model without the method: pipeline.gait_parameters after a download), with the window's translations
    where --trajectory made them -- as the database stores them, float32, so the file can be made again from the database.  The joints are
    pipeline.GAIT_JOINTS_KINECTV2."""

    def __init__(self, pipe, model, on_host, fps=20.0, sigma=2.0, window=5, min_excursion=0.05):
        self.pipe = pipe
        self.device_call = None if on_host or not hasattr(model, "gait_parameters") else model.gait_parameters
        self.kw = dict(fps=float(fps), sigma=float(sigma), window=int(window), min_excursion=float(min_excursion))
        self.videos = {}

    def add_window(self, keys, per_video, fitted=None):
        """keys[vi], per_video[vi] (T,75), fitted[vi] = (trans (T,3), ...) of WindowTrajectory or None -> per video the events (T,) uint8."""
        import torch
        if not keys:
            return []
        lengths = [int(per_video[vi].shape[0]) for vi in range(len(keys))]
        j3 = torch.cat([per_video[vi].reshape(-1, 25, 3) for vi in range(len(keys))], 0)
        trans = None if fitted is None else np.concatenate([np.asarray(f[0], np.float64) for f in fitted], 0)
        if self.device_call is not None:
            made = self.device_call(j3, lengths=lengths, trans=trans, **self.kw)
            out = {k: v.cpu().numpy() for k, v in made.items()}
        else:
            made = out = self.pipe.gait_parameters(j3.cpu().numpy(), lengths=lengths, trans=trans, **self.kw)
        self.window = (j3, lengths, made["events"])            # for WindowKinematics: the joints and the events as this call returned them
        self.rows = made["per_frame"]                          # for WindowTurns: the per-frame rows as this call returned them
        events, a = [], 0
        for key, T, row in zip(keys, lengths, out["per_sequence"]):
            events.append(out["events"][a:a + T].astype(np.uint8))
            self.videos[key] = {name: (None if np.isnan(v) else float(v)) for name, v in zip(self.pipe.GAIT_COLUMNS, row)}
            shown = self.videos[key]
            speed = "none" if shown["speed"] is None else f"{shown['speed']:.3f} m/s"
            if shown["trajectory_speed"] is not None:
                speed += f" ({shown['trajectory_speed']:.3f} m/s along the trajectory)"
            print(f"Gait: video {key}, {int(row[4])} steps, cadence {'none' if shown['cadence'] is None else format(shown['cadence'], '.1f') + ' steps/min'}, "
                  f"stride-time CV {'none' if shown['stride_time_cv'] is None else format(shown['stride_time_cv'], '.2f') + ' %'}, speed {speed}.")
            a += T
        return events

    def write(self, path):
        import json
        with open(path, "w") as f:
            json.dump(self.videos, f, indent=1, allow_nan=False)
        print(f"Save gait parameters of {len(self.videos)} videos to {path}.")
        return path


class WindowKinematics:
    """--gait_kinematics: one gait_kinematics call per database window on rank 0, directly after WindowGait's, on the same joints and on the events
    that call returned (model.gait_kinematics; on_host, or a model without the method: pipeline.gait_kinematics after a download).  Per video and
    channel (pipeline.KINEMATICS_CHANNELS) the six columns of pipeline.KINEMATICS_COLUMNS plus curve_mean and curve_sd, 101 numbers each.  The joints
    are pipeline.KINEMATICS_JOINTS_KINECTV2.  The database gains nothing: the per-frame angles can be made again from its joints and events."""

    def __init__(self, pipe, model, on_host, sigma=2.0, min_stride=8, max_stride=60):
        self.pipe = pipe
        self.device_call = None if on_host or not hasattr(model, "gait_kinematics") else model.gait_kinematics
        self.kw = dict(sigma=float(sigma), min_stride=int(min_stride), max_stride=int(max_stride))
        self.videos = {}

    def add_window(self, keys, j3, lengths, events):
        """keys[vi] and what WindowGait kept of its call: the window's joints (sum T,25,3), the videos' lengths and the events (sum T,)."""
        if not keys:
            return
        if self.device_call is not None:
            out = {k: v.cpu().numpy() for k, v in self.device_call(j3, events, lengths=lengths, **self.kw).items()}
        else:
            ev = events.cpu().numpy() if hasattr(events, "cpu") else np.asarray(events)
            out = self.pipe.gait_kinematics(j3.cpu().numpy(), ev, lengths=lengths, **self.kw)

        def number(v):
            return None if np.isnan(v) else float(v)

        def shown(v, unit=" deg"):
            return "none" if v is None else f"{v:.1f}{unit}"
        a = 0
        for key, T, rows, curves in zip(keys, lengths, out["per_sequence"], out["curves"]):
            video = {}
            for c, name in enumerate(self.pipe.KINEMATICS_CHANNELS):
                video[name] = {col: number(v) for col, v in zip(self.pipe.KINEMATICS_COLUMNS, rows[c])}
                video[name]["curve_mean"] = [number(v) for v in curves[c, :, 0]]
                video[name]["curve_sd"] = [number(v) for v in curves[c, :, 1]]
            self.videos[key] = video
            trunk = out["per_frame"][a:a + T, 12]
            trunk = None if not np.isfinite(trunk).any() else float(np.nanmean(trunk))
            print(f"Kinematics: video {key}, knee ROM {shown(video['knee_flexion_left']['rom_mean'])} / {shown(video['knee_flexion_right']['rom_mean'])}, "
                  f"arm swing ROM {shown(video['shoulder_flexion_left']['rom_mean'])} / {shown(video['shoulder_flexion_right']['rom_mean'])} "
                  f"(symmetry index {shown(video['shoulder_flexion_left']['symmetry_index'], ' %')}), mean trunk inclination {shown(trunk)}.")
            a += T

    def write(self, path):
        import json
        with open(path, "w") as f:
            json.dump(self.videos, f, indent=1, allow_nan=False)
        print(f"Save gait kinematics of {len(self.videos)} videos to {path}.")
        return path


class WindowTurns:
    """--gait_turns: one gait_turns call per database window on rank 0, directly after WindowGait's, on the same joints and on the events and per-frame
    rows that call returned (model.gait_turns; on_host, or a model without the method: pipeline.gait_turns after a download).  Per video the columns
    of pipeline.TURN_COLUMNS plus 'turns', the list of its stored turns keyed by pipeline.TURN_TABLE_COLUMNS.  The joints are
    pipeline.GAIT_JOINTS_KINECTV2, fps is WindowGait's.  The thresholds are unvalidated on the model's output; nothing is judged."""

    def __init__(self, pipe, model, on_host, fps=20.0, sigma=8.0, edge_rate=5.0, peak_rate=15.0, min_angle=45.0, min_frames=10, max_frames=200):
        self.pipe = pipe
        self.device_call = None if on_host or not hasattr(model, "gait_turns") else model.gait_turns
        self.kw = dict(fps=float(fps), sigma=float(sigma), edge_rate=float(edge_rate), peak_rate=float(peak_rate), min_angle=float(min_angle),
                       min_frames=int(min_frames), max_frames=int(max_frames))
        self.videos = {}

    def add_window(self, keys, j3, lengths, events, gait_rows, whole):
        """keys[vi] and what WindowGait kept of its call: the window's joints (sum T,25,3), the videos' lengths, the events (sum T,) and the per-frame
        rows (sum T,7); whole[key]: its row of the whole clip, for the line -> per video the phase (T,) uint8."""
        if not keys:
            return []
        if self.device_call is not None:
            made = self.device_call(j3, events, gait_rows, lengths=lengths, **self.kw)
            out = {k: v.cpu().numpy() for k, v in made.items()}
        else:
            ev, rows = (x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x) for x in (events, gait_rows))
            made = out = self.pipe.gait_turns(j3.cpu().numpy(), ev, rows, lengths=lengths, **self.kw)
        self.phase = made["phase"]                             # for WindowBootstrap: the phase as this call returned it

        def number(v):
            return None if np.isnan(v) else float(v)

        def shown(v, form, unit):
            return "none" if v is None else format(v, form) + unit
        phases, a = [], 0
        for key, T, row, table in zip(keys, lengths, out["per_sequence"], out["turns"]):
            phases.append(out["phase"][a:a + T].astype(np.uint8))
            video = {name: number(v) for name, v in zip(self.pipe.TURN_COLUMNS, row)}
            video["turns"] = [{name: number(v) for name, v in zip(self.pipe.TURN_TABLE_COLUMNS, turn)} for turn in table if not np.isnan(turn[0])]
            self.videos[key] = video
            clip = whole[key]
            print(f"Turns: video {key}, {int(row[0])} turns, mean turn time {shown(video['turn_duration_mean'], '.2f', ' s')}, stride-time CV "
                  f"{shown(clip['stride_time_cv'], '.2f', ' %')} over the whole clip against {shown(video['straight_stride_time_cv'], '.2f', ' %')} straight, "
                  f"speed {shown(clip['speed'], '.3f', ' m/s')} against {shown(video['straight_speed'], '.3f', ' m/s')}.")
            a += T
        return phases

    def write(self, path):
        import json
        with open(path, "w") as f:
            json.dump(self.videos, f, indent=1, allow_nan=False)
        print(f"Save turns of {len(self.videos)} videos to {path}.")
        return path


class WindowContacts:
    """--gait_contacts: one gait_contacts call per database window on rank 0, directly after WindowGait's, on the same joints and on the events that
    call returned (model.gait_contacts; on_host, or a model without the method: pipeline.gait_contacts after a download).  Per video the columns of
    pipeline.CONTACT_COLUMNS plus 'runs', the list of its stored attributed runs keyed by pipeline.CONTACT_RUN_COLUMNS.  The joints are
    pipeline.GAIT_JOINTS_KINECTV2, fps is WindowGait's.  The thresholds are unvalidated on the model's output; nothing is judged."""

    def __init__(self, pipe, model, on_host, fps=20.0, sigma=0.0, fraction=0.25, speed=0.0, reach=2, max_frames=20):
        self.pipe = pipe
        self.device_call = None if on_host or not hasattr(model, "gait_contacts") else model.gait_contacts
        self.kw = dict(fps=float(fps), sigma=float(sigma), fraction=float(fraction), speed=float(speed), reach=int(reach), max_frames=int(max_frames))
        self.videos = {}

    def add_window(self, keys, j3, lengths, events):
        """keys[vi] and what WindowGait kept of its call: the window's joints (sum T,25,3), the videos' lengths and the events (sum T,) -> per video the
        phases (T,) uint8."""
        if not keys:
            return []
        if self.device_call is not None:
            out = {k: v.cpu().numpy() for k, v in self.device_call(j3, events, lengths=lengths, **self.kw).items()}
        else:
            ev = events.cpu().numpy() if hasattr(events, "cpu") else np.asarray(events)
            out = self.pipe.gait_contacts(j3.cpu().numpy(), ev, lengths=lengths, **self.kw)

        def number(v):
            return None if np.isnan(v) else float(v)

        def shown(v, form, unit):
            return "none" if v is None else format(v, form) + unit
        phases, a = [], 0
        for key, T, row, table in zip(keys, lengths, out["per_sequence"], out["runs"]):
            phases.append(out["phase"][a:a + T].astype(np.uint8))
            video = {name: number(v) for name, v in zip(self.pipe.CONTACT_COLUMNS, row)}
            video["runs"] = [{name: number(v) for name, v in zip(self.pipe.CONTACT_RUN_COLUMNS, run)} for run in table if run[2] == 1 or run[2] == -1]
            self.videos[key] = video
            print(f"Contacts: video {key}, {int(row[3] + row[4])} double supports, double-support time {shown(video['double_support_time_mean'], '.3f', ' s')} "
                  f"({shown(video['double_support_share_mean'], '.1f', ' %')} of the stride), single-support time "
                  f"{shown(video['single_support_time_mean'], '.3f', ' s')}, left / right asymmetry {shown(video['double_support_asymmetry'], '.1f', ' %')}.")
            a += T
        return phases

    def write(self, path):
        import json
        with open(path, "w") as f:
            json.dump(self.videos, f, indent=1, allow_nan=False)
        print(f"Save contacts of {len(self.videos)} videos to {path}.")
        return path


class WindowBalance:
    """--gait_balance: one gait_balance call per database window on rank 0, directly after WindowGait's, on the same joints and on the events that
    call returned (model.gait_balance; on_host, or a model without the method: pipeline.gait_balance after a download).  Per video the columns of
    pipeline.BALANCE_COLUMNS plus 'step_table', the list of its stored steps keyed by pipeline.BALANCE_STEP_COLUMNS.  The joints are
    pipeline.GAIT_JOINTS_KINECTV2, the segments pipeline.BALANCE_SEGMENTS_KINECTV2, fps is WindowGait's.  The floor is the x-z plane of a level, fixed
    camera; the segment layout is unvalidated; nothing is judged."""

    def __init__(self, pipe, model, on_host, fps=20.0, gravity=9.81, window=4, settle=1, max_step=30):
        self.pipe = pipe
        self.device_call = None if on_host or not hasattr(model, "gait_balance") else model.gait_balance
        self.kw = dict(fps=float(fps), gravity=float(gravity), window=int(window), settle=int(settle), max_step=int(max_step))
        self.videos = {}

    def add_window(self, keys, j3, lengths, events, com=None):
        """keys[vi] and what WindowGait kept of its call: the window's joints (sum T,25,3), the videos' lengths and the events (sum T,) -> per video the
        stance side of every frame's step (T,) int8: +1 left, -1 right, 0 none.  com (--balance_com mesh): WindowBody's centres of the window (sum T,3)
        float64, handed to the call as they are, in place of the segment table's."""
        if not keys:
            return []
        more = {} if com is None else {"com": com}
        if self.device_call is not None:
            made = self.device_call(j3, events, lengths=lengths, **self.kw, **more)
            out = {k: v.cpu().numpy() for k, v in made.items()}
        else:
            ev = events.cpu().numpy() if hasattr(events, "cpu") else np.asarray(events)
            if com is not None:
                more = {"com": com.cpu().numpy() if hasattr(com, "cpu") else np.asarray(com)}
            made = out = self.pipe.gait_balance(j3.cpu().numpy(), ev, lengths=lengths, **self.kw, **more)
        self.tables = (made["steps"], made["per_sequence"])    # for WindowBootstrap: the step table and the rows as this call returned them

        def number(v):
            return float(v) if np.isfinite(v) else None          # a NaN is undefined; an asymmetry over a zero mean is infinite: null too, the file is strict JSON

        def shown(v, form, unit):
            return "none" if v is None else format(v, form) + unit
        phases, a = [], 0
        for key, T, row, table in zip(keys, lengths, out["per_sequence"], out["steps"]):
            phases.append(out["per_frame"][a:a + T, 6].astype(np.int8))
            video = {name: number(v) for name, v in zip(self.pipe.BALANCE_COLUMNS, row)}
            video["step_table"] = [{name: number(v) for name, v in zip(self.pipe.BALANCE_STEP_COLUMNS, step)} for step in table if not np.isnan(step[0])]
            self.videos[key] = video
            print(f"Balance: video {key}, {int(row[1])} steps in {int(row[2])} chains, stride length {shown(video['stride_length_mean'], '.3f', ' m')}, step width "
                  f"{shown(video['step_width_mean'], '.3f', ' m')}, ground speed {shown(video['ground_speed'], '.3f', ' m/s')}, margin of stability forward "
                  f"{shown(video['mos_ap_mean'], '.3f', ' m')}, sideways {shown(video['mos_ml_mean'], '.3f', ' m')}.")
            a += T
        return phases

    def write(self, path):
        import json
        with open(path, "w") as f:
            json.dump(self.videos, f, indent=1, allow_nan=False)
        print(f"Save balance of {len(self.videos)} videos to {path}.")
        return path


class WindowBody:
    """--gait_body: the mesh's volume, centre of mass and second moments of every frame were made on the rank that ran the forward,
    directly behind it (pipeline.run_on_frames(body=True): model.mesh_moments on the vertices where they lie), and came to rank 0 inside the
    window's one all-gather.  Here, on rank 0, pipeline.body_rows makes of them per video the columns of pipeline.BODY_COLUMNS -- one host function:
    the rows are downloaded for the database anyway.  The offsets are against DESIGN 4.22 rule 1's centre of mass (Winter's segment masses on the
    kinectv2 joints) on the same frames.  UNIFORM DENSITY IS AN ASSUMPTION; the mesh is a statistical body shape, not the subject's; the model
    predicts betas per frame, so the volume's CV measures the model's consistency, not the subject; nothing is judged."""

    def __init__(self, pipe, density=985.0):
        self.pipe = pipe
        self.density = float(density)
        self.videos = {}

    def add_window(self, keys, per_video, rows):
        """keys[vi], per_video[vi] (T,75) and rows[vi] (T,11) float64, the videos of one window -> per video (body_com (T,3) float32, body_volume (T,)
        float32).  Keeps `com`, the window's (sum T,3) float64 centres where the rows lie, for WindowBalance (--balance_com mesh)."""
        import torch
        if not keys:
            return []
        lengths = [int(rows[vi].shape[0]) for vi in range(len(keys))]
        both = torch.cat([rows[vi] for vi in range(len(keys))], 0)
        self.com = both[:, 1:4].contiguous()
        host = both.cpu().numpy()
        j3 = torch.cat([per_video[vi].reshape(-1, 25, 3) for vi in range(len(keys))], 0).cpu().numpy()
        table = self.pipe.body_rows(host, j3, lengths, density=self.density)

        def number(v):
            return float(v) if np.isfinite(v) else None          # a NaN is undefined: null, the file is strict JSON

        def shown(v, form, unit=""):
            return "none" if v is None else format(v, form) + unit
        made, a = [], 0
        for key, T, row in zip(keys, lengths, table):
            made.append((host[a:a + T, 1:4].astype(np.float32), host[a:a + T, 0].astype(np.float32)))
            video = {name: number(v) for name, v in zip(self.pipe.BODY_COLUMNS, row)}
            video["density"] = self.density
            self.videos[key] = video
            print(f"Body: video {key}, {int(row[1])} of {int(row[0])} frames with a volume, volume {shown(video['volume_mean'], '.4f', ' m^3')}, CV "
                  f"{shown(None if video['volume_cv'] is None else 100.0 * video['volume_cv'], '.2f', ' %')}, mass {shown(video['mass'], '.1f', ' kg')} at "
                  f"{self.density:g} kg/m^3, centre of mass {shown(video['com_distance_mean'], '.3f', ' m')} from the segment table's.")
            a += T
        return made

    def write(self, path):
        import json
        with open(path, "w") as f:
            json.dump(self.videos, f, indent=1, allow_nan=False)
        print(f"Save body measures of {len(self.videos)} videos to {path}.")
        return path


class WindowBootstrap:
    """--gait_bootstrap: per database window on rank 0, after WindowGait's call (and WindowTurns' and WindowBalance's, where those ran), the step and
    stride tables of that call's events and rows (model.gait_step_tables) and the bootstrap of their columns (model.bootstrap_table; on_host, or a
    model without the methods: the pipeline's statements after a download).  Streams: 0 the steps (step time, length, width), 1 the strides (stride
    time); with a phase of WindowTurns 2 and 3 the same over straight walking alone; 4 WindowBalance's step table (stride length, step length, step
    width, MoS forward and sideways), its count made int32 on the device.  Per video and parameter: estimate (the sample's own value), lo, median and
    hi of the `level` percent percentile interval, replicates (those that are not NaN) and n (the rows resampled); 'truncated', which names every
    table that found more rows than it stores (max_rows, the balance call's max_steps) with both counts -- its first n rows are resampled, its
    estimate is theirs and not the whole clip's column, and a line says so; the step and stride tables; the
    cadence as 60 / hi .. 60 / lo of the step-time mean, labelled as derived.  A percentile interval from some 15 strides under-covers, and steps
    within a walk are serially correlated (block = 2 keeps a left and a right step together); nothing is judged."""
    STEP_NAMES, STRIDE_NAMES = ("step_time", "step_length", "step_width"), ("stride_time",)
    BALANCE_COLUMNS, BALANCE_NAMES = (7, 8, 9, 11, 12), ("stride_length", "footprint_step_length", "footprint_step_width", "mos_ap", "mos_ml")

    def __init__(self, pipe, model, on_host, fps=20.0, replicates=2000, level=95.0, block=1, seed=0, max_rows=256):
        if int(replicates) != replicates or not 1 <= replicates <= 4096:
            raise ValueError(f"replicates {replicates} outside [1, 4096]")
        if not (np.isfinite(level) and 0 < level < 100):
            raise ValueError(f"level {level} outside (0, 100) percent")
        self.pipe = pipe
        on_device = not on_host and hasattr(model, "gait_step_tables") and hasattr(model, "bootstrap_table")
        self.device_call = model.bootstrap_table if on_device else None
        self.tables_call = model.gait_step_tables if on_device else pipe.gait_step_tables
        tail = int(round((100.0 - float(level)) * 50.0))       # basis points below the interval
        self.kw = dict(B=int(replicates), block=int(block), seed=int(seed), quantiles=(tail, 5000, 10000 - tail))
        self.fps, self.level, self.max_rows = float(fps), float(level), int(max_rows)
        self.videos = {}

    def _rows(self, table, counts, cols, stream):
        """(n_seq, n_cols, 3, 5) numpy of one bootstrap call: per statistic [estimate, f, lo, median, hi]."""
        if self.device_call is not None:
            return self.device_call(table, counts, cols, stream=stream, **self.kw)["out"].cpu().numpy()
        return self.pipe.bootstrap_table(table, counts, cols, stream=stream, **self.kw)["out"]

    def add_window(self, keys, lengths, events, gait_rows, phase=None, balance=None):
        """keys[vi], the videos' lengths and what WindowGait kept of its call: the events (sum T,) and the per-frame rows (sum T,7); phase (sum T,):
        what WindowTurns kept, or None; balance: WindowBalance's (steps, per_sequence), or None."""
        if not keys:
            return
        if self.device_call is None:
            events, gait_rows, phase = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in (events, gait_rows, phase))
            balance = None if balance is None else tuple(x.cpu().numpy() if hasattr(x, "cpu") else x for x in balance)

        def host(x):
            return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)

        def number(v):
            return float(v) if np.isfinite(v) else None          # a NaN is undefined, a CV over a zero mean infinite: null, the file is strict JSON

        found = {}                                              # name -> (out (n_seq,3,5), rows resampled (n_seq,), rows found (n_seq,))
        listed = None
        for prefix, straight, streams in (("", False, (0, 1)),) + ((("straight_", True, (2, 3)),) if phase is not None else ()):
            t = self.tables_call(events, gait_rows, lengths=lengths, fps=self.fps, max_rows=self.max_rows, phase=phase if straight else None, straight_only=straight)
            counts = t["counts"]
            seen = host(counts)
            n = np.minimum(seen, self.max_rows)
            for names, table, k, cols, stream in ((self.STEP_NAMES, t["steps"], 0, (3, 4, 5), streams[0]), (self.STRIDE_NAMES, t["strides"], 1, (3,), streams[1])):
                out = self._rows(table, counts[:, k].contiguous() if hasattr(counts, "contiguous") else np.ascontiguousarray(counts[:, k]), cols, stream)
                for i, name in enumerate(names):
                    found[prefix + name] = (out[:, i], n[:, k], seen[:, k])
            if not straight:
                listed = (host(t["steps"]), host(t["strides"]))
        if balance is not None:
            steps, per_seq = balance
            if hasattr(per_seq, "to"):
                import torch
                counts = per_seq[:, 1].to(torch.int32)         # the count of steps, made int32 on the device
            else:
                counts = np.asarray(per_seq[:, 1], np.int32)
            out = self._rows(steps, counts, self.BALANCE_COLUMNS, 4)
            seen = host(counts)
            n = np.minimum(seen, steps.shape[1])
            for i, name in enumerate(self.BALANCE_NAMES):
                found[name] = (out[:, i], n, seen)
        for vi, key in enumerate(keys):
            par, cut = {}, {}
            for name, (out, n, seen) in found.items():
                if seen[vi] > n[vi]:                            # more rows than the table stores: the first n are resampled, and the estimate is theirs
                    cut[name] = {"found": int(seen[vi]), "n": int(n[vi])}
                for s, stat in enumerate(self.pipe.BOOTSTRAP_STATISTICS):
                    est, f, lo, mid, hi = out[vi, s]
                    par[f"{name}_{stat}"] = {"estimate": number(est), "lo": number(lo), "median": number(mid), "hi": number(hi), "replicates": int(f), "n": int(n[vi])}
            step = par["step_time_mean"]
            cadence = {"estimate": None if not step["estimate"] else 60.0 / step["estimate"], "lo": None if not step["hi"] else 60.0 / step["hi"],
                       "hi": None if not step["lo"] else 60.0 / step["lo"], "derived": "60 / step_time_mean: lo from its hi, hi from its lo; not resampled itself"}
            self.videos[key] = {"replicates": self.kw["B"], "level": self.level, "block": self.kw["block"], "seed": self.kw["seed"], "method": "percentile",
                                "parameters": par, "cadence": cadence, "truncated": cut,
                                "step_table": [{c: number(v) for c, v in zip(self.pipe.STEP_TABLE_COLUMNS, row)} for row in listed[0][vi] if not np.isnan(row[0])],
                                "stride_table": [{c: number(v) for c, v in zip(self.pipe.STRIDE_TABLE_COLUMNS, row)} for row in listed[1][vi] if not np.isnan(row[0])]}

            def shown(p, form, unit):
                if p["estimate"] is None:
                    return "none"
                ends = "none" if p["lo"] is None or p["hi"] is None else f"{format(p['lo'], form)} to {format(p['hi'], form)}"
                return f"{format(p['estimate'], form)}{unit} ({ends})"
            print(f"Bootstrap: video {key}, stride time {shown(par['stride_time_mean'], '.3f', ' s')}, stride-time CV {shown(par['stride_time_cv'], '.2f', ' %')}: "
                  f"{self.level:g} % percentile intervals of {self.kw['B']} replicates over {par['stride_time_mean']['n']} strides.")
            if cut:
                print(f"Bootstrap: video {key}: " + ", ".join(f"{name} has {c['found']} rows of which the first {c['n']} are resampled" for name, c in cut.items()) +
                      ": these estimates are not the whole clip's columns.")

    def write(self, path):
        import json
        with open(path, "w") as f:
            json.dump(self.videos, f, indent=1, allow_nan=False)
        print(f"Save bootstrap intervals of {len(self.videos)} videos to {path}.")
        return path


class WindowRegularity:
    """--gait_regularity: one gait_regularity call per database window on rank 0, one sequence per video, on the joints the window's gather left on
    the device (model.gait_regularity; on_host, or a model without the method: pipeline.gait_regularity after a download) -- with the window's
    translations where --trajectory made them, and with --gait_turns' phase as `exclude`, so that only straight walking counts (straight_only).  It
    needs no events and so no --gait.  Per video and channel (pipeline.REGULARITY_CHANNELS) the ten columns of pipeline.REGULARITY_COLUMNS, step_time
    and stride_time in seconds, and the acf list.  The joints are pipeline.GAIT_JOINTS_KINECTV2.  The defaults are unvalidated on the model's output;
    the results are reported and never judged.  The database gains nothing."""

    def __init__(self, pipe, model, on_host, straight_only, fps=20.0, sigma=0.0, max_lag=60, min_lag=4, min_peak=0.25, min_pairs=20):
        self.pipe = pipe
        self.device_call = None if on_host or not hasattr(model, "gait_regularity") else model.gait_regularity
        self.straight_only = bool(straight_only)
        self.kw = dict(fps=float(fps), sigma=float(sigma), max_lag=int(max_lag), min_lag=int(min_lag), min_peak=float(min_peak), min_pairs=int(min_pairs))
        self.videos = {}

    def add_window(self, keys, per_video, fitted=None, gait_phase=None, whole=None):
        """keys[vi], per_video[vi] (T,75), fitted[vi] = (trans (T,3), ...) of WindowTrajectory or None, gait_phase[vi] (T,) of WindowTurns or None;
        whole: WindowGait's videos, for the event cadence in the line, or None."""
        import torch
        if not keys:
            return
        lengths = [int(per_video[vi].shape[0]) for vi in range(len(keys))]
        j3 = torch.cat([per_video[vi].reshape(-1, 25, 3) for vi in range(len(keys))], 0)
        trans = None if fitted is None else np.concatenate([np.asarray(f[0], np.float64) for f in fitted], 0)
        straight = self.straight_only and gait_phase is not None
        exclude = np.concatenate([np.asarray(ph, np.int32) for ph in gait_phase], 0) if straight else None
        if self.device_call is not None:
            out = {k: v.cpu().numpy() for k, v in self.device_call(j3, lengths=lengths, trans=trans, exclude=exclude, **self.kw).items()}
        else:
            out = self.pipe.gait_regularity(j3.cpu().numpy(), lengths=lengths, trans=trans, exclude=exclude, **self.kw)

        def number(v):
            return None if np.isnan(v) else float(v)

        def shown(v, form, unit=""):
            return "none" if v is None else format(v, form) + unit
        fps = self.kw["fps"]
        for key, rows, acf in zip(keys, out["per_sequence"], out["acf"]):
            video = {"straight_only": straight}
            for c, name in enumerate(self.pipe.REGULARITY_CHANNELS):
                video[name] = {col: number(v) for col, v in zip(self.pipe.REGULARITY_COLUMNS, rows[c])}
                video[name]["step_time"] = number(rows[c][3] / fps)
                video[name]["stride_time"] = number(rows[c][6] / fps)
                video[name]["acf"] = [number(v) for v in acf[c]]
            self.videos[key] = video
            sep = video["sep"]
            events = "" if whole is None or key not in whole else f" (events: {shown(whole[key]['cadence'], '.1f', ' steps/min')})"
            print(f"Regularity: video {key}, cadence {shown(sep['cadence'], '.1f', ' steps/min')} from the autocorrelation{events}, step regularity "
                  f"{shown(sep['step_regularity'], '.3f')}, stride regularity {shown(sep['stride_regularity'], '.3f')}, symmetry {shown(sep['symmetry'], '.3f')}"
                  f"{', straight walking only' if straight else ''}.")

    def write(self, path):
        import json
        with open(path, "w") as f:
            json.dump(self.videos, f, indent=1, allow_nan=False)
        print(f"Save gait regularity of {len(self.videos)} videos to {path}.")
        return path


class WindowHarmonics:
    """--gait_harmonics: one gait_harmonics call per database window on rank 0, directly after WindowGait's, on the same joints and on the events that
    call returned (model.gait_harmonics; on_host, or a model without the method: pipeline.gait_harmonics after a download) -- with the window's
    translations where --trajectory made them, and with --gait_turns' phase as `exclude`, so that only straight strides count (straight_only).  Per
    video and channel (pipeline.HARMONICS_CHANNELS) the twelve columns of pipeline.HARMONICS_COLUMNS, 'spectrum' (mean and SD of every harmonic's
    amplitude) and 'strides', the stored strides keyed by pipeline.HARMONICS_STRIDE_COLUMNS.  The joints are pipeline.GAIT_JOINTS_KINECTV2, fps is
    WindowGait's.  The defaults are unvalidated on the model's output; the results are reported and never judged.  The database gains nothing."""

    def __init__(self, pipe, model, on_host, straight_only, fps=20.0, sigma=0.0, n_harmonics=20, derivative=2, min_stride=8, max_stride=60):
        self.pipe = pipe
        self.device_call = None if on_host or not hasattr(model, "gait_harmonics") else model.gait_harmonics
        self.straight_only = bool(straight_only)
        self.kw = dict(fps=float(fps), sigma=float(sigma), n_harmonics=int(n_harmonics), derivative=int(derivative), min_stride=int(min_stride), max_stride=int(max_stride))
        self.videos = {}

    def add_window(self, keys, j3, lengths, events, fitted=None, gait_phase=None):
        """keys[vi] and what WindowGait kept of its call: the window's joints (sum T,25,3), the videos' lengths and the events (sum T,); fitted[vi] =
        (trans (T,3), ...) of WindowTrajectory or None, gait_phase[vi] (T,) of WindowTurns or None."""
        if not keys:
            return
        trans = None if fitted is None else np.concatenate([np.asarray(f[0], np.float64) for f in fitted], 0)
        straight = self.straight_only and gait_phase is not None
        exclude = np.concatenate([np.asarray(ph, np.int32) for ph in gait_phase], 0) if straight else None
        if self.device_call is not None:
            out = {k: v.cpu().numpy() for k, v in self.device_call(j3, events, lengths=lengths, trans=trans, exclude=exclude, **self.kw).items()}
        else:
            ev = events.cpu().numpy() if hasattr(events, "cpu") else np.asarray(events)
            out = self.pipe.gait_harmonics(j3.cpu().numpy(), ev, lengths=lengths, trans=trans, exclude=exclude, **self.kw)

        def number(v):
            return None if np.isnan(v) else float(v)

        def shown(v, form, unit=""):
            return "none" if v is None else format(v, form) + unit
        for key, rows, spectrum, strides in zip(keys, out["per_sequence"], out["spectrum"], out["strides"]):
            video = {"straight_only": straight}
            for c, name in enumerate(self.pipe.HARMONICS_CHANNELS):
                video[name] = {col: number(v) for col, v in zip(self.pipe.HARMONICS_COLUMNS, rows[c])}
                video[name]["spectrum"] = [{"mean": number(m), "sd": number(sd)} for m, sd in spectrum[c]]
                video[name]["strides"] = [{col: number(v) for col, v in zip(self.pipe.HARMONICS_STRIDE_COLUMNS, stride)} for stride in strides[c] if not np.isnan(stride[0])]
            self.videos[key] = video
            sep, bob = video["sep"], video["bob"]
            pelvis = f", of the pelvis' height {shown(bob['hr_mean'], '.3f')} ({shown(bob['ihr_mean'], '.1f', ' %')})" if trans is not None else ""
            print(f"Harmonics: video {key}, {int(rows[0][1])} of {int(rows[0][0])} strides used, harmonic ratio of the ankles' separation {shown(sep['hr_mean'], '.3f')} "
                  f"({shown(sep['ihr_mean'], '.1f', ' %')}){pelvis}, left / right index {shown(sep['hr_left_right_index'], '.1f', ' %')}"
                  f"{', straight strides only' if straight else ''}.")

    def write(self, path):
        import json
        with open(path, "w") as f:
            json.dump(self.videos, f, indent=1, allow_nan=False)
        print(f"Save gait harmonics of {len(self.videos)} videos to {path}.")
        return path


class WindowEntropy:
    """--gait_entropy: one gait_entropy call per database window on rank 0, one sequence per video, on the joints the window's gather left on the
    device (model.gait_entropy; on_host, or a model without the method: pipeline.gait_entropy after a download) -- with the window's translations
    where --trajectory made them, and with --gait_turns' phase as `exclude`, so that only straight walking counts (straight_only).  It needs no
    events and so no --gait.  Either way the logarithm is pipeline.entropy_rows' on the integer counts.  Per video and channel
    (pipeline.ENTROPY_CHANNELS) the columns of pipeline.ENTROPY_COLUMNS, per scale the counts (pipeline.ENTROPY_COUNTS) and 'sampen', and
    'complexity'; null where undefined.  The joints are pipeline.GAIT_JOINTS_KINECTV2.  The defaults are unvalidated on the model's output; the
    results are reported and never judged.  The database gains nothing."""

    def __init__(self, pipe, model, on_host, straight_only, sigma=0.0, m=2, fraction=0.2, derivative=2, scales=3, min_templates=50):
        self.pipe = pipe
        self.device_call = None if on_host or not hasattr(model, "gait_entropy") else model.gait_entropy
        self.straight_only = bool(straight_only)
        self.kw = dict(sigma=float(sigma), m=int(m), fraction=float(fraction), derivative=int(derivative), scales=int(scales))
        self.min_templates = int(min_templates)
        self.videos = {}

    def add_window(self, keys, per_video, fitted=None, gait_phase=None):
        """keys[vi], per_video[vi] (T,75), fitted[vi] = (trans (T,3), ...) of WindowTrajectory or None, gait_phase[vi] (T,) of WindowTurns or None."""
        import torch
        if not keys:
            return
        lengths = [int(per_video[vi].shape[0]) for vi in range(len(keys))]
        j3 = torch.cat([per_video[vi].reshape(-1, 25, 3) for vi in range(len(keys))], 0)
        trans = None if fitted is None else np.concatenate([np.asarray(f[0], np.float64) for f in fitted], 0)
        straight = self.straight_only and gait_phase is not None
        exclude = np.concatenate([np.asarray(ph, np.int32) for ph in gait_phase], 0) if straight else None
        if self.device_call is not None:
            out = {k: v.cpu().numpy() for k, v in self.device_call(j3, lengths=lengths, trans=trans, exclude=exclude, **self.kw).items()}
        else:
            out = self.pipe.gait_entropy(j3.cpu().numpy(), lengths=lengths, trans=trans, exclude=exclude, **self.kw)
        out.update(self.pipe.entropy_rows(out["counts"], self.min_templates))

        def number(v):
            return None if np.isnan(v) else float(v)

        def shown(v, form):
            return "none" if v is None else format(v, form)
        for key, rows, counts, sampen, complexity in zip(keys, out["per_sequence"], out["counts"], out["sampen"], out["complexity"]):
            video = {"straight_only": straight}
            for c, name in enumerate(self.pipe.ENTROPY_CHANNELS):
                video[name] = {col: number(v) for col, v in zip(self.pipe.ENTROPY_COLUMNS, rows[c])}
                video[name]["scales"] = [dict({col: int(v) for col, v in zip(self.pipe.ENTROPY_COUNTS, counts[c][k])}, sampen=number(sampen[c][k]))
                                         for k in range(self.kw["scales"])]
                video[name]["complexity"] = number(complexity[c])
            self.videos[key] = video
            sep, bob = video["sep"], video["bob"]
            pelvis = f", of the pelvis' height {shown(bob['scales'][0]['sampen'], '.3f')} ({shown(bob['complexity'], '.3f')})" if trans is not None else ""
            print(f"Entropy: video {key}, {sep['scales'][0]['templates']} templates, sample entropy of the ankles' separation {shown(sep['scales'][0]['sampen'], '.3f')} "
                  f"(complexity index over {self.kw['scales']} scales {shown(sep['complexity'], '.3f')}){pelvis}{', straight walking only' if straight else ''}.")

    def write(self, path):
        import json
        with open(path, "w") as f:
            json.dump(self.videos, f, indent=1, allow_nan=False)
        print(f"Save gait entropy of {len(self.videos)} videos to {path}.")
        return path


class WindowStability:
    """--gait_stability: one gait_stability call per database window on rank 0, one sequence per video, on the joints the window's gather left on the
    device (model.gait_stability; on_host, or a model without the method: pipeline.gait_stability after a download) -- with the window's
    translations where --trajectory made them, and with --gait_turns' phase as `exclude`, so that only straight walking counts (straight_only): a
    reference before a turn may then find its neighbour after it, which is intended, both being straight walking.  It needs no events and so no
    --gait.  Either way the logarithm and the slope are pipeline.stability_rows' on the integers and mantissas.  Per video and channel
    (pipeline.STABILITY_CHANNELS) a 'curve' with, per k, 'n', 'exponent', 'mantissa' and 'divergence', and 'lambda' in 1/s; null where undefined.
    The joints are pipeline.GAIT_JOINTS_KINECTV2.  The defaults are unvalidated on the model's output; the results are reported and never judged.
    The database gains nothing."""

    def __init__(self, pipe, model, on_host, straight_only, fps=20.0, sigma=0.0, derivative=1, dim=5, lag=2, theiler=20, horizon=20, fit_lo=0, fit_hi=None, min_pairs=50):
        self.pipe = pipe
        self.device_call = None if on_host or not hasattr(model, "gait_stability") else model.gait_stability
        self.straight_only = bool(straight_only)
        self.kw = dict(sigma=float(sigma), derivative=int(derivative), dim=int(dim), lag=int(lag), theiler=int(theiler), horizon=int(horizon))
        fit_hi = min(10, int(horizon)) if fit_hi is None else int(fit_hi)      # as the statements take None
        if not 0 <= int(fit_lo) < fit_hi <= int(horizon):                      # before any inference runs, in pipeline.stability_rows' words
            raise ValueError(f"the fit window {fit_lo} .. {fit_hi} must hold 0 <= fit_lo < fit_hi <= horizon = {horizon}")
        self.rows = dict(fps=float(fps), fit_lo=int(fit_lo), fit_hi=fit_hi, min_pairs=int(min_pairs))
        self.videos = {}

    def add_window(self, keys, per_video, fitted=None, gait_phase=None):
        """keys[vi], per_video[vi] (T,75), fitted[vi] = (trans (T,3), ...) of WindowTrajectory or None, gait_phase[vi] (T,) of WindowTurns or None."""
        import torch
        if not keys:
            return
        lengths = [int(per_video[vi].shape[0]) for vi in range(len(keys))]
        j3 = torch.cat([per_video[vi].reshape(-1, 25, 3) for vi in range(len(keys))], 0)
        trans = None if fitted is None else np.concatenate([np.asarray(f[0], np.float64) for f in fitted], 0)
        straight = self.straight_only and gait_phase is not None
        exclude = np.concatenate([np.asarray(ph, np.int32) for ph in gait_phase], 0) if straight else None
        if self.device_call is not None:
            out = {k: v.cpu().numpy() for k, v in self.device_call(j3, lengths=lengths, trans=trans, exclude=exclude, **self.kw).items()}
        else:
            out = self.pipe.gait_stability(j3.cpu().numpy(), lengths=lengths, trans=trans, exclude=exclude, **self.kw, **self.rows)
        out.update(self.pipe.stability_rows(out["pairs"], out["mant"], **self.rows))

        def number(v):
            return None if np.isnan(v) else float(v)

        def shown(v, form):
            return "none" if v is None else format(v, form)
        for key, pairs, mant, divergence, lam in zip(keys, out["pairs"], out["mant"], out["divergence"], out["lambda"]):
            video = {"straight_only": straight}
            for c, name in enumerate(self.pipe.STABILITY_CHANNELS):
                video[name] = {"curve": [dict({col: int(v) for col, v in zip(self.pipe.STABILITY_PAIRS, pairs[c][k])}, mantissa=float(mant[c][k]), divergence=number(divergence[c][k]))
                                         for k in range(self.kw["horizon"] + 1)],
                               "lambda": number(lam[c])}
            self.videos[key] = video
            sep, bob = video["sep"], video["bob"]
            pelvis = f", of the pelvis' height {shown(bob['lambda'], '.3f')}" if trans is not None else ""
            print(f"Stability: video {key}, {sep['curve'][0]['n']} pairs of neighbours, divergence exponent of the ankles' separation {shown(sep['lambda'], '.3f')} a second "
                  f"over frames {self.rows['fit_lo']} to {self.rows['fit_hi']}{pelvis}{', straight walking only' if straight else ''}.")

    def write(self, path):
        import json
        with open(path, "w") as f:
            json.dump(self.videos, f, indent=1, allow_nan=False)
        print(f"Save gait stability of {len(self.videos)} videos to {path}.")
        return path


class WindowRecurrence:
    """--gait_recurrence: one gait_recurrence call per database window on rank 0, one sequence per video, on the joints the window's gather left on
    the device (model.gait_recurrence; on_host, or a model without the method: pipeline.gait_recurrence after a download) -- with the window's
    translations where --trajectory made them, and with --gait_turns' phase as `exclude`, so that only straight walking counts (straight_only): a
    point before a turn may then recur with one after it, which is intended, both being straight walking, and a turn ends every line that runs
    into it.  It needs no events and so no --gait.  Either way the line threshold, the rates and the logarithm are pipeline.recurrence_rows' on the
    integers.  Per video and channel (pipeline.RECURRENCE_CHANNELS) the columns of pipeline.RECURRENCE_COLUMNS and RECURRENCE_COUNTS, every row of
    pipeline.RECURRENCE_ROWS, and 'hist', the [length, lines] of the non-empty bins; null where undefined.  The joints are
    pipeline.GAIT_JOINTS_KINECTV2.  The radius rule is this project's and the defaults are unvalidated on the model's output; the results are
    reported and never judged.  The database gains nothing."""

    def __init__(self, pipe, model, on_host, straight_only, sigma=0.0, derivative=1, dim=5, lag=2, theiler=8, radius=0.8, min_line=2, min_points=50):
        self.pipe = pipe
        self.device_call = None if on_host or not hasattr(model, "gait_recurrence") else model.gait_recurrence
        self.straight_only = bool(straight_only)
        self.kw = dict(sigma=float(sigma), derivative=int(derivative), dim=int(dim), lag=int(lag), theiler=int(theiler), radius=float(radius))
        self.rows = dict(min_line=int(min_line), min_points=int(min_points))
        pipe.recurrence_rows(np.zeros((1, 6), np.int64), np.zeros((1, pipe.RECURRENCE_BINS), np.int64), **self.rows)      # its refusals, before any inference runs
        self.videos = {}

    def add_window(self, keys, per_video, fitted=None, gait_phase=None):
        """keys[vi], per_video[vi] (T,75), fitted[vi] = (trans (T,3), ...) of WindowTrajectory or None, gait_phase[vi] (T,) of WindowTurns or None."""
        import torch
        if not keys:
            return
        lengths = [int(per_video[vi].shape[0]) for vi in range(len(keys))]
        j3 = torch.cat([per_video[vi].reshape(-1, 25, 3) for vi in range(len(keys))], 0)
        trans = None if fitted is None else np.concatenate([np.asarray(f[0], np.float64) for f in fitted], 0)
        straight = self.straight_only and gait_phase is not None
        exclude = np.concatenate([np.asarray(ph, np.int32) for ph in gait_phase], 0) if straight else None
        if self.device_call is not None:
            out = {k: v.cpu().numpy() for k, v in self.device_call(j3, lengths=lengths, trans=trans, exclude=exclude, **self.kw).items()}
        else:
            out = self.pipe.gait_recurrence(j3.cpu().numpy(), lengths=lengths, trans=trans, exclude=exclude, **self.kw, **self.rows)
        out.update(self.pipe.recurrence_rows(out["counts"], out["hist"], **self.rows))

        def number(v):
            return None if np.isnan(v) else float(v)

        def shown(v, form):
            return "none" if v is None else format(v, form)
        for q, key in enumerate(keys):
            video = {"straight_only": straight}
            for c, name in enumerate(self.pipe.RECURRENCE_CHANNELS):
                row = {col: number(v) for col, v in zip(self.pipe.RECURRENCE_COLUMNS, out["per_sequence"][q][c])}
                row.update({col: int(v) for col, v in zip(self.pipe.RECURRENCE_COUNTS, out["counts"][q][c])})
                for col in self.pipe.RECURRENCE_ROWS:
                    if col != "longest":                        # the count stays an integer; the row's NaN below min_line shows in 'divergence'
                        row[col] = int(out[col][q][c]) if col in ("lines", "line_points") else number(out[col][q][c])
                row["hist"] = [[int(k) + 1, int(out["hist"][q][c][k])] for k in np.flatnonzero(out["hist"][q][c])]
                video[name] = row
            self.videos[key] = video
            sep = video["sep"]
            print(f"Recurrence: video {key}, {sep['points']} points, recurrence rate {shown(sep['recurrence_rate'], '.3f')}, determinism {shown(sep['determinism'], '.3f')}, "
                  f"longest line {sep['longest']} of the ankles' separation{', straight walking only' if straight else ''}.")

    def write(self, path):
        import json
        with open(path, "w") as f:
            json.dump(self.videos, f, indent=1, allow_nan=False)
        print(f"Save gait recurrence of {len(self.videos)} videos to {path}.")
        return path


class WindowSpectrum:
    """--gait_spectrum: one gait_spectrum call per database window on rank 0, one sequence per video, on the joints the window's gather left on the
    device (model.gait_spectrum; on_host, or a model without the method: pipeline.gait_spectrum after a download) -- with the window's translations
    where --trajectory made them, and with --gait_turns' phase as `exclude` (straight_only): a turn then splits the walk into straight runs, and the
    segments of all of them are averaged.  It needs no events and so no --gait.  Either way the logarithm is pipeline.spectrum_rows' on the psd.
    Per video and channel (pipeline.SPECTRUM_CHANNELS) the columns of pipeline.SPECTRUM_COLUMNS, 'spectral_entropy', and the 'psd' list; per video
    the frequency axis 'freqs' in Hz; null where undefined.  The joints are pipeline.GAIT_JOINTS_KINECTV2.  The peak's width has a floor set by the
    segment length, not by the walker; the defaults are unvalidated on the model's output; the results are reported and never judged.  The database
    gains nothing."""

    def __init__(self, pipe, model, on_host, straight_only, fps=20.0, sigma=0.0, derivative=2, segment=64, hop=None, nfft=256, f_lo=0.5, f_hi=3.0, min_segments=2):
        self.pipe = pipe
        self.device_call = None if on_host or not hasattr(model, "gait_spectrum") else model.gait_spectrum
        self.straight_only = bool(straight_only)
        self.kw = dict(fps=float(fps), sigma=float(sigma), derivative=int(derivative), segment=int(segment), hop=int(segment) // 2 if hop is None else int(hop), nfft=int(nfft),
                       f_lo=float(f_lo), f_hi=float(f_hi), min_segments=int(min_segments))
        self.videos = {}

    def add_window(self, keys, per_video, fitted=None, gait_phase=None, whole=None, steady=None):
        """keys[vi], per_video[vi] (T,75), fitted[vi] = (trans (T,3), ...) of WindowTrajectory or None, gait_phase[vi] (T,) of WindowTurns or None;
        whole: WindowGait's videos and steady: WindowRegularity's, for their cadences in the line, or None."""
        import torch
        if not keys:
            return
        lengths = [int(per_video[vi].shape[0]) for vi in range(len(keys))]
        j3 = torch.cat([per_video[vi].reshape(-1, 25, 3) for vi in range(len(keys))], 0)
        trans = None if fitted is None else np.concatenate([np.asarray(f[0], np.float64) for f in fitted], 0)
        straight = self.straight_only and gait_phase is not None
        exclude = np.concatenate([np.asarray(ph, np.int32) for ph in gait_phase], 0) if straight else None
        if self.device_call is not None:
            out = {k: v.cpu().numpy() for k, v in self.device_call(j3, lengths=lengths, trans=trans, exclude=exclude, **self.kw).items()}
        else:
            out = self.pipe.gait_spectrum(j3.cpu().numpy(), lengths=lengths, trans=trans, exclude=exclude, **self.kw)
        out.update(self.pipe.spectrum_rows(out["psd"], out["per_sequence"], self.kw["fps"], self.kw["f_lo"], self.kw["f_hi"]))
        freqs = [k * self.kw["fps"] / self.kw["nfft"] for k in range(self.kw["nfft"] // 2 + 1)]

        def number(v):
            return None if np.isnan(v) else float(v)

        def shown(v, form, unit=""):
            return "none" if v is None else format(v, form) + unit
        for key, rows, psd, entropy in zip(keys, out["per_sequence"], out["psd"], out["spectral_entropy"]):
            video = {"straight_only": straight, "freqs": freqs}
            for c, name in enumerate(self.pipe.SPECTRUM_CHANNELS):
                video[name] = {col: number(v) for col, v in zip(self.pipe.SPECTRUM_COLUMNS, rows[c])}
                video[name]["spectral_entropy"] = number(entropy[c])
                video[name]["psd"] = [number(v) for v in psd[c]]
            self.videos[key] = video
            sep = video["sep"]
            events = "" if whole is None or key not in whole else f" (events: {shown(whole[key]['cadence'], '.1f', ' steps/min')})"
            lags = "" if steady is None or key not in steady else f" (autocorrelation: {shown(steady[key]['sep']['cadence'], '.1f', ' steps/min')})"
            print(f"Spectrum: video {key}, {int(sep['used'])} segments, cadence {shown(sep['cadence'], '.1f', ' steps/min')} from the spectral peak{events}{lags}, peak width "
                  f"{shown(sep['peak_width_hz'], '.3f', ' Hz')}, spectral entropy {shown(sep['spectral_entropy'], '.3f')} of the ankles' separation"
                  f"{', straight walking only' if straight else ''}.")

    def write(self, path):
        import json
        with open(path, "w") as f:
            json.dump(self.videos, f, indent=1, allow_nan=False)
        print(f"Save gait spectrum of {len(self.videos)} videos to {path}.")
        return path


class WindowSmoothness:
    """--gait_smoothness: one gait_smoothness call per database window on rank 0, one sequence per video, on the joints the window's gather left on
    the device (model.gait_smoothness; on_host, or a model without the method: pipeline.gait_smoothness after a download) -- with the window's
    translations where --trajectory made them, and with --gait_turns' phase as `exclude` (straight_only): a turn then splits the walk into straight
    runs, and every run's segments count.  It needs no events and so no --gait.  Either way the logarithm of the jerk is pipeline.smoothness_rows'.
    Per video and channel (pipeline.SMOOTHNESS_CHANNELS) the columns of pipeline.SMOOTHNESS_COLUMNS, 'ldlj_mean', 'ldlj_sd' and the list 'segments'
    (start, sparc, last_hz, ldlj); null where undefined.  The joints are pipeline.GAIT_JOINTS_KINECTV2.  THE INPUTS ARE JOINT POSITIONS OF A POSE
    MODEL AT 20 FPS, where 10 Hz is the Nyquist frequency; a segment's rectangular window alone sets a floor (SPARC about -4 at 64 frames) and with
    5 mm of joint noise a good part of the number is the noise; the defaults are unvalidated on the model's output; the results are reported and
    never judged.  The database gains nothing."""

    def __init__(self, pipe, model, on_host, straight_only, fps=20.0, sigma=0.0, derivative=1, segment=64, hop=None, nfft=1024, f_cut=None, amplitude=0.05,
                 min_segments=2):
        self.pipe = pipe
        self.device_call = None if on_host or not hasattr(model, "gait_smoothness") else model.gait_smoothness
        self.straight_only = bool(straight_only)
        self.kw = dict(fps=float(fps), sigma=float(sigma), derivative=int(derivative), segment=int(segment), hop=int(segment) // 2 if hop is None else int(hop), nfft=int(nfft),
                       f_cut=min(10.0, float(fps) / 2.0) if f_cut is None else float(f_cut), amplitude=float(amplitude), min_segments=int(min_segments))
        self.videos = {}

    def add_window(self, keys, per_video, fitted=None, gait_phase=None):
        """keys[vi], per_video[vi] (T,75), fitted[vi] = (trans (T,3), ...) of WindowTrajectory or None, gait_phase[vi] (T,) of WindowTurns or None."""
        import torch
        if not keys:
            return
        lengths = [int(per_video[vi].shape[0]) for vi in range(len(keys))]
        j3 = torch.cat([per_video[vi].reshape(-1, 25, 3) for vi in range(len(keys))], 0)
        trans = None if fitted is None else np.concatenate([np.asarray(f[0], np.float64) for f in fitted], 0)
        straight = self.straight_only and gait_phase is not None
        exclude = np.concatenate([np.asarray(ph, np.int32) for ph in gait_phase], 0) if straight else None
        if self.device_call is not None:
            out = {k: v if isinstance(v, np.ndarray) else v.cpu().numpy() for k, v in self.device_call(j3, lengths=lengths, trans=trans, exclude=exclude, **self.kw).items()}
        else:
            out = self.pipe.gait_smoothness(j3.cpu().numpy(), lengths=lengths, trans=trans, exclude=exclude, **self.kw)
        out.update(self.pipe.smoothness_rows(out["per_segment"], out["per_sequence"], out["slot_offsets"]))
        at = out["slot_offsets"]

        def number(v):
            return None if np.isnan(v) else float(v)

        def shown(v, form, unit=""):
            return "none" if v is None else format(v, form) + unit
        for q, (key, rows) in enumerate(zip(keys, out["per_sequence"])):
            video = {"straight_only": straight}
            for c, name in enumerate(self.pipe.SMOOTHNESS_CHANNELS):
                video[name] = {col: number(v) for col, v in zip(self.pipe.SMOOTHNESS_COLUMNS, rows[c])}
                video[name]["ldlj_mean"], video[name]["ldlj_sd"] = number(out["ldlj_mean"][q, c]), number(out["ldlj_sd"][q, c])
                video[name]["segments"] = [{"start": int(seg[c, 0]), "sparc": number(seg[c, 1]), "last_hz": number(seg[c, 3] * self.kw["fps"] / self.kw["nfft"]), "ldlj": number(ldlj[c])}
                                           for seg, ldlj in zip(out["per_segment"][at[q]:at[q + 1]], out["ldlj"][at[q]:at[q + 1]]) if not np.isnan(seg[c, 0])]
            self.videos[key] = video
            sep = video["sep"]
            print(f"Smoothness: video {key}, {int(sep['used'])} segments, SPARC {shown(sep['sparc_mean'], '.2f')} (SD {shown(sep['sparc_sd'], '.2f')}), LDLJ "
                  f"{shown(sep['ldlj_mean'], '.2f')} of the ankles' separation{', straight walking only' if straight else ''}.")

    def write(self, path):
        import json
        with open(path, "w") as f:
            json.dump(self.videos, f, indent=1, allow_nan=False)
        print(f"Save gait smoothness of {len(self.videos)} videos to {path}.")
        return path


class WindowCoordination:
    """--gait_coordination: one gait_coordination call per database window on rank 0, one sequence per video, on the joints the window's gather left
    on the device (model.gait_coordination; on_host, or a model without the method: pipeline.gait_coordination after a download) -- with
    --gait_turns' phase as `exclude` (straight_only): a turn then splits the walk into straight runs, and the segments of all of them are averaged.
    It needs no events and so no --gait.  Either way the amplitudes, asymmetries and the mean phase deviation are pipeline.coordination_rows' on
    the limbs' and pairs' rows.  Per video and limb (pipeline.COORDINATION_CHANNELS) the columns of pipeline.COORDINATION_LIMB_COLUMNS and
    'amplitude'; per pair (pipeline.COORDINATION_PAIR_NAMES) the columns of pipeline.COORDINATION_PAIR_COLUMNS; 'arm_asymmetry', 'leg_asymmetry',
    'arm_leg_ratio', 'phase_deviation_mean'; the frequency axis 'freqs' in Hz; null where undefined.  The joints are
    pipeline.KINEMATICS_JOINTS_KINECTV2.  With K segments the coherence of unrelated signals is about 1 / K, not 0; the defaults are unvalidated on
    the model's output; the results are reported and never judged.  The database gains nothing."""

    def __init__(self, pipe, model, on_host, straight_only, fps=20.0, sigma=0.0, derivative=0, segment=64, hop=None, nfft=256, f_lo=0.5, f_hi=3.0, min_segments=4):
        self.pipe = pipe
        self.device_call = None if on_host or not hasattr(model, "gait_coordination") else model.gait_coordination
        self.straight_only = bool(straight_only)
        self.kw = dict(fps=float(fps), sigma=float(sigma), derivative=int(derivative), segment=int(segment), hop=int(segment) // 2 if hop is None else int(hop), nfft=int(nfft),
                       f_lo=float(f_lo), f_hi=float(f_hi), min_segments=int(min_segments))
        self.videos = {}

    def add_window(self, keys, per_video, gait_phase=None):
        """keys[vi], per_video[vi] (T,75), gait_phase[vi] (T,) of WindowTurns or None."""
        import torch
        if not keys:
            return
        lengths = [int(per_video[vi].shape[0]) for vi in range(len(keys))]
        j3 = torch.cat([per_video[vi].reshape(-1, 25, 3) for vi in range(len(keys))], 0)
        straight = self.straight_only and gait_phase is not None
        exclude = np.concatenate([np.asarray(ph, np.int32) for ph in gait_phase], 0) if straight else None
        if self.device_call is not None:
            out = {k: v.cpu().numpy() for k, v in self.device_call(j3, lengths=lengths, exclude=exclude, **self.kw).items()}
        else:
            out = self.pipe.gait_coordination(j3.cpu().numpy(), lengths=lengths, exclude=exclude, **self.kw)
        out.update(self.pipe.coordination_rows(out["limbs"], out["pairs"]))
        freqs = [k * self.kw["fps"] / self.kw["nfft"] for k in range(self.kw["nfft"] // 2 + 1)]

        def number(v):
            return None if np.isnan(v) else float(v)

        def shown(v, form, unit=""):
            return "none" if v is None else format(v, form) + unit
        for q, key in enumerate(keys):
            video = {"straight_only": straight, "freqs": freqs}
            for c, name in enumerate(self.pipe.COORDINATION_CHANNELS):
                video[name] = {col: number(v) for col, v in zip(self.pipe.COORDINATION_LIMB_COLUMNS, out["limbs"][q, c])}
                video[name]["amplitude"] = number(out["amplitude"][q, c])
            for p, name in enumerate(self.pipe.COORDINATION_PAIR_NAMES):
                video[name] = {col: number(v) for col, v in zip(self.pipe.COORDINATION_PAIR_COLUMNS, out["pairs"][q, p])}
            for name in ("arm_asymmetry", "leg_asymmetry", "arm_leg_ratio", "phase_deviation_mean"):
                video[name] = number(out[name][q])
            self.videos[key] = video
            arms, legs = video[self.pipe.COORDINATION_PAIR_NAMES[0]], video[self.pipe.COORDINATION_PAIR_NAMES[1]]
            print(f"Coordination: video {key}, {int(video['arm_left']['used'])} segments, arm swing {shown(video['arm_left']['amplitude'], '.1f')} (left) and "
                  f"{shown(video['arm_right']['amplitude'], '.1f', ' degrees')} (right), asymmetry {shown(video['arm_asymmetry'], '.1f', ' %')}; arms: coherence "
                  f"{shown(arms['coherence_peak'], '.3f')}, {shown(arms['phase_deviation'], '.1f', ' degrees')} off antiphase; legs: coherence "
                  f"{shown(legs['coherence_peak'], '.3f')}, {shown(legs['phase_deviation'], '.1f', ' degrees')} off antiphase"
                  f"{', straight walking only' if straight else ''}.")

    def write(self, path):
        import json
        with open(path, "w") as f:
            json.dump(self.videos, f, indent=1, allow_nan=False)
        print(f"Save gait coordination of {len(self.videos)} videos to {path}.")
        return path


def prepare_data(fv, vid_folder, outpath, pretrained_file=None, synthetic_weights=False, max_frames=128, dtype="f32", chunk=None,
                 model_factory=None, backend="nccl", exchange="torch", full_arena=False, annos=None, gt_path=None, metrics_out=None,
                 metrics_on_host=False, trajectory=None, tracks=None, gait=None, kinematics=None, turns=None, contacts=None, regularity=None,
                 harmonics=None, entropy=None, stability=None, spectrum=None, recurrence=None, coordination=None, balance=None, bootstrap=None, smoothness=None,
                 body=None):
    """body: {'density', 'on_host', 'out'} (each optional; needs no gait) -- also the volume, centre of mass, central second moments and area of the mesh of
    every frame, made on the rank that ran the forward, directly behind it (pipeline.run_on_frames(body=True); 'on_host': the numpy
    statement after a download) and carried to rank 0 as 22 further float32 words of each row of the window's one all-gather; per video the columns of
    pipeline.BODY_COLUMNS (WindowBody), written to body['out'] (default: outpath with _body.json); the database gains 'body_com' (N,3) float32 and
    'body_volume' (N,) float32.  With balance['com'] == 'mesh' the balance call takes these centres in place of the segment table's (needs body).
    smoothness: {'fps', 'sigma', 'derivative', 'segment', 'hop', 'nfft', 'f_cut', 'amplitude', 'min_segments', 'all_frames', 'on_host', 'out'} (each optional;
    needs no gait, whose fps it takes where its own is not given, else 20) -- also the spectral arc length and the log dimensionless jerk of every video
    (WindowSmoothness), written to smoothness['out'] (default: outpath with _smoothness.json); with turns only straight walking counts unless
    'all_frames'; the database gains nothing.
    bootstrap: {'replicates', 'level', 'block', 'seed', 'on_host', 'out'} (each optional; needs gait, whose fps it takes) -- also the percentile
    intervals of the step and stride parameters of every video (WindowBootstrap; with turns also over straight walking alone, with balance also of
    its step table), written to bootstrap['out'] (default: outpath with _bootstrap.json); the database gains nothing.
    balance: {'gravity', 'window', 'settle', 'max_step', 'on_host', 'out'} (each optional; needs gait, whose fps it takes) -- also the footprints,
    stride length, step width, ground speed and margins of stability of every video (WindowBalance), written to balance['out'] (default: outpath with
    _balance.json); the database gains 'footprints_phase' (N,) int8 (the stance side of the frame's step: +1 left, -1 right, 0 none).
    coordination: {'fps', 'sigma', 'derivative', 'segment', 'hop', 'nfft', 'f_lo', 'f_hi', 'min_segments', 'all_frames', 'on_host', 'out'} (each
    optional; needs no gait, whose fps it takes where its own is not given, else 20) -- also the arm swing and inter-limb coordination of every video
    (WindowCoordination), written to coordination['out'] (default: outpath with _coordination.json); with turns only straight walking counts unless
    'all_frames'; the database gains nothing.
    recurrence: {'sigma', 'derivative', 'dim', 'lag', 'theiler', 'radius', 'min_line', 'min_points', 'all_frames', 'on_host', 'out'} (each optional;
    needs no gait) -- also the recurrence quantification of every video (WindowRecurrence), written to recurrence['out'] (default: outpath with
    _recurrence.json); with turns only straight walking counts unless 'all_frames'; the database gains nothing.
    spectrum: {'fps', 'sigma', 'derivative', 'segment', 'hop', 'nfft', 'f_lo', 'f_hi', 'min_segments', 'all_frames', 'on_host', 'out'} (each optional;
    needs no gait, whose fps it takes where its own is not given, else 20) -- also the Welch spectrum of every video (WindowSpectrum), written to
    spectrum['out'] (default: outpath with _spectrum.json); with turns only straight walking counts unless 'all_frames'; the database gains nothing.
    stability: {'sigma', 'derivative', 'dim', 'lag', 'theiler', 'horizon', 'fit_lo', 'fit_hi', 'min_pairs', 'all_frames', 'on_host', 'out'} (each optional;
    needs no gait, whose fps it takes where given, else 20) -- also the local dynamic stability of every video (WindowStability), written to
    stability['out'] (default: outpath with _stability.json); with turns only straight walking counts unless 'all_frames'; the database gains nothing.
    entropy: {'sigma', 'm', 'fraction', 'derivative', 'scales', 'min_templates', 'all_frames', 'on_host', 'out'} (each optional; needs no gait) -- also
    the sample entropy at several scales and the complexity index of every video (WindowEntropy), written to entropy['out'] (default: outpath with
    _entropy.json); with turns only straight walking counts unless 'all_frames'; the database gains nothing.
    harmonics: {'sigma', 'n_harmonics', 'derivative', 'min_stride', 'max_stride', 'all_frames', 'on_host', 'out'} (each optional; needs gait, whose fps it
    takes) -- also the harmonic ratios per stride of every video (WindowHarmonics), written to harmonics['out'] (default: outpath with _harmonics.json);
    with turns only straight strides count unless 'all_frames'; the database gains nothing.
    regularity: {'sigma', 'max_lag', 'min_lag', 'min_peak', 'min_pairs', 'all_frames', 'on_host', 'out'} (each optional, with 'fps'; needs no gait, whose
    fps it takes where it has none) -- also the step and stride regularity, the symmetry and the autocorrelation cadence of every video (WindowRegularity), written to
    regularity['out'] (default: outpath with _regularity.json); with turns only straight walking counts unless 'all_frames'; the database gains nothing.
    contacts: {'sigma', 'fraction', 'speed', 'reach', 'max_frames', 'on_host', 'out'} (each optional; needs gait, whose fps it takes) -- also the
    double supports of every video and its support, swing and stance times (WindowContacts), written to contacts['out'] (default: outpath with
    _contacts.json); the database gains 'gait_support' (N,) uint8 (0 moving, 1 left-led double support, 2 right-led, 3 static and unattributed, 4 unknown).
    turns: {'sigma', 'edge_rate', 'peak_rate', 'min_angle', 'min_frames', 'max_frames', 'on_host', 'out'} (each optional; needs gait, whose fps it
    takes) -- also the turns of every video and its gait parameters over straight walking alone (WindowTurns), written to turns['out'] (default:
    outpath with _turns.json); the database gains 'gait_phase' (N,) uint8 (0 straight, 1 left turn, 2 right turn, 3 unknown).
    kinematics: {'sigma', 'min_stride', 'max_stride', 'on_host', 'out'} (each optional; needs gait) -- also the joint angles per gait cycle of every
    video (WindowKinematics), written to kinematics['out'] (default: outpath with _kinematics.json); the database gains nothing.
    gait: {'fps', 'sigma', 'window', 'min_excursion', 'on_host', 'out'} (each optional) -- also read the gait events and parameters of every video
    off its joints (WindowGait), add 'gait_events' (N,) uint8 to the database (bit 0 heel strike left, 1 heel strike right, 2 toe-off left, 3 toe-off
    right) and write the parameters to gait['out'] (default: outpath with _gait.json).
    tracks: {vid_name: {'range': (start, end), 'frames': T, 'status': (end - start,) uint8}} of boxes_from_openpose(track=...) -- annos holds one
    box per frame of [start, end) of each video: only those frames are generated, the 2D joints of `trajectory` are taken as sliced alike, and the
    database gains 'bbox_status' (N,) uint8 (0 detected, 1 interpolated or held).
    trajectory: {'joints2d': {vid_name: (T,25,3) pixel joints}, 'focal_length': F or None, 'on_host': bool} -- also fit the camera-space
    translation of every frame (WindowTrajectory) and add 'trans' (N,3) float32, 'trans_status' (N,) uint8 and 'reproj' (N,) float32 to the database.
    gt_path: also compare the joints with that ground truth (WindowMetrics) and write metrics_out (default: outpath with _metrics.json).
    annos: the boxes themselves ({vid_name: (T,4)}, boxes_from_openpose) instead of the joblib file fv.
    model_factory(local_rank) -> model and backend="gloo" are the seam of the CPU tests (tests/test_host_cpu.py): the window / plan /
    run / gather / flush logic below then runs under two gloo ranks with a stand-in model and tensors on the CPU.
    exchange: "torch" = the window's all-gather through the launcher's process group; "capi" = through the C ABI's own RCCL communicator
    (harness.RcclComm: grnet_comm_create + grnet_allgather; needs one GPU per rank)."""
    import joblib
    import torch
    pkg = importlib.import_module(PKG)
    pipe = importlib.import_module(PKG + ".pipeline")
    harness = pkg.harness
    if annos is None:
        assert osp.isfile(fv), fv
        annos = joblib.load(fv)
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    on_gpu = backend == "nccl"
    if on_gpu:
        torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if on_gpu:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    if model_factory is not None:
        model = model_factory(local_rank)
    elif synthetic_weights:
        model = pkg.build_synthetic_model(max_frames=max_frames, device_id=local_rank, with_gru=False, dtype=dtype, compact_arena=not full_arena)
    else:
        model = pkg.GRNet(writer=None, seqlen=100, featcorr=None, max_frames=max_frames, device_id=local_rank, dtype=dtype, compact_arena=not full_arena)
        ckpt = torch.load(pretrained_file, map_location="cpu")["gen_state_dict"]
        model.load_state_dict(ckpt, strict=True)              # batch_generation.py:218
        model.finalize()
    if rank == 0 and hasattr(model, "arena_info"):
        ai = model.arena_info()
        print(f"Activation arena: {ai['bytes'] / 2**20:.0f} MiB for calls of up to {max_frames} frames "
              f"({'one buffer per tensor' if full_arena else 'buffers shared by liveness'}; the full layout takes {ai['full_bytes'] / 2**20:.0f} MiB)")
    chunk = int(chunk or max_frames)
    dev = torch.device("cuda", local_rank) if on_gpu else torch.device("cpu")
    comm = None
    if exchange == "capi" and world > 1:
        if not on_gpu:
            raise ValueError("exchange='capi' needs the nccl backend (one GPU per rank)")
        comm = harness.RcclComm(world, rank, dev, dist=dist)
    db = pipe.BatchDb(outpath) if rank == 0 else None
    metrics = WindowMetrics(load_ground_truth(gt_path), pipe, model, metrics_on_host) if gt_path and rank == 0 else None
    traj = WindowTrajectory(trajectory["joints2d"], pipe, model, trajectory.get("on_host", False), trajectory.get("focal_length")) \
        if trajectory is not None and rank == 0 else None
    walk = WindowGait(pipe, model, gait.get("on_host", False), **{k: gait[k] for k in ("fps", "sigma", "window", "min_excursion") if gait.get(k) is not None}) \
        if gait is not None and rank == 0 else None
    if kinematics is not None and gait is None:
        raise ValueError("kinematics needs gait: the cycles are cut at the heel strikes it finds")
    angles = WindowKinematics(pipe, model, kinematics.get("on_host", False),
                              **{k: kinematics[k] for k in ("sigma", "min_stride", "max_stride") if kinematics.get(k) is not None}) \
        if kinematics is not None and rank == 0 else None
    if turns is not None and gait is None:
        raise ValueError("turns needs gait: it runs on the events and rows of that call")
    rounds = WindowTurns(pipe, model, turns.get("on_host", False), **({"fps": gait["fps"]} if gait.get("fps") is not None else {}),
                         **{k: turns[k] for k in ("sigma", "edge_rate", "peak_rate", "min_angle", "min_frames", "max_frames") if turns.get(k) is not None}) \
        if turns is not None and rank == 0 else None
    if contacts is not None and gait is None:
        raise ValueError("contacts needs gait: it runs on the events of that call")
    stands = WindowContacts(pipe, model, contacts.get("on_host", False), **({"fps": gait["fps"]} if gait.get("fps") is not None else {}),
                            **{k: contacts[k] for k in ("sigma", "fraction", "speed", "reach", "max_frames") if contacts.get(k) is not None}) \
        if contacts is not None and rank == 0 else None
    if balance is not None and gait is None:
        raise ValueError("balance needs gait: it runs on the events of that call")
    prints = WindowBalance(pipe, model, balance.get("on_host", False), **({"fps": gait["fps"]} if gait.get("fps") is not None else {}),
                           **{k: balance[k] for k in ("gravity", "window", "settle", "max_step") if balance.get(k) is not None}) \
        if balance is not None and rank == 0 else None
    if balance is not None and balance.get("com", "table") not in ("table", "mesh"):
        raise ValueError("balance['com'] is 'table' or 'mesh'")
    mesh_com = balance is not None and balance.get("com", "table") == "mesh"
    if mesh_com and body is None:
        raise ValueError("balance['com'] == 'mesh' needs body: the centres of mass are made there")
    shape = WindowBody(pipe, **({"density": body["density"]} if body.get("density") is not None else {})) if body is not None and rank == 0 else None
    width = 75 if body is None else 75 + 22                    # a row of the all-gather: the joints, then the 11 doubles as 22 float32 words
    if bootstrap is not None and gait is None:
        raise ValueError("bootstrap needs gait: it resamples the steps and strides of that call")
    bars = WindowBootstrap(pipe, model, bootstrap.get("on_host", False), **({"fps": gait["fps"]} if gait.get("fps") is not None else {}),
                           **{k: bootstrap[k] for k in ("replicates", "level", "block", "seed") if bootstrap.get(k) is not None}) \
        if bootstrap is not None and rank == 0 else None
    steady = WindowRegularity(pipe, model, regularity.get("on_host", False), not regularity.get("all_frames", False),
                              **({"fps": gait["fps"]} if regularity.get("fps") is None and gait is not None and gait.get("fps") is not None else {}),
                              **{k: regularity[k] for k in ("fps", "sigma", "max_lag", "min_lag", "min_peak", "min_pairs") if regularity.get(k) is not None}) \
        if regularity is not None and rank == 0 else None
    if harmonics is not None and gait is None:
        raise ValueError("harmonics needs gait: the strides are cut at the heel strikes it finds")
    smooth = WindowHarmonics(pipe, model, harmonics.get("on_host", False), not harmonics.get("all_frames", False), **({"fps": gait["fps"]} if gait.get("fps") is not None else {}),
                             **{k: harmonics[k] for k in ("sigma", "n_harmonics", "derivative", "min_stride", "max_stride") if harmonics.get(k) is not None}) \
        if harmonics is not None and rank == 0 else None
    rough = WindowEntropy(pipe, model, entropy.get("on_host", False), not entropy.get("all_frames", False),
                          **{k: entropy[k] for k in ("sigma", "m", "fraction", "derivative", "scales", "min_templates") if entropy.get(k) is not None}) \
        if entropy is not None and rank == 0 else None
    apart = WindowStability(pipe, model, stability.get("on_host", False), not stability.get("all_frames", False),
                            **({"fps": gait["fps"]} if gait is not None and gait.get("fps") is not None else {}),
                            **{k: stability[k] for k in ("sigma", "derivative", "dim", "lag", "theiler", "horizon", "fit_lo", "fit_hi", "min_pairs") if stability.get(k) is not None}) \
        if stability is not None and rank == 0 else None
    bands = WindowSpectrum(pipe, model, spectrum.get("on_host", False), not spectrum.get("all_frames", False),
                           **({"fps": gait["fps"]} if spectrum.get("fps") is None and gait is not None and gait.get("fps") is not None else {}),
                           **{k: spectrum[k] for k in ("fps", "sigma", "derivative", "segment", "hop", "nfft", "f_lo", "f_hi", "min_segments") if spectrum.get(k) is not None}) \
        if spectrum is not None and rank == 0 else None
    fluent = WindowSmoothness(pipe, model, smoothness.get("on_host", False), not smoothness.get("all_frames", False),
                              **({"fps": gait["fps"]} if smoothness.get("fps") is None and gait is not None and gait.get("fps") is not None else {}),
                              **{k: smoothness[k] for k in ("fps", "sigma", "derivative", "segment", "hop", "nfft", "f_cut", "amplitude", "min_segments")
                                 if smoothness.get(k) is not None}) \
        if smoothness is not None and rank == 0 else None
    again = WindowRecurrence(pipe, model, recurrence.get("on_host", False), not recurrence.get("all_frames", False),
                             **{k: recurrence[k] for k in ("sigma", "derivative", "dim", "lag", "theiler", "radius", "min_line", "min_points") if recurrence.get(k) is not None}) \
        if recurrence is not None and rank == 0 else None
    limbs = WindowCoordination(pipe, model, coordination.get("on_host", False), not coordination.get("all_frames", False),
                               **({"fps": gait["fps"]} if coordination.get("fps") is None and gait is not None and gait.get("fps") is not None else {}),
                               **{k: coordination[k] for k in ("fps", "sigma", "derivative", "segment", "hop", "nfft", "f_lo", "f_hi", "min_segments")
                                  if coordination.get(k) is not None}) \
        if coordination is not None and rank == 0 else None
    vidnames = sorted(os.listdir(vid_folder), key=vid_sort_key)
    start, n_done = time.time(), 0
    for (wa, wb) in flush_windows(len(vidnames), pipe.MAX_VID):
        vids = []                                              # (key, image folder, boxes as the reference stores them)
        for vid_name in vidnames[wa:wb]:
            key = vid_name.split(".")[0]
            if key not in annos:
                if rank == 0 and not (tracks is not None and key in tracks and tracks[key] is None):
                    print(f"Skip video {vid_name}, no precomputed 2D joints!")
                continue
            img_dir = osp.join(vid_folder, vid_name)
            files = sorted(x for x in os.listdir(img_dir) if x.endswith(("png", "jpg", "npy")))
            bboxes = np.array(annos[key])                      # a copy in the annotation's own dtype
            first, status = 0, None
            if tracks is not None and tracks.get(key) is not None:
                (first, end), T, status = tracks[key]["range"], tracks[key]["frames"], tracks[key]["status"]
                assert abs(len(files) - T) < MIN_FDIFF
                if len(files) != T:
                    bboxes, status, stop = align_track(bboxes, status, first, end, T, len(files))
                    if rank == 0:
                        print(f"Track: video {key} has {len(files)} frames and {T} frames of 2D joints: the track [{first}, {end}) is "
                              f"{'held' if stop > end else 'cut'} to [{first}, {stop}).")
                    if traj is not None:                        # the 2D joints alike; a held frame has no detection to fit to (score 0: filled)
                        j2 = traj.joints2d[key][:stop - first]
                        traj.joints2d[key] = np.concatenate([j2, np.zeros((stop - first - j2.shape[0],) + j2.shape[1:], j2.dtype)], 0)
                    if stop <= first:
                        if rank == 0:
                            print(f"Skip video {vid_name}, its track begins behind its last frame!")
                        continue
            else:
                assert abs(len(files) - bboxes.shape[0]) < MIN_FDIFF
                if len(files) != bboxes.shape[0]:              # align frame number (batch_generation.py:258-261)
                    bboxes = np.repeat(bboxes[0, None, :], len(files), axis=0)
            vids.append((key, img_dir, bboxes, first, status))
        items = harness.plan_work_items([v[2].shape[0] for v in vids], world, chunk)
        mine = []
        for vi, lo, hi, r in items:
            if r != rank:
                continue
            # run_on_frames scales the boxes it is given by 1.1 in place (as Inference.__init__ does, inference.py:48):
            # hand it a copy of the UNSCALED rows; the database rows are scaled once below, on every rank alike
            # the joints stay on the device: no host synchronisation per work item, one all-gather per window
            if body is None:
                kp = pipe.run_on_frames(model, vids[vi][1], np.arange(lo, hi) + vids[vi][3], vids[vi][2][lo:hi].copy(), device=dev, batch_size=chunk, on_device=True)["kp_3d"]
                mine.append(kp.reshape(hi - lo, 75))
                continue
            made = pipe.run_on_frames(model, vids[vi][1], np.arange(lo, hi) + vids[vi][3], vids[vi][2][lo:hi].copy(), device=dev, batch_size=chunk, on_device=True,
                                      body=True, body_on_host=bool(body.get("on_host", False)))
            mine.append(torch.cat([made["kp_3d"].reshape(hi - lo, 75), made["body"].contiguous().view(torch.float32).reshape(hi - lo, 22)], 1))
        local = torch.cat(mine, 0) if mine else torch.zeros(0, width, device=dev)
        per_video = harness.gather_work_items(items, local, width, world, rank, dist, dev, comm=comm)
        body_rows = None
        if body is not None:                                   # the doubles viewed back, bit for bit (a copy: a view needs an even offset); the joints as every other stage takes them
            body_rows = {vi: rows[:, 75:].clone(memory_format=torch.contiguous_format).view(torch.float64) for vi, rows in per_video.items()}
            per_video = {vi: rows[:, :75].contiguous() for vi, rows in per_video.items()}
        if metrics is not None:
            metrics.add_window([v[0] for v in vids], per_video)
        fitted = traj.add_window([v[0] for v in vids], per_video) if traj is not None else None
        gait_events = walk.add_window([v[0] for v in vids], per_video, fitted) if walk is not None else None
        body_made = shape.add_window([v[0] for v in vids], per_video, body_rows) if shape is not None and vids else None
        footprints_phase = prints.add_window([v[0] for v in vids], *walk.window, **({"com": shape.com} if mesh_com else {})) if prints is not None and vids else None
        if angles is not None and vids:
            angles.add_window([v[0] for v in vids], *walk.window)
        gait_phase = rounds.add_window([v[0] for v in vids], *walk.window, walk.rows, walk.videos) if rounds is not None and vids else None
        gait_support = stands.add_window([v[0] for v in vids], *walk.window) if stands is not None and vids else None
        if bars is not None and vids:
            bars.add_window([v[0] for v in vids], walk.window[1], walk.window[2], walk.rows, rounds.phase if rounds is not None else None,
                            prints.tables if prints is not None else None)
        if steady is not None and vids:
            steady.add_window([v[0] for v in vids], per_video, fitted, gait_phase, walk.videos if walk is not None else None)
        if smooth is not None and vids:
            smooth.add_window([v[0] for v in vids], *walk.window, fitted, gait_phase)
        if rough is not None and vids:
            rough.add_window([v[0] for v in vids], per_video, fitted, gait_phase)
        if apart is not None and vids:
            apart.add_window([v[0] for v in vids], per_video, fitted, gait_phase)
        if bands is not None and vids:
            bands.add_window([v[0] for v in vids], per_video, fitted, gait_phase, walk.videos if walk is not None else None, steady.videos if steady is not None else None)
        if fluent is not None and vids:
            fluent.add_window([v[0] for v in vids], per_video, fitted, gait_phase)
        if again is not None and vids:
            again.add_window([v[0] for v in vids], per_video, fitted, gait_phase)
        if limbs is not None and vids:
            limbs.add_window([v[0] for v in vids], per_video, gait_phase)
        if rank == 0:
            for vi, (key, _, bboxes, _, status) in enumerate(vids):
                # the reference's db holds the boxes AFTER Inference scaled w,h by 1.1 in place (batch_generation.py:263-266
                # appends the very array the dataset modified)
                bboxes[:, 2:] *= BBOX_SCALE
                extra = dict(zip(("trans", "trans_status", "reproj"), fitted[vi])) if fitted is not None else {}
                if status is not None:
                    extra["bbox_status"] = status
                if gait_events is not None:
                    extra["gait_events"] = gait_events[vi]
                if gait_phase is not None:
                    extra["gait_phase"] = gait_phase[vi]
                if gait_support is not None:
                    extra["gait_support"] = gait_support[vi]
                if footprints_phase is not None:
                    extra["footprints_phase"] = footprints_phase[vi]
                if body_made is not None:
                    extra["body_com"], extra["body_volume"] = body_made[vi]
                db.add(key, bboxes, per_video[vi].cpu().numpy().reshape(-1, 25, 3), **extra)
                n_done += bboxes.shape[0]
            if wb < len(vidnames):
                print(f"Save database to {db.flush()}.")
    if rank == 0:
        print(f"=====>>> Generation frame rate: {n_done / max(time.time() - start, 1e-9):.1f}")
        print(f"Save database to {db.flush()}.")
    if metrics is not None:
        metrics.write(metrics_out or osp.splitext(outpath)[0] + "_metrics.json")
    if walk is not None:
        walk.write(gait.get("out") or osp.splitext(outpath)[0] + "_gait.json")
    if angles is not None:
        angles.write(kinematics.get("out") or osp.splitext(outpath)[0] + "_kinematics.json")
    if rounds is not None:
        rounds.write(turns.get("out") or osp.splitext(outpath)[0] + "_turns.json")
    if stands is not None:
        stands.write(contacts.get("out") or osp.splitext(outpath)[0] + "_contacts.json")
    if steady is not None:
        steady.write(regularity.get("out") or osp.splitext(outpath)[0] + "_regularity.json")
    if smooth is not None:
        smooth.write(harmonics.get("out") or osp.splitext(outpath)[0] + "_harmonics.json")
    if rough is not None:
        rough.write(entropy.get("out") or osp.splitext(outpath)[0] + "_entropy.json")
    if apart is not None:
        apart.write(stability.get("out") or osp.splitext(outpath)[0] + "_stability.json")
    if bands is not None:
        bands.write(spectrum.get("out") or osp.splitext(outpath)[0] + "_spectrum.json")
    if fluent is not None:
        fluent.write(smoothness.get("out") or osp.splitext(outpath)[0] + "_smoothness.json")
    if again is not None:
        again.write(recurrence.get("out") or osp.splitext(outpath)[0] + "_recurrence.json")
    if limbs is not None:
        limbs.write(coordination.get("out") or osp.splitext(outpath)[0] + "_coordination.json")
    if prints is not None:
        prints.write(balance.get("out") or osp.splitext(outpath)[0] + "_balance.json")
    if shape is not None:
        shape.write(body.get("out") or osp.splitext(outpath)[0] + "_body.json")
    if bars is not None:
        bars.write(bootstrap.get("out") or osp.splitext(outpath)[0] + "_bootstrap.json")
    if comm is not None:
        torch.cuda.synchronize()
        comm.close()
    if hasattr(model, "close"):
        model.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return db.written if rank == 0 else []


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--vid_folder", type=str, default="", help="folder containing one frame folder per video.")
    p.add_argument("--bbox_path", type=str, default="", help="joblib file with the precomputed bbox per video.")
    p.add_argument("--openpose_folder", type=str, default="", help="folder of OpenPose .mat files ('skeleton': (P,T,25,3), normalised): the boxes are made from them "
                   "(the reference's load_openpose_anno) instead of read from --bbox_path; without --vid_folder the script writes --bbox_out and exits")
    p.add_argument("--bbox_out", type=str, default="", help="with --openpose_folder: joblib file that receives the boxes (the files without usable joints: FILE.bad)")
    p.add_argument("--bbox_on_host", action="store_true", help="with --openpose_folder: the numpy float64 statement of the box instead of the GPU kernels")
    p.add_argument("--bbox_track", action="store_true", help="with --openpose_folder: one box PER FRAME for the chosen person of each video instead of the one fixed "
                   "box (the reference's lib/utils/smooth_bbox.py, as its Inference(joints2d=...) uses it): gaps without a detection are interpolated, frames before "
                   "the first and after the last detection are dropped, the database gains 'bbox_status' (N,) (0 detected, 1 interpolated)")
    p.add_argument("--bbox_smooth", action="store_true", help="with --bbox_track: the median and the Gaussian of smooth_bbox_params over the track")
    p.add_argument("--bbox_kernel", type=int, default=None, help="with --bbox_smooth: the median's window, odd, 1 to 31 (default 11)")
    p.add_argument("--bbox_sigma", type=float, default=None, help="with --bbox_smooth: the Gaussian's sigma in frames, 0 (none) to 16 (default 3)")
    p.add_argument("--bbox_pad", choices=("zero", "edge"), default=None, help="with --bbox_smooth: what the median's window holds outside the track: zeros (scipy's "
                   "medfilt, the reference; the first and last frames of a track then lose their box and the script stops) or the first / last value (default zero)")
    p.add_argument("--gt_path", type=str, default="", help="joblib database in this script's output schema ('vid_name' (F,), 'joints3D' (F,25,3) kinectv2): report MPJPE, "
                   "PA-MPJPE, acceleration and acceleration error per video against it (millimetres); a video it lacks, or of another length, is skipped")
    p.add_argument("--metrics_out", type=str, default="", help="with --gt_path: the JSON file of the metrics (default: --outpath with _metrics.json)")
    p.add_argument("--metrics_on_host", action="store_true", help="with --gt_path: the numpy float64 statement of the metrics instead of the GPU kernels")
    p.add_argument("--trajectory", action="store_true", help="with --openpose_folder and --vid_folder: fit the camera-space translation of every frame to the 2D joints "
                   "of the person the box was made from and add 'trans' (N,3), 'trans_status' (N,) (0 fitted, 1 too few joints, 2 degenerate, 3 filled) and "
                   "'reproj' (N,) pixels to the database; one line per video")
    p.add_argument("--focal_length", type=float, default=0.0, help="with --trajectory: the focal length in pixels.  The data carries no calibration: the default "
                   f"sqrt({IMG_W}^2 + {IMG_H}^2) (a 53 degree diagonal field of view) and the centre ({IMG_W // 2}, {IMG_H // 2}) are ASSUMPTIONS, and depth "
                   "scales with the focal length")
    p.add_argument("--trajectory_on_host", action="store_true", help="with --trajectory: the numpy float64 statement of the fit instead of the GPU kernels")
    p.add_argument("--gait", action="store_true", help="with --vid_folder: heel strikes, toe-offs and the gait parameters of every video from its 3D joints (cadence, step "
                   "and stride time with their variability, step length and width, stance share, speed; with --trajectory the speed along the fitted trajectory too): "
                   "'gait_events' (N,) in the database, the parameters in <outpath>_gait.json, one line per video")
    p.add_argument("--gait_out", type=str, default="", help="with --gait: the JSON file of the parameters (default: --outpath with _gait.json)")
    p.add_argument("--gait_fps", type=float, default=None, help="with --gait: frames a second of the extracted frames (default 20, what the reference extracts at)")
    p.add_argument("--gait_sigma", type=float, default=None, help="with --gait: sigma in frames of the Gaussian over the ankle and foot signals, 0 (none) to 16 (default 2)")
    p.add_argument("--gait_window", type=int, default=None, help="with --gait: an event is the extreme of this many frames on either side, 1 to 32 (default 5)")
    p.add_argument("--gait_min_excursion", type=float, default=None, help="with --gait: metres a signal must rise or fall within the window for an event (default 0.05)")
    p.add_argument("--gait_on_host", action="store_true", help="with --gait: the numpy float64 statement instead of the GPU kernels")
    p.add_argument("--gait_kinematics", action="store_true", help="with --gait: hip, knee, ankle, shoulder and elbow angles and the trunk's inclination per gait cycle "
                   "(101 points, mean and SD over the strides), each joint's range of motion and left / right symmetry, in <outpath>_kinematics.json, one line per video")
    p.add_argument("--kinematics_out", type=str, default="", help="with --gait_kinematics: the JSON file (default: --outpath with _kinematics.json)")
    p.add_argument("--kinematics_sigma", type=float, default=None, help="with --gait_kinematics: sigma in frames of the Gaussian over the angles, 0 (none) to 16 (default 2)")
    p.add_argument("--kinematics_min_stride", type=int, default=None, help="with --gait_kinematics: the shortest stride that is used, in frames (default 8: 0.4 s at 20 fps)")
    p.add_argument("--kinematics_max_stride", type=int, default=None, help="with --gait_kinematics: the longest stride that is used, in frames, at most 4096 (default 60: 3 s)")
    p.add_argument("--kinematics_on_host", action="store_true", help="with --gait_kinematics: the numpy float64 statement instead of the GPU kernels")
    p.add_argument("--gait_turns", action="store_true", help="with --gait: where the subject turns round (yaw rate of the pelvis in the camera's horizontal plane) and the "
                   "step and stride columns of --gait over straight walking alone: 'gait_phase' (N,) in the database, <outpath>_turns.json, one line per video; the "
                   "default thresholds follow El-Gohary et al. 2014 and are unvalidated on the model's output")
    p.add_argument("--turns_out", type=str, default="", help="with --gait_turns: the JSON file (default: --outpath with _turns.json)")
    p.add_argument("--turns_sigma", type=float, default=None, help="with --gait_turns: sigma in frames of the Gaussian over the yaw rate, 0 (none) to 16 (default 8)")
    p.add_argument("--turns_edge_rate", type=float, default=None, help="with --gait_turns: a turn is a run of yaw rate beyond this many degrees a second (default 5)")
    p.add_argument("--turns_peak_rate", type=float, default=None, help="with --gait_turns: ... that peaks at this many degrees a second or more (default 15)")
    p.add_argument("--turns_min_angle", type=float, default=None, help="with --gait_turns: ... and covers this many degrees or more (default 45)")
    p.add_argument("--turns_min_duration", type=float, default=None, help="with --gait_turns: the shortest turn in seconds, made frames through --gait_fps (default 0.5)")
    p.add_argument("--turns_max_duration", type=float, default=None, help="with --gait_turns: the longest turn in seconds, made frames through --gait_fps (default 10)")
    p.add_argument("--turns_on_host", action="store_true", help="with --gait_turns: the numpy float64 statement instead of the GPU kernels")
    p.add_argument("--gait_contacts", action="store_true", help="with --gait: when both feet are on the ground (low runs of the speed of the vector from one ankle to the "
                   "other, led by the heel strikes of --gait) and double-support, single-support, swing and stance time: 'gait_support' (N,) in the database, "
                   "<outpath>_contacts.json, one line per video; the thresholds are unvalidated on the model's output")
    p.add_argument("--contacts_out", type=str, default="", help="with --gait_contacts: the JSON file (default: --outpath with _contacts.json)")
    p.add_argument("--contacts_sigma", type=float, default=None, help="with --gait_contacts: sigma in frames of the Gaussian over the inter-foot vector, 0 (none) to 16 "
                   "(default 0: smoothing shortens the runs)")
    p.add_argument("--contacts_fraction", type=float, default=None, help="with --gait_contacts: static is below this share of the mean inter-foot speed (default 0.25)")
    p.add_argument("--contacts_speed", type=float, default=None, help="with --gait_contacts: above 0, static is below this many metres a second instead (default 0)")
    p.add_argument("--contacts_reach", type=int, default=None, help="with --gait_contacts: a heel strike leads a run within this many frames of it, 0 to 8 (default 2)")
    p.add_argument("--contacts_max_duration", type=float, default=None, help="with --gait_contacts: the longest double support in seconds, made frames through --gait_fps "
                   "(default 1.0); a longer run is standing")
    p.add_argument("--contacts_on_host", action="store_true", help="with --gait_contacts: the numpy float64 statement instead of the GPU kernels")
    p.add_argument("--gait_balance", action="store_true", help="with --gait: the footprints chained strike after strike (a foot on the ground stands still in the world), stride "
                   "length, step length and step width against the line of progression, the speed over the ground, and the margin of stability at foot placement forward "
                   "and sideways (Hof et al. 2005) from a centre of mass of Winter's segment masses: 'footprints_phase' (N,) in the database, <outpath>_balance.json, one "
                   "line per video; the floor is the x-z plane of a level, fixed camera, and the segment layout is unvalidated")
    p.add_argument("--balance_out", type=str, default="", help="with --gait_balance: the JSON file (default: --outpath with _balance.json)")
    p.add_argument("--balance_window", type=int, default=None, help="with --gait_balance: the centre of mass's velocity is the slope over this many frames before the landing, "
                   "1 to 16 (default 4)")
    p.add_argument("--balance_settle", type=int, default=None, help="with --gait_balance: the vector between the ankles is read this many frames after the heel strike, 0 to 4 "
                   "(default 1: the strike's extremum may fall on the frame before the landing)")
    p.add_argument("--balance_max_step", type=int, default=None, help="with --gait_balance: two heel strikes further apart than this many frames are no step (default 30)")
    p.add_argument("--balance_gravity", type=float, default=None, help="with --gait_balance: metres a second squared; the joints are SMPL metres (default 9.81)")
    p.add_argument("--balance_on_host", action="store_true", help="with --gait_balance: the numpy float64 statement instead of the GPU kernels")
    p.add_argument("--balance_com", type=str, default=None, choices=("table", "mesh"), help="with --gait_balance: the centre of mass it rests on: table = Winter's segment masses on "
                   "the kinectv2 joints (default), mesh = the mesh's own of --gait_body, which must be given")
    p.add_argument("--gait_body", action="store_true", help="with --vid_folder (no --gait needed): volume, centre of mass, central second moments and area of the SMPL mesh of every "
                   "frame, exact sums over its closed surface, made where the vertices lie: 'body_com' (N,3) and 'body_volume' (N,) in the database, <outpath>_body.json, one "
                   "'Body:' line per video.  Uniform density is an assumption; the mesh is a statistical body shape, not the subject's.  Reported, never judged")
    p.add_argument("--body_out", type=str, default="", help="with --gait_body: the JSON file (default: --outpath with _body.json)")
    p.add_argument("--body_density", type=float, default=None, help="with --gait_body: kilograms a cubic metre for the mass column (default 985, a whole-body textbook figure)")
    p.add_argument("--body_on_host", action="store_true", help="with --gait_body: the numpy float64 statement after a download instead of the GPU kernel")
    p.add_argument("--gait_bootstrap", action="store_true", help="with --gait: percentile intervals of the step and stride parameters (mean, SD and CV of step time, step "
                   "length, step width and stride time; with --gait_turns also over straight walking alone, with --gait_balance also of stride length, step length, "
                   "step width and the margins of stability) by resampling the steps and strides with replacement on the device.  An interval from some 15 strides "
                   "under-covers (about 0.91 where 0.95 is asked) and the steps of a walk are serially correlated; reported, never judged")
    p.add_argument("--bootstrap_out", type=str, default="", help="with --gait_bootstrap: the JSON file (default: --outpath with _bootstrap.json)")
    p.add_argument("--bootstrap_replicates", type=int, default=None, help="with --gait_bootstrap: the resamples B, 1 to 4096 (default 2000)")
    p.add_argument("--bootstrap_level", type=float, default=None, help="with --gait_bootstrap: the interval's level in percent (default 95: the 2.5 and 97.5 percent points)")
    p.add_argument("--bootstrap_block", type=int, default=None, help="with --gait_bootstrap: rows are drawn in circular blocks of this many consecutive ones, 1 to 1024; 2 keeps "
                   "a left and a right step together (default 1, the plain bootstrap)")
    p.add_argument("--bootstrap_seed", type=int, default=None, help="with --gait_bootstrap: the generator's seed, 0 to 2^64 - 1 (default 0); equal seeds give equal files")
    p.add_argument("--bootstrap_on_host", action="store_true", help="with --gait_bootstrap: the numpy statement instead of the GPU kernels (the same bits)")
    p.add_argument("--gait_regularity", action="store_true", help="with --vid_folder (no --gait needed): step and stride regularity, symmetry and a cadence WITHOUT events, "
                   "from the autocorrelation of four body signals (Moe-Nilssen and Helbostad 2004): <outpath>_regularity.json, one line per video; takes "
                   "--gait_fps where given; with --gait_turns only straight walking counts; the defaults are unvalidated on the model's output")
    p.add_argument("--regularity_out", type=str, default="", help="with --gait_regularity: the JSON file (default: --outpath with _regularity.json)")
    p.add_argument("--regularity_sigma", type=float, default=None, help="with --gait_regularity: sigma in frames of the Gaussian over the four signals, 0 (none) to 16 (default 0)")
    p.add_argument("--regularity_max_lag", type=int, default=None, help="with --gait_regularity: the largest lag in frames, 8 to 255 (default 60)")
    p.add_argument("--regularity_min_lag", type=int, default=None, help="with --gait_regularity: the first peak is looked for from this lag on, 2 to the largest lag - 2 (default 4)")
    p.add_argument("--regularity_min_peak", type=float, default=None, help="with --gait_regularity: the first peak is at least this high, above 0 up to 1 (default 0.25)")
    p.add_argument("--regularity_min_pairs", type=int, default=None, help="with --gait_regularity: a lag with fewer pairs of frames is undefined, 2 to 2^20 (default 20)")
    p.add_argument("--regularity_all_frames", action="store_true", help="with --gait_regularity and --gait_turns: count the frames of the turns too")
    p.add_argument("--regularity_on_host", action="store_true", help="with --gait_regularity: the numpy float64 statement instead of the GPU kernels")
    p.add_argument("--gait_harmonics", action="store_true", help="with --gait: the harmonic ratio of every stride between two heel strikes of one foot, of four body "
                   "signals (Smidt et al. 1971, Menz et al. 2003, Bellanca et al. 2013): <outpath>_harmonics.json, one line per video; the defaults are unvalidated on the "
                   "model's output")
    p.add_argument("--harmonics_out", type=str, default="", help="with --gait_harmonics: the JSON file (default: --outpath with _harmonics.json)")
    p.add_argument("--harmonics_sigma", type=float, default=None, help="with --gait_harmonics: sigma in frames of the Gaussian over the four signals, 0 (none) to 16 (default 0: "
                   "a Gaussian damps the harmonics)")
    p.add_argument("--harmonics_count", type=int, default=None, help="with --gait_harmonics: the harmonics of a stride, even, 2 to 32 (default 20)")
    p.add_argument("--harmonics_derivative", type=int, default=None, help="with --gait_harmonics: 0 the signal, 1 its velocity, 2 its acceleration (default 2)")
    p.add_argument("--harmonics_min_stride", type=int, default=None, help="with --gait_harmonics: the shortest stride in frames, 6 to the longest (default 8)")
    p.add_argument("--harmonics_max_stride", type=int, default=None, help="with --gait_harmonics: the longest stride in frames, up to 255 (default 60)")
    p.add_argument("--harmonics_all_frames", action="store_true", help="with --gait_harmonics and --gait_turns: count the strides of the turns too")
    p.add_argument("--harmonics_on_host", action="store_true", help="with --gait_harmonics: the numpy float64 statement instead of the GPU kernels")
    p.add_argument("--gait_entropy", action="store_true", help="with --vid_folder (no --gait needed): the sample entropy of four body signals at several scales and their "
                   "complexity index (Richman and Moorman 2000, Costa et al. 2002, Lamoth et al. 2011): <outpath>_entropy.json, one line per video; quadratic in a "
                   "video's frames; the defaults are unvalidated on the model's output")
    p.add_argument("--entropy_out", type=str, default="", help="with --gait_entropy: the JSON file (default: --outpath with _entropy.json)")
    p.add_argument("--entropy_sigma", type=float, default=None, help="with --gait_entropy: sigma in frames of the Gaussian over the four signals, 0 (none) to 16 (default 0)")
    p.add_argument("--entropy_m", type=int, default=None, help="with --gait_entropy: the template length, 1 to 4 (default 2)")
    p.add_argument("--entropy_r", type=float, default=None, help="with --gait_entropy: the tolerance as a fraction of the signal's SD, above 0 up to 10 (default 0.2)")
    p.add_argument("--entropy_derivative", type=int, default=None, help="with --gait_entropy: 0 the signal, 1 its velocity, 2 its acceleration (default 2)")
    p.add_argument("--entropy_scales", type=int, default=None, help="with --gait_entropy: the scales of the coarse-graining, 1 to 8 (default 3)")
    p.add_argument("--entropy_min_templates", type=int, default=None, help="with --gait_entropy: a scale with fewer valid templates has no sample entropy, at least 1 (default 50)")
    p.add_argument("--entropy_all_frames", action="store_true", help="with --gait_entropy and --gait_turns: count the frames of the turns too")
    p.add_argument("--entropy_on_host", action="store_true", help="with --gait_entropy: the numpy float64 statement instead of the GPU kernels")
    p.add_argument("--gait_stability", action="store_true", help="with --vid_folder (no --gait needed): the local dynamic stability of four body signals, the short-term "
                   "divergence exponent of nearest neighbours in the delay-embedded signal (Rosenstein et al. 1993, Dingwell and Cusumano 2000, Lamoth et al. 2011): "
                   "<outpath>_stability.json, one line per video; in 1/s through --gait_fps where --gait is given, else at 20 frames a second; quadratic in a video's "
                   "frames; the papers use a trunk sensor and 100+ strides, where these are joint positions of a pose model and 400 frames at 20 fps hold some 15 strides; "
                   "on a walker with 5 mm of joint noise the divergence curve saturates within about 5 frames, so on such data the slope mostly measures the noise; the "
                   "defaults are unvalidated on the model's output; reported, never judged")
    p.add_argument("--stability_out", type=str, default="", help="with --gait_stability: the JSON file (default: --outpath with _stability.json)")
    p.add_argument("--stability_sigma", type=float, default=None, help="with --gait_stability: sigma in frames of the Gaussian over the four signals, 0 (none) to 16 (default 0)")
    p.add_argument("--stability_derivative", type=int, default=None, help="with --gait_stability: 0 the signal, 1 its velocity, 2 its acceleration (default 1, this project's choice)")
    p.add_argument("--stability_dim", type=int, default=None, help="with --gait_stability: the embedding dimension, 2 to 8 (default 5)")
    p.add_argument("--stability_lag", type=int, default=None, help="with --gait_stability: the embedding delay in frames, 1 to 16 (default 2)")
    p.add_argument("--stability_theiler", type=int, default=None, help="with --gait_stability: a neighbour lies more than this many frames away, 0 to 4096 (default 20, about a stride)")
    p.add_argument("--stability_horizon", type=int, default=None, help="with --gait_stability: the frames a pair of neighbours is followed, 1 to 63 (default 20, one second)")
    p.add_argument("--stability_fit_lo", type=int, default=None, help="with --gait_stability: the first frame of the slope's window, at least 0 (default 0)")
    p.add_argument("--stability_fit_hi", type=int, default=None, help="with --gait_stability: the last frame of the slope's window, above --stability_fit_lo and at most "
                   "--stability_horizon (default 10, or the horizon where that is shorter)")
    p.add_argument("--stability_min_pairs", type=int, default=None, help="with --gait_stability: a frame of the curve with fewer pairs has no divergence, at least 1 (default 50)")
    p.add_argument("--stability_all_frames", action="store_true", help="with --gait_stability and --gait_turns: count the frames of the turns too")
    p.add_argument("--stability_on_host", action="store_true", help="with --gait_stability: the numpy float64 statement instead of the GPU kernels")
    p.add_argument("--gait_spectrum", action="store_true", help="with --vid_folder (no --gait needed): the Welch power spectral density of four body signals and, in the band "
                   "--spectrum_f_lo to --spectrum_f_hi, its dominant frequency, the peak's height and width, the spread of the power and a cadence (Welch 1967, Weiss et al. "
                   "2011): <outpath>_spectrum.json, one line per video; in Hz through --gait_fps where given, else at 20 frames a second; with --gait_turns only straight "
                   "walking counts; the peak's width has a floor set by --spectrum_segment, and the defaults are unvalidated on the model's output")
    p.add_argument("--spectrum_out", type=str, default="", help="with --gait_spectrum: the JSON file (default: --outpath with _spectrum.json)")
    p.add_argument("--spectrum_sigma", type=float, default=None, help="with --gait_spectrum: sigma in frames of the Gaussian over the four signals, 0 (none) to 16 (default 0)")
    p.add_argument("--spectrum_derivative", type=int, default=None, help="with --gait_spectrum: 0 the signal, 1 its velocity, 2 its acceleration (default 2)")
    p.add_argument("--spectrum_segment", type=int, default=None, help="with --gait_spectrum: the frames of a segment, even, 8 to 256 (default 64)")
    p.add_argument("--spectrum_hop", type=int, default=None, help="with --gait_spectrum: the frames between two segments, an eighth of a segment to a whole one (default half)")
    p.add_argument("--spectrum_nfft", type=int, default=None, help="with --gait_spectrum: the points of the zero-padded transform, even, a segment to 1024 (default 256)")
    p.add_argument("--spectrum_f_lo", type=float, default=None, help="with --gait_spectrum: the band's lower edge in Hz, above 0 (default 0.5)")
    p.add_argument("--spectrum_f_hi", type=float, default=None, help="with --gait_spectrum: the band's upper edge in Hz, above --spectrum_f_lo and at most half the frames a second "
                   "(default 3)")
    p.add_argument("--spectrum_min_segments", type=int, default=None, help="with --gait_spectrum: a video with fewer segments has no spectrum, at least 1 (default 2)")
    p.add_argument("--spectrum_all_frames", action="store_true", help="with --gait_spectrum and --gait_turns: count the frames of the turns too")
    p.add_argument("--spectrum_on_host", action="store_true", help="with --gait_spectrum: the numpy float64 statement instead of the GPU kernels")
    p.add_argument("--gait_smoothness", action="store_true", help="with --vid_folder (no --gait needed): the movement smoothness of four body signals, per segment of ongoing walking: "
                   "the spectral arc length (SPARC) and the log dimensionless jerk (LDLJ) of Balasubramanian et al. 2015: <outpath>_smoothness.json, one line per video; in Hz "
                   "through --gait_fps where given, else at 20 frames a second; with --gait_turns only straight walking counts; THE INPUTS ARE JOINT POSITIONS OF A POSE MODEL "
                   "AT 20 FPS, where the cut-off of 10 Hz is the Nyquist frequency; a segment's rectangular window alone gives a noiseless sinusoid SPARC about -4 at 64 "
                   "frames, with 5 mm of joint noise a good part of the number is the noise, and THE DEFAULTS ARE UNVALIDATED on the model's output")
    p.add_argument("--smoothness_out", type=str, default="", help="with --gait_smoothness: the JSON file (default: --outpath with _smoothness.json)")
    p.add_argument("--smoothness_sigma", type=float, default=None, help="with --gait_smoothness: sigma in frames of the Gaussian over the four signals, 0 (none) to 16 (default 0)")
    p.add_argument("--smoothness_derivative", type=int, default=None, help="with --gait_smoothness: 0 the signal, 1 its velocity, 2 its acceleration (default 1: a speed profile)")
    p.add_argument("--smoothness_segment", type=int, default=None, help="with --gait_smoothness: the frames of a segment, even, 8 to 256 (default 64)")
    p.add_argument("--smoothness_hop", type=int, default=None, help="with --gait_smoothness: the frames between two segments, an eighth of a segment to a whole one (default half)")
    p.add_argument("--smoothness_nfft", type=int, default=None, help="with --gait_smoothness: the points of the zero-padded transform, even, a segment to 4096 (default 1024)")
    p.add_argument("--smoothness_cutoff", type=float, default=None, help="with --gait_smoothness: the highest frequency of the arc in Hz, above 0 and at most half the frames a "
                   "second (default: 10, or half the frames a second where that is less)")
    p.add_argument("--smoothness_amplitude", type=float, default=None, help="with --gait_smoothness: the normalised magnitude that bounds the band, above 0 to 1 (default 0.05)")
    p.add_argument("--smoothness_min_segments", type=int, default=None, help="with --gait_smoothness: a video with fewer segments has no row, at least 1 (default 2)")
    p.add_argument("--smoothness_all_frames", action="store_true", help="with --gait_smoothness and --gait_turns: count the frames of the turns too")
    p.add_argument("--smoothness_on_host", action="store_true", help="with --gait_smoothness: the numpy float64 statement instead of the GPU kernels")
    p.add_argument("--gait_recurrence", action="store_true", help="with --vid_folder (no --gait needed): the recurrence quantification of four body signals -- recurrence rate, "
                   "determinism, mean and longest diagonal line, divergence and line entropy of the delay-embedded signal (Webber and Zbilut 1994, Marwan et al. 2007): "
                   "<outpath>_recurrence.json, one line per video; quadratic in a video's frames; with --gait_turns only straight walking counts; the radius rule is this "
                   "project's and the defaults are unvalidated on the model's output")
    p.add_argument("--recurrence_out", type=str, default="", help="with --gait_recurrence: the JSON file (default: --outpath with _recurrence.json)")
    p.add_argument("--recurrence_sigma", type=float, default=None, help="with --gait_recurrence: sigma in frames of the Gaussian over the four signals, 0 (none) to 16 (default 0)")
    p.add_argument("--recurrence_derivative", type=int, default=None, help="with --gait_recurrence: 0 the signal, 1 its velocity, 2 its acceleration (default 1, as --gait_stability)")
    p.add_argument("--recurrence_dim", type=int, default=None, help="with --gait_recurrence: the embedding dimension, 2 to 8 (default 5)")
    p.add_argument("--recurrence_lag", type=int, default=None, help="with --gait_recurrence: the embedding delay in frames, 1 to 16 (default 2)")
    p.add_argument("--recurrence_radius", type=float, default=None, help="with --gait_recurrence: the radius in SDs of the signal, above 0 and at most 10 (default 0.8); two points "
                   "recur where their squared distance is at most (radius SD)^2 times the dimension")
    p.add_argument("--recurrence_theiler", type=int, default=None, help="with --gait_recurrence: a pair's points lie more than this many frames apart, 0 to 4096 (default 8, the "
                   "default embedding's span)")
    p.add_argument("--recurrence_min_line", type=int, default=None, help="with --gait_recurrence: the shortest diagonal line that counts, 1 to 255 (default 2)")
    p.add_argument("--recurrence_min_points", type=int, default=None, help="with --gait_recurrence: a video with fewer valid points has no rates, at least 1 (default 50)")
    p.add_argument("--recurrence_all_frames", action="store_true", help="with --gait_recurrence and --gait_turns: count the frames of the turns too")
    p.add_argument("--recurrence_on_host", action="store_true", help="with --gait_recurrence: the numpy float64 statement instead of the GPU kernels")
    p.add_argument("--gait_coordination", action="store_true", help="with --vid_folder (no --gait needed): arm swing and inter-limb coordination from the shoulder and hip flexion "
                   "of both sides -- per limb the swing amplitude in the band --coordination_f_lo to --coordination_f_hi, the left / right asymmetry of arms and legs, and per "
                   "pair of limbs the coherence, the phase and its deviation from the expected 0 or 180 degrees at the stride frequency (Carter et al. 1973, Wagenaar and van "
                   "Emmerik 2000, Plotnik et al. 2007, Mirelman et al. 2016): <outpath>_coordination.json, one line per video; in Hz through --gait_fps where given, else at 20 "
                   "frames a second; with --gait_turns only straight walking counts; these are joint-position angles of a pose model over some 15 strides: with K segments "
                   "the coherence of two unrelated signals is about 1 / K (0.09 at the 11 segments of 400 frames), not 0, and with one segment it is identically 1; the "
                   "defaults are unvalidated on the model's output, and the numbers are reported, never judged")
    p.add_argument("--coordination_out", type=str, default="", help="with --gait_coordination: the JSON file (default: --outpath with _coordination.json)")
    p.add_argument("--coordination_sigma", type=float, default=None, help="with --gait_coordination: sigma in frames of the Gaussian over the four angles, 0 (none) to 16 (default 0)")
    p.add_argument("--coordination_derivative", type=int, default=None, help="with --gait_coordination: 0 the angle, so that amplitudes are degrees, 1 its velocity, 2 its "
                   "acceleration (default 0)")
    p.add_argument("--coordination_segment", type=int, default=None, help="with --gait_coordination: the frames of a segment, even, 8 to 256 (default 64)")
    p.add_argument("--coordination_hop", type=int, default=None, help="with --gait_coordination: the frames between two segments, an eighth of a segment to a whole one (default half)")
    p.add_argument("--coordination_nfft", type=int, default=None, help="with --gait_coordination: the points of the zero-padded transform, even, a segment to 1024 (default 256)")
    p.add_argument("--coordination_f_lo", type=float, default=None, help="with --gait_coordination: the band's lower edge in Hz, above 0 (default 0.5)")
    p.add_argument("--coordination_f_hi", type=float, default=None, help="with --gait_coordination: the band's upper edge in Hz, above --coordination_f_lo and at most half the "
                   "frames a second (default 3.0)")
    p.add_argument("--coordination_min_segments", type=int, default=None, help="with --gait_coordination: a video with fewer segments has no spectra, at least 2 -- the coherence "
                   "of one segment is 1 whatever the signals are (default 4)")
    p.add_argument("--coordination_all_frames", action="store_true", help="with --gait_coordination and --gait_turns: count the frames of the turns too")
    p.add_argument("--coordination_on_host", action="store_true", help="with --gait_coordination: the numpy float64 statement instead of the GPU kernels")
    p.add_argument("--outpath", type=str, default=f"data/{time.strftime('%Y%m%d-%H%M%S')}.json")
    p.add_argument("--pretrained_file", type=str, default="checkpoint/max-grnet.pth.tar")
    p.add_argument("--synthetic_weights", action="store_true")
    p.add_argument("--max_frames", type=int, default=400, help="frames per grnet_forward call (activation buffers are sized for it; 400 = the reference's MAX_seqlen: larger calls run the convolutions at a higher rate, 5 800 / 5 880 / 5 930 frames/s at 128 / 256 / 400)")
    p.add_argument("--chunk", type=int, default=None, help="frames per multi-GPU work item (default: --max_frames)")
    p.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    p.add_argument("--full_arena", action="store_true", help="one buffer per intermediate tensor (the library's default layout: 41 GB at 400 frames in f32 "
                   "against 5.5 GB); this script never reads intermediates, so it shares buffers by liveness -- same launches, bit-identical outputs")
    p.add_argument("--exchange", choices=("torch", "capi"), default="torch", help="multi-GPU: the all-gather through torch.distributed or through the C ABI's grnet_allgather")
    a = p.parse_args(argv)
    if a.bbox_path and a.openpose_folder:
        sys.exit("batch_generation.py: --bbox_path and --openpose_folder both name the source of the boxes: give one of them")
    if (a.bbox_out or a.bbox_on_host) and not a.openpose_folder:
        sys.exit("batch_generation.py: --bbox_out and --bbox_on_host belong to --openpose_folder, which was not given")
    if (a.bbox_track or a.bbox_smooth) and not a.openpose_folder:
        sys.exit("batch_generation.py: --bbox_track and --bbox_smooth belong to --openpose_folder, which was not given")
    if a.bbox_smooth and not a.bbox_track:
        sys.exit("batch_generation.py: --bbox_smooth belongs to --bbox_track, which was not given")
    if (a.bbox_kernel is not None or a.bbox_sigma is not None or a.bbox_pad is not None) and not a.bbox_smooth:
        sys.exit("batch_generation.py: --bbox_kernel, --bbox_sigma and --bbox_pad belong to --bbox_smooth, which was not given")
    if a.bbox_kernel is not None and not (1 <= a.bbox_kernel <= 31 and a.bbox_kernel % 2 == 1):
        sys.exit("batch_generation.py: --bbox_kernel must be odd and within 1 to 31")
    if a.bbox_sigma is not None and not (np.isfinite(a.bbox_sigma) and 0 <= a.bbox_sigma <= 16):
        sys.exit("batch_generation.py: --bbox_sigma must be within 0 to 16")
    if (a.metrics_out or a.metrics_on_host) and not a.gt_path:
        sys.exit("batch_generation.py: --metrics_out and --metrics_on_host belong to --gt_path, which was not given")
    if (a.focal_length or a.trajectory_on_host) and not a.trajectory:
        sys.exit("batch_generation.py: --focal_length and --trajectory_on_host belong to --trajectory, which was not given")
    if a.trajectory and a.bbox_path:
        sys.exit("batch_generation.py: --trajectory fits to the 2D joints of --openpose_folder; --bbox_path carries none")
    if a.trajectory and not (a.openpose_folder and a.vid_folder):
        sys.exit("batch_generation.py: --trajectory needs --openpose_folder (the 2D joints) and --vid_folder (the frames)")
    if a.trajectory and not (np.isfinite(a.focal_length) and a.focal_length >= 0):
        sys.exit("batch_generation.py: --focal_length must be a positive number of pixels")
    for flag, given in (("--gait_out", bool(a.gait_out)), ("--gait_fps", a.gait_fps is not None), ("--gait_sigma", a.gait_sigma is not None),
                        ("--gait_window", a.gait_window is not None), ("--gait_min_excursion", a.gait_min_excursion is not None), ("--gait_on_host", a.gait_on_host)):
        if given and not a.gait and not (flag == "--gait_fps" and (a.gait_regularity or a.gait_spectrum or a.gait_coordination or a.gait_smoothness)):
            sys.exit(f"batch_generation.py: {flag} belongs to --gait, which was not given")
    if a.gait and not a.vid_folder:
        sys.exit("batch_generation.py: --gait needs --vid_folder (the frames whose joints it reads)")
    if a.gait_fps is not None and not (np.isfinite(a.gait_fps) and a.gait_fps > 0):
        sys.exit("batch_generation.py: --gait_fps must be a positive number of frames a second")
    if a.gait_sigma is not None and not (np.isfinite(a.gait_sigma) and 0 <= a.gait_sigma <= 16):
        sys.exit("batch_generation.py: --gait_sigma must be within 0 to 16")
    if a.gait_window is not None and not 1 <= a.gait_window <= 32:
        sys.exit("batch_generation.py: --gait_window must be within 1 to 32")
    if a.gait_min_excursion is not None and not (np.isfinite(a.gait_min_excursion) and a.gait_min_excursion >= 0):
        sys.exit("batch_generation.py: --gait_min_excursion must be a number of metres, not negative")
    if a.gait_kinematics and not a.gait:
        sys.exit("batch_generation.py: --gait_kinematics belongs to --gait, which was not given (the cycles are cut at the heel strikes it finds)")
    for flag, given in (("--kinematics_out", bool(a.kinematics_out)), ("--kinematics_sigma", a.kinematics_sigma is not None),
                        ("--kinematics_min_stride", a.kinematics_min_stride is not None), ("--kinematics_max_stride", a.kinematics_max_stride is not None),
                        ("--kinematics_on_host", a.kinematics_on_host)):
        if given and not a.gait_kinematics:
            sys.exit(f"batch_generation.py: {flag} belongs to --gait_kinematics, which was not given")
    if a.kinematics_sigma is not None and not (np.isfinite(a.kinematics_sigma) and 0 <= a.kinematics_sigma <= 16):
        sys.exit("batch_generation.py: --kinematics_sigma must be within 0 to 16")
    lo, hi = 8 if a.kinematics_min_stride is None else a.kinematics_min_stride, 60 if a.kinematics_max_stride is None else a.kinematics_max_stride
    if a.gait_kinematics and not 1 <= lo <= hi <= 4096:
        sys.exit("batch_generation.py: --kinematics_min_stride and --kinematics_max_stride must be frames with 1 <= min <= max <= 4096")
    if a.gait_turns and not a.gait:
        sys.exit("batch_generation.py: --gait_turns belongs to --gait, which was not given (it runs on the events and rows of that call)")
    for flag, given in (("--turns_out", bool(a.turns_out)), ("--turns_sigma", a.turns_sigma is not None), ("--turns_edge_rate", a.turns_edge_rate is not None),
                        ("--turns_peak_rate", a.turns_peak_rate is not None), ("--turns_min_angle", a.turns_min_angle is not None),
                        ("--turns_min_duration", a.turns_min_duration is not None), ("--turns_max_duration", a.turns_max_duration is not None),
                        ("--turns_on_host", a.turns_on_host)):
        if given and not a.gait_turns:
            sys.exit(f"batch_generation.py: {flag} belongs to --gait_turns, which was not given")
    if a.turns_sigma is not None and not (np.isfinite(a.turns_sigma) and 0 <= a.turns_sigma <= 16):
        sys.exit("batch_generation.py: --turns_sigma must be within 0 to 16")
    edge, peak = 5.0 if a.turns_edge_rate is None else a.turns_edge_rate, 15.0 if a.turns_peak_rate is None else a.turns_peak_rate
    if a.gait_turns and not (np.isfinite(edge) and np.isfinite(peak) and 0 <= edge <= peak):
        sys.exit("batch_generation.py: --turns_edge_rate and --turns_peak_rate must be degrees a second with 0 <= edge <= peak")
    if a.turns_min_angle is not None and not (np.isfinite(a.turns_min_angle) and a.turns_min_angle >= 0):
        sys.exit("batch_generation.py: --turns_min_angle must be a number of degrees, not negative")
    turn_frames = None
    if a.gait_turns:
        lo, hi = 0.5 if a.turns_min_duration is None else a.turns_min_duration, 10.0 if a.turns_max_duration is None else a.turns_max_duration
        if not (np.isfinite(lo) and np.isfinite(hi) and 0 < lo <= hi):
            sys.exit("batch_generation.py: --turns_min_duration and --turns_max_duration must be seconds with 0 < min <= max")
        fps = 20.0 if a.gait_fps is None else a.gait_fps
        turn_frames = (max(1, int(round(lo * fps))), max(1, int(round(hi * fps))))       # whole frames, the nearest
    if a.gait_contacts and not a.gait:
        sys.exit("batch_generation.py: --gait_contacts belongs to --gait, which was not given (it runs on the events of that call)")
    for flag, given in (("--contacts_out", bool(a.contacts_out)), ("--contacts_sigma", a.contacts_sigma is not None), ("--contacts_fraction", a.contacts_fraction is not None),
                        ("--contacts_speed", a.contacts_speed is not None), ("--contacts_reach", a.contacts_reach is not None),
                        ("--contacts_max_duration", a.contacts_max_duration is not None), ("--contacts_on_host", a.contacts_on_host)):
        if given and not a.gait_contacts:
            sys.exit(f"batch_generation.py: {flag} belongs to --gait_contacts, which was not given")
    if a.contacts_sigma is not None and not (np.isfinite(a.contacts_sigma) and 0 <= a.contacts_sigma <= 16):
        sys.exit("batch_generation.py: --contacts_sigma must be within 0 to 16")
    share, fixed = 0.25 if a.contacts_fraction is None else a.contacts_fraction, 0.0 if a.contacts_speed is None else a.contacts_speed
    if a.gait_contacts and not (np.isfinite(share) and np.isfinite(fixed) and share >= 0 and fixed >= 0 and (share > 0 or fixed > 0)):
        sys.exit("batch_generation.py: --contacts_fraction and --contacts_speed must not be negative, and not both zero")
    if a.contacts_reach is not None and not 0 <= a.contacts_reach <= 8:
        sys.exit("batch_generation.py: --contacts_reach must be within 0 to 8 frames")
    if a.gait_balance and not a.gait:
        sys.exit("batch_generation.py: --gait_balance belongs to --gait, which was not given (it runs on the events of that call)")
    for flag, given in (("--balance_out", bool(a.balance_out)), ("--balance_window", a.balance_window is not None), ("--balance_settle", a.balance_settle is not None),
                        ("--balance_max_step", a.balance_max_step is not None), ("--balance_gravity", a.balance_gravity is not None), ("--balance_on_host", a.balance_on_host)):
        if given and not a.gait_balance:
            sys.exit(f"batch_generation.py: {flag} belongs to --gait_balance, which was not given")
    if a.gait_bootstrap and not a.gait:
        sys.exit("batch_generation.py: --gait_bootstrap belongs to --gait, which was not given (it resamples the steps and strides of that call)")
    for flag, given in (("--bootstrap_out", bool(a.bootstrap_out)), ("--bootstrap_replicates", a.bootstrap_replicates is not None), ("--bootstrap_level", a.bootstrap_level is not None),
                        ("--bootstrap_block", a.bootstrap_block is not None), ("--bootstrap_seed", a.bootstrap_seed is not None), ("--bootstrap_on_host", a.bootstrap_on_host)):
        if given and not a.gait_bootstrap:
            sys.exit(f"batch_generation.py: {flag} belongs to --gait_bootstrap, which was not given")
    if a.bootstrap_replicates is not None and not 1 <= a.bootstrap_replicates <= 4096:
        sys.exit("batch_generation.py: --bootstrap_replicates must be within 1 to 4096")
    if a.bootstrap_level is not None and not (np.isfinite(a.bootstrap_level) and 0 < a.bootstrap_level < 100):
        sys.exit("batch_generation.py: --bootstrap_level must lie between 0 and 100 percent")
    if a.bootstrap_block is not None and not 1 <= a.bootstrap_block <= 1024:
        sys.exit("batch_generation.py: --bootstrap_block must be within 1 to 1024 rows")
    if a.bootstrap_seed is not None and not 0 <= a.bootstrap_seed < 2**64:
        sys.exit("batch_generation.py: --bootstrap_seed must be within 0 to 2^64 - 1")
    if a.balance_window is not None and not 1 <= a.balance_window <= 16:
        sys.exit("batch_generation.py: --balance_window must be within 1 to 16 frames")
    if a.balance_settle is not None and not 0 <= a.balance_settle <= 4:
        sys.exit("batch_generation.py: --balance_settle must be within 0 to 4 frames")
    if a.balance_max_step is not None and not a.balance_max_step >= 1:
        sys.exit("batch_generation.py: --balance_max_step must be at least 1 frame")
    if a.balance_gravity is not None and not (np.isfinite(a.balance_gravity) and a.balance_gravity > 0):
        sys.exit("batch_generation.py: --balance_gravity must be a positive number of metres a second squared")
    contact_frames = None
    if a.gait_contacts:
        longest = 1.0 if a.contacts_max_duration is None else a.contacts_max_duration
        if not (np.isfinite(longest) and longest > 0):
            sys.exit("batch_generation.py: --contacts_max_duration must be a positive number of seconds")
        contact_frames = max(1, int(round(longest * (20.0 if a.gait_fps is None else a.gait_fps))))       # whole frames, the nearest
    for flag, given in (("--regularity_out", bool(a.regularity_out)), ("--regularity_sigma", a.regularity_sigma is not None),
                        ("--regularity_max_lag", a.regularity_max_lag is not None), ("--regularity_min_lag", a.regularity_min_lag is not None),
                        ("--regularity_min_peak", a.regularity_min_peak is not None), ("--regularity_min_pairs", a.regularity_min_pairs is not None),
                        ("--regularity_all_frames", a.regularity_all_frames), ("--regularity_on_host", a.regularity_on_host)):
        if given and not a.gait_regularity:
            sys.exit(f"batch_generation.py: {flag} belongs to --gait_regularity, which was not given")
    if a.gait_regularity and not a.vid_folder:
        sys.exit("batch_generation.py: --gait_regularity needs --vid_folder (the frames whose joints it reads)")
    if a.regularity_sigma is not None and not (np.isfinite(a.regularity_sigma) and 0 <= a.regularity_sigma <= 16):
        sys.exit("batch_generation.py: --regularity_sigma must be within 0 to 16")
    if a.regularity_max_lag is not None and not 8 <= a.regularity_max_lag <= 255:
        sys.exit("batch_generation.py: --regularity_max_lag must be within 8 to 255 frames")
    if a.regularity_min_lag is not None and not 2 <= a.regularity_min_lag <= (60 if a.regularity_max_lag is None else a.regularity_max_lag) - 2:
        sys.exit("batch_generation.py: --regularity_min_lag must be within 2 to --regularity_max_lag - 2 frames")
    if a.regularity_min_peak is not None and not 0 < a.regularity_min_peak <= 1:
        sys.exit("batch_generation.py: --regularity_min_peak must be above 0 and at most 1")
    if a.regularity_min_pairs is not None and not 2 <= a.regularity_min_pairs <= 2 ** 20:
        sys.exit("batch_generation.py: --regularity_min_pairs must be within 2 to 2^20")
    for flag, given in (("--harmonics_out", bool(a.harmonics_out)), ("--harmonics_sigma", a.harmonics_sigma is not None), ("--harmonics_count", a.harmonics_count is not None),
                        ("--harmonics_derivative", a.harmonics_derivative is not None), ("--harmonics_min_stride", a.harmonics_min_stride is not None),
                        ("--harmonics_max_stride", a.harmonics_max_stride is not None), ("--harmonics_all_frames", a.harmonics_all_frames),
                        ("--harmonics_on_host", a.harmonics_on_host)):
        if given and not a.gait_harmonics:
            sys.exit(f"batch_generation.py: {flag} belongs to --gait_harmonics, which was not given")
    if a.gait_harmonics and not a.vid_folder:
        sys.exit("batch_generation.py: --gait_harmonics needs --vid_folder (the frames whose joints it reads)")
    if a.gait_harmonics and not a.gait:
        sys.exit("batch_generation.py: --gait_harmonics needs --gait (the heel strikes its strides are cut at)")
    if a.harmonics_sigma is not None and not (np.isfinite(a.harmonics_sigma) and 0 <= a.harmonics_sigma <= 16):
        sys.exit("batch_generation.py: --harmonics_sigma must be within 0 to 16")
    if a.harmonics_count is not None and not (2 <= a.harmonics_count <= 32 and a.harmonics_count % 2 == 0):
        sys.exit("batch_generation.py: --harmonics_count must be even and within 2 to 32")
    if a.harmonics_derivative is not None and not 0 <= a.harmonics_derivative <= 2:
        sys.exit("batch_generation.py: --harmonics_derivative must be 0, 1 or 2")
    if a.harmonics_max_stride is not None and not 6 <= a.harmonics_max_stride <= 255:
        sys.exit("batch_generation.py: --harmonics_max_stride must be within 6 to 255 frames")
    if not 6 <= (8 if a.harmonics_min_stride is None else a.harmonics_min_stride) <= (60 if a.harmonics_max_stride is None else a.harmonics_max_stride):
        sys.exit("batch_generation.py: --harmonics_min_stride must be within 6 to --harmonics_max_stride frames")
    for flag, given in (("--entropy_out", bool(a.entropy_out)), ("--entropy_sigma", a.entropy_sigma is not None), ("--entropy_m", a.entropy_m is not None),
                        ("--entropy_r", a.entropy_r is not None), ("--entropy_derivative", a.entropy_derivative is not None), ("--entropy_scales", a.entropy_scales is not None),
                        ("--entropy_min_templates", a.entropy_min_templates is not None), ("--entropy_all_frames", a.entropy_all_frames),
                        ("--entropy_on_host", a.entropy_on_host)):
        if given and not a.gait_entropy:
            sys.exit(f"batch_generation.py: {flag} belongs to --gait_entropy, which was not given")
    if a.gait_entropy and not a.vid_folder:
        sys.exit("batch_generation.py: --gait_entropy needs --vid_folder (the frames whose joints it reads)")
    if a.entropy_sigma is not None and not (np.isfinite(a.entropy_sigma) and 0 <= a.entropy_sigma <= 16):
        sys.exit("batch_generation.py: --entropy_sigma must be within 0 to 16")
    if a.entropy_m is not None and not 1 <= a.entropy_m <= 4:
        sys.exit("batch_generation.py: --entropy_m must be within 1 to 4")
    if a.entropy_r is not None and not (np.isfinite(a.entropy_r) and 0 < a.entropy_r <= 10):
        sys.exit("batch_generation.py: --entropy_r must be above 0 and at most 10")
    if a.entropy_derivative is not None and not 0 <= a.entropy_derivative <= 2:
        sys.exit("batch_generation.py: --entropy_derivative must be 0, 1 or 2")
    if a.entropy_scales is not None and not 1 <= a.entropy_scales <= 8:
        sys.exit("batch_generation.py: --entropy_scales must be within 1 to 8")
    if a.entropy_min_templates is not None and a.entropy_min_templates < 1:
        sys.exit("batch_generation.py: --entropy_min_templates must be at least 1")
    for flag, given in (("--stability_out", bool(a.stability_out)), ("--stability_sigma", a.stability_sigma is not None), ("--stability_derivative", a.stability_derivative is not None),
                        ("--stability_dim", a.stability_dim is not None), ("--stability_lag", a.stability_lag is not None), ("--stability_theiler", a.stability_theiler is not None),
                        ("--stability_horizon", a.stability_horizon is not None), ("--stability_fit_lo", a.stability_fit_lo is not None),
                        ("--stability_fit_hi", a.stability_fit_hi is not None), ("--stability_min_pairs", a.stability_min_pairs is not None),
                        ("--stability_all_frames", a.stability_all_frames), ("--stability_on_host", a.stability_on_host)):
        if given and not a.gait_stability:
            sys.exit(f"batch_generation.py: {flag} belongs to --gait_stability, which was not given")
    if a.gait_stability and not a.vid_folder:
        sys.exit("batch_generation.py: --gait_stability needs --vid_folder (the frames whose joints it reads)")
    if a.stability_sigma is not None and not (np.isfinite(a.stability_sigma) and 0 <= a.stability_sigma <= 16):
        sys.exit("batch_generation.py: --stability_sigma must be within 0 to 16")
    if a.stability_derivative is not None and not 0 <= a.stability_derivative <= 2:
        sys.exit("batch_generation.py: --stability_derivative must be 0, 1 or 2")
    if a.stability_dim is not None and not 2 <= a.stability_dim <= 8:
        sys.exit("batch_generation.py: --stability_dim must be within 2 to 8")
    if a.stability_lag is not None and not 1 <= a.stability_lag <= 16:
        sys.exit("batch_generation.py: --stability_lag must be within 1 to 16")
    if a.stability_theiler is not None and not 0 <= a.stability_theiler <= 4096:
        sys.exit("batch_generation.py: --stability_theiler must be within 0 to 4096")
    if a.stability_horizon is not None and not 1 <= a.stability_horizon <= 63:
        sys.exit("batch_generation.py: --stability_horizon must be within 1 to 63")
    if a.stability_fit_lo is not None and a.stability_fit_lo < 0:
        sys.exit("batch_generation.py: --stability_fit_lo must be at least 0")
    if a.gait_stability and not (0 if a.stability_fit_lo is None else a.stability_fit_lo) < (min(10, 20 if a.stability_horizon is None else a.stability_horizon) if a.stability_fit_hi is None else a.stability_fit_hi) <= \
            (20 if a.stability_horizon is None else a.stability_horizon):
        sys.exit("batch_generation.py: --stability_fit_hi must be above --stability_fit_lo and at most --stability_horizon")
    if a.stability_min_pairs is not None and a.stability_min_pairs < 1:
        sys.exit("batch_generation.py: --stability_min_pairs must be at least 1")
    for flag, given in (("--spectrum_out", bool(a.spectrum_out)), ("--spectrum_sigma", a.spectrum_sigma is not None), ("--spectrum_derivative", a.spectrum_derivative is not None),
                        ("--spectrum_segment", a.spectrum_segment is not None), ("--spectrum_hop", a.spectrum_hop is not None), ("--spectrum_nfft", a.spectrum_nfft is not None),
                        ("--spectrum_f_lo", a.spectrum_f_lo is not None), ("--spectrum_f_hi", a.spectrum_f_hi is not None),
                        ("--spectrum_min_segments", a.spectrum_min_segments is not None), ("--spectrum_all_frames", a.spectrum_all_frames),
                        ("--spectrum_on_host", a.spectrum_on_host)):
        if given and not a.gait_spectrum:
            sys.exit(f"batch_generation.py: {flag} belongs to --gait_spectrum, which was not given")
    if a.gait_spectrum and not a.vid_folder:
        sys.exit("batch_generation.py: --gait_spectrum needs --vid_folder (the frames whose joints it reads)")
    if a.spectrum_sigma is not None and not (np.isfinite(a.spectrum_sigma) and 0 <= a.spectrum_sigma <= 16):
        sys.exit("batch_generation.py: --spectrum_sigma must be within 0 to 16")
    if a.spectrum_derivative is not None and not 0 <= a.spectrum_derivative <= 2:
        sys.exit("batch_generation.py: --spectrum_derivative must be 0, 1 or 2")
    if a.gait_spectrum:
        seg = 64 if a.spectrum_segment is None else a.spectrum_segment
        if not 8 <= seg <= 256 or seg % 2:
            sys.exit("batch_generation.py: --spectrum_segment must be even and within 8 to 256")
        if a.spectrum_hop is not None and not seg // 8 <= a.spectrum_hop <= seg:
            sys.exit("batch_generation.py: --spectrum_hop must be within an eighth of --spectrum_segment to the whole of it")
        nfft = 256 if a.spectrum_nfft is None else a.spectrum_nfft
        if not seg <= nfft <= 1024 or nfft % 2:
            sys.exit("batch_generation.py: --spectrum_nfft must be even and within --spectrum_segment to 1024")
        f_lo, f_hi = 0.5 if a.spectrum_f_lo is None else a.spectrum_f_lo, 3.0 if a.spectrum_f_hi is None else a.spectrum_f_hi
        if not (np.isfinite(f_lo) and np.isfinite(f_hi) and 0 < f_lo < f_hi <= (20.0 if a.gait_fps is None else a.gait_fps) / 2):
            sys.exit("batch_generation.py: --spectrum_f_lo and --spectrum_f_hi must obey 0 < f_lo < f_hi <= half the frames a second")
        if a.spectrum_min_segments is not None and a.spectrum_min_segments < 1:
            sys.exit("batch_generation.py: --spectrum_min_segments must be at least 1")
    for flag, given in (("--smoothness_out", bool(a.smoothness_out)), ("--smoothness_sigma", a.smoothness_sigma is not None),
                        ("--smoothness_derivative", a.smoothness_derivative is not None), ("--smoothness_segment", a.smoothness_segment is not None),
                        ("--smoothness_hop", a.smoothness_hop is not None), ("--smoothness_nfft", a.smoothness_nfft is not None),
                        ("--smoothness_cutoff", a.smoothness_cutoff is not None), ("--smoothness_amplitude", a.smoothness_amplitude is not None),
                        ("--smoothness_min_segments", a.smoothness_min_segments is not None), ("--smoothness_all_frames", a.smoothness_all_frames),
                        ("--smoothness_on_host", a.smoothness_on_host)):
        if given and not a.gait_smoothness:
            sys.exit(f"batch_generation.py: {flag} belongs to --gait_smoothness, which was not given")
    if a.gait_smoothness and not a.vid_folder:
        sys.exit("batch_generation.py: --gait_smoothness needs --vid_folder (the frames whose joints it reads)")
    if a.smoothness_sigma is not None and not (np.isfinite(a.smoothness_sigma) and 0 <= a.smoothness_sigma <= 16):
        sys.exit("batch_generation.py: --smoothness_sigma must be within 0 to 16")
    if a.smoothness_derivative is not None and not 0 <= a.smoothness_derivative <= 2:
        sys.exit("batch_generation.py: --smoothness_derivative must be 0, 1 or 2")
    if a.gait_smoothness:
        seg = 64 if a.smoothness_segment is None else a.smoothness_segment
        if not 8 <= seg <= 256 or seg % 2:
            sys.exit("batch_generation.py: --smoothness_segment must be even and within 8 to 256")
        if a.smoothness_hop is not None and not seg // 8 <= a.smoothness_hop <= seg:
            sys.exit("batch_generation.py: --smoothness_hop must be within an eighth of --smoothness_segment to the whole of it")
        nfft = 1024 if a.smoothness_nfft is None else a.smoothness_nfft
        if not seg <= nfft <= 4096 or nfft % 2:
            sys.exit("batch_generation.py: --smoothness_nfft must be even and within --smoothness_segment to 4096")
        if a.smoothness_cutoff is not None and not (np.isfinite(a.smoothness_cutoff) and 0 < a.smoothness_cutoff <= (20.0 if a.gait_fps is None else a.gait_fps) / 2):
            sys.exit("batch_generation.py: --smoothness_cutoff must obey 0 < cutoff <= half the frames a second")
        if a.smoothness_amplitude is not None and not 0 < a.smoothness_amplitude <= 1:
            sys.exit("batch_generation.py: --smoothness_amplitude must be above 0 and at most 1")
        if a.smoothness_min_segments is not None and a.smoothness_min_segments < 1:
            sys.exit("batch_generation.py: --smoothness_min_segments must be at least 1")
    for flag, given in (("--body_out", bool(a.body_out)), ("--body_density", a.body_density is not None), ("--body_on_host", a.body_on_host)):
        if given and not a.gait_body:
            sys.exit(f"batch_generation.py: {flag} belongs to --gait_body, which was not given")
    if a.gait_body and not a.vid_folder:
        sys.exit("batch_generation.py: --gait_body needs --vid_folder (the frames whose meshes it reads)")
    if a.body_density is not None and not (np.isfinite(a.body_density) and a.body_density > 0):
        sys.exit("batch_generation.py: --body_density must be a positive number of kilograms a cubic metre")
    if a.balance_com is not None and not a.gait_balance:
        sys.exit("batch_generation.py: --balance_com belongs to --gait_balance, which was not given")
    if a.balance_com == "mesh" and not a.gait_body:
        sys.exit("batch_generation.py: --balance_com mesh needs --gait_body, which was not given (the mesh's centre of mass is made there)")
    for flag, given in (("--coordination_out", bool(a.coordination_out)), ("--coordination_sigma", a.coordination_sigma is not None),
                        ("--coordination_derivative", a.coordination_derivative is not None), ("--coordination_segment", a.coordination_segment is not None),
                        ("--coordination_hop", a.coordination_hop is not None), ("--coordination_nfft", a.coordination_nfft is not None),
                        ("--coordination_f_lo", a.coordination_f_lo is not None), ("--coordination_f_hi", a.coordination_f_hi is not None),
                        ("--coordination_min_segments", a.coordination_min_segments is not None), ("--coordination_all_frames", a.coordination_all_frames),
                        ("--coordination_on_host", a.coordination_on_host)):
        if given and not a.gait_coordination:
            sys.exit(f"batch_generation.py: {flag} belongs to --gait_coordination, which was not given")
    if a.gait_coordination and not a.vid_folder:
        sys.exit("batch_generation.py: --gait_coordination needs --vid_folder (the frames whose joints it reads)")
    if a.coordination_sigma is not None and not (np.isfinite(a.coordination_sigma) and 0 <= a.coordination_sigma <= 16):
        sys.exit("batch_generation.py: --coordination_sigma must be within 0 to 16")
    if a.coordination_derivative is not None and not 0 <= a.coordination_derivative <= 2:
        sys.exit("batch_generation.py: --coordination_derivative must be 0, 1 or 2")
    if a.gait_coordination:
        seg = 64 if a.coordination_segment is None else a.coordination_segment
        if not 8 <= seg <= 256 or seg % 2:
            sys.exit("batch_generation.py: --coordination_segment must be even and within 8 to 256")
        if a.coordination_hop is not None and not seg // 8 <= a.coordination_hop <= seg:
            sys.exit("batch_generation.py: --coordination_hop must be within an eighth of --coordination_segment to the whole of it")
        nfft = 256 if a.coordination_nfft is None else a.coordination_nfft
        if not seg <= nfft <= 1024 or nfft % 2:
            sys.exit("batch_generation.py: --coordination_nfft must be even and within --coordination_segment to 1024")
        f_lo, f_hi = 0.5 if a.coordination_f_lo is None else a.coordination_f_lo, 3.0 if a.coordination_f_hi is None else a.coordination_f_hi
        if not (np.isfinite(f_lo) and np.isfinite(f_hi) and 0 < f_lo < f_hi <= (20.0 if a.gait_fps is None else a.gait_fps) / 2):
            sys.exit("batch_generation.py: --coordination_f_lo and --coordination_f_hi must obey 0 < f_lo < f_hi <= half the frames a second")
        if a.coordination_min_segments is not None and not 2 <= a.coordination_min_segments <= 2 ** 20:
            sys.exit("batch_generation.py: --coordination_min_segments must be at least 2 (the coherence of one segment is 1 whatever the signals are)")
    for flag, given in (("--recurrence_out", bool(a.recurrence_out)), ("--recurrence_sigma", a.recurrence_sigma is not None), ("--recurrence_derivative", a.recurrence_derivative is not None),
                        ("--recurrence_dim", a.recurrence_dim is not None), ("--recurrence_lag", a.recurrence_lag is not None), ("--recurrence_radius", a.recurrence_radius is not None),
                        ("--recurrence_theiler", a.recurrence_theiler is not None), ("--recurrence_min_line", a.recurrence_min_line is not None),
                        ("--recurrence_min_points", a.recurrence_min_points is not None), ("--recurrence_all_frames", a.recurrence_all_frames),
                        ("--recurrence_on_host", a.recurrence_on_host)):
        if given and not a.gait_recurrence:
            sys.exit(f"batch_generation.py: {flag} belongs to --gait_recurrence, which was not given")
    if a.gait_recurrence and not a.vid_folder:
        sys.exit("batch_generation.py: --gait_recurrence needs --vid_folder (the frames whose joints it reads)")
    if a.recurrence_sigma is not None and not (np.isfinite(a.recurrence_sigma) and 0 <= a.recurrence_sigma <= 16):
        sys.exit("batch_generation.py: --recurrence_sigma must be within 0 to 16")
    if a.recurrence_derivative is not None and not 0 <= a.recurrence_derivative <= 2:
        sys.exit("batch_generation.py: --recurrence_derivative must be 0, 1 or 2")
    if a.recurrence_dim is not None and not 2 <= a.recurrence_dim <= 8:
        sys.exit("batch_generation.py: --recurrence_dim must be within 2 to 8")
    if a.recurrence_lag is not None and not 1 <= a.recurrence_lag <= 16:
        sys.exit("batch_generation.py: --recurrence_lag must be within 1 to 16")
    if a.recurrence_radius is not None and not (np.isfinite(a.recurrence_radius) and 0 < a.recurrence_radius <= 10):
        sys.exit("batch_generation.py: --recurrence_radius must be above 0 and at most 10")
    if a.recurrence_theiler is not None and not 0 <= a.recurrence_theiler <= 4096:
        sys.exit("batch_generation.py: --recurrence_theiler must be within 0 to 4096")
    if a.recurrence_min_line is not None and not 1 <= a.recurrence_min_line <= 255:
        sys.exit("batch_generation.py: --recurrence_min_line must be within 1 to 255")
    if a.recurrence_min_points is not None and a.recurrence_min_points < 1:
        sys.exit("batch_generation.py: --recurrence_min_points must be at least 1")
    if a.openpose_folder and not a.vid_folder and not a.bbox_out:
        sys.exit("batch_generation.py: --openpose_folder without --vid_folder only writes the boxes: name the file with --bbox_out")
    annos = trajectory = tracks = None
    track = None
    if a.bbox_track:
        track = {"kernel_size": 11 if a.bbox_kernel is None else a.bbox_kernel, "sigma": 3.0 if a.bbox_sigma is None else a.bbox_sigma,
                 "pad": a.bbox_pad or "zero"} if a.bbox_smooth else {}
    if a.openpose_folder:
        found = boxes_from_openpose(a.openpose_folder, a.bbox_out, on_host=a.bbox_on_host, return_joints=True, track=track)
        annos, joints2d = found[:2]
        tracks = found[2] if track is not None else None
    if a.trajectory:
        trajectory = {"joints2d": joints2d, "focal_length": a.focal_length or None, "on_host": a.trajectory_on_host}
    if a.openpose_folder and not a.vid_folder:
        return
    gait = {"fps": a.gait_fps, "sigma": a.gait_sigma, "window": a.gait_window, "min_excursion": a.gait_min_excursion, "on_host": a.gait_on_host,
            "out": a.gait_out or None} if a.gait else None
    kinematics = {"sigma": a.kinematics_sigma, "min_stride": a.kinematics_min_stride, "max_stride": a.kinematics_max_stride, "on_host": a.kinematics_on_host,
                  "out": a.kinematics_out or None} if a.gait_kinematics else None
    turns = {"sigma": a.turns_sigma, "edge_rate": a.turns_edge_rate, "peak_rate": a.turns_peak_rate, "min_angle": a.turns_min_angle, "min_frames": turn_frames[0],
             "max_frames": turn_frames[1], "on_host": a.turns_on_host, "out": a.turns_out or None} if a.gait_turns else None
    contacts = {"sigma": a.contacts_sigma, "fraction": a.contacts_fraction, "speed": a.contacts_speed, "reach": a.contacts_reach, "max_frames": contact_frames,
                "on_host": a.contacts_on_host, "out": a.contacts_out or None} if a.gait_contacts else None
    regularity = {"fps": a.gait_fps, "sigma": a.regularity_sigma, "max_lag": a.regularity_max_lag, "min_lag": a.regularity_min_lag, "min_peak": a.regularity_min_peak,
                  "min_pairs": a.regularity_min_pairs, "all_frames": a.regularity_all_frames, "on_host": a.regularity_on_host,
                  "out": a.regularity_out or None} if a.gait_regularity else None
    harmonics = {"sigma": a.harmonics_sigma, "n_harmonics": a.harmonics_count, "derivative": a.harmonics_derivative, "min_stride": a.harmonics_min_stride,
                 "max_stride": a.harmonics_max_stride, "all_frames": a.harmonics_all_frames, "on_host": a.harmonics_on_host,
                 "out": a.harmonics_out or None} if a.gait_harmonics else None
    entropy = {"sigma": a.entropy_sigma, "m": a.entropy_m, "fraction": a.entropy_r, "derivative": a.entropy_derivative, "scales": a.entropy_scales,
               "min_templates": a.entropy_min_templates, "all_frames": a.entropy_all_frames, "on_host": a.entropy_on_host,
               "out": a.entropy_out or None} if a.gait_entropy else None
    stability = {"sigma": a.stability_sigma, "derivative": a.stability_derivative, "dim": a.stability_dim, "lag": a.stability_lag, "theiler": a.stability_theiler,
                 "horizon": a.stability_horizon, "fit_lo": a.stability_fit_lo, "fit_hi": a.stability_fit_hi, "min_pairs": a.stability_min_pairs,
                 "all_frames": a.stability_all_frames, "on_host": a.stability_on_host, "out": a.stability_out or None} if a.gait_stability else None
    spectrum = {"fps": a.gait_fps, "sigma": a.spectrum_sigma, "derivative": a.spectrum_derivative, "segment": a.spectrum_segment, "hop": a.spectrum_hop, "nfft": a.spectrum_nfft,
                "f_lo": a.spectrum_f_lo, "f_hi": a.spectrum_f_hi, "min_segments": a.spectrum_min_segments, "all_frames": a.spectrum_all_frames,
                "on_host": a.spectrum_on_host, "out": a.spectrum_out or None} if a.gait_spectrum else None
    smoothness = {"fps": a.gait_fps, "sigma": a.smoothness_sigma, "derivative": a.smoothness_derivative, "segment": a.smoothness_segment, "hop": a.smoothness_hop,
                  "nfft": a.smoothness_nfft, "f_cut": a.smoothness_cutoff, "amplitude": a.smoothness_amplitude, "min_segments": a.smoothness_min_segments,
                  "all_frames": a.smoothness_all_frames, "on_host": a.smoothness_on_host, "out": a.smoothness_out or None} if a.gait_smoothness else None
    recurrence = {"sigma": a.recurrence_sigma, "derivative": a.recurrence_derivative, "dim": a.recurrence_dim, "lag": a.recurrence_lag, "theiler": a.recurrence_theiler,
                  "radius": a.recurrence_radius, "min_line": a.recurrence_min_line, "min_points": a.recurrence_min_points, "all_frames": a.recurrence_all_frames,
                  "on_host": a.recurrence_on_host, "out": a.recurrence_out or None} if a.gait_recurrence else None
    coordination = {"fps": a.gait_fps, "sigma": a.coordination_sigma, "derivative": a.coordination_derivative, "segment": a.coordination_segment, "hop": a.coordination_hop,
                    "nfft": a.coordination_nfft, "f_lo": a.coordination_f_lo, "f_hi": a.coordination_f_hi, "min_segments": a.coordination_min_segments,
                    "all_frames": a.coordination_all_frames, "on_host": a.coordination_on_host, "out": a.coordination_out or None} if a.gait_coordination else None
    balance = {"gravity": a.balance_gravity, "window": a.balance_window, "settle": a.balance_settle, "max_step": a.balance_max_step, "on_host": a.balance_on_host,
               "out": a.balance_out or None, **({"com": a.balance_com} if a.balance_com is not None else {})} if a.gait_balance else None
    body = {"density": a.body_density, "on_host": a.body_on_host, "out": a.body_out or None} if a.gait_body else None
    bootstrap = {"replicates": a.bootstrap_replicates, "level": a.bootstrap_level, "block": a.bootstrap_block, "seed": a.bootstrap_seed, "on_host": a.bootstrap_on_host,
                 "out": a.bootstrap_out or None} if a.gait_bootstrap else None
    prepare_data(fv=a.bbox_path, vid_folder=a.vid_folder, outpath=a.outpath, pretrained_file=a.pretrained_file,
                 synthetic_weights=a.synthetic_weights, max_frames=a.max_frames, dtype=a.dtype, chunk=a.chunk, exchange=a.exchange, full_arena=a.full_arena, annos=annos,
                 gt_path=a.gt_path or None, metrics_out=a.metrics_out or None, metrics_on_host=a.metrics_on_host, trajectory=trajectory, tracks=tracks, gait=gait,
                 **({"kinematics": kinematics} if kinematics is not None else {}), **({"turns": turns} if turns is not None else {}),
                 **({"contacts": contacts} if contacts is not None else {}), **({"regularity": regularity} if regularity is not None else {}),
                 **({"harmonics": harmonics} if harmonics is not None else {}), **({"entropy": entropy} if entropy is not None else {}),
                 **({"stability": stability} if stability is not None else {}),
                 **({"spectrum": spectrum} if spectrum is not None else {}), **({"recurrence": recurrence} if recurrence is not None else {}),
                 **({"coordination": coordination} if coordination is not None else {}), **({"balance": balance} if balance is not None else {}),
                 **({"bootstrap": bootstrap} if bootstrap is not None else {}), **({"smoothness": smoothness} if smoothness is not None else {}),
                 **({"body": body} if body is not None else {}))


if __name__ == "__main__":
    main()
