#!/usr/bin/env python3
"""demo.py of the MI355X-native path: same flags, model loop and .pkl schema as the reference's
demo.py (argparse :391-456, loop :126-231, pickle :254-267), with the model running in libgrnet_hip.so.

Out of scope here (rows 12, 17, 19): ffmpeg video decoding, the YOLOv3+SORT tracker and the
matplotlib / pyrender output video.  So this entry point takes what the reference takes once those
steps are done: --img_folder (extracted frames) and --tracking_path (joblib {id: {'bbox','frames'}}).
The reference's --cpu_only (demo.py:46-49,403) is accepted and refused with one line: there is deliberately no CPU fallback.
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
MIN_NUM_FRAMES = 25          # demo.py:41
CPU_ONLY_MESSAGE = ("--cpu_only: this build has no CPU path (a CPU fallback would have to run the test oracle as the product); "
                    "BASELINE configs[0] is covered by tests/test_gpu_harness.py::test_demo_entry_point on the GPU")


def load_cfg(path):
    """The two values the reference consumes from the yaml (demo.py:109-110): DATASET.SEQLEN, MODEL.FEAT_CORR."""
    import yaml
    cfg = {"DATASET": {"SEQLEN": 100}, "MODEL": {"FEAT_CORR": None}}
    if path and osp.isfile(path):
        with open(path) as f:
            y = yaml.safe_load(f) or {}
        cfg["DATASET"].update(y.get("DATASET", {}))
        cfg["MODEL"].update(y.get("MODEL", {}))
    return cfg


def build_model(pkg, args, seqlen):
    import torch
    if args.synthetic_weights:
        return pkg.build_synthetic_model(max_frames=args.max_frames, with_gru=False, dtype=args.dtype, compact_arena=not args.full_arena)
    if not args.ckpt:
        sys.exit("!!! Please provide a pretrained checkpoint (--ckpt) or --synthetic_weights !!!")
    model = pkg.GRNet(writer=None, seqlen=seqlen, featcorr=None, max_frames=args.max_frames, dtype=args.dtype, compact_arena=not args.full_arena)
    ckpt = torch.load(args.ckpt, map_location="cpu")["gen_state_dict"]
    print(f"Load pretrained weights from '{args.ckpt}'")
    res = model.load_state_dict(ckpt, strict=False)
    if not model._smpl_loaded:
        smpl = osp.join(args.smpl_dir, "SMPL_NEUTRAL.npz")
        if not osp.isfile(smpl):
            sys.exit(f"the checkpoint holds no SMPL tables and {smpl} is missing")
        d = dict(np.load(smpl))
        d["J_regressor_extra"] = np.load(osp.join(args.smpl_dir, "J_regressor_extra.npy"))
        model.load_smpl(d)
    if res.missing_keys:
        print(f"warning: {len(res.missing_keys)} tensors missing from the checkpoint, e.g. {res.missing_keys[:3]}")
    return model.finalize()


def main(args):
    import joblib
    pkg = importlib.import_module(PKG)
    pipe = importlib.import_module(PKG + ".pipeline")
    cfg = load_cfg(args.cfg)
    if not args.img_folder or not osp.isdir(args.img_folder):
        sys.exit(f'Input image folder "{args.img_folder}" does not exist! (video decoding is out of scope: extract frames first)')
    if not args.tracking_path:
        sys.exit("--tracking_path is required (the YOLOv3+SORT tracker is a separate third-party model)")
    video_name = osp.basename(osp.normpath(args.vid_file)).split(".")[0] if args.vid_file else osp.basename(osp.normpath(args.img_folder))
    output_path = osp.join(args.output_folder, video_name, "normal" + time.strftime("-%m%d"))
    os.makedirs(output_path, exist_ok=True)

    tracking = joblib.load(args.tracking_path)
    for pid in list(tracking.keys()):                         # demo.py:101-103
        if tracking[pid]["frames"].shape[0] < MIN_NUM_FRAMES:
            del tracking[pid]
    model = build_model(pkg, args, cfg["DATASET"]["SEQLEN"])
    ai = model.arena_info()
    print(f"Activation arena: {ai['bytes'] / 2**20:.0f} MiB for calls of up to {args.max_frames} frames "
          f"({'one buffer per tensor' if args.full_arena else 'buffers shared by liveness'}; the full layout takes {ai['full_bytes'] / 2**20:.0f} MiB)")
    smpl_tables = None
    if args.smooth and args.smooth_on_host:                    # the host statement forms the 49 joints with J_regressor_extra on the CPU
        if args.synthetic_weights:
            smpl_tables = pkg.synth.make_smpl_tables()
        else:
            smpl_tables = {"J_regressor_extra": np.load(osp.join(args.smpl_dir, "J_regressor_extra.npy"))}
    t0 = time.time()
    results, n_frames = {}, 0
    for pid, tr in tracking.items():
        bboxes, frames = np.asarray(tr["bbox"], np.float32).copy(), np.asarray(tr["frames"])
        ds = pipe.InferenceFrames(args.img_folder, frames, bboxes, scale=1.0)
        on_device = args.smooth and not args.smooth_on_host
        pred = pipe.run_tracklet(model, ds.batches(args.grnet_batch_size, model=model), on_device=on_device)
        w, h = ds.image_size()
        if args.smooth:                                        # demo.py:191-196
            print(f"Running smoothing on person {pid}, min_cutoff: {args.smooth_min_cutoff}, beta: {args.smooth_beta}")
            if on_device:
                # filter, Rodrigues, SMPL and the 49 joints on the GPU, reading theta in place; only what the pickle holds is downloaded
                # (the first pass's verts and joints3d are dropped on the device)
                theta = pred.pop("theta")
                pred["verts"], pred["pose"], pred["joints3d"] = model.smooth_pose(
                    theta, theta[:, 75:], min_cutoff=args.smooth_min_cutoff, beta=args.smooth_beta, joints="spin49")
                pred = {k: v.cpu().numpy() for k, v in pred.items()}
            else:
                pred["verts"], pred["pose"], pred["joints3d"] = pipe.smooth_pose(
                    model, pred["pose"], pred["betas"], min_cutoff=args.smooth_min_cutoff, beta=args.smooth_beta,
                    smpl_tables=smpl_tables)
        results[pid] = pipe.make_demo_result(pred, ds.bboxes, ds.frames, w, h)
        if args.joint_type != "spin":                          # demo.py:224-229
            # the reference converts with src='spin' (49 joints); without --smooth the path emits the 29 'spin2' joints, on which
            # the reference's call raises IndexError -- here the source skeleton is the one the arrays really are
            src = "spin" if results[pid]["joints3d"].shape[1] == 49 else "spin2"
            try:
                results[pid]["joints3d"] = pipe.convert_kps(results[pid]["joints3d"], src, args.joint_type)
                j2 = results[pid]["joints2d"]
                j2 = np.concatenate([j2, np.zeros_like(j2[..., :1])], -1)      # convert_kps writes 3 columns; the third stays 0
                results[pid]["joints2d"] = pipe.convert_kps(j2, "spin2", args.joint_type)[..., :2]
            except NameError:
                print(f"Unknown skeleton type: {args.joint_type}.")
        n_frames += len(ds)
    dt = time.time() - t0
    print(f"GRNet FPS: {n_frames / max(dt, 1e-9):.2f}")
    stem = osp.basename(args.ckpt).split(".")[0] if args.ckpt else "synthetic"
    out = osp.join(output_path, stem + ".pkl")
    idx = 0
    while osp.isfile(out):                                     # demo.py:258-266: never overwrite
        idx += 1
        out = osp.join(output_path, f"{stem}{idx}.pkl")
    joblib.dump(results, out)
    print(f'Saving output results to "{out}".')
    return out


def parser():
    p = argparse.ArgumentParser()
    p.add_argument("--vid_file", type=str, default="", help="input video path (used for the output folder name only)")
    p.add_argument("--cfg", type=str, default="configs/config_grnet.yaml")
    p.add_argument("--ckpt", type=str, default="", help="path to the pretrained checkpoint.")
    p.add_argument("--output_folder", type=str, default="output/")
    p.add_argument("--detector", type=str, default="yolo", choices=["yolo"])
    p.add_argument("--yolo_img_size", type=int, default=416)
    p.add_argument("--tracker_batch_size", type=int, default=12)
    p.add_argument("--grnet_batch_size", type=int, default=450)
    p.add_argument("--display", action="store_true")
    p.add_argument("--mesh_render", action="store_true")
    p.add_argument("--wireframe", action="store_true")
    p.add_argument("--sideview", action="store_true")
    p.add_argument("--save_obj", action="store_true")
    p.add_argument("--smooth", action="store_true")
    p.add_argument("--smooth_min_cutoff", type=float, default=0.004)
    p.add_argument("--smooth_beta", type=float, default=0.7)
    p.add_argument("--smooth_on_host", action="store_true", help="--smooth with the filter, Rodrigues and the 49-joint regression on the CPU "
                   "(pipeline.smooth_pose, the host statement the device path is tested against); default: all of it on the GPU")
    p.add_argument("--tracking_path", type=str, default=None)
    p.add_argument("--img_folder", type=str, default=None)
    p.add_argument("--joint_type", type=str, default="spin")
    p.add_argument("--save_vid", action="store_false")
    p.add_argument("--cpu_only", action="store_true", help="the reference's CPU switch (demo.py:403): parsed, and refused -- this build has no CPU path")
    # additions of this implementation
    p.add_argument("--synthetic_weights", action="store_true", help="seed-defined weights (no checkpoint exists offline)")
    p.add_argument("--smpl_dir", type=str, default="data/smpl_data")
    p.add_argument("--dtype", choices=("f32", "bf16"), default="f32", help="f32: the reference's precision; bf16: bf16 storage, fp32 accumulation")
    p.add_argument("--max_frames", type=int, default=64, help="frames per grnet_forward call (activation buffers are sized for it)")
    p.add_argument("--full_arena", action="store_true", help="one buffer per intermediate tensor (the library's default layout, 7.5x the memory in f32); "
                   "this script never reads intermediates, so it shares buffers by liveness -- same launches, bit-identical outputs")
    return p


if __name__ == "__main__":
    a = parser().parse_args()
    if a.cpu_only:
        sys.exit(CPU_ONLY_MESSAGE)
    for flag in ("mesh_render", "display", "save_obj"):
        if getattr(a, flag):
            sys.exit(f"--{flag} belongs to steps outside the per-frame path (SURVEY 8f) and is not implemented")
    d = parser().parse_args([])
    for flag in ("detector", "yolo_img_size", "tracker_batch_size", "wireframe", "sideview", "save_vid"):
        if getattr(a, flag) != getattr(d, flag):
            print(f"warning: --{flag} configures a step outside the per-frame path (tracker / renderer, SURVEY 8f) and has no effect here")
    main(a)
