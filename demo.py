#!/usr/bin/env python3
"""demo.py of the MI355X-native path: same flags, model loop and .pkl schema as the reference's
demo.py (argparse :391-456, loop :126-231, pickle :254-267), with the model running in libgrnet_hip.so.

Out of scope here (rows 12, 17): ffmpeg video decoding and the YOLOv3+SORT tracker.  So this entry point takes what the
reference takes once those steps are done: --img_folder (extracted frames) and --tracking_path (joblib {id: {'bbox','frames'}}).
--mesh_render draws the overlay frames (demo.py:269-385) with the library's own rasteriser: OpenGL's geometry rules, a stated Lambert
shading that is NOT pyrender's; with --wireframe the overlay is the meshes' edges as 1-pixel lines (GL's polygon mode GL_LINE,
by the library's own line rule).  --skeleton_view writes the reference's OTHER output (demo.py:288-290, 303-361 without --mesh_render): the input
frame on the left and the 3D skeleton of every tracked person on the right, from matplotlib's viewpoint for the reference's settings, drawn on
the GPU by the library's own wide-line rule (no pane fills, no tick labels or titles, no caps, no anti-aliasing, the panel as large
as the input frame) -- NOT by matplotlib.  --display and --wireframe without --mesh_render stay refused.
The reference's --cpu_only (demo.py:46-49,403) is accepted and refused with one line: there is deliberately no CPU fallback.
"""
import argparse
import colorsys
import importlib
import os
import os.path as osp
import shutil
import subprocess
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


RENDER_CHUNK = 16            # frames uploaded, drawn and downloaded together
SKELETON_JOINT_TYPES = ("spin", "kinectv2")      # pipeline.skeleton_bones


def refusal(a):
    """One line for a flag this build parses and refuses, None otherwise."""
    if a.cpu_only:
        return CPU_ONLY_MESSAGE
    if a.wireframe and not a.mesh_render:
        return "--wireframe draws the lines of the --mesh_render overlay and needs it: add --mesh_render"
    if a.skeleton_view and a.mesh_render:
        return "--skeleton_view and --mesh_render are the reference's two alternative outputs (demo.py:285-290): give one of them"
    if a.skeleton_view and a.joint_type not in SKELETON_JOINT_TYPES:
        return (f"--skeleton_view has no bone table for --joint_type {a.joint_type}: the skeletons the library emits as 3D joints are "
                + " and ".join(SKELETON_JOINT_TYPES))
    if a.display:
        return "--display opens a window (cv2.imshow / matplotlib) and is not implemented: the frames of --mesh_render are written to disk"
    return None


def save_video(args, folder, output_path, stem):
    """demo.py:379-383, demo_utils.py:160-173: the frames of `folder` as <stem>.mp4, if ffmpeg is there and --save_vid has not switched it off."""
    if args.save_vid and shutil.which("ffmpeg"):
        save_name = osp.join(output_path, stem + ".mp4")
        command = ["ffmpeg", "-y", "-threads", "16", "-start_number", "0", "-i", f"{folder}/%06d.png", "-profile:v", "baseline", "-level", "3.0",
                   "-c:v", "libx264", "-pix_fmt", "yuv420p", "-an", "-v", "error", save_name]
        print(f"Saving result video to {save_name}")
        subprocess.call(command)
    else:
        print(f"The rendered frames are in {folder} (no video: {'--save_vid switches it off' if not args.save_vid else 'no ffmpeg on PATH'}).")


def skeleton_widths(H, W):
    """(bone, grid) line widths in pixels for an H x W panel: matplotlib's lw=2 pt is 2.78 px on its 225.45-px axes, its grid's 0.8 pt 1.11 px."""
    S = min(H, W)
    return max(2, int(round(S / 81))), max(1, int(round(S / 203)))


def image_frames(args):
    """The sorted .png / .jpg names of --img_folder for --skeleton_view; one line and out if the folder holds ready .npy crops (or nothing)."""
    names = sorted(x for x in os.listdir(args.img_folder) if x.endswith((".png", ".jpg")))
    every = sorted(x for x in os.listdir(args.img_folder) if x.endswith((".png", ".jpg", ".npy")))
    if not names or names != every:
        sys.exit("--skeleton_view puts the input frames (.png / .jpg) beside the skeletons: this folder holds ready .npy crops")
    return names


def render_skeleton_view(model, pipe, args, results, view_joints, rot, output_path, stem):
    """demo.py:288-290, 303-361 without --mesh_render: every image of the folder is written as %06d.png, (H, 2W, 3) -- the input on the left, and
    on the right an H x W panel: white, the grid of the three far panes, then the skeleton of every person of the frame in --joint_type's bones,
    turned by the body rotation `rot`, all persons in ONE depth buffer.  view_joints: person -> (T,J,3) joints in --joint_type's skeleton."""
    import torch
    from PIL import Image
    names = image_frames(args)
    n_frames = len(names)
    last = max((int(np.max(r["frame_ids"])) for r in results.values() if len(r["frame_ids"])), default=-1)
    if last >= n_frames:
        sys.exit(f"the tracking file names frame {last}, but {args.img_folder} holds {n_frames} frames")
    frame_results = pipe.prepare_rendering_results(results, list(range(n_frames)))
    bones, bone_colours = pipe.skeleton_bones(args.joint_type)
    grid_points, grid_segments = pipe.skeleton_grid()
    folder = osp.join(output_path, stem + "_output")
    os.makedirs(folder, exist_ok=True)
    print(f"Rendering output video, writing frames to {folder}.")
    for s in range(0, n_frames, RENDER_CHUNK):
        idxs = range(s, min(n_frames, s + RENDER_CHUNK))
        imgs = torch.from_numpy(np.stack([np.asarray(Image.open(osp.join(args.img_folder, names[i])).convert("RGB")) for i in idxs])).to(model.device)
        H, W = imgs.shape[1:3]
        bone_width, grid_width = skeleton_widths(H, W)
        panel = torch.full_like(imgs, 255)
        # the grid is not turned with the body: a call of its own, one copy of it per frame, under the skeletons
        model.render_segments(panel, np.repeat(grid_points[None], len(idxs), 0), grid_segments, [pipe.GRID_COLOUR] * len(grid_segments),
                              [grid_width] * len(grid_segments), list(range(len(idxs))))
        rows = [view_joints[pid][pd["row"]] for fi in idxs for pid, pd in frame_results[fi].items()]
        where = [k for k, fi in enumerate(idxs) for _ in frame_results[fi]]
        if rows:
            model.render_segments(panel, np.stack(rows), bones, bone_colours, [bone_width] * len(bones), where, R=rot)
        out = torch.cat([imgs, panel], 2).cpu().numpy()
        for k, fi in enumerate(idxs):
            Image.fromarray(out[k]).save(osp.join(folder, f"{fi:06d}.png"))
    save_video(args, folder, output_path, stem)
    return folder


def render_overlay(model, pipe, args, results, verts_dev, output_path, stem):
    """demo.py:269-385 with --mesh_render: every image of the folder is written as %06d.png -- the persons of the frame drawn far to near, each
    in its random HSV colour (--wireframe: only the edges of its front faces, as 1-pixel lines), over the frame; with --sideview the same meshes turned by 270 degrees about y on black, appended to the right of
    EVERY frame (the reference widens only frames with a person; frames of one size are what a video needs).  A frame without a person is its
    input.  --save_obj writes the turned mesh per person and frame, with or without --mesh_render."""
    import torch
    from PIL import Image
    names = sorted(x for x in os.listdir(args.img_folder) if x.endswith((".png", ".jpg")))
    every = sorted(x for x in os.listdir(args.img_folder) if x.endswith((".png", ".jpg", ".npy")))
    if args.mesh_render and (not names or names != every):
        sys.exit("--mesh_render draws over image frames (.png / .jpg): this folder holds ready .npy crops")
    n_frames = len(every)
    last = max((int(np.max(r["frame_ids"])) for r in results.values() if len(r["frame_ids"])), default=-1)
    if last >= n_frames:
        sys.exit(f"the tracking file names frame {last}, but {args.img_folder} holds {n_frames} frames")
    frame_results = pipe.prepare_rendering_results(results, list(range(n_frames)))
    mesh_color = {k: colorsys.hsv_to_rgb(np.random.rand(), 0.5, 1.0) for k in results}       # demo.py:277
    folder = osp.join(output_path, stem + "_output")
    if args.mesh_render:
        os.makedirs(folder, exist_ok=True)
        print(f"Rendering output video, writing frames to {folder}.")
    for s in range(0, n_frames, RENDER_CHUNK):
        idxs = range(s, min(n_frames, s + RENDER_CHUNK))
        rows, cams, cols, where = [], [], [], []
        for k, fi in enumerate(idxs):
            for pid, pd in frame_results[fi].items():
                cams.append(pd["cam"]), cols.append(mesh_color[pid]), where.append(k)
                if args.mesh_render:
                    rows.append(verts_dev[pid][pd["row"]])
                if args.save_obj:                                                            # demo.py:332-335
                    obj_dir = osp.join(output_path, "rendered", f"{pid:04d}")
                    os.makedirs(obj_dir, exist_ok=True)
                    pipe.write_obj(osp.join(obj_dir, f"{fi:06d}.obj"), pd["verts"], model.faces)
        if not args.mesh_render:
            continue
        imgs = torch.from_numpy(np.stack([np.asarray(Image.open(osp.join(args.img_folder, names[i])).convert("RGB")) for i in idxs])).to(model.device)
        verts = torch.stack(rows) if rows else None
        if rows:
            model.render(imgs, verts, np.stack(cams), cols, where, wireframe=args.wireframe)
        if args.sideview:
            side = torch.zeros_like(imgs)
            if rows:
                model.render(side, verts, np.stack(cams), cols, where, M=model.SIDE_VIEW, wireframe=args.wireframe)
            imgs = torch.cat([imgs, side], 2)
        out = imgs.cpu().numpy()
        for k, fi in enumerate(idxs):
            Image.fromarray(out[k]).save(osp.join(folder, f"{fi:06d}.png"))
    if not args.mesh_render:
        return None
    save_video(args, folder, output_path, stem)
    return folder


def main(args):
    import joblib
    pkg = importlib.import_module(PKG)
    pipe = importlib.import_module(PKG + ".pipeline")
    cfg = load_cfg(args.cfg)
    if not args.img_folder or not osp.isdir(args.img_folder):
        sys.exit(f'Input image folder "{args.img_folder}" does not exist! (video decoding is out of scope: extract frames first)')
    if not args.tracking_path:
        sys.exit("--tracking_path is required (the YOLOv3+SORT tracker is a separate third-party model)")
    if args.skeleton_view:
        image_frames(args)                                    # refused before the model runs
    video_name = osp.basename(osp.normpath(args.vid_file)).split(".")[0] if args.vid_file else osp.basename(osp.normpath(args.img_folder))
    output_path = osp.join(args.output_folder, video_name, "normal" + time.strftime("-%m%d"))
    os.makedirs(output_path, exist_ok=True)

    tracking = joblib.load(args.tracking_path)
    for pid in list(tracking.keys()):                         # demo.py:101-103
        if tracking[pid]["frames"].shape[0] < MIN_NUM_FRAMES:
            del tracking[pid]
    model = build_model(pkg, args, cfg["DATASET"]["SEQLEN"])
    if (args.mesh_render or args.save_obj) and model.faces is None:
        sys.exit("--mesh_render / --save_obj need the face table: the checkpoint holds no regressor.smpl.smpl.faces_tensor and SMPL_NEUTRAL.npz was not read")
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
    results, verts_dev, n_frames = {}, {}, 0
    view_joints, view_rot = {}, None
    for pid, tr in tracking.items():
        bboxes, frames = np.asarray(tr["bbox"], np.float32).copy(), np.asarray(tr["frames"])
        ds = pipe.InferenceFrames(args.img_folder, frames, bboxes, scale=1.0)
        device_smooth = args.smooth and not args.smooth_on_host
        # the overlay draws the vertices where the forward left them; the skeleton view forms the 49 joints from them
        on_device = device_smooth or args.mesh_render or args.skeleton_view
        pred = pipe.run_tracklet(model, ds.batches(args.grnet_batch_size, model=model), on_device=on_device)
        w, h = ds.image_size()
        theta = pred.pop("theta", None)
        if args.smooth:                                        # demo.py:191-196
            print(f"Running smoothing on person {pid}, min_cutoff: {args.smooth_min_cutoff}, beta: {args.smooth_beta}")
            if device_smooth:
                # filter, Rodrigues, SMPL and the 49 joints on the GPU, reading theta in place; only what the pickle holds is downloaded
                # (the first pass's verts and joints3d are dropped on the device)
                pred["verts"], pred["pose"], pred["joints3d"] = model.smooth_pose(
                    theta, theta[:, 75:], min_cutoff=args.smooth_min_cutoff, beta=args.smooth_beta, joints="spin49")
            else:
                if on_device:                                  # the host statement takes and returns numpy
                    pred = {k: v.cpu().numpy() for k, v in pred.items()}
                pred["verts"], pred["pose"], pred["joints3d"] = pipe.smooth_pose(
                    model, pred["pose"], pred["betas"], min_cutoff=args.smooth_min_cutoff, beta=args.smooth_beta,
                    smpl_tables=smpl_tables)
        if args.mesh_render:
            import torch
            verts_dev[pid] = torch.as_tensor(pred["verts"]).to(model.device)
        if args.skeleton_view:
            # the view and its body rotation are defined on the 49 SPIN joints (demo.py:239-247, 359): --smooth has them, a plain forward
            # emits the 29 spin2 joints, from which and from its vertices the device forms the 49; the pickle stays what it is
            j49 = pred["joints3d"] if args.smooth else model.spin_joints(pred["joints3d"], pred["verts"], joints="spin49")
            j49 = np.asarray(j49.cpu().numpy() if hasattr(j49, "cpu") else j49)
            view_joints[pid] = j49 if args.joint_type == "spin" else pipe.convert_kps(j49, "spin", args.joint_type)
            view_rot = pipe.body_rotation(j49[10])             # demo.py:241: frame 10 of the last person processed
        pred = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in pred.items()}
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
    if args.mesh_render or args.save_obj:
        render_overlay(model, pipe, args, results, verts_dev, output_path, osp.basename(out)[:-len(".pkl")])
    if args.skeleton_view:
        render_skeleton_view(model, pipe, args, results, view_joints, view_rot, output_path, osp.basename(out)[:-len(".pkl")])
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
    p.add_argument("--display", action="store_true", help="parsed, and refused: no window is opened")
    p.add_argument("--mesh_render", action="store_true", help="write the overlay frames (and the video, if ffmpeg is on PATH): the meshes drawn over the input frames on the GPU")
    p.add_argument("--wireframe", action="store_true", help="with --mesh_render: draw the meshes as wireframes (the edges of the front faces, 1-pixel lines) in the main and the side view")
    p.add_argument("--skeleton_view", action="store_true", help="write the reference's other output (and the video): the input frame on the left, the 3D skeletons "
                   "of the frame's persons on the right, from matplotlib's viewpoint, drawn on the GPU; not together with --mesh_render")
    p.add_argument("--sideview", action="store_true", help="with --mesh_render: append the meshes seen from the side, on black, to the right of every frame")
    p.add_argument("--save_obj", action="store_true", help="write rendered/<person>/<frame>.obj, the mesh as the renderer turns it")
    p.add_argument("--smooth", action="store_true")
    p.add_argument("--smooth_min_cutoff", type=float, default=0.004)
    p.add_argument("--smooth_beta", type=float, default=0.7)
    p.add_argument("--smooth_on_host", action="store_true", help="--smooth with the filter, Rodrigues and the 49-joint regression on the CPU "
                   "(pipeline.smooth_pose, the host statement the device path is tested against); default: all of it on the GPU")
    p.add_argument("--tracking_path", type=str, default=None)
    p.add_argument("--img_folder", type=str, default=None)
    p.add_argument("--joint_type", type=str, default="spin")
    p.add_argument("--save_vid", action="store_false", help="as in the reference this switch turns the video OFF (store_false): the frames are kept, ffmpeg is not run")
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
    if refusal(a):
        sys.exit(refusal(a))
    d = parser().parse_args([])
    for flag in ("detector", "yolo_img_size", "tracker_batch_size"):
        if getattr(a, flag) != getattr(d, flag):
            print(f"warning: --{flag} configures a step outside the per-frame path (the tracker, SURVEY 8f) and has no effect here")
    for flag in ("sideview", "save_vid"):
        if getattr(a, flag) != getattr(d, flag) and not a.mesh_render and not (a.skeleton_view and flag == "save_vid"):
            print(f"warning: --{flag} configures the output video and has no effect without --mesh_render")
    main(a)
