"""Host pipeline around the per-frame path: the model loops of the two entry points and their
output formats, restated for the HIP model (numpy on the host, no kernels here).

Reference counterparts:
  * demo model loop + result dict     demo.py:126-231  -> run_tracklet(), make_demo_result()
  * batch 3D-joint generation         batch_generation.py:289-371, 222-284 -> run_on_frames(), BatchDb
  * boxes from OpenPose 2D joints     batch_generation.py:39-93, 95-178 -> bbox_from_joints2d(), openpose_boxes()
  * pose metrics (no counterpart)     DESIGN 4.8 -> pose_metrics()
  * crop-cam / crop-coords -> image   lib/utils/demo_utils.py:176-209
  * spin2 -> kinectv2 joints          lib/data_utils/kp_utils.py:26-36 with the tables :211-242, :904-931
  * crop + normalise of a frame       lib/dataset/inference.py:71-87, lib/data_utils/img_utils.py:252-285,355-363
    (SURVEY 8f-1 "next": OpenCV's warpAffine is third-party and absent offline -- parity UNPINNED; the
    PIL bilinear crop below follows the same geometry: box centre/size * scale -> 224x224, border 0)
"""
import math
import os
import os.path as osp
from collections import defaultdict

import numpy as np
import torch

from . import netspec
from ._lib import BALANCE_SEGMENTS_KINECTV2, GAIT_JOINTS_KINECTV2, KINEMATICS_JOINTS_KINECTV2

IMAGENET_MEAN = np.array([0.485, 0.456, 0.406], np.float32)
IMAGENET_STD = np.array([0.229, 0.224, 0.225], np.float32)
MAX_VID = 50          # batch_generation.py:36
MAX_SEQLEN = 400      # batch_generation.py:37 (MAX_seqlen)


# ----------------------------------------------------------------------------- output conversions
def convert_crop_cam_to_orig_img(cam, bbox, img_width, img_height):
    """(n,3) weak-perspective crop camera [s,tx,ty] -> (n,4) [sx,sy,tx,ty] in the full image (demo_utils.py:176-193)."""
    cx, cy, h = bbox[:, 0], bbox[:, 1], bbox[:, 2]
    hw, hh = img_width / 2.0, img_height / 2.0
    sx = cam[:, 0] * (1.0 / (img_width / h))
    sy = cam[:, 0] * (1.0 / (img_height / h))
    tx = ((cx - hw) / hw / sx) + cam[:, 1]
    ty = ((cy - hh) / hh / sy) + cam[:, 2]
    return np.stack([sx, sy, tx, ty]).T


def convert_crop_coords_to_orig_img(bbox, keypoints, crop_size=224):
    """normalised crop keypoints (n,J,2) in [-1,1] -> image pixels (demo_utils.py:196-209)."""
    cx, cy, h = bbox[:, 0], bbox[:, 1], bbox[:, 2]
    kp = 0.5 * crop_size * (np.asarray(keypoints, np.float32) + 1.0)
    kp = kp * (h[..., None, None] / crop_size)
    kp[:, :, 0] = (cx - h / 2)[..., None] + kp[:, :, 0]
    kp[:, :, 1] = (cy - h / 2)[..., None] + kp[:, :, 1]
    return kp


_KPS = None


def _kps_tables():
    global _KPS
    if _KPS is None:
        import json
        with open(osp.join(osp.dirname(osp.abspath(__file__)), "kps_tables.json")) as f:
            _KPS = json.load(f)
    return _KPS


def convert_kps(joints, src, dst):
    """convert_kps (kp_utils.py:26-36): (n,J_src,3) joints of skeleton ``src`` -> (n,J_dst,3) float64 in skeleton ``dst``; joints
    ``dst`` names that ``src`` lacks stay 0.  ``src`` is 'spin' (49) or 'spin2' (29) -- the two layouts the path emits; the index
    tables are derived by running the reference's joint-name functions (tools/make_kps_tables.py).  An unknown ``dst`` raises
    NameError, as the reference's eval() does (demo.py:227 catches exactly that)."""
    t = _kps_tables()
    if src not in ("spin", "spin2"):
        raise NameError(f"name 'get_{src}_joint_names' is not defined")
    if dst not in t["sizes"]:
        raise NameError(f"name 'get_{dst}_joint_names' is not defined")
    joints = np.asarray(joints)
    idx = t["from_" + src][dst]
    out = np.zeros((joints.shape[0], len(idx), 3))
    for k, i in enumerate(idx):
        if i >= 0:
            out[:, k] = joints[:, i]                          # IndexError / shape error on a wrong-sized input, like the reference
    return out


def spin2_to_kinectv2(joints):
    """(n,29,3) spin2 joints -> (n,25,3) kinectv2 joints (convert_kps(src='spin2', dst='kinectv2'))."""
    joints = np.asarray(joints)
    return joints[:, netspec.SPIN2_TO_KINECTV2].astype(np.float64)      # the reference returns float64 zeros-based arrays


# ----------------------------------------------------------------------------- --smooth (row f3)
def one_euro_filter(x, min_cutoff=0.004, beta=0.7, d_cutoff=1.0):
    """The One-Euro filter as smooth_pose drives it (one_euro_filter.py:5-46, smooth_pose.py:47-52,84-88): unit time
    steps, state initialised with x[0] and dx = 0; x (T, ...) -> filtered (T, ...), element-wise."""
    x = np.asarray(x)
    out = np.zeros_like(x)
    out[0] = x[0]
    x_prev, dx_prev = x[0], np.zeros_like(x[0])

    def alpha(cutoff):                                       # smoothing_factor with t_e = 1
        r = 2 * np.pi * cutoff
        return r / (r + 1)

    a_d = alpha(d_cutoff)
    for t in range(1, x.shape[0]):
        dx = x[t] - x_prev
        dx_hat = a_d * dx + (1 - a_d) * dx_prev
        a = alpha(min_cutoff + beta * np.abs(dx_hat))
        x_hat = a * x[t] + (1 - a) * x_prev
        out[t] = x_hat
        x_prev, dx_prev = x_hat, dx_hat
    return out


def rodrigues(aa):
    """Axis-angle (n,3) -> rotation matrices (n,3,3): smplx's batch_rodrigues (angle = |aa + 1e-8|, R = I + sin K +
    (1 - cos) K^2), the conversion smplx.SMPL applies when smooth_pose passes axis-angle poses.  Third-party: unpinned."""
    aa = np.asarray(aa, np.float32)
    angle = np.linalg.norm(aa + np.float32(1e-8), axis=1, keepdims=True)
    d = aa / angle
    K = np.zeros((aa.shape[0], 3, 3), np.float32)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -d[:, 2], d[:, 1], d[:, 2], -d[:, 0], -d[:, 1], d[:, 0]
    s, c = np.sin(angle)[..., None], np.cos(angle)[..., None]
    return (np.eye(3, dtype=np.float32)[None] + s * K + (1 - c) * (K @ K)).astype(np.float32)


def smooth_pose(model, pred_pose, pred_betas, min_cutoff=0.004, beta=0.7, kinectv2=False, smpl_tables=None):
    """lib/utils/smooth_pose.py:28-116: One-Euro filter over the axis-angle pose, then SMPL re-evaluated per frame with
    the betas of frame 0 (smooth_pose.py:97) -- batched into one LBS launch here.  Returns (verts, pose_hat, joints3d)
    with joints3d in the 49-joint SPIN order (kinectv2=False, what demo.py gets) or 25 kinectv2 joints."""
    T = pred_betas.shape[0]
    pose = np.asarray(pred_pose, np.float32).reshape(T, 24, 3)
    pose_hat = one_euro_filter(pose, min_cutoff, beta).astype(np.float32)
    rot = rodrigues(pose_hat.reshape(-1, 3)).reshape(T, 24, 3, 3)
    betas0 = np.repeat(np.asarray(pred_betas, np.float32)[:1], T, axis=0)
    verts, kp29, _ = model.smpl_forward(torch.from_numpy(betas0), torch.from_numpy(rot))
    verts, kp29 = verts.cpu().numpy(), kp29.cpu().numpy()
    if kinectv2:
        joints = spin2_to_kinectv2(kp29)
    else:
        if smpl_tables is None:
            raise ValueError("the 49-joint SPIN output needs J_regressor_extra (smpl_tables)")
        j45 = np.concatenate([kp29[:, :24], verts[:, netspec.SMPL_EXTRA_VERT_IDS]], 1)
        extra = np.einsum("jv,nvk->njk", np.asarray(smpl_tables["J_regressor_extra"], np.float32), verts)
        joints = np.concatenate([j45, extra], 1)[:, netspec.SPIN49_FROM_54]
    return verts, pose_hat.reshape(T, 72), joints


def smooth_pose_device(model, pred_pose, pred_betas, min_cutoff=0.004, beta=0.7, kinectv2=False):
    """smooth_pose() with every step on the GPU (GRNet.smooth_pose: filter, Rodrigues, SMPL and the joint selection in one C call):
    pred_pose (T,72) or a (T,85) theta and pred_betas (T,10), host arrays or device tensors.  Same return contract as smooth_pose --
    numpy (verts, pose_hat, joints3d), joints3d the 49 SPIN joints in float32 or, with kinectv2, 25 joints in float64 as convert_kps
    returns them -- and no smpl_tables argument: the handle holds all nine rows of J_regressor_extra.  The filtered pose is the
    reference's bit for bit (smooth_pose's one_euro_filter forms a_d in double and is within 1e-6 of it)."""
    verts, pose_hat, joints = model.smooth_pose(pred_pose, pred_betas, min_cutoff=min_cutoff, beta=beta,
                                                joints="kinectv2" if kinectv2 else "spin49")
    joints = joints.cpu().numpy()
    return verts.cpu().numpy(), pose_hat.cpu().numpy(), joints.astype(np.float64) if kinectv2 else joints


# ----------------------------------------------------------------------------- the crop's affine map, as the reference forms it
def _affine_from_box(cx, cy, w, h, dst_w, dst_h, scale):
    """gen_trans_from_patch_cv (img_utils.py:54-88, rot = 0) + cv2.getAffineTransform, then the inversion cv2.warpAffine applies:
      * src_w = w*scale, src_h = h*scale in double (numpy 1.18 promotes float32-scalar * Python float to float64);
      * the two triangles as FLOAT32 points: centre, centre + (0, src_h/2), centre + (src_w/2, 0) and (dst_w/2, dst_h/2), + (0, dst_h/2), + (dst_w/2, 0);
      * getAffineTransform: the 6x6 system of the three point pairs solved in double (LU with partial pivoting);
      * warpAffine (no WARP_INVERSE_MAP) inverts the 2x3 matrix in double: D = 1/(M0*M4 - M1*M3), ...
    The LU's last-bit rounding can differ between LAPACK and OpenCV; it matters only where cvRound(x*1024) sits on an exact tie."""
    src_w, src_h = float(w) * float(scale), float(h) * float(scale)
    centre = np.array([cx, cy], np.float64)
    src = np.zeros((3, 2), np.float32)
    src[0] = centre
    src[1] = centre + np.array([0, src_h * 0.5], np.float32)
    src[2] = centre + np.array([src_w * 0.5, 0], np.float32)
    dc = np.array([dst_w * 0.5, dst_h * 0.5], np.float32)
    dst = np.zeros((3, 2), np.float32)
    dst[0] = dc
    dst[1] = dc + np.array([0, dst_h * 0.5], np.float32)
    dst[2] = dc + np.array([dst_w * 0.5, 0], np.float32)
    a = np.zeros((6, 6), np.float64)
    b = np.zeros(6, np.float64)
    for k in range(3):
        a[2 * k, 0:2], a[2 * k, 2] = src[k], 1.0
        a[2 * k + 1, 3:5], a[2 * k + 1, 5] = src[k], 1.0
        b[2 * k], b[2 * k + 1] = dst[k]
    m = np.linalg.solve(a, b)                              # [M0 M1 M2 M3 M4 M5]
    d = m[0] * m[4] - m[1] * m[3]
    d = 1.0 / d if d != 0 else 0.0
    a11, a22 = m[4] * d, m[0] * d
    m0, m1, m3, m4 = a11, m[1] * -d, m[3] * -d, a22
    return (m0, m1, -m0 * m[2] - m1 * m[5], m3, m4, -m3 * m[2] - m4 * m[5])


def cv_crop_maps(bboxes, scale=1.0, crop_size=224):
    """(n,4) boxes [cx,cy,w,h] -> (n,10) float64 records for grnet_crop_normalise_cv_maps: what generate_patch_image_cv
    (img_utils.py:90-113, called by get_single_image_crop_demo :252-285 with do_flip = False, rot = 0) makes cv2.warpAffine evaluate.
      * w == h (what the tracker path of demo.py produces): ONE warp into the patch -- record = [inverse map (6), 0, 0, 0, 0];
      * w != h (:97-106; precomputed annotations may hold such boxes): TWO warps -- the scaled box resized, aspect kept, to
        (iw, ih) = (int(s*w), int(s*h)) with s = crop/max(w, h), whose uint8 result is then moved by (crop/2 - iw/2, crop/2 - ih/2)
        into the patch (the letterbox stays 0; a half-pixel offset blends neighbours) -- record = [inverse of the first map (6), iw, ih,
        tx, ty] with (tx, ty) the inverse translation.  The comparison is exact, as the reference's `bb_width != bb_height` is."""
    bboxes = np.asarray(bboxes)
    out = np.zeros((bboxes.shape[0], 10), np.float64)
    for i, (cx, cy, w, h) in enumerate(bboxes):
        if float(w) != float(h):
            s = crop_size / max(float(h), float(w))
            iw, ih = int(s * float(w)), int(s * float(h))
            if iw < 1 or ih < 1:
                raise ValueError(f"box {i} is {float(w)} x {float(h)}: its aspect-preserving resize has an empty side ({iw} x {ih}); the reference's cv2.warpAffine refuses that size too")
            out[i, :6] = _affine_from_box(cx, cy, w, h, iw, ih, scale)
            dx, dy = crop_size / 2 - iw / 2, crop_size / 2 - ih / 2
            out[i, 6:] = (iw, ih, -1.0 * dx - (-0.0) * dy, -(-0.0) * dx - 1.0 * dy)      # warpAffine's inversion of [[1,0,dx],[0,1,dy]]
        else:
            out[i, :6] = _affine_from_box(cx, cy, w, h, crop_size, crop_size, scale)
    return out


def cv_inverse_affine(bboxes, scale=1.0, crop_size=224):
    """(n,4) SQUARE boxes -> (n,6) float64: the inverse affine map of the single-warp crop (the first six entries of cv_crop_maps).
    A box with w != h takes the reference's two-warp branch, which one map cannot describe: ValueError -- use cv_crop_maps."""
    maps = cv_crop_maps(bboxes, scale, crop_size)
    if np.any(maps[:, 6] != 0):
        raise ValueError(f"box {int(np.nonzero(maps[:, 6])[0][0])} is not square: the reference crops it in two warps (img_utils.py:97-106); cv_crop_maps describes both")
    return np.ascontiguousarray(maps[:, :6])


# ----------------------------------------------------------------------------- frame sources
def crop_and_normalise(img_rgb_u8, bbox, scale=1.0, crop_size=224):
    """One frame: uint8 HxWx3 RGB + [cx,cy,w,h] -> float32 (3,224,224), ImageNet-normalised.

    Geometry of get_single_image_crop_demo / generate_patch_image_cv without rotation: the square box
    of side max(w,h)*scale ... the reference passes w == h boxes; pixels outside the image are 0.
    """
    from PIL import Image
    cx, cy, w, h = [float(v) for v in bbox]
    a, e = w * scale / crop_size, h * scale / crop_size
    # cv2.warpAffine geometry (integer coordinates are pixel centres): x = (u - 112) * a + cx.  PIL samples at pixel
    # centres u + 0.5 and expects source coordinates in the same half-pixel convention, hence the +-0.5 terms.
    c0 = cx - 0.5 * crop_size * a + 0.5 - 0.5 * a
    f0 = cy - 0.5 * crop_size * e + 0.5 - 0.5 * e
    img = Image.fromarray(img_rgb_u8)
    crop = img.transform((crop_size, crop_size), Image.AFFINE, (a, 0.0, c0, 0.0, e, f0), resample=Image.BILINEAR, fillcolor=0)
    x = np.asarray(crop, np.float32) / 255.0
    x = (x - IMAGENET_MEAN) / IMAGENET_STD
    return np.ascontiguousarray(x.transpose(2, 0, 1))


class InferenceFrames:
    """Counterpart of lib/dataset/inference.py:Inference for a folder of extracted frames.

    Accepts .png/.jpg (cropped + normalised on the fly) or .npy files holding already-normalised
    (3,224,224) crops (the synthetic-frame configs).  As in the reference, ``bboxes[:, 2:]`` is multiplied
    by ``scale`` in place at construction AND ``scale`` is applied again in the crop (inference.py:48,80).
    """

    def __init__(self, image_folder, frames, bboxes, scale=1.0, crop_size=224):
        names = sorted(x for x in os.listdir(image_folder) if x.endswith((".png", ".jpg", ".npy")))
        self.files = np.array([osp.join(image_folder, x) for x in names])[frames]
        self.bboxes = bboxes
        self.bboxes[:, 2:] *= scale
        self.frames = frames
        self.scale, self.crop_size = scale, crop_size

    def __len__(self):
        return len(self.files)

    def __getitem__(self, idx):
        f = self.files[idx]
        if f.endswith(".npy"):
            return np.load(f).astype(np.float32)
        from PIL import Image
        img = np.asarray(Image.open(f).convert("RGB"))
        return crop_and_normalise(img, self.bboxes[idx], self.scale, self.crop_size)

    def image_size(self):
        f = self.files[0]
        if f.endswith(".npy"):
            return 224, 224
        from PIL import Image
        with Image.open(f) as im:
            return im.size

    def batches(self, batch_size, model=None):
        """(<=batch,3,224,224) crops.  With ``model`` (a GRNet) and image files, the raw uint8 frames are uploaded and
        cropped + normalised by the HIP kernel (grnet_crop_normalise) instead of on the host."""
        from PIL import Image
        device_crop = model is not None and len(self) and not self.files[0].endswith(".npy")
        for s in range(0, len(self), batch_size):
            idx = range(s, min(s + batch_size, len(self)))
            if not device_crop:
                yield np.stack([self[i] for i in idx])
                continue
            raw = np.stack([np.asarray(Image.open(self.files[i]).convert("RGB")) for i in idx])
            yield model.crop_normalise(torch.from_numpy(raw).cuda(), torch.from_numpy(np.ascontiguousarray(self.bboxes[list(idx)])),
                                       scale=self.scale)


# ----------------------------------------------------------------------------- model loops
def run_tracklet(model, batches, device="cuda", on_device=False):
    """demo.py:151-188: feed (<=batch,3,224,224) batches, slice theta, concatenate, to numpy.
    on_device: the same dict as tensors on ``device`` plus "theta" (T,85), whose rows GRNet.smooth_pose reads in place; nothing is
    downloaded and nothing synchronises with the host."""
    acc = defaultdict(list)
    for batch in batches:
        x = torch.as_tensor(batch, dtype=torch.float32).unsqueeze(0).to(device)
        bs, t = x.shape[:2]
        out = model(x)[-1]
        acc["pred_cam"].append(out["theta"][:, :, :3].reshape(bs * t, -1))
        acc["verts"].append(out["verts"].reshape(bs * t, -1, 3))
        acc["pose"].append(out["theta"][:, :, 3:75].reshape(bs * t, -1))
        acc["betas"].append(out["theta"][:, :, 75:].reshape(bs * t, -1))
        acc["joints3d"].append(out["kp_3d"].reshape(bs * t, -1, 3))
        acc["smpl_joints2d"].append(out["kp_2d"].reshape(bs * t, -1, 2))
        if on_device:
            acc["theta"].append(out["theta"].reshape(bs * t, -1))
    if on_device:
        return {k: torch.cat(v, 0) for k, v in acc.items()}
    return {k: torch.cat(v, 0).cpu().numpy() for k, v in acc.items()}


def run_tracks_overlapped(model, tracks, batch_size=64, scale=1.1):
    """BASELINE configs[4] on one GPU: several person tracks, each a list of (raw uint8 frames (n,H,W,3), boxes (n,4)) batches.
    Upload + crop/normalise (grnet_crop_normalise, row f1) of batch k+1 run on a side HIP stream while the forward of batch k
    (a replayed hipGraph when GRNET_OPT_USE_GRAPH is set: fixed crop buffers make the pointers repeat) runs on the current
    stream; two crop buffers alternate and events order the hand-over.  Returns one demo-style dict per track
    (demo.py:151-188 slicing), identical to calling crop_normalise + model() batch after batch."""
    dev = model.device
    main = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(device=dev)
    work = [(ti, raw, bb) for ti, batches in enumerate(tracks) for (raw, bb) in batches]
    n_max = max((len(bb) for _, _, bb in work), default=0)
    if n_max > batch_size:
        raise ValueError("a batch is larger than batch_size")
    bufs = [torch.empty(n_max, 3, 224, 224, dtype=torch.float32, device=dev) for _ in range(2)]
    ready = [torch.cuda.Event() for _ in range(2)]         # crop k has landed in bufs[k % 2]
    free = [torch.cuda.Event() for _ in range(2)]          # the forward that read bufs[k % 2] is done
    for e in free:
        e.record(main)

    def stage(k):
        _, raw, bb = work[k]
        with torch.cuda.stream(side):
            side.wait_event(free[k % 2])
            crop = model.crop_normalise(torch.as_tensor(raw).to(dev, non_blocking=True), torch.as_tensor(bb), scale=scale)
            bufs[k % 2][:len(bb)].copy_(crop)
            ready[k % 2].record(side)

    acc = [defaultdict(list) for _ in tracks]
    if work:
        stage(0)
    for k, (ti, _, bb) in enumerate(work):
        if k + 1 < len(work):
            stage(k + 1)                                    # overlaps the forward below
        main.wait_event(ready[k % 2])
        out = model(bufs[k % 2][:len(bb)].unsqueeze(0))[-1]
        free[k % 2].record(main)
        t = len(bb)
        a = acc[ti]
        a["pred_cam"].append(out["theta"][:, :, :3].reshape(t, -1))
        a["verts"].append(out["verts"].reshape(t, -1, 3))
        a["pose"].append(out["theta"][:, :, 3:75].reshape(t, -1))
        a["betas"].append(out["theta"][:, :, 75:].reshape(t, -1))
        a["joints3d"].append(out["kp_3d"].reshape(t, -1, 3))
        a["smpl_joints2d"].append(out["kp_2d"].reshape(t, -1, 2))
    return [{k: torch.cat(v, 0).cpu().numpy() for k, v in a.items()} for a in acc]


def make_demo_result(pred, bboxes, frames, orig_width, orig_height):
    """The per-person dict the demo pickles (demo.py:198-222)."""
    return {
        "pred_cam": pred["pred_cam"],
        "orig_cam": convert_crop_cam_to_orig_img(pred["pred_cam"], bboxes, orig_width, orig_height),
        "verts": pred["verts"],
        "pose": pred["pose"],
        "betas": pred["betas"],
        "joints3d": pred["joints3d"],
        "joints2d": convert_crop_coords_to_orig_img(bboxes, pred["smpl_joints2d"], crop_size=224),
        "bboxes": bboxes,
        "frame_ids": frames,
    }


def prepare_rendering_results(results, nframes):
    """demo_utils.py:212-247 in its non-concat form: {person: per-person dict} -> {frame: OrderedDict person -> {'verts','cam','j3d','j2d'}}
    for the frames listed in ``nframes``, the persons of a frame sorted far to near by the y-scale of the camera in the original image
    (orig_cam[1] ascending, :242-246).  Added here: 'row', the index of the frame in the person's arrays, so that a caller which keeps the
    vertices on the device draws row ``row`` of its own tensor instead of the host copy."""
    from collections import OrderedDict
    if not isinstance(nframes, list):
        raise TypeError("Input should be list of valid frames !!")
    frame_results = {nf: {} for nf in nframes}
    for person_id, person_data in results.items():
        for idx, frame_id in enumerate(person_data["frame_ids"]):
            frame_results[int(frame_id)][person_id] = {
                "verts": person_data["verts"][idx],
                "cam": person_data["orig_cam"][idx],
                "j3d": person_data["joints3d"][idx],
                "j2d": person_data["joints2d"][idx],
                "row": idx,
            }
    for frame_id, frame_data in frame_results.items():
        keys = list(frame_data.keys())
        sort_idx = np.argsort([frame_data[k]["cam"][1] for k in keys])
        frame_results[frame_id] = OrderedDict((keys[i], frame_data[keys[i]]) for i in sort_idx)
    return frame_results


# ----------------------------------------------------------------------------- the 3D skeleton view (demo.py:238-247, 303-361; vis.py:571-587)
SKELETON_ELEV, SKELETON_AZIM = 200.0, -27.0                   # demo.py:311 view_init
SKELETON_LIMITS = ((-0.6, 0.6), (-1.0, 1.0), (-1.0, 1.0))     # demo.py:312-314
SKELETON_TICKS = (7, 11, 11)                                  # demo.py:315-319: linspace over the limits
SKELETON_WINDOW = (-0.095, 0.09, -0.095, 0.09)                # what matplotlib's 3D axes show of the projected plane: (x0, x1, y0, y1)
BONE_COLOURS = ((215, 48, 39), (69, 117, 180))                # vis.py:575-585: even bones, odd bones (RGB)
GRID_COLOUR = (176, 176, 176)                                 # matplotlib's grid colour, #b0b0b0
# Bones as pairs of joint indices, in the order the reference draws them (the order decides the colour and, at equal depth, the winner).
# 'spin': over the 49 SPIN joints, whose first 25 are OpenPose's BODY_25 -- head and trunk, arms, legs, face, feet, and nose -> headtop (38).
# 'kinectv2': over the 25 Kinect v2 joints -- spine, arms from the thorax (20), hands, legs.  tests/golden/skeleton_view.npz pins both.
_BONES = {
    "spin": ((0, 1), (1, 2), (1, 5), (2, 3), (5, 6), (3, 4), (6, 7), (1, 8), (8, 12), (8, 9), (12, 13), (9, 10), (13, 14), (10, 11), (0, 16), (0, 15),
             (16, 18), (15, 17), (21, 20), (24, 23), (19, 20), (22, 23), (19, 21), (22, 24), (14, 21), (11, 24), (0, 38)),
    "kinectv2": ((0, 1), (20, 2), (1, 20), (2, 3), (20, 4), (20, 8), (4, 5), (8, 9), (5, 6), (9, 10), (6, 7), (10, 11), (7, 21), (11, 23), (6, 22),
                 (10, 24), (0, 12), (0, 16), (12, 13), (16, 17), (13, 14), (17, 18), (14, 15), (18, 19)),
}


def skeleton_view():
    """(P (4,4) float64, window (x0, x1, y0, y1)): matplotlib's Axes3D.get_proj() for the reference's axes -- view_init(elev=200, azim=-27), the
    limits above, and matplotlib's defaults: box aspect 4:4:3 (times 25/21), eye distance 10, focal length 1, roll 0, vertical axis z -- by closed
    formula; matplotlib is not imported.  Projected coordinates are (P p)[0,1] / (P p)[3]; the axes show the window of them."""
    e, a = np.deg2rad(SKELETON_ELEV), np.deg2rad(SKELETON_AZIM)
    lim = np.array(SKELETON_LIMITS)
    aspect = np.array([4.0, 4.0, 3.0])
    aspect *= 1.8294640721620434 * 25 / 24 / np.linalg.norm(aspect)        # matplotlib's set_box_aspect: (4, 4, 3) * 25/84 to 1e-9, i.e. x and y 25/21
    dist, focal = 10.0, 1.0
    world = np.eye(4)                                          # the limits -> the box [0, aspect]
    world[[0, 1, 2], [0, 1, 2]] = aspect / (lim[:, 1] - lim[:, 0])
    world[:3, 3] = -lim[:, 0] * aspect / (lim[:, 1] - lim[:, 0])
    w = np.array([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)])      # unit, from the box's centre to the eye
    eye = aspect / 2 + dist * focal * w
    norm_elev = (SKELETON_ELEV + 180.0) % 360.0 - 180.0       # beyond +-90 degrees the axes stand on their head
    up = np.array([0.0, 0.0, -1.0 if abs(norm_elev) > 90.0 else 1.0])
    u = np.cross(up, w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    look = np.eye(4)
    look[:3, :3] = np.stack([u, v, w])
    look[:3, 3] = -np.stack([u, v, w]) @ eye
    zfront, zback = -dist, dist
    persp = np.array([[focal, 0, 0, 0], [0, focal, 0, 0], [0, 0, (zfront + zback) / (zfront - zback), -2 * zfront * zback / (zfront - zback)], [0, 0, -1, 0]])
    return persp @ look @ world, SKELETON_WINDOW


def skeleton_bones(name):
    """(bones (B,2) int64, colours (B,3) uint8 RGB) of the skeleton the view draws for --joint_type ``name``: 'spin' (the 49 joints) or
    'kinectv2' (25), the two skeletons the library emits as 3D joints; the colours alternate (vis.py:585).  Any other name raises NameError,
    as convert_kps does."""
    if name not in _BONES:
        raise NameError(f"name 'get_{name}_skeleton' is not defined")
    bones = np.array(_BONES[name], np.int64)
    return bones, np.array([BONE_COLOURS[i % 2] for i in range(len(bones))], np.uint8)


def skeleton_grid():
    """(points (N,3) float64, segments (N/2,2) int64): the grid lines on the three FAR panes of the view's box, at the reference's ticks.  Of
    the two panes of an axis the far one is that whose centre has the larger homogeneous coordinate P[3] . (c, 1)."""
    P, _ = skeleton_view()
    lim = np.array(SKELETON_LIMITS)
    ticks = [np.linspace(lo, hi, k) for (lo, hi), k in zip(SKELETON_LIMITS, SKELETON_TICKS)]
    pts = []
    for axis in range(3):
        far = lim[axis, 1] if P[3, axis] * lim[axis, 1] > P[3, axis] * lim[axis, 0] else lim[axis, 0]
        b, c = [k for k in range(3) if k != axis]
        for along, across in ((b, c), (c, b)):                 # lines at the ticks of `along`, spanning `across`
            for t in ticks[along]:
                for end in lim[across]:
                    p = np.zeros(3)
                    p[axis], p[along], p[across] = far, t, end
                    pts.append(p)
    pts = np.array(pts)
    return pts, np.arange(len(pts), dtype=np.int64).reshape(-1, 2)


def body_rotation(j49):
    """demo.py:239-247: the rotation that turns the body towards the view's x axis, from ONE frame of the 49 SPIN joints (49,3): h = lhip - rhip
    (joints 28, 27), v = thorax - hip (40, 39), both normalised; R = orthogonal_procrustes([[1,0,0]], cross(h, v)) by scipy's formula.  The input
    has rank 1: only the first row, e_x R = cross(h, v) / |cross(h, v)|, is determined; the rest is what LAPACK's SVD returns, in the
    reference as here.  Points are drawn as R p (demo.py:325)."""
    j = np.asarray(j49, np.float64).reshape(49, 3)
    h, v = j[28] - j[27], j[40] - j[39]
    h, v = h / np.linalg.norm(h), v / np.linalg.norm(v)
    A, B = np.array([[1.0, 0.0, 0.0]]), np.cross(h, v).reshape(1, 3)
    u, _, vt = np.linalg.svd((B.T @ A).T)
    return u @ vt


def write_obj(path, verts, faces):
    """The mesh renderer.py:82-86 exports per person and frame: the vertices turned by 180 degrees about x, (x, -y, -z), and the faces, 1-based."""
    v = np.asarray(verts, np.float64) * np.array([1.0, -1.0, -1.0])
    with open(path, "w") as f:
        f.write("".join(f"v {x:.8f} {y:.8f} {z:.8f}\n" for x, y, z in v))
        f.write("".join(f"f {a} {b} {c}\n" for a, b, c in np.asarray(faces, np.int64) + 1))


# ----------------------------------------------------------------------------- boxes from 2D joints
BBOX_MIN_PIXEL, BBOX_SMALL_SCALE = 500, 1.8                   # batch_generation.py:27-28 (MIN_PIXEL, BS)
OPENPOSE_INTERACTIONS = (44, 45, 46, 47, 48)                  # :99, actions with two people
OPENPOSE_MIN_CREDIBLE, OPENPOSE_MIN_SDIFF, OPENPOSE_MAX_THRESH = 3, 0.01, 0.3      # :30-32 (M, MIN_sdiff, MAX_THRESH)


def medoid_index(points, block=256):
    """The exact 1-medoid of float32 points: argmin_i sum_j |p_i - p_j| with the distances and sums in float64, lowest index on ties.  Row
    blocks, so no n x n array is formed."""
    cols = np.ascontiguousarray(np.asarray(points, np.float32).astype(np.float64).T)
    best, at = np.inf, 0
    for a in range(0, cols.shape[1], block):
        d2 = sum((c[a:a + block, None] - c[None, :]) ** 2 for c in cols)
        c = np.sqrt(d2).sum(axis=1)
        k = int(np.argmin(c))
        if c[k] < best:
            best, at = c[k], a + k
    return at


def bbox_from_joints2d(kp_2d, threshold=0.1):
    """get_bbox_from_joints2d(kp_2d, smooth=False, threshold) of batch_generation.py:39-93 in numpy float64, the host statement of
    GRNet.bbox_from_joints2d: kp_2d (T,K,3) rows (x, y, score) in pixels -> (T,4) float64, the one box [cx, cy, nw, nh] repeated.  Joints
    whose score is below the threshold take the frame's first joint of highest score; the centre is the exact 1-medoid of the T K float32
    points over ALL THREE columns (the reference hands x, y and the score to euclidean_distances), which is the fixed point of its
    kmedoids.fasterpam with one medoid; nw = nh = median(h) * 1.1, times 1.8 below 500 (the median of w is computed there and dropped)."""
    kp = np.array(kp_2d, dtype=np.float64)
    if kp.ndim != 3 or kp.shape[2] != 3 or kp.shape[0] < 1 or kp.shape[1] < 1:
        raise ValueError(f"kp_2d must be (T,K,3) with T, K >= 1, got {kp.shape}")
    if not np.isfinite(kp).all():
        raise ValueError("kp_2d has a non-finite entry")
    T, K = kp.shape[:2]
    invalid = kp[:, :, 2] < threshold
    ref = np.repeat(kp[np.arange(T), np.argmax(kp[:, :, 2], axis=-1)][:, None, :], K, axis=1)
    kp[invalid] = ref[invalid]
    ul_y, lr_y = kp[:, :, 1].min(axis=1), kp[:, :, 1].max(axis=1)
    ul_y -= (lr_y - ul_y) * 0.10                               # prevent cutting the head
    h = lr_y - ul_y
    points = kp.reshape(-1, 3).astype(np.float32)
    c_xy = points[medoid_index(points), :2]
    nh = np.median(h) * 1.1
    if nh < BBOX_MIN_PIXEL:
        nh = nh * BBOX_SMALL_SCALE
    return np.repeat(np.array([c_xy[0], c_xy[1], nh, nh], np.float64)[None, :], T, axis=0)


def openpose_boxes(anno_folder, model=None, img_w=1920, img_h=1080, return_joints=False, track=None):
    """load_openpose_anno of batch_generation.py:95-178 without its vis branches: one box per OpenPose .mat file of anno_folder ->
    (boxes {vid_name: (T,4) float64, or None where no candidate's box has a positive size}, bad [file names]).  Every rule is the
    reference's as written: files are 'A<action>_...' and the interaction actions 44-48 are skipped; 'skeleton' is (P,T,25,3), normalised;
    an empty array, no person with more than 3 joints of positive score in every frame (:114), or no person passing the :120 test is a
    bad file -- :120 indexes the 4-D array as joints2d[:,:,2], so it looks at the three components of JOINT 2 only; of several persons those
    within 0.01 of the best mean score stay; x and y are scaled to pixels; the candidate with the strictly largest box wins, the first of
    equal ones.  np.bool (:126) no longer exists in numpy: it is bool here.  Files are visited in sorted order (the reference: os.listdir
    order), and a 'skeleton' of another dtype is widened to float64 first.
    model=None: pipeline.bbox_from_joints2d per candidate.  With a GRNet, EVERY candidate of every file goes into ONE
    model.bbox_from_joints2d call and the choice runs on the returned boxes.
    return_joints: a third value, {vid_name: the scaled (T,25,3) float64 joints (x, y in pixels, score) of the candidate whose box won, or None}
    -- what fit_translation needs beside the 3D joints.
    track: {'kernel_size', 'sigma', 'pad', 'vis_thresh'} (each optional: 1, 0, 'zero', 0.3) -- per-frame boxes instead of the one fixed box
    (DESIGN 4.10).  The person is chosen exactly as above, by the fixed box; then the winners of ALL files go into ONE track_boxes call
    (model.track_boxes, or pipeline.track_boxes with model=None) and a video keeps the frames [start, end) from its first to its last
    detection, as the reference's Inference does (lib/dataset/inference.py:64-66): boxes[vid_name] is (end - start, 4), the returned joints
    are sliced the same way, and a further last value {vid_name: {'range': (start, end), 'frames': T, 'status': (end - start,) uint8}} says
    which frames they were.  A video without any detection has None for all three."""
    import scipy.io as sio
    assert osp.isdir(anno_folder), anno_folder
    boxes, bad, cands = {}, [], []                             # cands: (vid_name, [scaled (T,25,3) candidates])
    for name in sorted(os.listdir(anno_folder)):
        if int(name.split("_")[0][1:]) in OPENPOSE_INTERACTIONS:
            continue
        joints2d = np.asarray(sio.loadmat(osp.join(anno_folder, name))["skeleton"], dtype=np.float64)
        if joints2d.size == 0:
            bad.append(name)
            continue
        if not np.logical_and.reduce((joints2d[:, :, :, 2] > 0).sum(-1) > OPENPOSE_MIN_CREDIBLE, axis=-1).sum():
            bad.append(name)
            continue
        seqlen = joints2d.shape[1]
        valid = np.logical_and.reduce(np.logical_or.reduce(joints2d[:, :, 2] > OPENPOSE_MAX_THRESH, axis=-1), axis=-1)
        if valid.sum() == 0:
            bad.append(name)
            continue
        joints2d = joints2d[valid].reshape(-1, seqlen, 25, 3)
        mask = np.array([True]).astype(bool)
        if joints2d.shape[0] > 1:
            scores = joints2d[:, :, :, 2].mean(-1).mean(-1)
            mask = (scores.max() - scores) < OPENPOSE_MIN_SDIFF
        j2ds = joints2d[mask].reshape(-1, seqlen, 25, 3)
        j2ds[:, :, :, 0] *= img_w
        j2ds[:, :, :, 1] *= img_h
        cands.append((name.split(".")[0], list(j2ds)))
    flat = [j for _, js in cands for j in js]
    if model is None or not flat:
        rows = [bbox_from_joints2d(j)[0] for j in flat]
    else:
        rows = list(model.bbox_from_joints2d(np.concatenate(flat, 0), lengths=[j.shape[0] for j in flat]).cpu().numpy())
    k = 0
    winners = {}
    for vid_name, js in cands:
        area, chosen, winner = 0, None, None
        for j in js:
            if rows[k][2] > area:
                area, chosen, winner = rows[k][2], np.repeat(rows[k][None, :], j.shape[0], axis=0), j
            k += 1
        boxes[vid_name] = chosen
        winners[vid_name] = winner
    tracks = {}
    if track is not None:
        names = [v for v, _ in cands if winners[v] is not None]
        for v, _ in cands:
            if winners[v] is None:
                boxes[v], tracks[v] = None, None
        if names:
            kw = dict(lengths=[winners[v].shape[0] for v in names], vis_thresh=track.get("vis_thresh", 0.3), kernel_size=track.get("kernel_size", 1),
                      sigma=track.get("sigma", 0.0), pad=track.get("pad", "zero"))
            joints = np.concatenate([winners[v] for v in names], 0)
            if model is None:
                out = track_boxes(joints, **kw)
            else:
                out = {k: t.cpu().numpy() for k, t in model.track_boxes(joints, **kw).items()}
            a = 0
            for v, (start, end) in zip(names, out["range"]):
                T = winners[v].shape[0]
                if start < 0:
                    boxes[v] = winners[v] = tracks[v] = None
                else:
                    boxes[v] = out["boxes"][a + start:a + end].copy()
                    tracks[v] = {"range": (int(start), int(end)), "frames": T, "status": out["status"][a + start:a + end].astype(np.uint8)}
                    winners[v] = winners[v][start:end]
                a += T
    result = (boxes, bad) + ((winners,) if return_joints else ()) + ((tracks,) if track is not None else ())
    return result


def _sequence_lengths(n, lengths):
    """The lengths of the sequences that cut n frames lying back to back, as a list (None: one sequence of them all); each has at least one frame."""
    lengths = [n] if lengths is None else [int(v) for v in lengths]
    if sum(lengths) != n or min(lengths) < 1:
        raise ValueError(f"lengths {lengths if len(lengths) < 8 else len(lengths)} do not cut {n} frames into sequences of at least one frame")
    return lengths


def _widened(x, what, finite=False):
    """x (n,K,3) with n, K >= 1 as the device takes it: rounded to float32, then widened to float64.  finite: ValueError on a NaN or an infinity."""
    a = np.asarray(x)
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"{what} must be (n,K,3) with n, K >= 1, got {a.shape}")
    if finite and not np.isfinite(a).all():
        raise ValueError(f"{what} has a non-finite entry")
    return a.astype(np.float32).astype(np.float64)


def pose_metrics(pred_joints, gt_joints, lengths=None, root=None, select=None, pred_verts=None, gt_verts=None, unit=1000.0, return_transform=False):
    """MPJPE, PA-MPJPE, PVE, acceleration and acceleration error in numpy float64 with np.linalg.svd: the host statement of
    GRNet.pose_metrics, same arguments, a dict of numpy arrays.  The inputs are taken as float32 and widened, as the device takes them.
    per_frame (n,5) = [mpjpe, pa_mpjpe, pve, accel, accel_err] times unit, NaN where undefined by structure; per_sequence (n_seq,5) and
    total (5,): means over the defined entries (the total from the sequences' sums and counts); transform (n,13) = [s, R row-major, t]."""
    p, g = _widened(pred_joints, "pred_joints", finite=True), _widened(gt_joints, "gt_joints", finite=True)
    if p.shape != g.shape:
        raise ValueError(f"pred_joints and gt_joints differ in shape: {p.shape}, {g.shape}")
    if (pred_verts is None) != (gt_verts is None):
        raise ValueError("pred_verts and gt_verts go together")
    n, J = p.shape[:2]
    lengths = _sequence_lengths(n, lengths)
    sel = np.arange(J) if select is None else np.asarray(select, np.int64).reshape(-1)
    rt = np.zeros(0, np.int64) if root is None else np.asarray(root, np.int64).reshape(-1)
    for idx, what in ((sel, "select"), (rt, "root")):
        if idx.size > 64 or (what == "select" and idx.size < 1) or (idx.size and (idx.min() < 0 or idx.max() >= J)):
            raise ValueError(f"{what} must hold at most 64 indices into the {J} joints")
    if J > 64:
        raise ValueError(f"J {J} > 64")
    if not np.isfinite(unit):
        raise ValueError("unit must be finite")
    if rt.size:
        p = p - p[:, rt].mean(axis=1, keepdims=True)
        g = g - g[:, rt].mean(axis=1, keepdims=True)
    P, G = p[:, sel], g[:, sel]
    per_frame = np.full((n, 5), np.nan)
    per_frame[:, 0] = np.linalg.norm(P - G, axis=2).mean(axis=1)
    mu1, mu2 = P.mean(axis=1, keepdims=True), G.mean(axis=1, keepdims=True)
    X1, X2 = P - mu1, G - mu2
    var1 = (X1 ** 2).sum(axis=(1, 2))
    K = np.einsum("nja,njb->nab", X1, X2)
    U, S, Vt = np.linalg.svd(K)
    d = np.sign(np.linalg.det(np.einsum("nab,nbc->nac", U, Vt)))
    d[d == 0] = 1.0
    Z = np.tile(np.eye(3), (n, 1, 1))
    Z[:, 2, 2] = d
    R = np.einsum("nba,nbc,ndc->nad", Vt, Z, U)                 # V Z U^T
    degenerate = var1 == 0                                     # all selected pred joints equal: s = 0, R = I
    R[degenerate] = np.eye(3)
    s = np.where(degenerate, 0.0, np.einsum("nab,nba->n", R, K) / np.where(degenerate, 1.0, var1))
    t = mu2[:, 0] - s[:, None] * np.einsum("nab,nb->na", R, mu1[:, 0])
    aligned = s[:, None, None] * np.einsum("nab,njb->nja", R, P) + t[:, None, :]
    per_frame[:, 1] = np.linalg.norm(aligned - G, axis=2).mean(axis=1)
    if pred_verts is not None:
        pv, gv = _widened(pred_verts, "pred_verts", finite=True), _widened(gt_verts, "gt_verts", finite=True)
        if pv.shape != gv.shape or pv.shape[0] != n:
            raise ValueError(f"pred_verts and gt_verts must both be ({n},V,3), got {pv.shape} and {gv.shape}")
        per_frame[:, 2] = np.linalg.norm(pv - gv, axis=2).mean(axis=1)
    sums, counts = np.zeros((len(lengths), 5)), np.zeros((len(lengths), 5), np.int64)
    a = 0
    for q, T in enumerate(lengths):
        if T >= 3:
            acc = P[a:a + T - 2] - 2.0 * P[a + 1:a + T - 1] + P[a + 2:a + T]
            E = P[a:a + T] - G[a:a + T]
            err = E[:-2] - 2.0 * E[1:-1] + E[2:]
            per_frame[a + 1:a + T - 1, 3] = np.linalg.norm(acc, axis=2).mean(axis=1)
            per_frame[a + 1:a + T - 1, 4] = np.linalg.norm(err, axis=2).mean(axis=1)
        a += T
    per_frame *= float(unit)
    a = 0
    for q, T in enumerate(lengths):
        rows = per_frame[a:a + T]
        defined = ~np.isnan(rows)                              # NaN here is structural: the input is finite
        counts[q] = defined.sum(axis=0)
        sums[q] = np.where(defined, rows, 0.0).sum(axis=0)
        a += T
    with np.errstate(invalid="ignore", divide="ignore"):
        per_seq = np.where(counts > 0, sums / np.maximum(counts, 1), np.nan)
        total = np.where(counts.sum(axis=0) > 0, sums.sum(axis=0) / np.maximum(counts.sum(axis=0), 1), np.nan)
    out = {"per_frame": per_frame, "per_sequence": per_seq, "total": total}
    if return_transform:
        out["transform"] = np.concatenate([s[:, None], R.reshape(n, 9), t], axis=1)
    return out


# ----------------------------------------------------------------------------- the camera-space trajectory
# (kinectv2 index, BODY_25 index) of the joints both lists of kp_utils.py name alike; Thorax / Neck and the feet are defined differently and left out
BODY25_FROM_KINECTV2 = ((0, 8), (4, 5), (5, 6), (6, 7), (8, 2), (9, 3), (10, 4), (12, 12), (13, 13), (14, 14), (16, 9), (17, 10), (18, 11))
TRANS_FITTED, TRANS_TOO_FEW, TRANS_DEGENERATE, TRANS_FILLED = 0, 1, 2, 3


def _solve3(A, b):
    """x of the 3x3 system A x = b by elimination with partial pivoting (the first of equal pivots), one float64 rounding per operation; None at a
    zero or NaN pivot."""
    A, b = [[float(v) for v in row] for row in A], [float(v) for v in b]
    for k in range(3):
        p, best = k, abs(A[k][k])
        for r in range(k + 1, 3):
            if abs(A[r][k]) > best:
                p, best = r, abs(A[r][k])
        if not best > 0.0:
            return None
        A[k], A[p], b[k], b[p] = A[p], A[k], b[p], b[k]
        for r in range(k + 1, 3):
            m = A[r][k] / A[k][k]
            for c in range(k + 1, 3):
                A[r][c] = A[r][c] - m * A[k][c]
            b[r] = b[r] - m * b[k]
    x2 = b[2] / A[2][2]
    x1 = (b[1] - A[1][2] * x2) / A[1][1]
    x0 = ((b[0] - A[0][1] * x1) - A[0][2] * x2) / A[0][0]
    return x0, x1, x2


def fit_translation(joints3d, joints2d, pairs, lengths=None, focal_length=5000.0, centre=(112.0, 112.0), conf_threshold=0.1, min_joints=4, root=0, fill=True):
    """estimate_translation_np (lib/utils/geometry.py:296-337) per frame in numpy float64 with the statuses, the fill and the summary of DESIGN 4.9:
    the host statement of GRNet.fit_translation, same arguments, a dict of numpy arrays.  The inputs are taken as float32 and widened, as the device
    takes them.  per_frame (n,6) = [tx, ty, tz, reproj_px, n_used, status], per_sequence (n_seq,4) = [fitted, filled, mean reproj, path length]."""
    j3, j2 = _widened(joints3d, "joints3d"), _widened(joints2d, "joints2d")
    n = j3.shape[0]
    if j2.shape[0] != n:
        raise ValueError(f"joints3d has {n} frames and joints2d {j2.shape[0]}")
    lengths = _sequence_lengths(n, lengths)
    table = np.asarray(pairs, np.int64)
    if table.ndim != 2 or table.shape[1] != 2 or not 1 <= table.shape[0] <= 64:
        raise ValueError(f"pairs must be (P,2) of (3D index, 2D index) with 1 <= P <= 64, got {table.shape}")
    if table.min() < 0 or table[:, 0].max() >= j3.shape[1] or table[:, 1].max() >= j2.shape[1]:
        raise ValueError(f"a pair index lies outside the {j3.shape[1]} 3D joints or the {j2.shape[1]} 2D joints")
    n_seq = len(lengths)
    cam = np.empty((n_seq, 3), np.float64)
    try:
        cam[:, 0] = np.asarray(focal_length, np.float64)
        cam[:, 1:] = np.asarray(centre, np.float64)
    except ValueError:
        raise ValueError(f"focal_length must be one number or {n_seq} of them, centre (cx, cy) or ({n_seq},2)") from None
    if not np.isfinite(cam).all() or (cam[:, 0] <= 0).any():
        raise ValueError("focal_length must be finite and positive, centre finite")
    if not np.isfinite(conf_threshold) or conf_threshold < 0:
        raise ValueError("conf_threshold must be finite and not negative")
    if min_joints < 2:
        raise ValueError(f"min_joints {min_joints} < 2")
    if not 0 <= root < j3.shape[1]:
        raise ValueError(f"root {root} outside the {j3.shape[1]} 3D joints")
    per_frame = np.full((n, 6), np.nan)
    per_seq = np.zeros((n_seq, 4))
    a = 0
    with np.errstate(all="ignore"):
        for q, T in enumerate(lengths):
            f, cx, cy = (float(v) for v in cam[q])
            rows = per_frame[a:a + T]
            for i in range(T):
                S, D = j3[a + i, table[:, 0]], j2[a + i, table[:, 1]]
                used = np.flatnonzero((D[:, 2] > conf_threshold) & np.isfinite(D[:, 2]))
                rows[i, 4], rows[i, 5] = used.size, TRANS_TOO_FEW
                if used.size < min_joints:
                    continue
                rows[i, 5] = TRANS_DEGENERATE
                sw = swu = swv = swr = sbx = sby = sbz = 0.0
                for j in used:                                   # table order, one rounding per operation
                    X, Y, Z, w = float(S[j, 0]), float(S[j, 1]), float(S[j, 2]), float(D[j, 2])
                    u, v = float(D[j, 0]) - cx, float(D[j, 1]) - cy
                    ex, ey = u * Z - f * X, v * Z - f * Y
                    sw, swu, swv, swr = sw + w, swu + w * u, swv + w * v, swr + w * (u * u + v * v)
                    sbx, sby, sbz = sbx + w * ex, sby + w * ey, sbz + w * (u * ex + v * ey)
                d0, ax, ay = (f * f) * sw, -(f * swu), -(f * swv)
                t = _solve3([[d0, 0.0, ax], [0.0, d0, ay], [ax, ay, swr]], [f * sbx, f * sby, -sbz])
                if t is None or not np.isfinite(t).all():
                    continue
                depth = S[used, 2] + t[2]
                if not (depth > 0).all():
                    continue
                px = ((f * (S[used, 0] + t[0])) / depth + cx) - D[used, 0]
                py = ((f * (S[used, 1] + t[1])) / depth + cy) - D[used, 1]
                acc = 0.0
                for e in D[used, 2] * np.sqrt(px * px + py * py):
                    acc = acc + float(e)
                if not np.isfinite(acc / sw):
                    continue
                rows[i] = (t[0], t[1], t[2], acc / sw, used.size, TRANS_FITTED)
            fitted = np.flatnonzero(rows[:, 5] == TRANS_FITTED)
            if fill and fitted.size:
                todo = rows[:, 5] != TRANS_FITTED
                rows[:fitted[0], :3], rows[fitted[-1] + 1:, :3] = rows[fitted[0], :3], rows[fitted[-1], :3]
                for lo, hi in zip(fitted[:-1], fitted[1:]):
                    if hi - lo > 1:
                        rows[lo + 1:hi, :3] = np.linspace(rows[lo, :3], rows[hi, :3], hi - lo + 1)[1:-1]
                rows[todo, 3], rows[todo, 5] = np.nan, TRANS_FILLED
            pos = j3[a:a + T, root] + rows[:, :3]
            steps = np.sqrt((np.diff(pos, axis=0) ** 2).sum(axis=1))
            path = 0.0
            for s in steps[np.isfinite(steps)]:                  # a step is finite exactly where both t are
                path = path + float(s)
            acc = 0.0
            for e in rows[fitted, 3]:
                acc = acc + float(e)
            per_seq[q] = (fitted.size, (rows[:, 5] == TRANS_FILLED).sum(), acc / fitted.size if fitted.size else np.nan, path)
            a += T
    return {"per_frame": per_frame, "per_sequence": per_seq}


# ----------------------------------------------------------------------------- per-frame boxes from 2D joints
TRACK_DETECTED, TRACK_INTERPOLATED, TRACK_OUTSIDE, TRACK_BAD_SCALE = 0, 1, 2, 3
TRACK_MIN_HEIGHT, TRACK_PERSON_PIXELS = 0.5, 150.0             # lib/utils/smooth_bbox.py:60,64


def track_reflect(j, n):
    """Index into [0, n) of position j of scipy.ndimage's mode 'reflect' (d c b a | a b c d | d c b a): period 2n, any integer j (arrays too)."""
    m = np.mod(j, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def median_filter1d(x, kernel_size=11, pad="zero"):
    """scipy.signal.medfilt(x, kernel_size) of a float64 column by sorting every window; pad 'zero' (scipy's) or 'edge' (the first / last value)."""
    x = np.asarray(x, np.float64)
    if x.ndim != 1 or x.size < 1:
        raise ValueError(f"x must be (n,) with n >= 1, got {x.shape}")
    if kernel_size < 1 or kernel_size > 31 or kernel_size % 2 == 0:
        raise ValueError(f"kernel_size {kernel_size} must be odd and within [1, 31]")
    if pad not in ("zero", "edge"):
        raise ValueError(f"pad must be 'zero' or 'edge', got {pad!r}")
    half = kernel_size // 2
    ext = np.pad(x, half, mode="constant" if pad == "zero" else "edge")
    windows = np.lib.stride_tricks.sliding_window_view(ext, kernel_size)
    return np.sort(windows, axis=1)[:, half].copy()


def gauss_weights(sigma):
    """The 2r + 1 weights of scipy.ndimage.gaussian_filter1d(sigma) with its defaults (order 0, truncate 4): r = int(4 sigma + 0.5)."""
    r = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def gauss_filter1d(x, sigma=3.0):
    """scipy.ndimage.gaussian_filter1d(x, sigma) of a float64 column: np.dot of the weights against the reflected extension, however short x is."""
    x = np.asarray(x, np.float64)
    if x.ndim != 1 or x.size < 1:
        raise ValueError(f"x must be (n,) with n >= 1, got {x.shape}")
    if not np.isfinite(sigma) or not 0 < sigma <= 16:
        raise ValueError("sigma must be within (0, 16]")
    w = gauss_weights(sigma)
    r, n = w.size // 2, x.size
    ext = x[track_reflect(np.arange(-r, n + r), n)]
    return np.array([np.dot(ext[l:l + 2 * r + 1], w) for l in range(n)])


_GAIT_JOINT_NAMES = "pelvis, spine-shoulder, left / right hip, ankle, foot"
_KIN_JOINT_NAMES = "pelvis, spine-shoulder, left / right hip, knee, ankle, foot, shoulder, elbow, wrist"


def _joint_table(joints, count, J, names):
    """The `count` joint indices of a gait statement as int64, each within [0, J); `names` says in the message which joints they are."""
    tab = np.asarray(joints, np.int64).reshape(-1)
    if tab.size != count or tab.min() < 0 or tab.max() >= J:
        raise ValueError(f"joints must be {count} indices into the {J} joints ({names})")
    return tab


def _sigma_check(sigma):
    if not np.isfinite(sigma) or not 0 <= sigma <= 16:
        raise ValueError("sigma must be 0 (no Gaussian) or within (0, 16]")


def track_boxes(joints2d, lengths=None, vis_thresh=0.3, kernel_size=1, sigma=0.0, pad="zero", return_params=False):
    """One box per frame from 2D joints in numpy float64: the reference's lib/utils/smooth_bbox.py (kp_to_bbox_param squared=True,
    get_all_bbox_params, smooth_bbox_params) and the box of lib/dataset/inference.py:57-66 -- the host statement of GRNet.track_boxes, same
    arguments, a dict of numpy arrays (the rules: DESIGN 4.10).  Per frame: min and max of x and y over the joints with score > vis_thresh,
    height = sqrt(dx^2 + dy^2), a detection where height >= 0.5 (and everything is finite), centre = (min + max) / 2, scale = 150 / height.
    Per sequence: [start, end) from the first to the last detection, np.linspace across the frames without one, then per column the median
    (kernel_size > 1) and the Gaussian (sigma > 0) over [start, end), and box = [cx, cy, 150 / scale, 150 / scale].  boxes (n,4); status (n,)
    int32: 0 detected, 1 interpolated, 2 outside [start, end), 3 no positive finite smoothed scale (2 and 3: zeros); range (n_seq,2) int32,
    [-1, 0) without any detection.  return_params: also params (n,3) = the smoothed [cx, cy, scale], zeros outside [start, end)."""
    kp = np.asarray(joints2d, np.float64)
    if kp.ndim != 3 or kp.shape[2] != 3 or kp.shape[0] < 1 or not 1 <= kp.shape[1] <= 64:
        raise ValueError(f"joints2d must be (T,K,3) with T >= 1 and 1 <= K <= 64, got {kp.shape}")
    n = kp.shape[0]
    lengths = _sequence_lengths(n, lengths)
    if not np.isfinite(vis_thresh):
        raise ValueError("vis_thresh must be finite")
    if kernel_size < 1 or kernel_size > 31 or kernel_size % 2 == 0:
        raise ValueError(f"kernel_size {kernel_size} must be odd and within [1, 31]")
    _sigma_check(sigma)
    if pad not in ("zero", "edge"):
        raise ValueError(f"pad must be 'zero' or 'edge', got {pad!r}")
    boxes, status = np.zeros((n, 4)), np.full(n, TRACK_OUTSIDE, np.int32)
    params, rng = np.zeros((n, 3)), np.empty((len(lengths), 2), np.int32)
    a = 0
    with np.errstate(all="ignore"):
        for q, T in enumerate(lengths):
            rows = np.zeros((T, 3))
            detected = np.zeros(T, bool)
            for i in range(T):
                vis = kp[a + i, :, 2] > vis_thresh
                if not vis.any():
                    continue
                lo, hi = kp[a + i, vis, :2].min(axis=0), kp[a + i, vis, :2].max(axis=0)
                d = hi - lo
                height = np.sqrt(d[0] * d[0] + d[1] * d[1])
                if not (np.isfinite(kp[a + i, vis, :2]).all() and height >= TRACK_MIN_HEIGHT and np.isfinite(height)):
                    continue
                rows[i, :2], rows[i, 2] = (lo + hi) / 2.0, TRACK_PERSON_PIXELS / height
                detected[i] = True
            found = np.flatnonzero(detected)
            if not found.size:
                rng[q] = (-1, 0)
                a += T
                continue
            start, end = int(found[0]), int(found[-1]) + 1
            rng[q] = (start, end)
            for lo, hi in zip(found[:-1], found[1:]):
                if hi - lo > 1:                                  # column by column, on scalars, as the reference calls np.linspace
                    for c in range(3):
                        rows[lo + 1:hi, c] = np.linspace(rows[lo, c], rows[hi, c], hi - lo + 1)[1:-1]
            cols = rows[start:end].copy()
            for c in range(3):
                if kernel_size > 1:
                    cols[:, c] = median_filter1d(cols[:, c], kernel_size, pad)
                if sigma > 0:
                    cols[:, c] = gauss_filter1d(cols[:, c], sigma)
            good = (cols[:, 2] > 0) & np.isfinite(cols[:, 2])
            side = TRACK_PERSON_PIXELS / np.where(good, cols[:, 2], 1.0)
            inside = np.stack([cols[:, 0], cols[:, 1], side, side], axis=1)
            boxes[a + start:a + end] = np.where(good[:, None], inside, 0.0)
            status[a + start:a + end] = np.where(good, np.where(detected[start:end], TRACK_DETECTED, TRACK_INTERPOLATED), TRACK_BAD_SCALE)
            params[a + start:a + end] = cols
            a += T
    out = {"boxes": boxes, "status": status, "range": rng}
    if return_params:
        out["params"] = params
    return out


# ----------------------------------------------------------------------------- gait events and parameters from the 3D joints
# GAIT_JOINTS_KINECTV2 (imported above) = (0, 20, 12, 16, 14, 18, 15, 19): pelvis, spine-shoulder, left hip, right hip, left ankle, right ankle, left foot, right foot
GAIT_HEEL_L, GAIT_HEEL_R, GAIT_TOE_L, GAIT_TOE_R = 1, 2, 4, 8   # the bits of an events entry
GAIT_COLUMNS = ("heel_strikes_left", "heel_strikes_right", "toe_offs_left", "toe_offs_right", "steps", "step_time_mean", "step_time_sd", "cadence",
                "stride_time_mean", "stride_time_sd", "stride_time_cv", "step_length_mean", "step_length_sd", "step_width_mean", "step_width_sd",
                "stance_share", "speed", "trajectory_speed")


def gait_events(signals, window=5, min_excursion=0.05):
    """The events rule of DESIGN 4.11 on ONE sequence: signals (T,4) float64 [hL, hR, tL, tR] -> (T,) int32.  Frame t with all of
    [t - window, t + window] inside: a heel strike where h(t) > 0, h(t) > every earlier and >= every later value of the window, and h(t) - the
    window's minimum >= min_excursion; a toe-off where t(t) < 0, < before, <= after, and the window's maximum - t(t) >= min_excursion.  Every test
    is a comparison, false for NaN."""
    s = np.asarray(signals, np.float64)
    if s.ndim != 2 or s.shape[1] != 4 or s.shape[0] < 1:
        raise ValueError(f"signals must be (T,4) with T >= 1, got {s.shape}")
    T, w = s.shape[0], int(window)
    ev = np.zeros(T, np.int32)
    if T < 2 * w + 1:
        return ev
    with np.errstate(invalid="ignore"):
        for k in range(4):
            x = s[:, k] if k < 2 else -s[:, k]                 # a toe-off is a heel strike of the negated signal: negation is exact
            win = np.lib.stride_tricks.sliding_window_view(x, 2 * w + 1)     # row i: frames i .. i + 2w, its centre t = i + w
            v = win[:, w]
            hit = (v > 0) & (v[:, None] > win[:, :w]).all(axis=1) & (v[:, None] >= win[:, w + 1:]).all(axis=1) & (v - win.min(axis=1) >= min_excursion)
            ev[w:T - w] |= np.where(hit, 1 << k, 0).astype(np.int32)
    return ev


def _gait_sum(values):
    """The sum in the order given, one rounding per addition (np.sum adds pairwise)."""
    return float(np.cumsum(np.asarray(values, np.float64))[-1])


def _gait_mean_sd(values):
    """(S / n, sqrt(sum((x - mean)^2) / n)) with both sums in the order given; (nan, nan) of nothing."""
    x = np.asarray(values, np.float64)
    if x.size == 0:
        return np.nan, np.nan
    mean = _gait_sum(x) / x.size
    d = x - mean
    return mean, float(np.sqrt(_gait_sum(d * d) / x.size))


def gait_parameters(joints3d, lengths=None, trans=None, fps=20.0, sigma=2.0, window=5, min_excursion=0.05, joints=GAIT_JOINTS_KINECTV2):
    """Heel strikes, toe-offs and gait parameters from 3D joints in numpy float64 (the coordinate-based events of Zeni, Richards and Higginson 2008;
    the rules: DESIGN 4.11): the host statement of GRNet.gait_parameters, same arguments, a dict of numpy arrays -- the same operations in the same
    order, every sum a cumulative sum.  joints3d (n,J,3) in the camera frame of the SMPL stage (x right, y down, z away), taken as float32 and
    widened; joints: the indices of pelvis, spine-shoulder, left hip, right hip, left ankle, right ankle, left foot, right foot; trans (n,3) float64
    or None.  per_frame (n,7) = [hL, hR, tL, tR (as smoothed), wd, step_length, step_width]; events (n,) int32 (GAIT_HEEL_L, GAIT_HEEL_R,
    GAIT_TOE_L, GAIT_TOE_R); per_sequence (n_seq,18), columns GAIT_COLUMNS."""
    j3 = _widened(joints3d, "joints3d")
    n, J = j3.shape[:2]
    lengths = _sequence_lengths(n, lengths)
    tab = _joint_table(joints, 8, J, _GAIT_JOINT_NAMES)
    if not np.isfinite(fps) or not fps > 0:
        raise ValueError("fps must be positive and finite")
    _sigma_check(sigma)
    if not 1 <= int(window) <= 32 or int(window) != window:
        raise ValueError(f"window {window} outside [1, 32]")
    if not np.isfinite(min_excursion) or min_excursion < 0:
        raise ValueError("min_excursion must be finite and not negative")
    tr = None
    if trans is not None:
        tr = np.asarray(trans, np.float64)
        if tr.shape != (n, 3):
            raise ValueError(f"trans must be ({n},3), got {tr.shape}")
    fps, w = float(fps), int(window)

    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    pelvis, spine, lhip, rhip, lank, rank_, lfoot, rfoot = (j3[:, i] for i in tab)
    per_frame = np.full((n, 7), np.nan)
    with np.errstate(all="ignore"):
        l, u = lhip - rhip, spine - pelvis
        c = np.stack([l[:, 1] * u[:, 2] - l[:, 2] * u[:, 1], l[:, 2] * u[:, 0] - l[:, 0] * u[:, 2], l[:, 0] * u[:, 1] - l[:, 1] * u[:, 0]], axis=1)
        nc, nl = np.sqrt(dot(c, c)), np.sqrt(dot(l, l))
        valid = (nc > 0) & np.isfinite(nc) & (nl > 0) & np.isfinite(nl)
        f, side = c / nc[:, None], l / nl[:, None]
        for k, joint in enumerate((lank, rank_, lfoot, rfoot)):
            per_frame[:, k] = np.where(valid, dot(joint - pelvis, f), np.nan)
        per_frame[:, 4] = np.where(valid, np.abs(dot(lank - rank_, side)), np.nan)
    events = np.zeros(n, np.int32)
    per_seq = np.full((len(lengths), 18), np.nan)
    a = 0
    with np.errstate(all="ignore"):
        for q, T in enumerate(lengths):
            rows = per_frame[a:a + T]
            if sigma > 0:
                for k in range(4):
                    rows[:, k] = gauss_filter1d(rows[:, k].copy(), sigma)
            ev = events[a:a + T]
            ev[:] = gait_events(rows[:, :4], w, min_excursion)
            heel = [np.flatnonzero(ev & GAIT_HEEL_L), np.flatnonzero(ev & GAIT_HEEL_R)]
            toe = [np.flatnonzero(ev & GAIT_TOE_L), np.flatnonzero(ev & GAIT_TOE_R)]
            for foot in (1, 0):                                  # the left foot's values where both strike in one frame
                rows[heel[foot], 5] = rows[heel[foot], foot] - rows[heel[foot], 1 - foot]
                rows[heel[foot], 6] = rows[heel[foot], 4]
            out = per_seq[q]
            out[:4] = heel[0].size, heel[1].size, toe[0].size, toe[1].size
            strikes = sorted([(int(t), 0) for t in heel[0]] + [(int(t), 1) for t in heel[1]])      # time order, the left foot first within a frame
            steps = [(t1, t2, f2) for (t1, f1), (t2, f2) in zip(strikes[:-1], strikes[1:]) if f1 != f2]
            out[4] = len(steps)
            if steps:
                out[5], out[6] = _gait_mean_sd([float(t2 - t1) / fps for t1, t2, _ in steps])
                out[7] = 60.0 / out[5]
                out[11], out[12] = _gait_mean_sd([rows[t2, f2] - rows[t2, 1 - f2] for _, t2, f2 in steps])
                out[13], out[14] = _gait_mean_sd([rows[t2, 4] for _, t2, _ in steps])
                out[16] = (out[11] * out[7]) / 60.0
            strides = [(int(t1), int(t2), foot) for foot in (0, 1) for t1, t2 in zip(heel[foot][:-1], heel[foot][1:])]     # the left foot's first
            if strides:
                out[8], out[9] = _gait_mean_sd([float(t2 - t1) / fps for t1, t2, _ in strides])
                out[10] = (100.0 * out[9]) / out[8]
            stance = []
            for t1, t2, foot in strides:
                off = toe[foot][(toe[foot] > t1) & (toe[foot] < t2)]
                if off.size:
                    stance.append((100.0 * float(off[0] - t1)) / float(t2 - t1))
            if stance:
                out[15] = _gait_sum(stance) / len(stance)
            if tr is not None:
                seen = [t for t, _ in strikes if np.isfinite(tr[a + t]).all()]
                if seen and seen[0] != seen[-1]:
                    ta, tb = seen[0], seen[-1]
                    d = (pelvis[a + tb] + tr[a + tb]) - (pelvis[a + ta] + tr[a + ta])
                    out[17] = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) / (float(tb - ta) / fps)
            a += T
    return {"per_frame": per_frame, "events": events, "per_sequence": per_seq}


# ----------------------------------------------------------------------------- joint-angle kinematics per gait cycle
# KINEMATICS_JOINTS_KINECTV2 (imported above) = (0, 20, 12, 16, 13, 17, 14, 18, 15, 19, 4, 8, 5, 9, 6, 10): pelvis, spine-shoulder, then left and right
# hip, knee, ankle, foot, shoulder, elbow, wrist
KINEMATICS_CHANNELS = ("hip_flexion_left", "hip_flexion_right", "hip_abduction_left", "hip_abduction_right", "knee_flexion_left", "knee_flexion_right",
                       "ankle_dorsiflexion_left", "ankle_dorsiflexion_right", "shoulder_flexion_left", "shoulder_flexion_right", "elbow_flexion_left",
                       "elbow_flexion_right", "trunk_inclination")
KINEMATICS_COLUMNS = ("strides", "max_mean", "min_mean", "rom_mean", "rom_sd", "symmetry_index")
KINEMATICS_POINTS = 101
KINEMATICS_DEGREES = 57.29577951308232
_KIN_ATAN_COEFFS = tuple((-1.0 if k % 2 else 1.0) * (1.0 / (2 * k + 1)) for k in range(12))       # 1, -1/3, 1/5, ... -1/23


def gait_atan2(y, x):
    """atan2 out of + - * / and sqrt alone, elementwise in float64 (csrc/gait_angles.h states the same operations in the same order, so the kernels
    give the same bits): t = min(|y|, |x|) / max(|y|, |x|); twice t <- t / (1 + sqrt(1 + t t)); the 12 terms of atan's Taylor series by Horner; times
    4; then pi / 2 - a where |y| > |x|, pi - a where x < 0, -a where y < 0.  NaN where both arguments are zero or either is not finite."""
    y, x = np.broadcast_arrays(np.asarray(y, np.float64), np.asarray(x, np.float64))
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(y) | ~np.isfinite(x) | ((y == 0) & (x == 0))
        ay, ax = np.abs(y), np.abs(x)
        steep = ay > ax
        t = np.where(steep, ax, ay) / np.where(bad, 1.0, np.where(steep, ay, ax))
        t = t / (1.0 + np.sqrt(1.0 + t * t))
        t = t / (1.0 + np.sqrt(1.0 + t * t))
        z = t * t
        p = np.full(z.shape, _KIN_ATAN_COEFFS[11])
        for c in _KIN_ATAN_COEFFS[10::-1]:
            p = p * z + c
        a = 4.0 * (t * p)
        a = np.where(steep, 1.5707963267948966 - a, a)
        a = np.where(x < 0, 3.141592653589793 - a, a)
        a = np.where(y < 0, -a, a) + 0.0
        return np.where(bad, np.nan, a)


def _kin_dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _kin_cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _kin_bend(a, b):
    """The angle between the rows of a and b in degrees: atan2(|a x b|, a . b)."""
    c = _kin_cross(a, b)
    return gait_atan2(np.sqrt(_kin_dot(c, c)), _kin_dot(a, b)) * KINEMATICS_DEGREES


def _kin_sum(values):
    """The sum along axis 0 in the order given from +0.0, one rounding per addition."""
    v = np.asarray(values, np.float64)
    return np.cumsum(np.concatenate([np.zeros((1,) + v.shape[1:]), v]), axis=0)[-1]


def _kin_strides_check(min_stride, max_stride):
    if int(min_stride) != min_stride or int(max_stride) != max_stride:
        raise ValueError("min_stride and max_stride must be whole numbers of frames")
    if min_stride < 1:
        raise ValueError(f"min_stride {min_stride} < 1")
    if max_stride < min_stride or max_stride > 4096:
        raise ValueError(f"max_stride {max_stride} outside [min_stride, 4096]")
    return int(min_stride), int(max_stride)


def gait_cycles(angles, events, lengths=None, min_stride=8, max_stride=60):
    """Rules 5 to 7 of DESIGN 4.12 on given angle columns: the host statement of GRNet.op_gait_cycles.  angles (n,13) float64, events (n,) with the
    bits of gait_parameters; a stride of a channel's foot -- two consecutive heel strikes t0 < t1 -- is used where min_stride <= t1 - t0 <=
    max_stride and the channel is finite on all of [t0, t1].  Returns {'curves': (n_seq,13,101,2) mean and SD of every cycle point over the used
    strides, 'per_sequence': (n_seq,13,6), columns KINEMATICS_COLUMNS}."""
    x = np.asarray(angles, np.float64)
    if x.ndim != 2 or x.shape[1] != 13 or x.shape[0] < 1:
        raise ValueError(f"angles must be (n,13) with n >= 1, got {x.shape}")
    n = x.shape[0]
    ev = np.asarray(events)
    if ev.shape != (n,):
        raise ValueError(f"events must be ({n},), got {ev.shape}")
    ev = ev.astype(np.int64)
    lengths = _sequence_lengths(n, lengths)
    lo, hi = _kin_strides_check(min_stride, max_stride)
    curves = np.full((len(lengths), 13, KINEMATICS_POINTS, 2), np.nan)
    rows = np.full((len(lengths), 13, 6), np.nan)
    points = np.arange(KINEMATICS_POINTS)
    a = 0
    with np.errstate(all="ignore"):
        for q, T in enumerate(lengths):
            heel = [np.flatnonzero(ev[a:a + T] & GAIT_HEEL_L), np.flatnonzero(ev[a:a + T] & GAIT_HEEL_R)]
            for c in range(13):
                col = x[a:a + T, c]
                hs = heel[0 if c == 12 else c & 1]
                used = [(int(t0), int(t1 - t0)) for t0, t1 in zip(hs[:-1], hs[1:]) if lo <= t1 - t0 <= hi and np.isfinite(col[t0:t1 + 1]).all()]
                k = len(used)
                rows[q, c, 0] = k
                if not k:
                    continue
                top = np.array([col[t0:t0 + L + 1].max() for t0, L in used]) + 0.0         # a zero has the sign +, whatever order the maximum took
                low = np.array([col[t0:t0 + L + 1].min() for t0, L in used]) + 0.0
                rom = top - low
                pts = np.empty((k, KINEMATICS_POINTS))
                for i, (t0, L) in enumerate(used):
                    at, r = t0 + (points * L) // 100, (points * L) % 100
                    v = col[at]
                    pts[i] = np.where(r == 0, v, v + (col[np.minimum(at + 1, t0 + L)] - v) * (r / 100.0))
                mean = _kin_sum(pts) / k
                d = pts - mean
                curves[q, c, :, 0], curves[q, c, :, 1] = mean, np.sqrt(_kin_sum(d * d) / k)
                m_rom = _kin_sum(rom) / k
                e = rom - m_rom
                rows[q, c, 1:5] = _kin_sum(top) / k, _kin_sum(low) / k, m_rom, np.sqrt(_kin_sum(e * e) / k)
            for c in range(0, 12, 2):
                l, r = rows[q, c], rows[q, c + 1]
                den = 0.5 * (l[3] + r[3])
                if l[0] > 0 and r[0] > 0 and den > 0:
                    rows[q, c, 5] = rows[q, c + 1, 5] = (100.0 * abs(l[3] - r[3])) / den
            a += T
    return {"curves": curves, "per_sequence": rows}


def gait_kinematics(joints3d, events, lengths=None, sigma=2.0, min_stride=8, max_stride=60, joints=KINEMATICS_JOINTS_KINECTV2):
    """Joint angles over time and per gait cycle from 3D joints in numpy float64 (the rules: DESIGN 4.12): the host statement of
    GRNet.gait_kinematics, same arguments, a dict of numpy arrays -- the same operations in the same order, every sum a cumulative sum.  joints3d
    (n,J,3) in the camera frame of the SMPL stage (x right, y down, z away), taken as float32 and widened; events (n,): what gait_parameters
    returned; joints: the 16 indices of pelvis, spine-shoulder, then left and right hip, knee, ankle, foot, shoulder, elbow, wrist.  per_frame
    (n,13): the channels KINEMATICS_CHANNELS in degrees, as smoothed; curves (n_seq,13,101,2); per_sequence (n_seq,13,6), columns
    KINEMATICS_COLUMNS.  Channel 12, the trunk's inclination, is measured from the camera's vertical: it assumes a level camera."""
    j3 = _widened(joints3d, "joints3d")
    n, J = j3.shape[:2]
    lengths = _sequence_lengths(n, lengths)
    tab = _joint_table(joints, 16, J, _KIN_JOINT_NAMES)
    _sigma_check(sigma)
    _kin_strides_check(min_stride, max_stride)
    if np.asarray(events).shape != (n,):
        raise ValueError(f"events must be ({n},), got {np.asarray(events).shape}")
    p = [j3[:, i] for i in tab]
    per_frame = np.full((n, 13), np.nan)
    with np.errstate(all="ignore"):
        l, u = p[2] - p[3], p[1] - p[0]
        c = _kin_cross(l, u)
        nc, nl = np.sqrt(_kin_dot(c, c)), np.sqrt(_kin_dot(l, l))
        valid = (nc > 0) & np.isfinite(nc) & (nl > 0) & np.isfinite(nl)
        f, side = c / np.where(valid, nc, 1.0)[:, None], l / np.where(valid, nl, 1.0)[:, None]
        w = _kin_cross(f, side)
        for s in (0, 1):
            d, sh, g = p[4 + s] - p[2 + s], p[6 + s] - p[4 + s], p[8 + s] - p[6 + s]
            arm, fore = p[12 + s] - p[10 + s], p[14 + s] - p[12 + s]
            down, out_d = -_kin_dot(d, w), _kin_dot(d, side)
            per_frame[:, 0 + s] = np.where(valid, gait_atan2(_kin_dot(d, f), down) * KINEMATICS_DEGREES, np.nan)
            per_frame[:, 2 + s] = np.where(valid, gait_atan2(-out_d if s else out_d, down) * KINEMATICS_DEGREES, np.nan)
            per_frame[:, 4 + s] = _kin_bend(d, sh)
            per_frame[:, 6 + s] = _kin_bend(sh, g) - 90.0
            per_frame[:, 8 + s] = np.where(valid, gait_atan2(_kin_dot(arm, f), -_kin_dot(arm, w)) * KINEMATICS_DEGREES, np.nan)
            per_frame[:, 10 + s] = _kin_bend(arm, fore)
        per_frame[:, 12] = np.where(valid, _kin_bend(u, np.broadcast_to(np.array([0.0, -1.0, 0.0]), u.shape)), np.nan)
        if sigma > 0:
            a = 0
            for T in lengths:
                for k in range(13):
                    per_frame[a:a + T, k] = gauss_filter1d(per_frame[a:a + T, k].copy(), sigma)
                a += T
    out = gait_cycles(per_frame, events, lengths, min_stride, max_stride)
    out["per_frame"] = per_frame
    return out


# ----------------------------------------------------------------------------- turns and straight-walking gait parameters
TURN_STRAIGHT, TURN_LEFT, TURN_RIGHT, TURN_UNKNOWN = 0, 1, 2, 3          # a frame's phase
TURN_COLUMNS = ("n_turns", "n_turns_left", "n_turns_right", "turn_frames", "unknown_frames", "straight_bouts", "straight_frames", "turn_duration_mean",
                "turn_angle_mean", "turn_peak_rate_mean", "turn_steps_mean") + tuple("straight_" + name for name in GAIT_COLUMNS[4:17])
TURN_TABLE_COLUMNS = ("first_frame", "last_frame", "direction", "angle", "duration", "peak_rate", "steps")


def _turn_rule_check(fps, edge_rate, peak_rate, min_angle, min_frames, max_frames, max_turns):
    if not np.isfinite(fps) or not fps > 0:
        raise ValueError("fps must be positive and finite")
    if not np.isfinite(edge_rate) or edge_rate < 0:
        raise ValueError("edge_rate must be finite and not negative")
    if not np.isfinite(peak_rate) or peak_rate < edge_rate:
        raise ValueError("peak_rate must be finite and not below edge_rate")
    if not np.isfinite(min_angle) or min_angle < 0:
        raise ValueError("min_angle must be finite and not negative")
    if int(min_frames) != min_frames or int(max_frames) != max_frames or int(max_turns) != max_turns:
        raise ValueError("min_frames, max_frames and max_turns must be whole numbers")
    if min_frames < 1:
        raise ValueError(f"min_frames {min_frames} < 1")
    if max_frames < min_frames:
        raise ValueError(f"max_frames {max_frames} < min_frames {min_frames}")
    if not 1 <= max_turns <= 64:
        raise ValueError(f"max_turns {max_turns} outside [1, 64]")


def _turn_runs_of(mask):
    """[(first, behind)] of the maximal runs of True in a boolean column, in time order."""
    edges = np.flatnonzero(np.diff(np.concatenate([[0], mask.astype(np.int8), [0]])))
    return [(int(a), int(b)) for a, b in zip(edges[::2], edges[1::2])]


def gait_turn_runs(rates, events, gait_rows, lengths=None, fps=20.0, edge_rate=5.0, peak_rate=15.0, min_angle=45.0, min_frames=10, max_frames=200, max_turns=8):
    """Rules 4 to 7 of DESIGN 4.13 on given rates: the host statement of GRNet.op_gait_turn_runs.  rates (n,2) float64 [yaw step in degrees, yaw rate
    in degrees a second], events (n,) and gait_rows (n,7) as gait_parameters returned them.  A maximal run of rate > edge_rate (left) or
    < -edge_rate (right) is a turn where max |rate| >= peak_rate, |sum of its steps| >= min_angle and min_frames <= its length <= max_frames.  Returns
    {'phase': (n,) int32, 'turns': (n_seq,max_turns,7), columns TURN_TABLE_COLUMNS, 'per_sequence': (n_seq,24), columns TURN_COLUMNS}; every sum in
    time order from +0.0, every comparison false for NaN."""
    x = np.asarray(rates, np.float64)
    if x.ndim != 2 or x.shape[1] != 2 or x.shape[0] < 1:
        raise ValueError(f"rates must be (n,2) with n >= 1, got {x.shape}")
    n = x.shape[0]
    ev = np.asarray(events)
    if ev.shape != (n,):
        raise ValueError(f"events must be ({n},), got {ev.shape}")
    ev = ev.astype(np.int64)
    g = np.asarray(gait_rows, np.float64)
    if g.shape != (n, 7):
        raise ValueError(f"gait_rows must be ({n},7), got {g.shape}")
    lengths = _sequence_lengths(n, lengths)
    _turn_rule_check(fps, edge_rate, peak_rate, min_angle, min_frames, max_frames, max_turns)
    fps, max_turns = float(fps), int(max_turns)
    phase = np.zeros(n, np.int32)
    turns = np.full((len(lengths), max_turns, 7), np.nan)
    per_seq = np.full((len(lengths), 24), np.nan)
    a = 0
    with np.errstate(all="ignore"):
        for q, T in enumerate(lengths):
            step, rate, e, rows, ph = x[a:a + T, 0], x[a:a + T, 1], ev[a:a + T], g[a:a + T], phase[a:a + T]
            strike = ((e & GAIT_HEEL_L) != 0).astype(np.int64) + ((e & GAIT_HEEL_R) != 0).astype(np.int64)
            ph[np.isnan(rate)] = TURN_UNKNOWN
            found = []
            for sign, mask in ((1, rate > edge_rate), (-1, rate < -edge_rate)):
                for first, behind in _turn_runs_of(mask):
                    peak = float(np.abs(rate[first:behind]).max())
                    angle = float(_kin_sum(step[first:behind]))
                    if peak >= peak_rate and abs(angle) >= min_angle and min_frames <= behind - first <= max_frames:
                        found.append([float(first), float(behind - 1), float(sign), angle, float(behind - first) / fps, peak, float(strike[first:behind].sum())])
                        ph[first:behind] = TURN_LEFT if sign > 0 else TURN_RIGHT
            found.sort()                                       # by the first frame: time order
            for i, row in enumerate(found[:max_turns]):
                turns[q, i] = row
            out = per_seq[q]
            out[0], out[1], out[2] = len(found), sum(r[2] > 0 for r in found), sum(r[2] < 0 for r in found)
            out[3], out[4] = np.count_nonzero((ph == TURN_LEFT) | (ph == TURN_RIGHT)), np.count_nonzero(ph == TURN_UNKNOWN)
            out[5], out[6] = len(_turn_runs_of(ph == TURN_STRAIGHT)), np.count_nonzero(ph == TURN_STRAIGHT)
            if found:
                for k, values in enumerate(([r[4] for r in found], [abs(r[3]) for r in found], [r[5] for r in found], [r[6] for r in found])):
                    out[7 + k] = float(_kin_sum(values)) / len(found)
            busy = np.concatenate([[0], np.cumsum(ph != TURN_STRAIGHT)])

            def straight(t1, t2):
                return busy[t2 + 1] == busy[t1]

            # columns 11 .. 23: gait_parameters' 4 .. 16 with one test more per link
            heel = [np.flatnonzero(e & GAIT_HEEL_L), np.flatnonzero(e & GAIT_HEEL_R)]
            toe = [np.flatnonzero(e & GAIT_TOE_L), np.flatnonzero(e & GAIT_TOE_R)]
            strikes = sorted([(int(t), 0) for t in heel[0]] + [(int(t), 1) for t in heel[1]])
            steps = [(t1, t2, f2) for (t1, f1), (t2, f2) in zip(strikes[:-1], strikes[1:]) if f1 != f2 and straight(t1, t2)]
            out[11] = len(steps)
            if steps:
                out[12], out[13] = _gait_mean_sd([float(t2 - t1) / fps for t1, t2, _ in steps])
                out[14] = 60.0 / out[12]
                out[18], out[19] = _gait_mean_sd([rows[t2, f2] - rows[t2, 1 - f2] for _, t2, f2 in steps])
                out[20], out[21] = _gait_mean_sd([rows[t2, 4] for _, t2, _ in steps])
                out[23] = (out[18] * out[14]) / 60.0
            strides = [(int(t1), int(t2), foot) for foot in (0, 1) for t1, t2 in zip(heel[foot][:-1], heel[foot][1:]) if straight(int(t1), int(t2))]
            if strides:
                out[15], out[16] = _gait_mean_sd([float(t2 - t1) / fps for t1, t2, _ in strides])
                out[17] = (100.0 * out[16]) / out[15]
            stance = []
            for t1, t2, foot in strides:
                off = toe[foot][(toe[foot] > t1) & (toe[foot] < t2)]
                if off.size:
                    stance.append((100.0 * float(off[0] - t1)) / float(t2 - t1))
            if stance:
                out[22] = _gait_sum(stance) / len(stance)
            a += T
    return {"phase": phase, "turns": turns, "per_sequence": per_seq}


def gait_turns(joints3d, events, gait_rows, lengths=None, fps=20.0, sigma=8.0, edge_rate=5.0, peak_rate=15.0, min_angle=45.0, min_frames=10, max_frames=200,
               max_turns=8, joints=GAIT_JOINTS_KINECTV2):
    """Turns and the gait parameters of straight walking from 3D joints in numpy float64 (the rules: DESIGN 4.13; the thresholds after El-Gohary et al.
    2014, unvalidated on the model's output): the host statement of GRNet.gait_turns, same arguments, a dict of numpy arrays -- the same operations in
    the same order.  joints3d (n,J,3) as gait_parameters takes them; events and gait_rows: its events and per_frame; joints: its table, of which
    pelvis, spine-shoulder, left hip and right hip are read.  The ground heading g = (f_x, f_z) assumes a level camera.  per_frame (n,2) = [yaw step
    in degrees, positive towards the subject's left; yaw rate in degrees a second as smoothed]; phase, turns, per_sequence: gait_turn_runs'."""
    j3 = _widened(joints3d, "joints3d")
    n, J = j3.shape[:2]
    lengths = _sequence_lengths(n, lengths)
    tab = _joint_table(joints, 8, J, _GAIT_JOINT_NAMES)
    _turn_rule_check(fps, edge_rate, peak_rate, min_angle, min_frames, max_frames, max_turns)
    _sigma_check(sigma)
    pelvis, spine, lhip, rhip = (j3[:, i] for i in tab[:4])
    per_frame = np.zeros((n, 2))
    with np.errstate(all="ignore"):
        l, u = lhip - rhip, spine - pelvis
        c = _kin_cross(l, u)
        nc, nl = np.sqrt(_kin_dot(c, c)), np.sqrt(_kin_dot(l, l))
        valid = (nc > 0) & np.isfinite(nc) & (nl > 0) & np.isfinite(nl)
        gx, gz = np.where(valid, c[:, 0] / nc, np.nan), np.where(valid, c[:, 2] / nc, np.nan)
        a = 0
        for T in lengths:
            x, z = gx[a:a + T], gz[a:a + T]
            step = per_frame[a:a + T, 0]
            step[1:] = gait_atan2(x[:-1] * z[1:] - z[:-1] * x[1:], x[:-1] * x[1:] + z[:-1] * z[1:]) * KINEMATICS_DEGREES
            raw = step * float(fps)
            per_frame[a:a + T, 1] = gauss_filter1d(raw, sigma) if sigma > 0 else raw
            a += T
    out = gait_turn_runs(per_frame, events, gait_rows, lengths, fps, edge_rate, peak_rate, min_angle, min_frames, max_frames, max_turns)
    out["per_frame"] = per_frame
    return out


# ----------------------------------------------------------------------------- foot contact phases and double support
CONTACT_MOVING, CONTACT_LEFT, CONTACT_RIGHT, CONTACT_UNATTRIBUTED, CONTACT_NAN = 0, 1, 2, 3, 4          # an interval's phase, held by its first frame
CONTACT_COLUMNS = ("threshold", "interfoot_speed_mean", "static_runs", "double_supports_left", "double_supports_right", "unattributed_runs",
                   "double_support_time_mean", "double_support_time_sd", "double_support_time_left", "double_support_time_right",
                   "double_support_asymmetry", "strides", "stride_time_mean", "stride_time_sd", "stance_time_mean", "swing_time_mean",
                   "single_support_time_mean", "stance_share_mean", "double_support_share_mean", "stride_time_cv")
CONTACT_RUN_COLUMNS = ("t_start", "t_end", "lead", "heel_strike_frame", "duration", "speed_min")


def _contact_rule_check(fps, fraction, speed, reach, max_frames, max_runs):
    if not np.isfinite(fps) or not fps > 0:
        raise ValueError("fps must be positive and finite")
    if not np.isfinite(fraction) or fraction < 0:
        raise ValueError("fraction must be finite and not negative")
    if not np.isfinite(speed) or speed < 0:
        raise ValueError("speed must be finite and not negative")
    if fraction == 0 and speed == 0:
        raise ValueError("fraction and speed are both zero: no threshold")
    if int(reach) != reach or int(max_frames) != max_frames or int(max_runs) != max_runs:
        raise ValueError("reach, max_frames and max_runs must be whole numbers")
    if not 0 <= reach <= 8:
        raise ValueError(f"reach {reach} outside [0, 8]")
    if max_frames < 1:
        raise ValueError(f"max_frames {max_frames} < 1")
    if not 1 <= max_runs <= 512:
        raise ValueError(f"max_runs {max_runs} outside [1, 512]")


def contact_tree_sum(s):
    """Rule 3's sum of the finite entries of s (n,) in its fixed shape, as reshapes: blocks of 64 consecutive entries, inside a block adjacent pairs
    (0+1, 2+3, ...), then pairs of those, a non-finite or missing entry +0.0; the block sums added in time order from +0.0 -> (S, count)."""
    s = np.asarray(s, np.float64)
    fin = np.isfinite(s)
    x = np.concatenate([np.where(fin, s, 0.0), np.zeros((-s.size) % 64)]).reshape(-1, 64)
    while x.shape[1] > 1:
        x = x[:, 0::2] + x[:, 1::2]
    return float(_kin_sum(x[:, 0])), int(np.count_nonzero(fin))


def gait_contact_runs(speeds, events, lengths=None, fps=20.0, fraction=0.25, speed=0.0, reach=2, max_frames=20, max_runs=128):
    """Rules 3 to 9 of DESIGN 4.14 on given speeds: the host statement of GRNet.op_gait_contact_runs.  speeds (n,) float64: entry k of a sequence is the
    inter-foot speed of the interval between its frames k and k + 1 (the last entry of every sequence is not read); events (n,) as gait_parameters
    returned them.  Returns {'phase': (n,) int32, 'runs': (n_seq,max_runs,6), columns CONTACT_RUN_COLUMNS, 'per_sequence': (n_seq,20), columns
    CONTACT_COLUMNS}; every sum in the stated order, every comparison false for NaN."""
    x = np.asarray(speeds, np.float64)
    if x.ndim != 1 or x.shape[0] < 1:
        raise ValueError(f"speeds must be (n,) with n >= 1, got {x.shape}")
    n = x.shape[0]
    ev = np.asarray(events)
    if ev.shape != (n,):
        raise ValueError(f"events must be ({n},), got {ev.shape}")
    ev = ev.astype(np.int64)
    lengths = _sequence_lengths(n, lengths)
    _contact_rule_check(fps, fraction, speed, reach, max_frames, max_runs)
    fps, fraction, speed, reach, max_frames, max_runs = float(fps), float(fraction), float(speed), int(reach), int(max_frames), int(max_runs)
    phase = np.zeros(n, np.int32)
    runs = np.full((len(lengths), max_runs, 6), np.nan)
    per_seq = np.full((len(lengths), 20), np.nan)
    f0 = 0
    with np.errstate(all="ignore"):
        for q, T in enumerate(lengths):
            s, e, ph = x[f0:f0 + T - 1], ev[f0:f0 + T], phase[f0:f0 + T]
            S, count = contact_tree_sum(s)
            mean = S / count if count else np.nan
            thr = speed if speed > 0 else fraction * mean
            ph[T - 1] = CONTACT_NAN
            ph[:T - 1][np.isnan(s)] = CONTACT_NAN
            heel = [np.flatnonzero(e & GAIT_HEEL_L), np.flatnonzero(e & GAIT_HEEL_R)]
            found = []                                         # (lead, t_start, t_end) of every static run in time order
            for a, behind in _turn_runs_of(s < thr):
                b = behind - 1
                closed = a >= 1 and b <= T - 3 and bool(np.isfinite(s[a - 1])) and bool(np.isfinite(s[b + 1]))
                t0 = t1 = strike = np.nan
                lead = 0
                if closed:
                    t0 = (a - 0.5) + (s[a - 1] - thr) / (s[a - 1] - s[a])
                    t1 = (b + 0.5) + (thr - s[b]) / (s[b + 1] - s[b])
                    if b - a + 1 <= max_frames:
                        lo, hi = max(a - reach, 0), min(b + 1 + reach, T - 1)
                        hit = [h[(h >= lo) & (h <= hi)] for h in heel]
                        if (hit[0].size > 0) != (hit[1].size > 0):
                            lead = 1 if hit[0].size else -1
                            strike = float(hit[0][0] if hit[0].size else hit[1][0])
                ph[a:b + 1] = CONTACT_LEFT if lead > 0 else CONTACT_RIGHT if lead < 0 else CONTACT_UNATTRIBUTED
                if len(found) < max_runs:
                    runs[q, len(found)] = [t0, t1, float(lead), strike, (t1 - t0) / fps, s[a:b + 1].min()]
                found.append((lead, t0, t1))
            out = per_seq[q]
            out[0], out[1], out[2] = thr, mean, len(found)
            out[3], out[4] = sum(r[0] > 0 for r in found), sum(r[0] < 0 for r in found)
            out[5] = out[2] - out[3] - out[4]
            support = [(lead, (t1 - t0) / fps) for lead, t0, t1 in found if lead]
            if support:
                out[6], out[7] = _gait_mean_sd([d for _, d in support])
                for col, sign in ((8, 1), (9, -1)):
                    side = [d for lead, d in support if lead == sign]
                    if side:
                        out[col] = _gait_sum(side) / len(side)
                if not np.isnan(out[8]) and not np.isnan(out[9]):
                    out[10] = (100.0 * abs(out[8] - out[9])) / (0.5 * (out[8] + out[9]))
            strides = []
            for X in (1, -1):                                  # the left foot's strides first
                for (l0, a0, b0), (l1, a1, b1), (l2, a2, _) in zip(found[:-2], found[1:-1], found[2:]):
                    if l0 == X and l1 == -X and l2 == X:
                        length = a2 - a0
                        strides.append((length / fps, (b1 - a0) / fps, (a2 - b1) / fps, (a1 - b0) / fps, (100.0 * (b1 - a0)) / length,
                                        (100.0 * ((b0 - a0) + (b1 - a1))) / length))
            out[11] = len(strides)
            if strides:
                cols = list(zip(*strides))
                out[12], out[13] = _gait_mean_sd(cols[0])
                for col, values in zip((14, 15, 16, 17, 18), cols[1:]):
                    out[col] = _gait_sum(values) / len(values)
                out[19] = (100.0 * out[13]) / out[12]
            f0 += T
    return {"phase": phase, "runs": runs, "per_sequence": per_seq}


def gait_contacts(joints3d, events, lengths=None, fps=20.0, sigma=0.0, fraction=0.25, speed=0.0, reach=2, max_frames=20, max_runs=128,
                  joints=GAIT_JOINTS_KINECTV2):
    """Foot contact phases and double support from 3D joints in numpy float64 (the rules: DESIGN 4.14; the thresholds are unvalidated on the model's
    output): the host statement of GRNet.gait_contacts, same arguments, a dict of numpy arrays -- the same operations in the same order.  joints3d
    (n,J,3) as gait_parameters takes them; events: its events; joints: its table, of which the two ankles are read.  per_frame (n,4) = [s, d_x, d_y,
    d_z]: d = left ankle - right ankle, smoothed by sigma frames per column inside each sequence; s(k) = |d(k + 1) - d(k)| fps, NaN in the last row of
    every sequence.  phase, runs, per_sequence: gait_contact_runs'."""
    j3 = _widened(joints3d, "joints3d")
    n, J = j3.shape[:2]
    lengths = _sequence_lengths(n, lengths)
    tab = _joint_table(joints, 8, J, _GAIT_JOINT_NAMES)
    _contact_rule_check(fps, fraction, speed, reach, max_frames, max_runs)
    _sigma_check(sigma)
    per_frame = np.full((n, 4), np.nan)
    with np.errstate(all="ignore"):
        d = j3[:, tab[4]] - j3[:, tab[5]]
        a = 0
        for T in lengths:
            seq = d[a:a + T]
            if sigma > 0:
                seq = np.stack([gauss_filter1d(seq[:, k], sigma) for k in range(3)], axis=1)
            per_frame[a:a + T, 1:] = seq
            step = seq[1:] - seq[:-1]
            per_frame[a:a + T - 1, 0] = np.sqrt((step[:, 0] * step[:, 0] + step[:, 1] * step[:, 1]) + step[:, 2] * step[:, 2]) * float(fps)
            a += T
    out = gait_contact_runs(per_frame[:, 0], events, lengths, fps, fraction, speed, reach, max_frames, max_runs)
    out["per_frame"] = per_frame
    return out


# ----------------------------------------------------------------------------- gait regularity and symmetry from the autocorrelation
REGULARITY_CHANNELS = ("sep", "lift", "sway", "bob")           # 0 .. 2 odd (a step is half a stride with the sign turned), 3 even (it repeats every step)
REGULARITY_COLUMNS = ("n", "variance", "step_lag", "step_lag_refined", "step_regularity", "stride_lag", "stride_lag_refined", "stride_regularity",
                      "symmetry", "cadence")


def _regularity_rule_check(fps, max_lag, min_lag, min_peak, min_pairs):
    if not np.isfinite(fps) or not fps > 0:
        raise ValueError("fps must be positive and finite")
    if int(max_lag) != max_lag or int(min_lag) != min_lag or int(min_pairs) != min_pairs:
        raise ValueError("max_lag, min_lag and min_pairs must be whole numbers")
    if not 8 <= max_lag <= 255:
        raise ValueError(f"max_lag {max_lag} outside [8, 255]")
    if not 2 <= min_lag <= max_lag - 2:
        raise ValueError(f"min_lag {min_lag} outside [2, max_lag - 2]")
    if not 0 < min_peak <= 1:
        raise ValueError("min_peak outside (0, 1]")
    if not 2 <= min_pairs <= 2 ** 20:
        raise ValueError(f"min_pairs {min_pairs} outside [2, 2^20]")


def _regularity_sum(values):
    """The sum in the order given from +0.0, one rounding per addition."""
    return float(np.cumsum(np.concatenate([[0.0], np.asarray(values, np.float64)]))[-1])


def _regularity_refine(rho, m):
    a, b, c = rho[m - 1], rho[m], rho[m + 1]
    den = (a - 2.0 * b) + c
    return float(m) if den == 0 else m + (0.5 * (a - c)) / den


def gait_autocorr(signals, lengths=None, exclude=None, fps=20.0, max_lag=60, min_lag=4, min_peak=0.25, min_pairs=20, return_pairs=False):
    """Rules 4 to 8 of DESIGN 4.15 on given signals: the host statement of GRNet.op_gait_autocorr.  signals (n,4) float64, columns
    REGULARITY_CHANNELS; exclude (n,) or None: a frame whose entry is not 0 does not count.  Returns {'acf': (n_seq,4,max_lag+1), 'per_sequence':
    (n_seq,4,10), columns REGULARITY_COLUMNS}; every sum in time order from +0.0, every comparison false for NaN.  return_pairs: also 'pairs'
    (n_seq,4,max_lag+1) int64, the N(m) of rule 5."""
    x = np.asarray(signals, np.float64)
    if x.ndim != 2 or x.shape[1] != 4 or x.shape[0] < 1:
        raise ValueError(f"signals must be (n,4) with n >= 1, got {x.shape}")
    n = x.shape[0]
    lengths = _sequence_lengths(n, lengths)
    ex = None
    if exclude is not None:
        ex = np.asarray(exclude)
        if ex.shape != (n,):
            raise ValueError(f"exclude must be ({n},), got {ex.shape}")
    _regularity_rule_check(fps, max_lag, min_lag, min_peak, min_pairs)
    fps, L, min_lag, min_peak, min_pairs = float(fps), int(max_lag), int(min_lag), float(min_peak), int(min_pairs)
    acf = np.full((len(lengths), 4, L + 1), np.nan)
    per_seq = np.full((len(lengths), 4, 10), np.nan)
    pairs = np.zeros((len(lengths), 4, L + 1), np.int64)
    f0 = 0
    with np.errstate(all="ignore"):
        for q, T in enumerate(lengths):
            for ch in range(4):
                s = x[f0:f0 + T, ch]
                valid = np.isfinite(s)
                if ex is not None:
                    valid &= ex[f0:f0 + T] == 0
                run = np.cumsum(~valid) - (~valid)                 # the invalid frames before t
                count = int(valid.sum())
                out, rho = per_seq[q, ch], acf[q, ch]
                out[0] = count
                if count == 0:
                    continue
                d = s - _regularity_sum(s[valid]) / count
                sums, N = np.zeros(L + 1), np.zeros(L + 1, np.int64)
                for m in range(min(L, T - 1) + 1):
                    pair = valid[:T - m] & valid[m:] & (run[:T - m] == run[m:])
                    N[m] = int(pair.sum())
                    sums[m] = _regularity_sum(d[:T - m][pair] * d[m:][pair])
                pairs[q, ch] = N
                if N[0] < min_pairs or not sums[0] / N[0] > 0:
                    continue
                A0 = sums[0] / N[0]
                ok = N >= min_pairs
                rho[ok] = (sums[ok] / N[ok]) / A0
                out[1] = A0
                inner = np.arange(1, L)
                is_max, is_min = np.zeros(L + 1, bool), np.zeros(L + 1, bool)
                is_max[inner] = (rho[inner] > rho[inner - 1]) & (rho[inner] >= rho[inner + 1])
                is_min[inner] = (-rho[inner] > -rho[inner - 1]) & (-rho[inner] >= -rho[inner + 1])
                lag = np.arange(L + 1)
                first = np.flatnonzero(is_max & (rho >= min_peak) & (lag >= min_lag) & (lag <= L - 1))
                first = int(first[0]) if first.size else -1
                d1 = d2 = -1
                odd = ch < 3
                if odd:
                    d2 = first
                    if d2 >= 0:
                        cand = np.flatnonzero(is_min & (lag >= d2 - 3 * d2 // 4) & (lag <= d2 - d2 // 4))
                        if cand.size:
                            d1 = int(cand[np.argmin(rho[cand])])   # argmin and argmax take the earliest of a tie
                else:
                    d1 = first
                    if d1 >= 0:
                        cand = np.flatnonzero(is_max & (lag >= max(2 * d1 - d1 // 2, 1)) & (lag <= min(2 * d1 + d1 // 2, L - 1)))
                        if cand.size:
                            d2 = int(cand[np.argmax(rho[cand])])
                out[2], out[5] = d1, d2
                if d1 >= 0:
                    out[3], out[4] = _regularity_refine(rho, d1), (-rho[d1] if odd else rho[d1])
                if d2 >= 0:
                    out[6], out[7] = _regularity_refine(rho, d2), rho[d2]
                    out[9] = (120.0 * fps) / out[6]
                    if d1 >= 0 and out[7] > 0:
                        out[8] = out[4] / out[7]
            f0 += T
    out = {"acf": acf, "per_sequence": per_seq}
    if return_pairs:
        out["pairs"] = pairs
    return out


def gait_regularity(joints3d, lengths=None, trans=None, exclude=None, fps=20.0, sigma=0.0, max_lag=60, min_lag=4, min_peak=0.25, min_pairs=20,
                    joints=GAIT_JOINTS_KINECTV2):
    """Gait regularity and symmetry without events, from the autocorrelation of four body signals in numpy float64 (Moe-Nilssen and Helbostad 2004, on
    trunk accelerations; the rules: DESIGN 4.15; the defaults are unvalidated on the model's output): the host statement of GRNet.gait_regularity,
    same arguments, a dict of numpy arrays -- the same operations in the same order, every sum a cumulative sum.  joints3d (n,J,3) and joints as
    gait_parameters takes them (the foot entries are not read); trans (n,3) or None; exclude (n,) or None.  per_frame (n,4) = [sep, lift, sway, bob]
    as smoothed by sigma frames; acf and per_sequence: gait_autocorr's."""
    lengths, per_frame = _regularity_signals(joints3d, lengths, trans, sigma, joints, lambda: _regularity_rule_check(fps, max_lag, min_lag, min_peak, min_pairs))
    out = gait_autocorr(per_frame, lengths, exclude, fps, max_lag, min_lag, min_peak, min_pairs)
    out["per_frame"] = per_frame
    return out


def _regularity_signals(joints3d, lengths, trans, sigma, joints, rule_check):
    """(the sequences' lengths, per_frame (n,4)) of gait_regularity and gait_harmonics: rules 1 to 3 of DESIGN 4.15.  rule_check() refuses the caller's
    own scalars, behind the joint table and before sigma, as the C ABI does."""
    j3 = _widened(joints3d, "joints3d")
    n, J = j3.shape[:2]
    lengths = _sequence_lengths(n, lengths)
    tab = _joint_table(joints, 8, J, _GAIT_JOINT_NAMES)
    rule_check()
    _sigma_check(sigma)
    tr = None
    if trans is not None:
        tr = np.asarray(trans, np.float64)
        if tr.shape != (n, 3):
            raise ValueError(f"trans must be ({n},3), got {tr.shape}")

    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    pelvis, spine, lhip, rhip, lank, rank_ = (j3[:, i] for i in tab[:6])
    per_frame = np.full((n, 4), np.nan)
    with np.errstate(all="ignore"):
        l, u = lhip - rhip, spine - pelvis
        c = np.stack([l[:, 1] * u[:, 2] - l[:, 2] * u[:, 1], l[:, 2] * u[:, 0] - l[:, 0] * u[:, 2], l[:, 0] * u[:, 1] - l[:, 1] * u[:, 0]], axis=1)
        nc, nl, nu = np.sqrt(dot(c, c)), np.sqrt(dot(l, l)), np.sqrt(dot(u, u))
        valid = (nc > 0) & np.isfinite(nc) & (nl > 0) & np.isfinite(nl)
        f, side, up, d = c / nc[:, None], l / nl[:, None], u / nu[:, None], lank - rank_
        per_frame[:, 0] = np.where(valid, dot(d, f), np.nan)
        per_frame[:, 1] = np.where(valid, dot(d, up), np.nan)
        per_frame[:, 2] = np.where(valid, dot(up, side), np.nan)
        if tr is not None:
            per_frame[:, 3] = np.where(np.isfinite(tr).all(axis=1), -(pelvis[:, 1] + tr[:, 1]), np.nan)
        if sigma > 0:
            a = 0
            for T in lengths:
                for k in range(4):
                    per_frame[a:a + T, k] = gauss_filter1d(per_frame[a:a + T, k].copy(), sigma)
                a += T
    return lengths, per_frame


# ----------------------------------------------------------------------------- harmonic ratios per stride
HARMONICS_CHANNELS = REGULARITY_CHANNELS
HARMONICS_COLUMNS = ("candidates", "used", "hr_mean", "hr_sd", "hr_left", "hr_right", "hr_left_right_index", "ihr_mean", "ihr_sd", "stride_frames",
                     "strides_per_second", "least_harmonics")
HARMONICS_STRIDE_COLUMNS = ("t0", "t1", "side", "harmonics", "hr", "ihr")
_HARMONICS_SIN = tuple((-1.0) ** k / math.factorial(2 * k + 1) for k in range(9))      # every factorial here is a double: the division rounds once
_HARMONICS_COS = tuple((-1.0) ** k / math.factorial(2 * k) for k in range(10))


def _harmonics_rule_check(fps, n_harmonics, derivative, min_stride, max_stride, max_strides):
    if not np.isfinite(fps) or not fps > 0:
        raise ValueError("fps must be positive and finite")
    if any(int(v) != v for v in (n_harmonics, derivative, min_stride, max_stride, max_strides)):
        raise ValueError("n_harmonics, derivative, min_stride, max_stride and max_strides must be whole numbers")
    if not 2 <= n_harmonics <= 32 or n_harmonics % 2:
        raise ValueError(f"n_harmonics {n_harmonics} must be even and within [2, 32]")
    if not 0 <= derivative <= 2:
        raise ValueError(f"derivative {derivative} outside [0, 2]")
    if max_stride > 255:
        raise ValueError(f"max_stride {max_stride} above 255")
    if not 6 <= min_stride <= max_stride:
        raise ValueError(f"min_stride {min_stride} outside [6, max_stride]")
    if not 1 <= max_strides <= 512:
        raise ValueError(f"max_strides {max_strides} outside [1, 512]")


def harmonics_twiddles(L):
    """Rule 5 of DESIGN 4.16: (sin, cos) of 2 pi j / L for j = 0 .. L - 1 without libm -- the reduction in integers, two Horner polynomials on [0, pi/4],
    then selection and negation alone.  The device and the host checker make the same bits."""
    j = np.arange(int(L), dtype=np.int64)
    r = 4 * j
    q, m = r // L, r % L
    swap = 2 * m > L
    phi = (1.5707963267948966 * np.where(swap, L - m, m).astype(np.float64)) / float(L)
    z = phi * phi
    p = np.full(z.shape, _HARMONICS_SIN[-1])
    for coef in _HARMONICS_SIN[-2::-1]:
        p = p * z + coef
    s = phi * p
    c = np.full(z.shape, _HARMONICS_COS[-1])
    for coef in _HARMONICS_COS[-2::-1]:
        c = c * z + coef
    a, b = np.where(swap, c, s), np.where(swap, s, c)
    return np.choose(q, [a, b, -a, -b]), np.choose(q, [b, -a, -b, a])


def _harmonics_moments(values):
    """(S / n, the two-pass SD with ddof 0) of the values in the order given, or (NaN, NaN) of none."""
    v = np.asarray(values, np.float64)
    if v.size == 0:
        return np.nan, np.nan
    m = _regularity_sum(v) / v.size
    d = v - m
    return m, float(np.sqrt(_regularity_sum(d * d) / v.size))


def gait_stride_dft(signals, events, lengths=None, exclude=None, fps=20.0, n_harmonics=20, derivative=2, min_stride=8, max_stride=60, max_strides=128,
                    return_sums=False):
    """Rules 3 to 8 of DESIGN 4.16 on given signals: the host statement of GRNet.op_gait_stride_dft.  signals (n,4) float64, columns
    HARMONICS_CHANNELS; events (n,) as gait_parameters returns them (bits 0 and 1 are read); exclude (n,) or None.  Returns {'strides':
    (n_seq,4,max_strides,6), columns HARMONICS_STRIDE_COLUMNS, 'spectrum': (n_seq,4,n_harmonics,2), 'per_sequence': (n_seq,4,12), columns
    HARMONICS_COLUMNS}; every sum in the order of the rules from +0.0, every comparison false for NaN.  return_sums: also 'sums', a list of
    (sequence, channel, t0, t1, y, C, S) of every used stride, in order."""
    x = np.asarray(signals, np.float64)
    if x.ndim != 2 or x.shape[1] != 4 or x.shape[0] < 1:
        raise ValueError(f"signals must be (n,4) with n >= 1, got {x.shape}")
    n = x.shape[0]
    ev = np.asarray(events)
    if ev.shape != (n,):
        raise ValueError(f"events must be ({n},), got {ev.shape}")
    ev = ev.astype(np.int64)
    lengths = _sequence_lengths(n, lengths)
    ex = None
    if exclude is not None:
        ex = np.asarray(exclude)
        if ex.shape != (n,):
            raise ValueError(f"exclude must be ({n},), got {ex.shape}")
    _harmonics_rule_check(fps, n_harmonics, derivative, min_stride, max_stride, max_strides)
    fps, n_h, d, max_strides = float(fps), int(n_harmonics), int(derivative), int(max_strides)
    strides = np.full((len(lengths), 4, max_strides, 6), np.nan)
    spectrum = np.full((len(lengths), 4, n_h, 2), np.nan)
    per_seq = np.full((len(lengths), 4, 12), np.nan)
    tables, sums = {}, []
    f0 = 0
    with np.errstate(all="ignore"):
        for q, T in enumerate(lengths):
            e = ev[f0:f0 + T]
            cand = []
            for bit, side in ((1, 1.0), (2, -1.0)):
                at = np.flatnonzero(e & bit)
                cand += [(int(t0), int(t1), side) for t0, t1 in zip(at[:-1], at[1:])]
            for ch in range(4):
                s = x[f0:f0 + T, ch]
                valid = np.isfinite(s)
                if ex is not None:
                    valid &= ex[f0:f0 + T] == 0
                used = []                                         # (side, L, H, HR, iHR, amplitudes)
                for c, (t0, t1, side) in enumerate(cand):
                    L = t1 - t0
                    H, HR, iHR = 0, np.nan, np.nan
                    if min_stride <= L <= max_stride and valid[t0:t1 + 1].all():
                        i = np.arange(L)
                        y = (s[t0:t1] - s[t0]) - (s[t1] - s[t0]) * (i.astype(np.float64) / float(L))
                        if L not in tables:
                            tables[L] = harmonics_twiddles(L)
                        sn, cs = tables[L]
                        H = min(n_h, (L - 1) // 2) & ~1
                        C, S = np.zeros(H), np.zeros(H)
                        for k in range(1, H + 1):
                            j = (k * i) % L
                            C[k - 1], S[k - 1] = _regularity_sum(y * cs[j]), _regularity_sum(y * sn[j])
                        a = np.sqrt(C * C + S * S) * (2.0 / float(L))
                        k = np.arange(1, H + 1)
                        kf = k.astype(np.float64)
                        w = a * (1.0 if d == 0 else kf if d == 1 else kf * kf)
                        E, O = _regularity_sum(w[1::2]), _regularity_sum(w[0::2])
                        PE, PO = _regularity_sum(w[1::2] * w[1::2]), _regularity_sum(w[0::2] * w[0::2])
                        if E > 0 and np.isfinite(E) and O > 0 and np.isfinite(O):
                            odd = ch < 3
                            HR = O / E if odd else E / O
                            iHR = (100.0 * (PO if odd else PE)) / (PE + PO)
                            used.append((side, L, H, HR, iHR, a))
                            if return_sums:
                                sums.append((q, ch, t0, t1, y, C, S))
                        else:
                            H = 0
                    if c < max_strides:
                        strides[q, ch, c] = (t0, t1, side, H, HR, iHR)
                out = per_seq[q, ch]
                out[0], out[1] = len(cand), len(used)
                out[2], out[3] = _harmonics_moments([u[3] for u in used])
                out[4] = _harmonics_moments([u[3] for u in used if u[0] > 0])[0]
                out[5] = _harmonics_moments([u[3] for u in used if u[0] < 0])[0]
                out[6] = (100.0 * np.abs(out[4] - out[5])) / (0.5 * (out[4] + out[5]))
                out[7], out[8] = _harmonics_moments([u[4] for u in used])
                out[9] = _harmonics_moments([float(u[1]) for u in used])[0]
                out[10] = fps / out[9]
                out[11] = min((u[2] for u in used), default=np.nan)
                for k in range(1, n_h + 1):
                    spectrum[q, ch, k - 1] = _harmonics_moments([u[5][k - 1] for u in used if u[2] >= k])
            f0 += T
    out = {"strides": strides, "spectrum": spectrum, "per_sequence": per_seq}
    if return_sums:
        out["sums"] = sums
    return out


def gait_harmonics(joints3d, events, lengths=None, trans=None, exclude=None, fps=20.0, sigma=0.0, n_harmonics=20, derivative=2, min_stride=8, max_stride=60,
                   max_strides=128, joints=GAIT_JOINTS_KINECTV2):
    """Harmonic ratios per stride in numpy float64 (Smidt et al. 1971, Menz et al. 2003, Bellanca et al. 2013, on trunk accelerations; the rules: DESIGN
    4.16; the defaults are unvalidated on the model's output): the host statement of GRNet.gait_harmonics, same arguments, a dict of numpy arrays --
    the same operations in the same order, every sum a cumulative sum.  per_frame (n,4) is gait_regularity's at the same sigma; strides, spectrum and
    per_sequence: gait_stride_dft's."""
    lengths, per_frame = _regularity_signals(joints3d, lengths, trans, sigma, joints,
                                             lambda: _harmonics_rule_check(fps, n_harmonics, derivative, min_stride, max_stride, max_strides))
    out = gait_stride_dft(per_frame, events, lengths, exclude, fps, n_harmonics, derivative, min_stride, max_stride, max_strides)
    out["per_frame"] = per_frame
    return out


# ----------------------------------------------------------------------------- sample entropy at several scales
ENTROPY_CHANNELS = REGULARITY_CHANNELS
ENTROPY_COLUMNS = ("n", "mean", "sd", "r")
ENTROPY_COUNTS = ("templates", "B", "A")
ENTROPY_MAX_FRAMES = 32768


def _entropy_rule_check(m, fraction, derivative, scales):
    """The refusals of csrc/gait_entropy.h's ent_rule_error, in its words."""
    if any(int(v) != v for v in (m, derivative, scales)):
        raise ValueError("m, derivative and scales must be whole numbers")
    if not 1 <= m <= 4:
        raise ValueError("m outside [1, 4]")
    if not np.isfinite(fraction) or not 0 < fraction <= 10:
        raise ValueError("fraction must be finite and within (0, 10]")
    if not 0 <= derivative <= 2:
        raise ValueError("derivative outside [0, 2]")
    if not 1 <= scales <= 8:
        raise ValueError("scales outside [1, 8]")


def _entropy_lengths_check(lengths):
    for q, T in enumerate(lengths):
        if T > ENTROPY_MAX_FRAMES:
            raise ValueError(f"sequence {q} has {T} frames, more than {ENTROPY_MAX_FRAMES} (the work is quadratic in them)")


def entropy_rows(counts, min_templates=50):
    """Rule 8 of DESIGN 4.17, the one place where the logarithm is taken: counts (..., scales, 3) integers = (valid templates, B, A), from the device
    or from gait_sampen -> {'sampen': (..., scales) float64 = ln(B / A), NaN where there are fewer than min_templates valid templates or A or B is 0;
    'complexity': (...) = their sum over the scales in order from +0.0, NaN where one is}."""
    c = np.asarray(counts)
    if c.ndim < 2 or c.shape[-1] != 3 or c.dtype.kind not in "iu":
        raise ValueError(f"counts must be integers of shape (..., scales, 3), got {c.dtype} {c.shape}")
    if int(min_templates) != min_templates or min_templates < 1:
        raise ValueError(f"min_templates {min_templates} must be a whole number of at least 1")
    flat = c.reshape(-1, 3)
    sampen = np.full(flat.shape[0], np.nan)
    for k, (templates, B, A) in enumerate(flat.tolist()):      # Python integers: B / A is their correctly rounded quotient
        if templates >= min_templates and A > 0 and B > 0:
            sampen[k] = math.log(B / A)
    sampen = sampen.reshape(c.shape[:-1])
    complexity = np.cumsum(np.concatenate([np.zeros(sampen.shape[:-1] + (1,)), sampen], axis=-1), axis=-1)[..., -1]
    return {"sampen": sampen, "complexity": complexity}


def gait_sampen(signals, lengths=None, exclude=None, m=2, fraction=0.2, derivative=2, scales=3, min_templates=50):
    """Rules 2 to 8 of DESIGN 4.17 on given signals: the host statement of GRNet.op_gait_sampen.  signals (n,4) float64, columns ENTROPY_CHANNELS;
    exclude (n,) or None: a frame whose entry is not 0 does not count.  Returns {'counts': (n_seq,4,scales,3) int64, columns ENTROPY_COUNTS,
    'per_sequence': (n_seq,4,4), columns ENTROPY_COLUMNS, and entropy_rows' 'sampen' and 'complexity'}.  Every pair of templates is compared, one
    offset between the two at a time; every sum in time order from +0.0, every comparison false for NaN."""
    x = np.asarray(signals, np.float64)
    if x.ndim != 2 or x.shape[1] != 4 or x.shape[0] < 1:
        raise ValueError(f"signals must be (n,4) with n >= 1, got {x.shape}")
    n = x.shape[0]
    lengths = _sequence_lengths(n, lengths)
    ex = None
    if exclude is not None:
        ex = np.asarray(exclude)
        if ex.shape != (n,):
            raise ValueError(f"exclude must be ({n},), got {ex.shape}")
    _entropy_rule_check(m, fraction, derivative, scales)
    _entropy_lengths_check(lengths)
    m, fraction, d, scales = int(m), float(fraction), int(derivative), int(scales)
    counts = np.zeros((len(lengths), 4, scales, 3), np.int64)
    per_seq = np.full((len(lengths), 4, 4), np.nan)
    f0 = 0
    with np.errstate(all="ignore"):
        for q, T in enumerate(lengths):
            for ch in range(4):
                s = x[f0:f0 + T, ch]
                valid = np.isfinite(s)
                if ex is not None:
                    valid &= ex[f0:f0 + T] == 0
                y = np.where(valid, s, np.nan)
                for _ in range(d):
                    y = np.concatenate([y[1:] - y[:-1], [np.nan]])
                y[~np.isfinite(y)] = np.nan
                ok = np.isfinite(y)
                count = int(ok.sum())
                mu = _regularity_sum(y[ok]) / count if count else np.nan
                e = y[ok] - mu
                sd = float(np.sqrt(_regularity_sum(e * e) / (count - 1))) if count >= 2 else np.nan
                r = fraction * sd
                per_seq[q, ch] = (count, mu, sd, r)
                for tau in range(1, scales + 1):
                    N = T // tau
                    parts = y[:N * tau].reshape(N, tau)
                    z = parts[:, 0].copy()
                    for k in range(1, tau):
                        z = z + parts[:, k]
                    z = z / float(tau)
                    z[~np.isfinite(z)] = np.nan
                    Nt = N - m
                    if Nt <= 0:
                        continue
                    fin = np.isfinite(z)
                    tv = fin[:Nt].copy()
                    for k in range(1, m + 1):
                        tv &= fin[k:k + Nt]
                    B = A = 0
                    if r > 0:
                        for step in range(1, Nt):
                            w = Nt - step
                            hit = tv[:w] & tv[step:]
                            for k in range(m):
                                hit &= np.abs(z[k:k + w] - z[k + step:k + step + w]) <= r
                            B += int(hit.sum())
                            hit &= np.abs(z[m:m + w] - z[m + step:m + step + w]) <= r
                            A += int(hit.sum())
                    counts[q, ch, tau - 1] = (int(tv.sum()), B, A)
            f0 += T
    out = {"counts": counts, "per_sequence": per_seq}
    out.update(entropy_rows(counts, min_templates))
    return out


def gait_entropy(joints3d, lengths=None, trans=None, exclude=None, sigma=0.0, m=2, fraction=0.2, derivative=2, scales=3, min_templates=50,
                 joints=GAIT_JOINTS_KINECTV2):
    """Sample entropy of four body signals at several scales in numpy float64 and Python integers (Richman and Moorman 2000, Costa et al. 2002, Lamoth et
    al. 2011 on trunk accelerations; the rules: DESIGN 4.17; the defaults are unvalidated on the model's output): the host statement of
    GRNet.gait_entropy, same arguments, a dict of numpy arrays.  per_frame (n,4) is gait_regularity's at the same sigma; counts, per_sequence, sampen and
    complexity: gait_sampen's."""
    def rule_check():
        _entropy_rule_check(m, fraction, derivative, scales)
        _entropy_lengths_check(_sequence_lengths(np.asarray(joints3d).shape[0], lengths))
    lengths, per_frame = _regularity_signals(joints3d, lengths, trans, sigma, joints, rule_check)
    out = gait_sampen(per_frame, lengths, exclude, m, fraction, derivative, scales, min_templates)
    out["per_frame"] = per_frame
    return out


# ----------------------------------------------------------------------------- local dynamic stability
STABILITY_CHANNELS = REGULARITY_CHANNELS
STABILITY_PAIRS = ("n", "exponent")
STABILITY_MAX_FRAMES = ENTROPY_MAX_FRAMES


def _stability_rule_check(derivative, dim, lag, theiler, horizon):
    """The refusals of csrc/gait_stability.h's stab_rule_error, in its words."""
    if any(int(v) != v for v in (derivative, dim, lag, theiler, horizon)):
        raise ValueError("derivative, dim, lag, theiler and horizon must be whole numbers")
    if not 0 <= derivative <= 2:
        raise ValueError("derivative outside [0, 2]")
    if not 2 <= dim <= 8:
        raise ValueError("dim outside [2, 8]")
    if not 1 <= lag <= 16:
        raise ValueError("lag outside [1, 16]")
    if not 0 <= theiler <= 4096:
        raise ValueError("theiler outside [0, 4096]")
    if not 1 <= horizon <= 63:
        raise ValueError("horizon outside [1, 63]")


def stability_rows(pairs, mant, fps=20.0, fit_lo=0, fit_hi=10, min_pairs=50):
    """Rule 7 of DESIGN 4.18, the one place where the logarithm is taken: pairs (..., K+1, 2) integers = (n, S) and mant (..., K+1) float64 = P, from
    the device or from gait_divergence -> {'divergence': (..., K+1) float64 = (ln P + S ln 2) / (2 n), the mean logarithm of the distance (the 2: the
    distances are squared), NaN where n < min_pairs; 'lambda': (...) = the least-squares slope of divergence over k = fit_lo .. fit_hi times fps, in
    1/s, every sum in k order from +0.0, NaN if a point of the window is}."""
    c, P = np.asarray(pairs), np.asarray(mant, np.float64)
    if c.ndim < 2 or c.shape[-1] != 2 or c.dtype.kind not in "iu" or P.shape != c.shape[:-1]:
        raise ValueError(f"pairs must be integers of shape (..., K+1, 2) and mant (..., K+1), got {c.dtype} {c.shape} and {P.shape}")
    K = c.shape[-2] - 1
    if int(min_pairs) != min_pairs or min_pairs < 1:
        raise ValueError(f"min_pairs {min_pairs} must be a whole number of at least 1")
    if int(fit_lo) != fit_lo or int(fit_hi) != fit_hi or fit_lo < 0 or fit_hi <= fit_lo or fit_hi > K:
        raise ValueError(f"the fit window {fit_lo} .. {fit_hi} must hold 0 <= fit_lo < fit_hi <= horizon = {K}")
    if not np.isfinite(fps) or not fps > 0:
        raise ValueError("fps must be positive and finite")
    fit_lo, fit_hi, fps = int(fit_lo), int(fit_hi), float(fps)
    flat = np.full(P.size, np.nan)
    for at, ((n, S), p) in enumerate(zip(c.reshape(-1, 2).tolist(), P.reshape(-1).tolist())):
        if n >= min_pairs:
            flat[at] = (math.log(p) + S * math.log(2.0)) / (2 * n)
    div = flat.reshape(P.shape)
    rows = div.reshape(-1, K + 1)
    lam = np.full(rows.shape[0], np.nan)
    count = float(fit_hi - fit_lo + 1)
    for at, row in enumerate(rows.tolist()):
        sk = sv = 0.0
        for k in range(fit_lo, fit_hi + 1):
            sk = sk + float(k)
            sv = sv + row[k]
        mk, mv = sk / count, sv / count
        num = den = 0.0
        for k in range(fit_lo, fit_hi + 1):
            num = num + (float(k) - mk) * (row[k] - mv)
            den = den + (float(k) - mk) * (float(k) - mk)
        lam[at] = (num / den) * fps
    lam[~np.isfinite(lam)] = np.nan
    return {"divergence": div, "lambda": lam.reshape(P.shape[:-1])}


def _stability_dist2(y, a, b, dim, lag):
    """D2 of the points a (n,1) and b (1,m) or of two index arrays of one shape: rule 4's order, the first term, then one addition a term."""
    t = y[a] - y[b]
    d2 = t * t
    for c in range(1, dim):
        t = y[a + c * lag] - y[b + c * lag]
        d2 = d2 + t * t
    return d2


def gait_divergence(signals, lengths=None, exclude=None, derivative=1, dim=5, lag=2, theiler=20, horizon=20, fps=20.0, fit_lo=0, fit_hi=None, min_pairs=50):
    """Rules 1 (from the differencing on) to 7 of DESIGN 4.18 on given signals: the host statement of GRNet.op_gait_divergence.  signals (n,4) float64,
    columns STABILITY_CHANNELS; exclude (n,) or None: a frame whose entry is not 0 does not count.  Returns {'nn': (n,4) int32, the nearest neighbour
    of every eligible valid point, sequence-relative, else -1; 'pairs': (n_seq,4,horizon+1,2) int64, columns STABILITY_PAIRS; 'mant':
    (n_seq,4,horizon+1) float64; and stability_rows' 'divergence' and 'lambda'; fit_hi None: 10, or the horizon where that is shorter}.  Every pair of points is compared, a block of references at a time."""
    x = np.asarray(signals, np.float64)
    if x.ndim != 2 or x.shape[1] != 4 or x.shape[0] < 1:
        raise ValueError(f"signals must be (n,4) with n >= 1, got {x.shape}")
    n = x.shape[0]
    lengths = _sequence_lengths(n, lengths)
    ex = None
    if exclude is not None:
        ex = np.asarray(exclude)
        if ex.shape != (n,):
            raise ValueError(f"exclude must be ({n},), got {ex.shape}")
    _stability_rule_check(derivative, dim, lag, theiler, horizon)
    _entropy_lengths_check(lengths)
    d, dim, lag, w, K = int(derivative), int(dim), int(lag), int(theiler), int(horizon)
    nn = np.full((n, 4), -1, np.int32)
    pairs = np.zeros((len(lengths), 4, K + 1, 2), np.int64)
    mant = np.ones((len(lengths), 4, K + 1))
    span = (dim - 1) * lag
    ks = np.arange(K + 1)
    f0 = 0
    with np.errstate(all="ignore"):
        for q, T in enumerate(lengths):
            E = T - span - K
            for ch in range(4):
                if E <= 0:
                    break
                s = x[f0:f0 + T, ch]
                valid = np.isfinite(s)
                if ex is not None:
                    valid &= ex[f0:f0 + T] == 0
                y = np.where(valid, s, np.nan)
                for _ in range(d):
                    y = np.concatenate([y[1:] - y[:-1], [np.nan]])
                y[~np.isfinite(y)] = np.nan
                cand = np.arange(E)
                found = np.full(E, -1, np.int64)
                for i0 in range(0, E, 512):
                    ref = np.arange(i0, min(i0 + 512, E))
                    d2 = _stability_dist2(y, ref[:, None], cand[None, :], dim, lag)
                    ok = (np.abs(ref[:, None] - cand[None, :]) > w) & (d2 > 0)
                    best = np.argmin(np.where(ok, d2, np.inf), axis=1)                  # the first of equal minima: the smallest j
                    late = ~ok[np.arange(len(ref)), best]                               # only infinite candidates, or none
                    best[late] = np.argmax(ok[late], axis=1)
                    found[ref] = np.where(ok.any(axis=1), best, -1)
                nn[f0:f0 + E, ch] = found
                refs = np.flatnonzero(found >= 0)
                if not len(refs):
                    continue
                d2 = _stability_dist2(y, refs[:, None] + ks[None, :], found[refs][:, None] + ks[None, :], dim, lag)
                counts = (d2 > 0) & np.isfinite(d2)
                f, e = np.frexp(np.where(counts, d2, 0.5))
                P, S = np.ones(K + 1), np.zeros(K + 1, np.int64)
                for r in range(len(refs)):                     # rule 6: the references in increasing i, one rounding a product
                    new, e2 = np.frexp(P * f[r])
                    P = np.where(counts[r], new, P)
                    S = S + np.where(counts[r], e[r].astype(np.int64) + e2, 0)
                pairs[q, ch, :, 0] = counts.sum(axis=0)
                pairs[q, ch, :, 1] = S
                mant[q, ch] = P
            f0 += T
    out = {"nn": nn, "pairs": pairs, "mant": mant}
    out.update(stability_rows(pairs, mant, fps, fit_lo, min(10, K) if fit_hi is None else fit_hi, min_pairs))
    return out


def gait_stability(joints3d, lengths=None, trans=None, exclude=None, sigma=0.0, derivative=1, dim=5, lag=2, theiler=20, horizon=20, fps=20.0, fit_lo=0,
                   fit_hi=None, min_pairs=50, joints=GAIT_JOINTS_KINECTV2):
    """Local dynamic stability of four body signals in numpy float64 and Python integers (the short-term largest Lyapunov exponent of Rosenstein,
    Collins and De Luca 1993; Dingwell and Cusumano 2000, Bruijn et al. 2013 and Lamoth et al. 2011 on trunk sensors over 100+ strides; the rules:
    DESIGN 4.18; the defaults are unvalidated on the model's output, and on noisy joints the slope mostly measures the noise): the host statement of
    GRNet.gait_stability, same arguments, a dict of numpy arrays.  per_frame (n,4) is gait_regularity's at the same sigma; nn, pairs, mant, divergence
    and lambda: gait_divergence's."""
    def rule_check():
        _stability_rule_check(derivative, dim, lag, theiler, horizon)
        _entropy_lengths_check(_sequence_lengths(np.asarray(joints3d).shape[0], lengths))
    lengths, per_frame = _regularity_signals(joints3d, lengths, trans, sigma, joints, rule_check)
    out = gait_divergence(per_frame, lengths, exclude, derivative, dim, lag, theiler, horizon, fps, fit_lo, fit_hi, min_pairs)
    out["per_frame"] = per_frame
    return out


# ----------------------------------------------------------------------------- recurrence quantification
RECURRENCE_CHANNELS = REGULARITY_CHANNELS
RECURRENCE_COLUMNS = ("n", "mean", "sd", "r", "eps2")
RECURRENCE_COUNTS = ("points", "comparable", "recurrent", "long_lines", "long_points", "longest")
RECURRENCE_BINS = 255
RECURRENCE_MAX_FRAMES = ENTROPY_MAX_FRAMES
RECURRENCE_ROWS = ("lines", "line_points", "recurrence_rate", "determinism", "mean_line", "longest", "divergence", "line_entropy", "ratio")


def _recurrence_rule_check(derivative, dim, lag, theiler, radius):
    """The refusals of csrc/gait_recurrence.h's rec_rule_error, in its words."""
    if any(int(v) != v for v in (derivative, dim, lag, theiler)):
        raise ValueError("derivative, dim, lag and theiler must be whole numbers")
    if not 0 <= derivative <= 2:
        raise ValueError("derivative outside [0, 2]")
    if not 2 <= dim <= 8:
        raise ValueError("dim outside [2, 8]")
    if not 1 <= lag <= 16:
        raise ValueError("lag outside [1, 16]")
    if not 0 <= theiler <= 4096:
        raise ValueError("theiler outside [0, 4096]")
    if not np.isfinite(radius) or not 0 < radius <= 10:
        raise ValueError("radius must be finite and within (0, 10]")


def recurrence_rows(counts, hist, min_line=2, min_points=50):
    """Rule 7 of DESIGN 4.20, the one place where the line threshold is applied and the logarithm taken: counts (..., 6) integers, columns
    RECURRENCE_COUNTS, and hist (..., 255) integers, from the device or from gait_recurrence_counts -> a dict of (...) arrays, keys RECURRENCE_ROWS.
    lines and line_points (int64) count the lines of min_line (1 .. 255) pairs and more, the long ones (256 and more) among them; recurrence_rate =
    recurrent / comparable; determinism = line_points / recurrent; mean_line = line_points / lines; longest and divergence = 1 / longest, both NaN
    where longest < min_line; line_entropy = -sum p ln p over the classes l = min_line .. 255 in rising l from +0.0 and ONE further class of all lines
    of 256 and more; ratio = determinism / recurrence_rate.  Everything but the two integers is NaN where points < min_points or its own denominator
    is 0.  Python integers and floats: a quotient of two counts is their correctly rounded quotient."""
    c, h = np.asarray(counts), np.asarray(hist)
    if c.ndim < 1 or c.shape[-1] != 6 or c.dtype.kind not in "iu" or h.dtype.kind not in "iu" or h.shape != c.shape[:-1] + (RECURRENCE_BINS,):
        raise ValueError(f"counts must be integers of shape (..., 6) and hist (..., {RECURRENCE_BINS}), got {c.dtype} {c.shape} and {h.dtype} {h.shape}")
    if int(min_line) != min_line or not 1 <= min_line <= RECURRENCE_BINS:
        raise ValueError(f"min_line {min_line} must be a whole number within [1, {RECURRENCE_BINS}]")
    if int(min_points) != min_points or min_points < 1:
        raise ValueError(f"min_points {min_points} must be a whole number of at least 1")
    min_line = int(min_line)
    lead = c.shape[:-1]
    flat_c, flat_h = c.reshape(-1, 6).tolist(), h.reshape(-1, RECURRENCE_BINS).tolist()
    nan = float("nan")
    out = {k: np.zeros(len(flat_c), np.int64) if k in ("lines", "line_points") else np.full(len(flat_c), nan) for k in RECURRENCE_ROWS}
    for at, ((points, comparable, recurrent, long_lines, long_points, longest), bins) in enumerate(zip(flat_c, flat_h)):
        lines, line_points = long_lines, long_points
        for length in range(min_line, RECURRENCE_BINS + 1):
            lines += bins[length - 1]
            line_points += length * bins[length - 1]
        out["lines"][at] = lines
        out["line_points"][at] = line_points
        if points < min_points:
            continue
        rate = recurrent / comparable if comparable > 0 else nan
        det = line_points / recurrent if recurrent > 0 else nan
        out["recurrence_rate"][at] = rate
        out["determinism"][at] = det
        if lines > 0:
            out["mean_line"][at] = line_points / lines
            acc = 0.0
            for k in list(bins[min_line - 1:]) + [long_lines]:
                if k > 0:
                    p = k / lines
                    acc = acc + p * math.log(p)
            out["line_entropy"][at] = -acc
        if longest >= min_line:
            out["longest"][at] = float(longest)
            out["divergence"][at] = 1.0 / longest
        if rate > 0:                                          # false for NaN
            out["ratio"][at] = det / rate
    return {k: v.reshape(lead) for k, v in out.items()}


def gait_recurrence_counts(signals, lengths=None, exclude=None, derivative=1, dim=5, lag=2, theiler=8, radius=0.8, min_line=2, min_points=50):
    """Rules 1 (from the differencing on) to 7 of DESIGN 4.20 on given signals: the host statement of GRNet.op_gait_recurrence_counts.  signals (n,4)
    float64, columns RECURRENCE_CHANNELS; exclude (n,) or None: a frame whose entry is not 0 does not count.  Returns {'per_sequence': (n_seq,4,5),
    columns RECURRENCE_COLUMNS; 'hist': (n_seq,4,255) int64, the lines of length 1 .. 255; 'counts': (n_seq,4,6) int64, columns RECURRENCE_COUNTS; and
    recurrence_rows' (n_seq,4) arrays}.  Every pair of points is compared, one diagonal j - i at a time; the runs of a diagonal are the differences
    of its recurrent pairs as a boolean vector padded with a False at either end."""
    x = np.asarray(signals, np.float64)
    if x.ndim != 2 or x.shape[1] != 4 or x.shape[0] < 1:
        raise ValueError(f"signals must be (n,4) with n >= 1, got {x.shape}")
    n = x.shape[0]
    lengths = _sequence_lengths(n, lengths)
    ex = None
    if exclude is not None:
        ex = np.asarray(exclude)
        if ex.shape != (n,):
            raise ValueError(f"exclude must be ({n},), got {ex.shape}")
    _recurrence_rule_check(derivative, dim, lag, theiler, radius)
    _entropy_lengths_check(lengths)
    d, dim, lag, w, radius = int(derivative), int(dim), int(lag), int(theiler), float(radius)
    per_seq = np.full((len(lengths), 4, 5), np.nan)
    hist = np.zeros((len(lengths), 4, RECURRENCE_BINS), np.int64)
    counts = np.zeros((len(lengths), 4, 6), np.int64)
    span = (dim - 1) * lag
    f0 = 0
    with np.errstate(all="ignore"):
        for q, T in enumerate(lengths):
            M = max(T - span, 0)
            for ch in range(4):
                s = x[f0:f0 + T, ch]
                valid = np.isfinite(s)
                if ex is not None:
                    valid &= ex[f0:f0 + T] == 0
                y = np.where(valid, s, np.nan)
                for _ in range(d):
                    y = np.concatenate([y[1:] - y[:-1], [np.nan]])
                y[~np.isfinite(y)] = np.nan
                ok = np.isfinite(y)
                count = int(ok.sum())
                mu = _regularity_sum(y[ok]) / count if count else np.nan
                e = y[ok] - mu
                sd = float(np.sqrt(_regularity_sum(e * e) / (count - 1))) if count >= 2 else np.nan
                r = radius * sd
                eps2 = (r * r) * float(dim)
                per_seq[q, ch] = (count, mu, sd, r, eps2)
                if M == 0:
                    continue
                pv = ok[:M].copy()
                for k in range(1, dim):
                    pv &= ok[k * lag:k * lag + M]
                lines = np.zeros(T + 1, np.int64)                 # lines[l]: the lines of length l
                comparable = recurrent = 0
                for step in range(w + 1, M):
                    m = M - step
                    both = pv[:m] & pv[step:]
                    comparable += int(both.sum())
                    if not r > 0:
                        continue
                    t = y[:m] - y[step:M]
                    d2 = t * t
                    for k in range(1, dim):
                        t = y[k * lag:k * lag + m] - y[k * lag + step:k * lag + M]
                        d2 = d2 + t * t
                    hit = both & (d2 <= eps2) & np.isfinite(d2)       # an infinite distance never recurs, whatever eps2
                    recurrent += int(hit.sum())
                    edge = np.diff(np.concatenate([[False], hit, [False]]).astype(np.int8))
                    lines += np.bincount(np.flatnonzero(edge == -1) - np.flatnonzero(edge == 1), minlength=T + 1)
                long_at = np.flatnonzero(lines[RECURRENCE_BINS + 1:]) + RECURRENCE_BINS + 1
                hist[q, ch] = lines[1:RECURRENCE_BINS + 1] if T >= RECURRENCE_BINS else np.pad(lines[1:], (0, RECURRENCE_BINS - T))
                every = np.flatnonzero(lines)
                counts[q, ch] = (int(pv.sum()), comparable, recurrent, int(lines[long_at].sum()), int((lines[long_at] * long_at).sum()),
                                 int(every[-1]) if len(every) else 0)
            f0 += T
    out = {"per_sequence": per_seq, "hist": hist, "counts": counts}
    out.update(recurrence_rows(counts, hist, min_line, min_points))
    return out


def gait_recurrence(joints3d, lengths=None, trans=None, exclude=None, sigma=0.0, derivative=1, dim=5, lag=2, theiler=8, radius=0.8, min_line=2,
                    min_points=50, joints=GAIT_JOINTS_KINECTV2):
    """Recurrence quantification of four body signals in numpy float64 and Python integers (Webber and Zbilut 1994, Marwan et al. 2007; Labini et al.
    2012 and Riva et al. 2013 on trunk sensors over minutes of walking; the rules: DESIGN 4.20; the radius rule is this project's and the defaults are
    unvalidated on the model's output): the host statement of GRNet.gait_recurrence, same arguments, a dict of numpy arrays.  per_frame (n,4) is
    gait_regularity's at the same sigma; per_sequence, hist, counts and the rows: gait_recurrence_counts'."""
    def rule_check():
        _recurrence_rule_check(derivative, dim, lag, theiler, radius)
        _entropy_lengths_check(_sequence_lengths(np.asarray(joints3d).shape[0], lengths))
    lengths, per_frame = _regularity_signals(joints3d, lengths, trans, sigma, joints, rule_check)
    out = gait_recurrence_counts(per_frame, lengths, exclude, derivative, dim, lag, theiler, radius, min_line, min_points)
    out["per_frame"] = per_frame
    return out


# ----------------------------------------------------------------------------- the Welch spectrum
SPECTRUM_CHANNELS = REGULARITY_CHANNELS
SPECTRUM_COLUMNS = ("n", "candidates", "used", "band_power", "total_power", "peak_bin", "peak_hz", "peak_height", "peak_width_hz", "dominance", "centroid_hz",
                    "edge_hz", "cadence")
SPECTRUM_MAX_FRAMES = ENTROPY_MAX_FRAMES


def _spectrum_rule_check(fps, derivative, segment, hop, nfft, f_lo, f_hi, min_segments):
    """The refusals of csrc/gait_spectrum.h's spec_rule_error, in its words."""
    if not np.isfinite(fps) or not fps > 0:
        raise ValueError("fps must be positive and finite")
    if any(int(v) != v for v in (derivative, segment, hop, nfft, min_segments)):
        raise ValueError("derivative, segment, hop, nfft and min_segments must be whole numbers")
    if not 0 <= derivative <= 2:
        raise ValueError("derivative outside [0, 2]")
    if not 8 <= segment <= 256 or segment % 2:
        raise ValueError("segment must be even and within [8, 256]")
    if not segment // 8 <= hop <= segment:
        raise ValueError("hop outside [segment / 8, segment]")
    if not segment <= nfft <= 1024 or nfft % 2:
        raise ValueError("nfft must be even and within [segment, 1024]")
    if not (np.isfinite(f_lo) and np.isfinite(f_hi) and 0 < f_lo < f_hi <= fps / 2.0):
        raise ValueError("f_lo and f_hi must obey 0 < f_lo < f_hi <= fps / 2")
    if not 1 <= min_segments <= 2 ** 20:
        raise ValueError("min_segments outside [1, 2^20]")


def _spectrum_band(fps, nfft, f_lo, f_hi):
    """spec_band: (k_lo, k_hi) of the bins 0 .. nfft / 2 whose frequency (k fps) / nfft lies in [f_lo, f_hi]; k_lo > k_hi where there is none."""
    f = (np.arange(nfft // 2 + 1, dtype=np.float64) * float(fps)) / float(nfft)
    inside = np.flatnonzero((f >= f_lo) & (f <= f_hi))
    return (int(inside[0]), int(inside[-1])) if inside.size else (nfft // 2 + 1, -1)


def _spectrum_row(P, fps, nfft, f_lo, f_hi, odd, n, candidates, used):
    """spec_row on Python floats, one operation at a time in the header's order."""
    nan = float("nan")
    out = [float(n), float(candidates), float(used)] + [nan] * 10
    if used < 1:
        return out
    P = [float(v) for v in P]
    fps, N, half = float(fps), float(nfft), nfft // 2
    df = fps / N
    k_lo, k_hi = _spectrum_band(fps, nfft, f_lo, f_hi)
    band = total = sum_p = sum_fp = 0.0
    best = -1
    for k in range(1, half + 1):
        total = total + P[k] * df
    for k in range(k_lo, k_hi + 1):
        band = band + P[k] * df
        sum_p = sum_p + P[k]
        sum_fp = sum_fp + ((float(k) * fps) / N) * P[k]
        if P[k] > 0.0 and math.isfinite(P[k]) and (best < 0 or P[k] > P[best]):
            best = k
    out[3], out[4] = band, total
    if sum_p > 0.0 and math.isfinite(sum_p):
        out[10] = sum_fp / sum_p
    if band > 0.0 and math.isfinite(band):
        bar, running = 0.95 * band, 0.0
        for k in range(k_lo, k_hi + 1):
            running = running + P[k] * df
            if running >= bar:
                out[11] = (float(k) * fps) / N
                break
    if best < 0:
        return out
    b, at = P[best], float(best)
    if 0 < best < half:
        a, c = P[best - 1], P[best + 1]
        den = (a - 2.0 * b) + c
        if den < 0.0 and b >= a and b >= c:
            at = float(best) + (0.5 * (a - c)) / den
    out[5], out[6], out[7] = float(best), (at * fps) / N, b
    out[12] = (120.0 if odd else 60.0) * out[6]
    level, left, right = 0.5 * b, nan, nan
    for j in range(best - 1, -1, -1):
        if P[j] < level:
            left = float(j) + (level - P[j]) / (P[j + 1] - P[j])
            break
    for j in range(best + 1, half + 1):
        if P[j] < level:
            right = float(j - 1) + (P[j - 1] - level) / (P[j - 1] - P[j])
            break
    out[8] = ((right - left) * fps) / N
    three = 0.0
    for j in range(best - 1, best + 2):
        if k_lo <= j <= k_hi:
            three = three + P[j] * df
    if band > 0.0 and math.isfinite(band):
        out[9] = three / band
    return out


def spectrum_rows(psd, per_sequence, fps=20.0, f_lo=0.5, f_hi=3.0):
    """Rule 6 of DESIGN 4.19, the one place where the logarithm is taken: psd (..., nfft / 2 + 1) and per_sequence (..., 13), from the device or from
    gait_welch -> {'spectral_entropy': (...) float64 = -sum p ln p / ln(bins) over the band's bins, p = P / sum P there; NaN where used is 0, the band
    has fewer than 2 bins or its power is not positive}.  fps, f_lo and f_hi as the call had them."""
    P, rows = np.asarray(psd, np.float64), np.asarray(per_sequence, np.float64)
    if P.ndim < 1 or P.shape[-1] < 5 or rows.shape != P.shape[:-1] + (len(SPECTRUM_COLUMNS),):
        raise ValueError(f"psd must be (..., nfft / 2 + 1) and per_sequence (..., {len(SPECTRUM_COLUMNS)}) of the same rows, got {P.shape} and {rows.shape}")
    nfft = 2 * (P.shape[-1] - 1)
    k_lo, k_hi = _spectrum_band(fps, nfft, f_lo, f_hi)
    bins = k_hi - k_lo + 1
    flat, used = P.reshape(-1, P.shape[-1]), rows.reshape(-1, rows.shape[-1])[:, 2]
    out = np.full(flat.shape[0], np.nan)
    for e in range(flat.shape[0]):
        if bins < 2 or not used[e] >= 1:
            continue
        band = flat[e, k_lo:k_hi + 1].tolist()
        total = math.fsum(band)
        if not (total > 0.0 and math.isfinite(total)):
            continue
        h = 0.0
        for v in band:
            p = v / total
            if p > 0.0:
                h = h - p * math.log(p)
        out[e] = h / math.log(bins)
    return {"spectral_entropy": out.reshape(P.shape[:-1])}


def gait_welch(signals, lengths=None, exclude=None, fps=20.0, derivative=2, segment=64, hop=None, nfft=256, f_lo=0.5, f_hi=3.0, min_segments=2):
    """Rules 1 (from the differencing on) to 6 of DESIGN 4.19 on given signals: the host statement of GRNet.op_gait_welch.  signals (n,4) float64,
    columns SPECTRUM_CHANNELS; exclude (n,) or None: a frame whose entry is not 0 does not count; hop None: segment / 2.  Returns {'psd':
    (n_seq,4,nfft/2+1), 'per_sequence': (n_seq,4,13), columns SPECTRUM_COLUMNS, 'freqs': (nfft/2+1,), and spectrum_rows' 'spectral_entropy'}.  Every
    sum in rising index from +0.0 (a cumulative sum, or one addition a loop turn), the twiddles harmonics_twiddles' at (k i) mod nfft."""
    x = np.asarray(signals, np.float64)
    if x.ndim != 2 or x.shape[1] != 4 or x.shape[0] < 1:
        raise ValueError(f"signals must be (n,4) with n >= 1, got {x.shape}")
    n = x.shape[0]
    lengths = _sequence_lengths(n, lengths)
    ex = None
    if exclude is not None:
        ex = np.asarray(exclude)
        if ex.shape != (n,):
            raise ValueError(f"exclude must be ({n},), got {ex.shape}")
    if hop is None:
        hop = segment // 2 if int(segment) == segment else segment
    _spectrum_rule_check(fps, derivative, segment, hop, nfft, f_lo, f_hi, min_segments)
    _entropy_lengths_check(lengths)
    fps, d, L, hop, N, min_segments = float(fps), int(derivative), int(segment), int(hop), int(nfft), int(min_segments)
    half = N // 2
    sn, cs = harmonics_twiddles(N)
    w = 0.5 - 0.5 * harmonics_twiddles(L)[1]
    W2 = float(np.cumsum(np.concatenate([[0.0], w * w]))[-1])
    kk = np.arange(half + 1, dtype=np.int64)
    g = np.where((kk > 0) & (kk < half), 2.0, 1.0)
    psd = np.full((len(lengths), 4, half + 1), np.nan)
    per_seq = np.full((len(lengths), 4, len(SPECTRUM_COLUMNS)), np.nan)
    f0 = 0
    with np.errstate(all="ignore"):
        for q, T in enumerate(lengths):
            for ch in range(4):
                s = x[f0:f0 + T, ch]
                valid = np.isfinite(s)
                if ex is not None:
                    valid &= ex[f0:f0 + T] == 0
                y = np.where(valid, s, np.nan)
                for _ in range(d):
                    y = np.concatenate([y[1:] - y[:-1], [np.nan]])
                y[~np.isfinite(y)] = np.nan
                ok = np.isfinite(y)
                edges = np.flatnonzero(np.diff(np.concatenate([[False], ok, [False]]).astype(np.int8)))
                starts = [t0 for a, e in zip(edges[0::2], edges[1::2]) for t0 in range(int(a), int(e) - L + 1, hop)]
                candidates = len(starts)
                used = candidates if candidates >= min_segments else 0
                if used:
                    seg = y[np.asarray(starts)[:, None] + np.arange(L)[None, :]]
                    mu = np.cumsum(np.concatenate([np.zeros((used, 1)), seg], axis=1), axis=1)[:, -1] / float(L)
                    v = (seg - mu[:, None]) * w[None, :]
                    C, S = np.zeros((used, half + 1)), np.zeros((used, half + 1))
                    for i in range(L):
                        j = (kk * i) % N
                        C = C + v[:, i, None] * cs[j][None, :]
                        S = S + v[:, i, None] * sn[j][None, :]
                    acc = np.cumsum(np.concatenate([np.zeros((1, half + 1)), C * C + S * S], axis=0), axis=0)[-1]
                    psd[q, ch] = (g * acc) / ((float(used) * fps) * W2)
                per_seq[q, ch] = _spectrum_row(psd[q, ch], fps, N, f_lo, f_hi, ch < 3, int(ok.sum()), candidates, used)
            f0 += T
    out = {"psd": psd, "per_sequence": per_seq, "freqs": (np.arange(half + 1, dtype=np.float64) * fps) / float(N)}
    out.update(spectrum_rows(psd, per_seq, fps, f_lo, f_hi))
    return out


def gait_spectrum(joints3d, lengths=None, trans=None, exclude=None, fps=20.0, sigma=0.0, derivative=2, segment=64, hop=None, nfft=256, f_lo=0.5, f_hi=3.0,
                  min_segments=2, joints=GAIT_JOINTS_KINECTV2):
    """The Welch power spectral density of four body signals in numpy float64 (Welch 1967; Weiss et al. 2011 and Sejdic et al. 2014 on trunk
    accelerations; the rules: DESIGN 4.19; the defaults are unvalidated on the model's output, and the peak's width has a floor set by the segment
    length, not by the walker): the host statement of GRNet.gait_spectrum, same arguments, a dict of numpy arrays.  per_frame (n,4) is
    gait_regularity's at the same sigma; psd, per_sequence, freqs and spectral_entropy: gait_welch's."""
    if hop is None:
        hop = segment // 2 if int(segment) == segment else segment

    def rule_check():
        _spectrum_rule_check(fps, derivative, segment, hop, nfft, f_lo, f_hi, min_segments)
        _entropy_lengths_check(_sequence_lengths(np.asarray(joints3d).shape[0], lengths))
    lengths, per_frame = _regularity_signals(joints3d, lengths, trans, sigma, joints, rule_check)
    out = gait_welch(per_frame, lengths, exclude, fps, derivative, segment, hop, nfft, f_lo, f_hi, min_segments)
    out["per_frame"] = per_frame
    return out


# ----------------------------------------------------------------------------- movement smoothness
SMOOTHNESS_CHANNELS = REGULARITY_CHANNELS
SMOOTHNESS_SEGMENT_COLUMNS = ("start", "sparc", "k_first", "k_last", "peak_bin", "peak_magnitude", "dj", "v_peak")
SMOOTHNESS_COLUMNS = ("n", "candidates", "used", "defined", "sparc_mean", "sparc_sd", "sparc_min", "sparc_max", "last_hz_mean", "dj_defined")
SMOOTHNESS_MAX_FRAMES = ENTROPY_MAX_FRAMES


def _smoothness_rule_check(fps, derivative, segment, hop, nfft, f_cut, amplitude, min_segments):
    """The refusals of csrc/gait_smoothness.h's smo_rule_error, in its words and its order."""
    if not np.isfinite(fps) or not fps > 0:
        raise ValueError("fps must be positive and finite")
    if any(int(v) != v for v in (derivative, segment, hop, nfft, min_segments)):
        raise ValueError("derivative, segment, hop, nfft and min_segments must be whole numbers")
    _spectrum_rule_check(fps, derivative, segment, hop, segment, fps / 4.0, fps / 2.0, min_segments)
    if not segment <= nfft <= 4096 or nfft % 2:
        raise ValueError("nfft must be even and within [segment, 4096]")
    if not (np.isfinite(f_cut) and 0 < f_cut <= fps / 2.0):
        raise ValueError("f_cut must obey 0 < f_cut <= fps / 2")
    if not 0 < amplitude <= 1:
        raise ValueError("amplitude must be within (0, 1]")


def smoothness_slots(lengths, segment=64, hop=None):
    """The prefix sums of the slots of sequences of `lengths` frames lying back to back: a sequence of T frames has (T - segment) // hop + 1 slots, the
    most it can hold (0 where T < segment).  (n_seq + 1,) int64: grnet_gait_smoothness_slots' formula."""
    if hop is None:
        hop = segment // 2
    at = np.zeros(len(lengths) + 1, np.int64)
    at[1:] = np.cumsum([(int(T) - int(segment)) // int(hop) + 1 if int(T) >= int(segment) else 0 for T in lengths])
    return at


def _smoothness_row(rows, fps, nfft, n, candidates, used):
    """smo_row on Python floats: rows the (candidates, 8) slot rows of one (sequence, channel) in time order."""
    nan = float("nan")
    out = [float(n), float(candidates), float(used)] + [nan] * 7
    if used < 1:
        return out
    fps, N = float(fps), float(nfft)
    defined = dj_defined = 0
    S = H = lo = hi = 0.0
    for row in rows:
        sparc, last, dj = float(row[1]), float(row[3]), float(row[6])
        if math.isfinite(dj):
            dj_defined += 1
        if not math.isfinite(sparc):
            continue
        if defined == 0 or sparc < lo:
            lo = sparc
        if defined == 0 or sparc > hi:
            hi = sparc
        S = S + sparc
        H = H + (last * fps) / N
        defined += 1
    out[3], out[9] = float(defined), float(dj_defined)
    if defined < 1:
        return out
    mean, Q = S / float(defined), 0.0
    for row in rows:
        sparc = float(row[1])
        if math.isfinite(sparc):
            d = sparc - mean
            Q = Q + d * d
    out[4], out[5], out[6], out[7], out[8] = mean, math.sqrt(Q / float(defined)), lo, hi, H / float(defined)
    return out


def smoothness_rows(per_segment, per_sequence, slot_offsets):
    """Rule 8 of DESIGN 4.24, the one place where the logarithm is taken: per_segment (slots,4,8), per_sequence (n_seq,4,10) and slot_offsets
    (n_seq+1,), from the device or from gait_sparc -> {'ldlj': (slots,4) float64 = -ln(dj), the log dimensionless jerk of every slot, NaN where dj is
    not positive and finite; 'ldlj_mean', 'ldlj_sd': (n_seq,4) over a sequence's slots in time order from +0.0, the SD sqrt(sum d^2 / n); NaN where
    used is 0 or no slot has one}."""
    seg, rows, at = np.asarray(per_segment, np.float64), np.asarray(per_sequence, np.float64), np.asarray(slot_offsets, np.int64)
    if seg.ndim != 3 or seg.shape[1:] != (4, len(SMOOTHNESS_SEGMENT_COLUMNS)) or rows.ndim != 3 or rows.shape[1:] != (4, len(SMOOTHNESS_COLUMNS)):
        raise ValueError(f"per_segment must be (slots,4,{len(SMOOTHNESS_SEGMENT_COLUMNS)}) and per_sequence (n_seq,4,{len(SMOOTHNESS_COLUMNS)}), got {seg.shape} and {rows.shape}")
    if at.shape != (rows.shape[0] + 1,) or at[0] != 0 or at[-1] != seg.shape[0] or (np.diff(at) < 0).any():
        raise ValueError(f"slot_offsets must be the {rows.shape[0] + 1} prefix sums of per_segment's {seg.shape[0]} slots")
    ldlj = np.full(seg.shape[:2], np.nan)
    mean, sd = np.full(rows.shape[:2], np.nan), np.full(rows.shape[:2], np.nan)
    for s in range(seg.shape[0]):
        for ch in range(4):
            dj = float(seg[s, ch, 6])
            if dj > 0.0 and math.isfinite(dj):
                ldlj[s, ch] = -math.log(dj)
    for q in range(rows.shape[0]):
        for ch in range(4):
            if not rows[q, ch, 2] >= 1:
                continue
            have = [float(v) for v in ldlj[at[q]:at[q + 1], ch] if math.isfinite(v)]
            if not have:
                continue
            S = 0.0
            for v in have:
                S = S + v
            m, Q = S / float(len(have)), 0.0
            for v in have:
                Q = Q + (v - m) * (v - m)
            mean[q, ch], sd[q, ch] = m, math.sqrt(Q / float(len(have)))
    return {"ldlj": ldlj, "ldlj_mean": mean, "ldlj_sd": sd}


def gait_sparc(signals, lengths=None, exclude=None, fps=20.0, derivative=1, segment=64, hop=None, nfft=1024, f_cut=None, amplitude=0.05, min_segments=2):
    """Rules 1 (from the differencing on) to 8 of DESIGN 4.24 on given signals: the host statement of GRNet.op_gait_sparc.  signals (n,4) float64,
    columns SMOOTHNESS_CHANNELS; exclude (n,) or None: a frame whose entry is not 0 does not count; hop None: segment / 2; f_cut None: min(10, fps / 2).
    Returns {'per_segment': (slots,4,8), columns SMOOTHNESS_SEGMENT_COLUMNS, 'per_sequence': (n_seq,4,10), columns SMOOTHNESS_COLUMNS, 'slot_offsets':
    (n_seq+1,) int64, and smoothness_rows' 'ldlj', 'ldlj_mean', 'ldlj_sd'}.  Every sum in rising index from +0.0 (a cumulative sum, or one addition a
    loop turn), the twiddles harmonics_twiddles' at (k i) mod nfft."""
    x = np.asarray(signals, np.float64)
    if x.ndim != 2 or x.shape[1] != 4 or x.shape[0] < 1:
        raise ValueError(f"signals must be (n,4) with n >= 1, got {x.shape}")
    n = x.shape[0]
    lengths = _sequence_lengths(n, lengths)
    ex = None
    if exclude is not None:
        ex = np.asarray(exclude)
        if ex.shape != (n,):
            raise ValueError(f"exclude must be ({n},), got {ex.shape}")
    if hop is None:
        hop = segment // 2 if int(segment) == segment else segment
    if f_cut is None:
        f_cut = min(10.0, float(fps) / 2.0)
    _smoothness_rule_check(fps, derivative, segment, hop, nfft, f_cut, amplitude, min_segments)
    _entropy_lengths_check(lengths)
    fps, d, L, hop, N, min_segments, amplitude = float(fps), int(derivative), int(segment), int(hop), int(nfft), int(min_segments), float(amplitude)
    freqs = (np.arange(N // 2 + 1, dtype=np.float64) * fps) / float(N)
    kc = int(np.flatnonzero(freqs <= f_cut)[-1])
    sn, cs = harmonics_twiddles(N)
    kk = np.arange(kc + 1, dtype=np.int64)
    l1 = float(L - 1)
    cube = (l1 * l1) * l1
    at = smoothness_slots(lengths, L, hop)
    per_seg = np.full((int(at[-1]), 4, len(SMOOTHNESS_SEGMENT_COLUMNS)), np.nan)
    per_seq = np.full((len(lengths), 4, len(SMOOTHNESS_COLUMNS)), np.nan)
    f0 = 0
    with np.errstate(all="ignore"):
        for q, T in enumerate(lengths):
            for ch in range(4):
                s = x[f0:f0 + T, ch]
                valid = np.isfinite(s)
                if ex is not None:
                    valid &= ex[f0:f0 + T] == 0
                y = np.where(valid, s, np.nan)
                for _ in range(d):
                    y = np.concatenate([y[1:] - y[:-1], [np.nan]])
                y[~np.isfinite(y)] = np.nan
                ok = np.isfinite(y)
                edges = np.flatnonzero(np.diff(np.concatenate([[False], ok, [False]]).astype(np.int8)))
                starts = [t0 for a, e in zip(edges[0::2], edges[1::2]) for t0 in range(int(a), int(e) - L + 1, hop)]
                candidates = len(starts)
                used = candidates if candidates >= min_segments else 0
                rows = per_seg[at[q]:at[q] + candidates, ch]
                if candidates:
                    seg = y[np.asarray(starts)[:, None] + np.arange(L)[None, :]]
                    C, S = np.zeros((candidates, kc + 1)), np.zeros((candidates, kc + 1))
                    for i in range(L):
                        j = (kk * i) % N
                        C = C + seg[:, i, None] * cs[j][None, :]
                        S = S + seg[:, i, None] * sn[j][None, :]
                    M = np.sqrt(C * C + S * S)
                for e, t0 in enumerate(starts):
                    rows[e, 0] = float(t0)
                    peak = int(np.argmax(np.where(np.isnan(M[e]), -1.0, M[e])))      # the largest, at the smallest k of a tie; a NaN is never it
                    top = float(M[e, peak])
                    if not (top > 0.0 and math.isfinite(top)):
                        continue
                    m = M[e] / top
                    band = np.flatnonzero(m >= amplitude)
                    ka, kb = int(band[0]), int(band[-1])
                    sparc = 0.0
                    if kb > ka:
                        u = 1.0 / float(kb - ka)
                        step = m[ka + 1:kb + 1] - m[ka:kb]
                        sparc = 0.0 - float(np.cumsum(np.concatenate([[0.0], np.sqrt(u * u + step * step)]))[-1])
                    xs = s[t0:t0 + L]
                    v_peak = float(np.max(np.abs(xs[1:] - xs[:-1])))
                    jerk = ((xs[3:] - 3.0 * xs[2:-1]) + 3.0 * xs[1:-2]) - xs[:-3]
                    J = float(np.cumsum(np.concatenate([[0.0], jerk * jerk]))[-1])
                    dj = (J * cube) / (v_peak * v_peak) if v_peak > 0.0 else float("nan")
                    rows[e, 1:] = (sparc, float(ka), float(kb), float(peak), top, dj, v_peak)
                per_seq[q, ch] = _smoothness_row(rows, fps, N, int(ok.sum()), candidates, used)
            f0 += T
    out = {"per_segment": per_seg, "per_sequence": per_seq, "slot_offsets": at}
    out.update(smoothness_rows(per_seg, per_seq, at))
    return out


def gait_smoothness(joints3d, lengths=None, trans=None, exclude=None, fps=20.0, sigma=0.0, derivative=1, segment=64, hop=None, nfft=1024, f_cut=None,
                    amplitude=0.05, min_segments=2, joints=GAIT_JOINTS_KINECTV2):
    """Movement smoothness of four body signals in numpy float64: the spectral arc length and the dimensionless jerk of every segment (Balasubramanian
    et al. 2015; on gait Beck et al. 2018; the rules: DESIGN 4.24).  THE INPUTS ARE JOINT POSITIONS OF A POSE MODEL AT 20 FPS, where the cut-off of
    10 Hz is the Nyquist frequency; A SEGMENT'S RECTANGULAR WINDOW ALONE gives a noiseless sinusoid SPARC = -3.96 +- 0.30 at 64 frames; with 5 mm of
    joint noise a good part of the number is the noise; THE DEFAULTS ARE UNVALIDATED on the model's output.  The host statement of
    GRNet.gait_smoothness, same arguments, a dict of numpy arrays.  per_frame (n,4) is gait_regularity's at the same sigma; the rest is gait_sparc's."""
    if hop is None:
        hop = segment // 2 if int(segment) == segment else segment
    if f_cut is None:
        f_cut = min(10.0, float(fps) / 2.0)

    def rule_check():
        _smoothness_rule_check(fps, derivative, segment, hop, nfft, f_cut, amplitude, min_segments)
        _entropy_lengths_check(_sequence_lengths(np.asarray(joints3d).shape[0], lengths))
    lengths, per_frame = _regularity_signals(joints3d, lengths, trans, sigma, joints, rule_check)
    out = gait_sparc(per_frame, lengths, exclude, fps, derivative, segment, hop, nfft, f_cut, amplitude, min_segments)
    out["per_frame"] = per_frame
    return out


# ----------------------------------------------------------------------------- arm swing and inter-limb coordination
COORDINATION_CHANNELS = ("arm_left", "arm_right", "leg_left", "leg_right")      # gait_kinematics's channels 8, 9, 0, 1: shoulder and hip flexion
COORDINATION_KINEMATICS_COLUMNS = (8, 9, 0, 1)
COORDINATION_PAIRS = ((0, 1), (2, 3), (0, 3), (1, 2), (0, 2), (1, 3))
COORDINATION_PAIR_NAMES = ("arm_left__arm_right", "leg_left__leg_right", "arm_left__leg_right", "arm_right__leg_left", "arm_left__leg_left",
                           "arm_right__leg_right")
COORDINATION_EXPECTED_PHASE = (180.0, 180.0, 0.0, 0.0, 180.0, 180.0)          # degrees: an arm swings with the other side's leg
COORDINATION_LIMB_COLUMNS = SPECTRUM_COLUMNS
COORDINATION_PAIR_COLUMNS = ("used", "peak_bin", "peak_hz", "cross_amplitude", "coherence_peak", "phase_peak", "phase_deviation", "lag_seconds",
                             "coherence_band", "coherence_bins")
COORDINATION_ROWS = ("amplitude", "arm_asymmetry", "leg_asymmetry", "arm_leg_ratio", "phase_deviation_mean")
COORDINATION_MAX_FRAMES = ENTROPY_MAX_FRAMES


def _coordination_rule_check(fps, derivative, segment, hop, nfft, f_lo, f_hi, min_segments):
    """The refusals of csrc/gait_coordination.h's coord_rule_error, in its words: spec_rule_error's, and one segment is refused."""
    _spectrum_rule_check(fps, derivative, segment, hop, nfft, f_lo, f_hi, 2)
    if int(min_segments) != min_segments:
        raise ValueError("derivative, segment, hop, nfft and min_segments must be whole numbers")
    if not 2 <= min_segments <= 2 ** 20:
        raise ValueError("min_segments outside [2, 2^20]")


def _coordination_pair_row(Paa, Pbb, Re, Im, fps, nfft, f_lo, f_hi, antiphase, used):
    """coord_pair_row on Python floats, one operation at a time in the header's order."""
    nan = float("nan")
    out = [float(used)] + [nan] * 9
    if used < 1:
        return out
    fps, N = float(fps), float(nfft)
    k_lo, k_hi = _spectrum_band(fps, nfft, f_lo, f_hi)
    best, bins, top, total = -1, 0, 0.0, 0.0
    for k in range(k_lo, k_hi + 1):
        re, im = float(Re[k]), float(Im[k])
        m2, den = re * re + im * im, float(Paa[k]) * float(Pbb[k])
        if m2 > 0.0 and math.isfinite(m2) and (best < 0 or m2 > top):
            best, top = k, m2
        if den > 0.0 and math.isfinite(den):
            total = total + m2 / den
            bins += 1
    if best < 0:
        return out
    hz, den = (float(best) * fps) / N, float(Paa[best]) * float(Pbb[best])
    phase = float(gait_atan2(float(Im[best]), float(Re[best]))) * KINEMATICS_DEGREES
    out[1], out[2], out[3] = float(best), hz, math.sqrt(top)
    if den > 0.0 and math.isfinite(den):
        out[4] = top / den
    out[5] = phase
    out[6] = abs(180.0 - abs(phase)) if antiphase else abs(phase)
    out[7] = phase / (360.0 * hz)
    if bins > 0:
        out[8] = total / float(bins)
    out[9] = float(bins)
    return out


def coordination_rows(limbs, pairs):
    """Rule 8 of DESIGN 4.21, the one function the device path and the host path call: limbs (..., 4, 13) and pairs (..., 6, 10), from the device or
    from gait_cross_welch -> {'amplitude': (..., 4) = sqrt(2 band_power), the amplitude of the sinusoid with the band's power (degrees at derivative
    0); 'arm_asymmetry', 'leg_asymmetry': (...) = 100 |L - R| / (0.5 (L + R)); 'arm_leg_ratio': (...) = (0.5 (arm_left + arm_right)) / (0.5
    (leg_left + leg_right)); 'phase_deviation_mean': (...) over the pairs whose phase_deviation is defined}.  NaN where a denominator is not positive."""
    L, P = np.asarray(limbs, np.float64), np.asarray(pairs, np.float64)
    if L.ndim < 2 or L.shape[-2:] != (4, len(COORDINATION_LIMB_COLUMNS)) or P.shape != L.shape[:-2] + (6, len(COORDINATION_PAIR_COLUMNS)):
        raise ValueError(f"limbs must be (..., 4, 13) and pairs (..., 6, 10) of the same sequences, got {L.shape} and {P.shape}")
    lead = L.shape[:-2]
    flat_l, flat_p = L.reshape(-1, 4, L.shape[-1]), P.reshape(-1, 6, P.shape[-1])
    n = flat_l.shape[0]
    amp, arm, leg, ratio, dev = np.full((n, 4), np.nan), np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    for e in range(n):
        a = [math.sqrt(2.0 * float(v)) if float(v) >= 0.0 else float("nan") for v in flat_l[e, :, 3]]
        amp[e] = a
        den_arm, den_leg = 0.5 * (a[0] + a[1]), 0.5 * (a[2] + a[3])
        if den_arm > 0.0:
            arm[e] = (100.0 * abs(a[0] - a[1])) / den_arm
        if den_leg > 0.0:
            leg[e] = (100.0 * abs(a[2] - a[3])) / den_leg
            ratio[e] = den_arm / den_leg
        total, count = 0.0, 0
        for v in flat_p[e, :, 6].tolist():
            if not math.isnan(v):
                total, count = total + v, count + 1
        if count > 0:
            dev[e] = total / float(count)
    return {"amplitude": amp.reshape(lead + (4,)), "arm_asymmetry": arm.reshape(lead), "leg_asymmetry": leg.reshape(lead), "arm_leg_ratio": ratio.reshape(lead),
            "phase_deviation_mean": dev.reshape(lead)}


def gait_cross_welch(signals, lengths=None, exclude=None, fps=20.0, derivative=0, segment=64, hop=None, nfft=256, f_lo=0.5, f_hi=3.0, min_segments=4):
    """Rules 2 to 8 of DESIGN 4.21 on given signals: the host statement of GRNet.op_gait_cross_welch.  signals (n,4) float64, columns
    COORDINATION_CHANNELS; exclude (n,) or None: a frame whose entry is not 0 does not count; hop None: segment / 2.  A frame counts iff all four
    differenced values are finite: ONE mask, so every limb and every pair is estimated on the same segments.  Returns {'auto': (n_seq,4,nfft/2+1)
    densities, 'cross': (n_seq,6,nfft/2+1,2) real and imaginary part of conj(X_a) X_b (scipy.signal.csd(a, b)'s sign: a positive phase means b leads
    a) of COORDINATION_PAIRS, 'limbs': (n_seq,4,13), columns COORDINATION_LIMB_COLUMNS, 'pairs': (n_seq,6,10), columns COORDINATION_PAIR_COLUMNS,
    'freqs': (nfft/2+1,), and coordination_rows' values}.  Every sum in rising index from +0.0, the twiddles harmonics_twiddles' at (k i) mod nfft."""
    x = np.asarray(signals, np.float64)
    if x.ndim != 2 or x.shape[1] != 4 or x.shape[0] < 1:
        raise ValueError(f"signals must be (n,4) with n >= 1, got {x.shape}")
    n = x.shape[0]
    lengths = _sequence_lengths(n, lengths)
    ex = None
    if exclude is not None:
        ex = np.asarray(exclude)
        if ex.shape != (n,):
            raise ValueError(f"exclude must be ({n},), got {ex.shape}")
    if hop is None:
        hop = segment // 2 if int(segment) == segment else segment
    _coordination_rule_check(fps, derivative, segment, hop, nfft, f_lo, f_hi, min_segments)
    _entropy_lengths_check(lengths)
    fps, d, L, hop, N, min_segments = float(fps), int(derivative), int(segment), int(hop), int(nfft), int(min_segments)
    half = N // 2
    sn, cs = harmonics_twiddles(N)
    w = 0.5 - 0.5 * harmonics_twiddles(L)[1]
    W2 = float(np.cumsum(np.concatenate([[0.0], w * w]))[-1])
    kk = np.arange(half + 1, dtype=np.int64)
    g = np.where((kk > 0) & (kk < half), 2.0, 1.0)
    n_seq = len(lengths)
    auto, cross = np.full((n_seq, 4, half + 1), np.nan), np.full((n_seq, 6, half + 1, 2), np.nan)
    limbs, pairs = np.full((n_seq, 4, len(COORDINATION_LIMB_COLUMNS)), np.nan), np.full((n_seq, 6, len(COORDINATION_PAIR_COLUMNS)), np.nan)

    def total(values):
        return np.cumsum(np.concatenate([np.zeros((1, half + 1)), values], axis=0), axis=0)[-1]
    f0 = 0
    with np.errstate(all="ignore"):
        for q, T in enumerate(lengths):
            ys = []
            for ch in range(4):
                s = x[f0:f0 + T, ch]
                valid = np.isfinite(s)
                if ex is not None:
                    valid &= ex[f0:f0 + T] == 0
                y = np.where(valid, s, np.nan)
                for _ in range(d):
                    y = np.concatenate([y[1:] - y[:-1], [np.nan]])
                ys.append(y)
            ok = np.isfinite(ys[0]) & np.isfinite(ys[1]) & np.isfinite(ys[2]) & np.isfinite(ys[3])
            edges = np.flatnonzero(np.diff(np.concatenate([[False], ok, [False]]).astype(np.int8)))
            starts = [t0 for a, e in zip(edges[0::2], edges[1::2]) for t0 in range(int(a), int(e) - L + 1, hop)]
            candidates = len(starts)
            used = candidates if candidates >= min_segments else 0
            if used:
                C, S = [], []
                for ch in range(4):
                    seg = ys[ch][np.asarray(starts)[:, None] + np.arange(L)[None, :]]
                    mu = np.cumsum(np.concatenate([np.zeros((used, 1)), seg], axis=1), axis=1)[:, -1] / float(L)
                    v = (seg - mu[:, None]) * w[None, :]
                    Cc, Sc = np.zeros((used, half + 1)), np.zeros((used, half + 1))
                    for i in range(L):
                        j = (kk * i) % N
                        Cc = Cc + v[:, i, None] * cs[j][None, :]
                        Sc = Sc + v[:, i, None] * sn[j][None, :]
                    C.append(Cc)
                    S.append(Sc)
                    auto[q, ch] = (g * total(Cc * Cc + Sc * Sc)) / ((float(used) * fps) * W2)
                for p, (a, b) in enumerate(COORDINATION_PAIRS):
                    cross[q, p, :, 0] = (g * total(C[a] * C[b] + S[a] * S[b])) / ((float(used) * fps) * W2)
                    cross[q, p, :, 1] = (g * total(S[a] * C[b] - C[a] * S[b])) / ((float(used) * fps) * W2)
            for ch in range(4):
                limbs[q, ch] = _spectrum_row(auto[q, ch], fps, N, f_lo, f_hi, True, int(ok.sum()), candidates, used)
            for p, (a, b) in enumerate(COORDINATION_PAIRS):
                pairs[q, p] = _coordination_pair_row(auto[q, a], auto[q, b], cross[q, p, :, 0], cross[q, p, :, 1], fps, N, f_lo, f_hi,
                                                     COORDINATION_EXPECTED_PHASE[p] == 180.0, used)
            f0 += T
    out = {"auto": auto, "cross": cross, "limbs": limbs, "pairs": pairs, "freqs": (np.arange(half + 1, dtype=np.float64) * fps) / float(N)}
    out.update(coordination_rows(limbs, pairs))
    return out


def _coordination_signals(joints3d, lengths, sigma, joints, rule_check):
    """(the sequences' lengths, per_frame (n,4)) of gait_coordination: rule 1 of DESIGN 4.21, gait_kinematics's operations for its channels 8, 9, 0
    and 1 alone.  rule_check() refuses the caller's own scalars, behind the joint table and before sigma, as the C ABI does."""
    j3 = _widened(joints3d, "joints3d")
    n, J = j3.shape[:2]
    lengths = _sequence_lengths(n, lengths)
    tab = _joint_table(joints, 16, J, _KIN_JOINT_NAMES)
    rule_check()
    _sigma_check(sigma)
    p = [j3[:, i] for i in tab]
    per_frame = np.full((n, 4), np.nan)
    with np.errstate(all="ignore"):
        l, u = p[2] - p[3], p[1] - p[0]
        c = _kin_cross(l, u)
        nc, nl = np.sqrt(_kin_dot(c, c)), np.sqrt(_kin_dot(l, l))
        valid = (nc > 0) & np.isfinite(nc) & (nl > 0) & np.isfinite(nl)
        f, side = c / np.where(valid, nc, 1.0)[:, None], l / np.where(valid, nl, 1.0)[:, None]
        w = _kin_cross(f, side)
        for s in (0, 1):
            d, arm = p[4 + s] - p[2 + s], p[12 + s] - p[10 + s]
            per_frame[:, 0 + s] = np.where(valid, gait_atan2(_kin_dot(arm, f), -_kin_dot(arm, w)) * KINEMATICS_DEGREES, np.nan)
            per_frame[:, 2 + s] = np.where(valid, gait_atan2(_kin_dot(d, f), -_kin_dot(d, w)) * KINEMATICS_DEGREES, np.nan)
        if sigma > 0:
            a = 0
            for T in lengths:
                for k in range(4):
                    per_frame[a:a + T, k] = gauss_filter1d(per_frame[a:a + T, k].copy(), sigma)
                a += T
    return lengths, per_frame


def gait_coordination(joints3d, lengths=None, exclude=None, fps=20.0, sigma=0.0, derivative=0, segment=64, hop=None, nfft=256, f_lo=0.5, f_hi=3.0,
                      min_segments=4, joints=KINEMATICS_JOINTS_KINECTV2):
    """Arm swing and inter-limb coordination in numpy float64 (Carter, Knapp and Nuttall 1973 on the coherence by Welch's segments; Wagenaar and van
    Emmerik 2000, Plotnik et al. 2007 and Mirelman et al. 2016 on arms and legs in gait; the rules: DESIGN 4.21): the host statement of
    GRNet.gait_coordination, same arguments, a dict of numpy arrays.  per_frame (n,4): shoulder flexion left / right and hip flexion left / right in
    degrees, the bits of gait_kinematics's per_frame[:, (8, 9, 0, 1)] at the same sigma; auto, cross, limbs, pairs, freqs and the host rows:
    gait_cross_welch's.  The signals are joint-position angles of a pose model over some 15 strides: with K segments the coherence of two unrelated
    signals is about 1 / K (0.09 at the 11 segments of 400 frames), not 0.  The defaults are unvalidated on the model's output; the numbers are
    reported, never judged."""
    if hop is None:
        hop = segment // 2 if int(segment) == segment else segment

    def rule_check():
        _coordination_rule_check(fps, derivative, segment, hop, nfft, f_lo, f_hi, min_segments)
        _entropy_lengths_check(_sequence_lengths(np.asarray(joints3d).shape[0], lengths))
    lengths, per_frame = _coordination_signals(joints3d, lengths, sigma, joints, rule_check)
    out = gait_cross_welch(per_frame, lengths, exclude, fps, derivative, segment, hop, nfft, f_lo, f_hi, min_segments)
    out["per_frame"] = per_frame
    return out


# ----------------------------------------------------------------------------- footprints, centre of mass and margin of stability
# BALANCE_SEGMENTS_KINECTV2 (imported above): rows of (proximal joint, distal joint, mass, the COM's fraction from the proximal joint)
BALANCE_FRAME_COLUMNS = ("com_x", "com_y", "com_z", "path_x", "path_y", "path_z", "stance_side", "chain")
BALANCE_STEP_COLUMNS = ("t1", "t2", "landing_side", "chain", "footprint_x", "footprint_y", "footprint_z", "stride_length", "step_length", "step_width",
                        "com_speed", "mos_ap", "mos_ml", "vertical_excursion", "lateral_excursion")
BALANCE_COLUMNS = ("strikes", "steps", "chains", "strides", "stride_length_mean", "stride_length_sd", "step_length_mean", "step_length_sd",
                   "step_width_mean", "step_width_sd", "step_length_asymmetry", "com_speed_mean", "com_speed_sd", "ground_speed", "mos_ap_mean",
                   "mos_ap_sd", "mos_ml_mean", "mos_ml_sd", "mos_ml_left", "mos_ml_right", "vertical_excursion_mean", "vertical_excursion_sd",
                   "lateral_excursion_mean", "lateral_excursion_sd")


def _balance_rule_check(fps, gravity, window, settle, max_step, max_steps):
    if not np.isfinite(fps) or not fps > 0:
        raise ValueError("fps must be positive and finite")
    if not np.isfinite(gravity) or not gravity > 0:
        raise ValueError("gravity must be positive and finite")
    if int(window) != window or int(settle) != settle or int(max_step) != max_step or int(max_steps) != max_steps:
        raise ValueError("window, settle, max_step and max_steps must be whole numbers")
    if not 1 <= window <= 16:
        raise ValueError(f"window {window} outside [1, 16]")
    if not 0 <= settle <= 4:
        raise ValueError(f"settle {settle} outside [0, 4]")
    if max_step < 1:
        raise ValueError(f"max_step {max_step} < 1")
    if not 1 <= max_steps <= 1024:
        raise ValueError(f"max_steps {max_steps} outside [1, 1024]")


def _balance_segments(segments, J):
    """(proximal (n_seg,), distal (n_seg,), mass (n_seg,), fraction (n_seg,)) of a segment table, checked as the C ABI checks it."""
    seg = np.asarray(segments, np.float64)
    if seg.ndim != 2 or seg.shape[1] != 4 or not 1 <= seg.shape[0] <= 16:
        raise ValueError(f"segments must be 1 to 16 rows of (proximal joint, distal joint, mass, fraction), got shape {seg.shape}")
    idx = seg[:, :2]
    if not np.array_equal(idx, np.floor(idx)) or idx.min() < 0 or idx.max() >= J:
        raise ValueError(f"a segment joint lies outside [0, {J})")
    if not (np.isfinite(seg[:, 2]).all() and (seg[:, 2] > 0).all()):
        raise ValueError("a segment mass is not positive and finite")
    if not np.isfinite(seg[:, 3]).all():
        raise ValueError("a segment fraction is not finite")
    return idx[:, 0].astype(np.int64), idx[:, 1].astype(np.int64), seg[:, 2], seg[:, 3]


def balance_table_com(j3, segments=BALANCE_SEGMENTS_KINECTV2):
    """Rule 1 of DESIGN 4.22 alone: the centre of mass (n,3) float64 of widened joints j3 (n,J,3) from a segment table."""
    n, J = j3.shape[:2]
    prox, dist, mass, frac = _balance_segments(segments, J)
    with np.errstate(all="ignore"):
        num, den = np.zeros((n, 3)), 0.0
        for i in range(len(mass)):
            P, Dj = j3[:, prox[i]], j3[:, dist[i]]
            num = num + mass[i] * (P + frac[i] * (Dj - P))
            den = den + mass[i]
        return num / den


def gait_balance_steps(rel, events, lengths=None, fps=20.0, gravity=9.81, window=4, settle=1, max_step=30, max_steps=256):
    """Rules 2 to 8 of DESIGN 4.22 on given rel (n,9) float64 = [c, rL, rR]: the host statement of GRNet.op_gait_balance_steps.  events (n,) as
    gait_parameters returned them (bits 0 and 1 are read).  Returns {'per_frame': (n,8), columns BALANCE_FRAME_COLUMNS, 'steps': (n_seq,max_steps,15),
    columns BALANCE_STEP_COLUMNS, 'per_sequence': (n_seq,24), columns BALANCE_COLUMNS}; every sum in the stated order from +0.0, every comparison false
    for NaN.  The pairs of a sequence are handled side by side, the footprints are np.cumsum (one addition after the other) along each chain."""
    x = np.asarray(rel, np.float64)
    if x.ndim != 2 or x.shape[1] != 9 or x.shape[0] < 1:
        raise ValueError(f"rel must be (n,9) with n >= 1, got {x.shape}")
    n = x.shape[0]
    ev = np.asarray(events)
    if ev.shape != (n,):
        raise ValueError(f"events must be ({n},), got {ev.shape}")
    ev = ev.astype(np.int64) & (GAIT_HEEL_L | GAIT_HEEL_R)
    lengths = _sequence_lengths(n, lengths)
    _balance_rule_check(fps, gravity, window, settle, max_step, max_steps)
    fps, gravity, w, settle, max_step, max_steps = float(fps), float(gravity), int(window), int(settle), int(max_step), int(max_steps)
    per_frame = np.full((n, 8), np.nan)
    per_frame[:, :3] = x[:, :3]
    per_frame[:, 6] = 0.0
    steps = np.full((len(lengths), max_steps, 15), np.nan)
    per_seq = np.full((len(lengths), 24), np.nan)
    k = np.arange(w + 1, dtype=np.float64) - w / 2.0
    D = _gait_sum(k * k)
    f0 = 0
    with np.errstate(all="ignore"):
        for q, T in enumerate(lengths):
            r, e, out = x[f0:f0 + T], ev[f0:f0 + T], per_frame[f0:f0 + T]
            R = np.stack([r[:, 3:6], r[:, 6:9]])                # R[0] = rL, R[1] = rR
            bad = np.concatenate([np.zeros((2, 1), np.int64), np.cumsum(~np.isfinite(R).all(axis=2), axis=1)], axis=1)
            marks = np.flatnonzero(e)
            feet = e[marks]
            t1, t2, X, Y = marks[:-1], marks[1:], feet[:-1], feet[1:]
            ok = (X != 3) & (Y != 3) & (X != Y) & (t2 - t1 >= w) & (t2 - t1 <= max_step) & (t2 + settle <= T - 1)
            ix, iy, tb = (X == GAIT_HEEL_R).astype(np.int64), (Y == GAIT_HEEL_R).astype(np.int64), np.minimum(t2 + settle, T - 1)
            ok &= bad[ix, t2 + 1] - bad[ix, t1] == 0
            b = R[ix, tb] - R[iy, tb]
            ok &= np.isfinite(b).all(axis=1)
            N = np.zeros((len(t1), 3))
            for i in range(w + 1):
                N = N + k[i] * R[ix, np.maximum(t2 - w + i, 0)]
            v = (N / D) * fps
            sp = np.sqrt(v[:, 0] * v[:, 0] + v[:, 2] * v[:, 2])
            ok &= (sp > 0) & np.isfinite(sp)
            ax, az = v[:, 0] / sp, v[:, 2] / sp
            lx, lz = -az, ax
            at2 = R[ix, t2]
            ell = -at2[:, 1]
            ok &= ell > 0
            w0 = np.sqrt(gravity / ell)
            dx, dz = b[:, 0] - (at2[:, 0] + v[:, 0] / w0), b[:, 2] - (at2[:, 2] + v[:, 2] / w0)
            sY = np.where(Y == GAIT_HEEL_L, 1.0, -1.0)
            ap, ml = dx * ax + dz * az, sY * (dx * lx + dz * lz)
            rows, chain = [], -1                               # every step's 15 columns in time order
            for a, behind in _turn_runs_of(ok):                # a chain: a maximal run of consecutive pairs that are steps
                chain += 1
                m = behind - a
                G = np.cumsum(np.concatenate([np.zeros((1, 3)), b[a:behind]]), axis=0)      # G_0 .. G_m
                table = np.full((m, 15), np.nan)
                table[:, 0], table[:, 1], table[:, 2], table[:, 3], table[:, 4:7] = t1[a:behind], t2[a:behind], sY[a:behind], chain, G[1:]
                table[:, 10], table[:, 11], table[:, 12] = sp[a:behind], ap[a:behind], ml[a:behind]
                qx, qz = G[2:, 0] - G[:-2, 0], G[2:, 2] - G[:-2, 2]
                L = np.sqrt(qx * qx + qz * qz)
                has = L > 0
                px, pz = qx / L, qz / L
                bx, bz = b[a + 1:behind, 0], b[a + 1:behind, 2]
                table[1:, 7] = np.where(has, L, np.nan)
                table[1:, 8] = np.where(has, bx * px + bz * pz, np.nan)
                table[1:, 9] = np.where(has, np.abs(bx * (-pz) + bz * px), np.nan)
                for j in range(m):
                    foot, lo, hi = ix[a + j], t1[a + j], t2[a + j]
                    out[lo:hi + 1, 3:6] = G[j] + R[foot, lo:hi + 1]                # a later step overwrites the frame it shares: the largest t1
                    out[lo:hi + 1, 6], out[lo:hi + 1, 7] = -sY[a + j], chain
                    if j >= 1:
                        W = np.concatenate([G[j - 1] + R[ix[a + j - 1], t1[a + j - 1]:lo], G[j] + R[foot, lo:hi + 1]])
                        table[j, 13] = (W[:, 1].max() - W[:, 1].min()) + 0.0       # + 0.0: a spread of zeros of either sign is +0.0
                        if has[j - 1]:
                            lat = (W[:, 0] - G[j - 1, 0]) * (-pz[j - 1]) + (W[:, 2] - G[j - 1, 2]) * px[j - 1]
                            table[j, 14] = (lat.max() - lat.min()) + 0.0
                rows.extend(table)
            rows = np.asarray(rows).reshape(-1, 15)
            steps[q, :min(len(rows), max_steps)] = rows[:max_steps]
            row = per_seq[q]
            row[0], row[1], row[2] = np.count_nonzero(feet != 3), len(rows), chain + 1
            row[3] = np.count_nonzero(~np.isnan(rows[:, 7]))
            for col, src in zip((4, 6, 8, 11, 14, 16, 20, 22), (7, 8, 9, 10, 11, 12, 13, 14)):
                values = rows[:, src]
                row[col], row[col + 1] = _gait_mean_sd(values[~np.isnan(values)])
            side = []
            for src in (8, 12):
                for sign in (1.0, -1.0):
                    values = rows[rows[:, 2] == sign, src]
                    values = values[~np.isnan(values)]
                    side.append(_gait_sum(values) / len(values) if len(values) else np.nan)
            if not np.isnan(side[0]) and not np.isnan(side[1]):
                row[10] = (100.0 * abs(side[0] - side[1])) / (0.5 * (side[0] + side[1]))
            row[18], row[19] = side[2], side[3]
            if len(rows):
                bs = b[ok]
                row[13] = _gait_sum(np.sqrt(bs[:, 0] * bs[:, 0] + bs[:, 2] * bs[:, 2])) / _gait_sum((rows[:, 1] - rows[:, 0]) / fps)
            f0 += T
    return {"per_frame": per_frame, "steps": steps, "per_sequence": per_seq}


def gait_balance(joints3d, events, lengths=None, fps=20.0, gravity=9.81, window=4, settle=1, max_step=30, max_steps=256,
                 segments=None, joints=GAIT_JOINTS_KINECTV2, com=None):
    """Footprints on the floor, the centre of mass over them and the margin of stability at foot placement from 3D joints in numpy float64 (Hof, Gagey
    and Halbertsma 2005; Winter 2009; the rules: DESIGN 4.22): the host statement of GRNet.gait_balance, same arguments, a dict of numpy arrays -- the
    same operations in the same order.  joints3d (n,J,3) as gait_parameters takes them; events: its events; joints: its table, of which the two
    ankles are read; segments: rows of (proximal joint, distal joint, mass, fraction).  THE FLOOR IS THE x-z PLANE OF A LEVEL, FIXED CAMERA; the
    segment layout is unvalidated; the numbers are reported, never judged.  Also returns 'rel' (n,9) = [c, rL, rR].  segments: None stands for
    BALANCE_SEGMENTS_KINECTV2.  com (n,3) float64: the centre of mass of every frame in place of the segment table's (the mesh's, DESIGN 4.25: columns
    1 to 3 of mesh_moments' rows); together with segments it is refused."""
    j3 = _widened(joints3d, "joints3d")
    n, J = j3.shape[:2]
    lengths = _sequence_lengths(n, lengths)
    tab = _joint_table(joints, 8, J, _GAIT_JOINT_NAMES)
    _balance_rule_check(fps, gravity, window, settle, max_step, max_steps)
    if com is not None:
        if segments is not None:
            raise ValueError("segments and com are two sources of the centre of mass: give one")
        c = np.asarray(com, np.float64)
        if c.shape != (n, 3):
            raise ValueError(f"com must be ({n},3), got {c.shape}")
    else:
        c = balance_table_com(j3, BALANCE_SEGMENTS_KINECTV2 if segments is None else segments)
    with np.errstate(all="ignore"):
        rel = np.concatenate([c, c - j3[:, tab[4]], c - j3[:, tab[5]]], axis=1)
    out = gait_balance_steps(rel, events, lengths, fps, gravity, window, settle, max_step, max_steps)
    out["rel"] = rel
    return out


# ----------------------------------------------------------------------------- mesh volume, centre of mass and second moments
MESH_MOMENT_COLUMNS = ("volume", "com_x", "com_y", "com_z", "c_xx", "c_yy", "c_zz", "c_xy", "c_xz", "c_yz", "area")
MESH_COLUMNS = 1024                                              # NCOL of rule 3
_MESH_SECOND = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
BODY_COLUMNS = ("frames", "frames_valid", "volume_mean", "volume_sd", "volume_cv", "mass", "area_mean", "gyration_x_mean", "gyration_y_mean",
                "gyration_z_mean", "com_offset_x_mean", "com_offset_y_mean", "com_offset_z_mean", "com_distance_mean", "com_distance_max")
BODY_DENSITY = 985.0                                             # kg / m^3: a whole-body textbook figure, an assumption


def _faces_table(faces, V=None):
    f = np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3 or f.dtype.kind not in "iu":
        raise ValueError(f"faces must be an integer (F,3) table, got {f.dtype} {f.shape}")
    if f.shape[0] < 1:
        raise ValueError(f"n_faces {f.shape[0]} < 1")
    f = f.astype(np.int64)
    if V is not None:
        bad = np.flatnonzero((f.reshape(-1) < 0) | (f.reshape(-1) >= V))
        if bad.size:
            raise ValueError(f"face {bad[0] // 3} names vertex {f.reshape(-1)[bad[0]]}, outside [0, {V})")
    return f


def faces_closed(faces, V=netspec.NUM_VERTS):
    """Rule 5 of DESIGN 4.25, the host statement of GRNet.faces_closed: how many of the 3 F directed edges (i, j) of an (F,3) table share their
    pair with another edge, have no reverse edge (j, i), or join a vertex to itself.  0: a closed, consistently oriented surface."""
    f = _faces_table(faces, V)
    i, j = f.reshape(-1), np.roll(f, -1, axis=1).reshape(-1)
    keys, back = i * V + j, j * V + i
    uniq, counts = np.unique(keys, return_counts=True)
    twice = counts[np.searchsorted(uniq, keys)] > 1
    at = np.minimum(np.searchsorted(uniq, back), len(uniq) - 1)
    answered = (uniq[at] == back) & (i != j)
    return int(np.count_nonzero(twice | ~answered))


def mesh_face_terms(a, b, c):
    """Rule 2 of DESIGN 4.25 on corners a, b, c (...,3) float64 relative to the origin: the eleven terms (...,11)."""
    ax, ay, az = a[..., 0], a[..., 1], a[..., 2]
    bx, by, bz = b[..., 0], b[..., 1], b[..., 2]
    cx, cy, cz = c[..., 0], c[..., 1], c[..., 2]
    d = (ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz)) + az * (bx * cy - by * cx)
    s = (a + b) + c
    t = np.empty(a.shape[:-1] + (11,))
    t[..., 0] = d
    for k in range(3):
        t[..., 1 + k] = d * s[..., k]
    for q, (k, l) in enumerate(_MESH_SECOND):
        t[..., 4 + q] = d * (((a[..., k] * a[..., l] + b[..., k] * b[..., l]) + c[..., k] * c[..., l]) + s[..., k] * s[..., l])
    u, w = b - a, c - a
    nx, ny, nz = u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2], u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]
    t[..., 10] = np.sqrt((nx * nx + ny * ny) + nz * nz)
    return t


def mesh_column_sums(terms):
    """Rule 3 of DESIGN 4.25 on terms (n,F,K): column l of 1024 adds faces l, l + 1024, ... in rising order from +0.0, then the tree
    col[l] += col[l + h] for l < h, h = 512 .. 1 -> (n,K)."""
    n, F, K = terms.shape
    col = np.zeros((n, MESH_COLUMNS, K))
    for lo in range(0, F, MESH_COLUMNS):
        step = terms[:, lo:lo + MESH_COLUMNS]
        col[:, :step.shape[1]] = col[:, :step.shape[1]] + step
    h = MESH_COLUMNS // 2
    while h >= 1:
        col[:, :h] = col[:, :h] + col[:, h:2 * h]
        h //= 2
    return col[:, 0].copy()


def mesh_rows_of(sums, origin):
    """Rule 4 of DESIGN 4.25: sums (n,11) and origins (n,3) -> rows (n,11), columns MESH_MOMENT_COLUMNS."""
    S = np.asarray(sums, np.float64)
    rows = np.full((S.shape[0], 11), np.nan)
    S0 = S[:, 0]
    has = S0 > 0
    m = S[:, 1:4] / (4.0 * S0)[:, None]
    E = S[:, 4:10] / (20.0 * S0)[:, None]
    rows[:, 0] = S0 / 6.0
    rows[:, 1:4] = np.where(has[:, None], origin + m, np.nan)
    for q, (k, l) in enumerate(_MESH_SECOND):
        rows[:, 4 + q] = np.where(has, E[:, q] - m[:, k] * m[:, l], np.nan)
    rows[:, 10] = S[:, 10] / 2.0
    return rows


def mesh_moments(verts, faces, return_sums=False, chunk=16):
    """Volume, centre of mass, central second moments per unit volume and area of a closed mesh in numpy float64: the host statement
    of GRNet.mesh_moments -- the same operations in the same order, so the same bits.  verts (n,V,3), rounded to float32 and widened; faces (F,3),
    which must be a closed, consistently oriented surface over [0, V) (faces_closed).  Returns rows (n,11), columns MESH_MOMENT_COLUMNS; with
    return_sums also the sums (n,11).  UNIFORM DENSITY IS AN ASSUMPTION; the numbers are reported, never judged."""
    v = _widened(verts, "verts")
    f = _faces_table(faces, v.shape[1])
    bad = faces_closed(f, v.shape[1])
    if bad:
        raise ValueError(f"the face table is not a closed, consistently oriented surface: {bad} directed edges are duplicated or lack their reverse edge")
    sums, origin = np.empty((v.shape[0], 11)), v[:, f[0, 0]].copy()
    with np.errstate(all="ignore"):
        for lo in range(0, v.shape[0], chunk):
            x = v[lo:lo + chunk]
            o = origin[lo:lo + chunk, None, :]
            sums[lo:lo + chunk] = mesh_column_sums(mesh_face_terms(x[:, f[:, 0]] - o, x[:, f[:, 1]] - o, x[:, f[:, 2]] - o))
        rows = mesh_rows_of(sums, origin)
    return (rows, sums) if return_sums else rows


def body_rows(rows, joints3d, lengths=None, density=BODY_DENSITY, segments=BALANCE_SEGMENTS_KINECTV2, joints=GAIT_JOINTS_KINECTV2):
    """Per video the columns BODY_COLUMNS from mesh_moments' rows (n,11) and the joints (n,J,3) of the same frames, on the host: a
    frame is valid where its nine columns of centre and moments are finite; volume, area and the radii of gyration sqrt(C_kk) are means over the
    valid frames, volume_sd two-pass with ddof 0, volume_cv = sd / mean, mass = density * volume_mean; com_offset and com_distance are the mesh's
    centre of mass minus DESIGN 4.22 rule 1's (the segment table's on the same joints) over the valid frames where that one is finite too.  Sums run in
    time order from +0.0; a value is NaN where its count is 0.  joints: gait_balance's table, checked as there.  Returns (n_seq,15)."""
    r = np.asarray(rows, np.float64)
    if r.ndim != 2 or r.shape[1] != 11 or r.shape[0] < 1:
        raise ValueError(f"rows must be (n,11) with n >= 1, got {r.shape}")
    j3 = _widened(joints3d, "joints3d")
    if j3.shape[0] != r.shape[0]:
        raise ValueError(f"joints3d has {j3.shape[0]} frames, rows {r.shape[0]}")
    lengths = _sequence_lengths(r.shape[0], lengths)
    _joint_table(joints, 8, j3.shape[1], _GAIT_JOINT_NAMES)
    if not np.isfinite(density) or not density > 0:
        raise ValueError("density must be positive and finite")
    table = balance_table_com(j3, segments)
    out = np.full((len(lengths), len(BODY_COLUMNS)), np.nan)
    a = 0
    with np.errstate(all="ignore"):
        for q, T in enumerate(lengths):
            x, c = r[a:a + T], table[a:a + T]
            a += T
            valid = np.isfinite(x[:, 1:10]).all(axis=1) & np.isfinite(x[:, 0]) & np.isfinite(x[:, 10])
            y = x[valid]
            row = out[q]
            row[0], row[1] = T, len(y)
            row[2], row[3] = _gait_mean_sd(y[:, 0])
            if len(y):
                row[4], row[5] = row[3] / row[2], float(density) * row[2]
                row[6] = _gait_sum(y[:, 10]) / len(y)
                for k in range(3):
                    row[7 + k] = _gait_sum(np.sqrt(y[:, 4 + k])) / len(y)
            both = valid & np.isfinite(c).all(axis=1)
            d = x[both, 1:4] - c[both]
            if len(d):
                for k in range(3):
                    row[10 + k] = _gait_sum(d[:, k]) / len(d)
                dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
                row[13], row[14] = _gait_sum(dist) / len(dist), float(dist.max())
    return out


# ----------------------------------------------------------------------------- step and stride tables, bootstrap intervals
STEP_TABLE_COLUMNS =("t_prev", "t", "landing_foot", "step_time", "step_length", "step_width")
STRIDE_TABLE_COLUMNS = ("t0", "t1", "foot", "stride_time")
BOOTSTRAP_STATISTICS = ("mean", "sd", "cv")
BOOTSTRAP_OUT_COLUMNS = ("estimate", "replicates")            # then one column per quantile
_BOOT_GOLDEN, _BOOT_M1, _BOOT_M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def gait_step_tables(events, per_frame, lengths=None, fps=20.0, max_rows=256, phase=None, straight_only=False):
    """The samples behind gait_parameters' step and stride columns in numpy float64: the host statement of GRNet.gait_step_tables, same
    arguments, a dict of numpy arrays.  events (n,) and per_frame (n,7) as gait_parameters returned them; phase (n,): gait_turns' phase -- with
    straight_only only the steps and strides with no frame of [opening strike, closing strike] in a phase other than 0 are listed.  steps
    (n_seq,max_rows,6), columns STEP_TABLE_COLUMNS, in time order; strides (n_seq,max_rows,4), columns STRIDE_TABLE_COLUMNS, the left foot's first;
    counts (n_seq,2) int32: rows past max_rows are counted, not stored; rows past the count are NaN."""
    rows = np.asarray(per_frame, np.float64)
    if rows.ndim != 2 or rows.shape[1] != 7 or rows.shape[0] < 1:
        raise ValueError(f"per_frame must be (n,7) with n >= 1, got {rows.shape}")
    n = rows.shape[0]
    ev = np.asarray(events)
    if ev.shape != (n,):
        raise ValueError(f"events must be ({n},), got {ev.shape}")
    ev = ev.astype(np.int64)
    ph = None
    if phase is not None:
        ph = np.asarray(phase)
        if ph.shape != (n,):
            raise ValueError(f"phase must be ({n},), got {ph.shape}")
    if straight_only and ph is None:
        raise ValueError("straight_only needs a phase")
    lengths = _sequence_lengths(n, lengths)
    if not np.isfinite(fps) or not fps > 0:
        raise ValueError("fps must be positive and finite")
    if int(max_rows) != max_rows or not 1 <= max_rows <= 1024:
        raise ValueError(f"max_rows {max_rows} outside [1, 1024]")
    fps, max_rows = float(fps), int(max_rows)
    steps = np.full((len(lengths), max_rows, 6), np.nan)
    strides = np.full((len(lengths), max_rows, 4), np.nan)
    counts = np.zeros((len(lengths), 2), np.int32)
    a = 0
    with np.errstate(all="ignore"):
        for q, T in enumerate(lengths):
            e, r = ev[a:a + T], rows[a:a + T]
            busy = np.concatenate([[0], np.cumsum(ph[a:a + T] != TURN_STRAIGHT)]) if straight_only else np.zeros(T + 1, np.int64)
            heel = [np.flatnonzero(e & GAIT_HEEL_L), np.flatnonzero(e & GAIT_HEEL_R)]
            strikes = sorted([(int(t), 0) for t in heel[0]] + [(int(t), 1) for t in heel[1]])      # time order, the left foot first within a frame
            found = [(t1, t2, f2) for (t1, f1), (t2, f2) in zip(strikes[:-1], strikes[1:]) if f1 != f2 and busy[t2 + 1] == busy[t1]]
            for i, (t1, t2, f2) in enumerate(found[:max_rows]):
                steps[q, i] = t1, t2, f2, float(t2 - t1) / fps, r[t2, f2] - r[t2, 1 - f2], r[t2, 4]
            pairs = [(int(t1), int(t2), foot) for foot in (0, 1) for t1, t2 in zip(heel[foot][:-1], heel[foot][1:]) if busy[int(t2) + 1] == busy[int(t1)]]
            for i, (t1, t2, foot) in enumerate(pairs[:max_rows]):
                strides[q, i] = t1, t2, foot, float(t2 - t1) / fps
            counts[q] = len(found), len(pairs)
            a += T
    return {"steps": steps, "strides": strides, "counts": counts}


def bootstrap_mix(z):
    """splitmix64's output function on a numpy uint64 array (Steele, Lea and Flood 2014): integers alone, wrapping."""
    with np.errstate(over="ignore"):
        z = np.asarray(z, np.uint64)
        z = (z ^ (z >> np.uint64(30))) * _BOOT_M1
        z = (z ^ (z >> np.uint64(27))) * _BOOT_M2
        return z ^ (z >> np.uint64(31))


def bootstrap_u(seed, stream, r, j):
    """u(seed, stream, r, j) = mix(mix(mix(seed + G (stream + 1)) + G (r + 1)) + G (j + 1)) in uint64, wrapping; r and j broadcast."""
    with np.errstate(over="ignore"):
        one = np.uint64(1)
        key = bootstrap_mix(np.array(int(seed) % 2**64, np.uint64) + _BOOT_GOLDEN * (np.uint64(int(stream)) + one))
        key = bootstrap_mix(key + _BOOT_GOLDEN * (np.asarray(r).astype(np.uint64) + one))
        return bootstrap_mix(key + _BOOT_GOLDEN * (np.asarray(j).astype(np.uint64) + one))


def bootstrap_index(u, n):
    """((u >> 32) n) >> 32: an index below n whose bias is below n / 2^32 -- stated, not corrected."""
    return ((np.asarray(u, np.uint64) >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)


def bootstrap_indices(n, B, block=1, seed=0, stream=0):
    """(B + 1, n) int64: row 0 is the sample itself, row r = 1 .. B the circular block bootstrap idx(p) = (index(u(seed, stream, r, p / block), n) +
    p % block) % n.  Nothing here depends on which sequence asks: two sequences with equal n get equal indices."""
    p = np.arange(n, dtype=np.int64)
    idx = np.empty((B + 1, n), np.int64)
    idx[0] = p
    if n:
        start = bootstrap_index(bootstrap_u(seed, stream, np.arange(1, B + 1)[:, None], (p // block)[None, :]), n).astype(np.int64)
        idx[1:] = (start + p % block) % n
    return idx


def _bootstrap_rule_check(max_rows, C, cols, B, block, seed, stream, quantiles):
    if not 1 <= max_rows <= 1024:
        raise ValueError(f"max_rows {max_rows} outside [1, 1024]")
    if not 1 <= C <= 16:
        raise ValueError(f"C {C} outside [1, 16]")
    if not 1 <= len(cols) <= 8:
        raise ValueError(f"n_cols {len(cols)} outside [1, 8]")
    if any(int(c) != c or not 0 <= c < C for c in cols):
        raise ValueError(f"column outside [0, {C})")
    if int(B) != B or not 1 <= B <= 4096:
        raise ValueError(f"B {B} outside [1, 4096]")
    if int(block) != block or not 1 <= block <= 1024:
        raise ValueError(f"block {block} outside [1, 1024]")
    if int(seed) != seed or not 0 <= seed < 2**64:
        raise ValueError(f"seed {seed} outside [0, 2^64)")
    if int(stream) != stream or not 0 <= stream <= 65535:
        raise ValueError(f"stream {stream} outside [0, 65535]")
    if len(quantiles) > 5:
        raise ValueError(f"n_q {len(quantiles)} outside [0, 5]")
    if any(int(v) != v or not 0 <= v <= 10000 for v in quantiles):
        raise ValueError("quantile outside [0, 10000] basis points")


def bootstrap_select(values, quantiles):
    """[f, the quantiles] of one statistic's replicates 1 .. B: those that are not NaN in the order (value under <, then replicate number) -- a stable
    sort, under which -0 and +0 tie -- f their count, a quantile of q basis points the element of rank (q (f - 1)) // 10000, NaN where f = 0."""
    v = np.asarray(values, np.float64)
    kept = v[~np.isnan(v)]
    kept = kept[np.argsort(kept, kind="stable")]
    return [float(kept.size)] + [kept[(int(q) * (kept.size - 1)) // 10000] if kept.size else np.nan for q in quantiles]


def bootstrap_table(table, counts, cols, B=2000, block=1, seed=0, stream=0, quantiles=(250, 5000, 9750), return_replicates=False):
    """Nonparametric bootstrap of mean, SD and CV of columns of a per-step table in numpy float64 (Efron 1979; block > 1: the circular block bootstrap
    of Politis and Romano 1992; the rules: DESIGN 4.23): the host statement of GRNet.bootstrap_table, same arguments, a dict of numpy arrays.  table
    (n_seq,max_rows,C); counts (n_seq,): the rows of each sequence, above max_rows read as max_rows.  Rows are resampled: all columns of a replicate
    share the indices (bootstrap_indices).  Per replicate and column, over the rows in order from +0.0 and skipping NaN values (m kept): mean = S / m,
    SD = sqrt(sum (x - mean)^2 / m), CV = (100 SD) / mean, NaN where m = 0 -- gait_strides' operations in its order, every sum a cumulative sum.  out
    (n_seq,n_cols,3,2 + n_q): per statistic [replicate 0, f, the quantiles] (bootstrap_select); replicates (n_seq,n_cols,3,B) on request.  A
    PERCENTILE INTERVAL FROM SOME 15 STRIDES UNDER-COVERS, and steps within a walk are serially correlated; the numbers are reported, never judged."""
    t = np.asarray(table, np.float64)
    if t.ndim != 3 or min(t.shape) < 1:
        raise ValueError(f"table must be (n_seq,max_rows,C), got {t.shape}")
    n_seq, max_rows, C = t.shape
    cnt = np.asarray(counts)
    if cnt.shape != (n_seq,):
        raise ValueError(f"counts must be ({n_seq},), got {cnt.shape}")
    cols, quantiles = [v for v in np.asarray(cols).reshape(-1).tolist()], [v for v in np.asarray(quantiles).reshape(-1).tolist()]
    _bootstrap_rule_check(max_rows, C, cols, B, block, seed, stream, quantiles)
    cols, quantiles, B, block = [int(c) for c in cols], [int(v) for v in quantiles], int(B), int(block)
    out = np.full((n_seq, len(cols), 3, 2 + len(quantiles)), np.nan)
    reps = np.full((n_seq, len(cols), 3, B), np.nan)
    made = {}
    with np.errstate(all="ignore"):
        for q in range(n_seq):
            n = int(min(max(int(cnt[q]), 0), max_rows))
            if n not in made:
                made[n] = bootstrap_indices(n, B, block, seed, stream)
            for k, c in enumerate(cols):
                stats = np.full((B + 1, 3), np.nan)
                if n:
                    x = t[q, :n, c][made[n]]                      # (B + 1, n)
                    gone = np.isnan(x)
                    m = (n - gone.sum(axis=1)).astype(np.float64)
                    some = m > 0
                    # both sums begin at +0.0 (the column of zeros in front: -0.0 alone sums to +0.0), so a sum is never -0.0 and a skipped value,
                    # which adds +0.0 here, changes no bit of it
                    zero = np.zeros((B + 1, 1))
                    mean = np.cumsum(np.concatenate([zero, np.where(gone, 0.0, x)], axis=1), axis=1)[:, -1] / m
                    d = np.where(gone, 0.0, x - mean[:, None])
                    sd = np.sqrt(np.cumsum(np.concatenate([zero, d * d], axis=1), axis=1)[:, -1] / m)
                    stats[:, 0], stats[:, 1], stats[:, 2] = np.where(some, mean, np.nan), np.where(some, sd, np.nan), np.where(some, (100.0 * sd) / mean, np.nan)
                for s in range(3):
                    out[q, k, s, 0] = stats[0, s]
                    out[q, k, s, 1:] = bootstrap_select(stats[1:, s], quantiles)
                    reps[q, k, s] = stats[1:, s]
    result = {"out": out}
    if return_replicates:
        result["replicates"] = reps
    return result


def run_on_frames(model, image_folder, frames, bboxes, device="cuda", batch_size=None, on_device=False, body=False, body_on_host=False):
    """batch_generation.py:289-371: one batch per video (batch_size = max(n_frames, 400)), kp_3d -> kinectv2.  ``bboxes`` is scaled
    by 1.1 IN PLACE, as the reference's Inference.__init__ does to the caller's array (inference.py:48).  Image files are cropped
    and normalised by the HIP kernel (grnet_crop_normalise, row f1); .npy files hold ready crops.
    on_device: return {"kp_3d": (n,25,3) float32 tensor on ``device``} and never synchronise with the host (the multi-GPU driver
    keeps every work item's joints on the device until its single all-gather); default: the reference's numpy array.
    body: also return "body", the (n,11) float64 rows of DESIGN 4.25 (MESH_MOMENT_COLUMNS) -- model.mesh_moments on the vertices of each forward call
    where they lie, a tensor on ``device`` (on_device) or a numpy array; body_on_host, or a model without the method: mesh_moments here, on
    model.faces, after a download of the vertices."""
    ds = InferenceFrames(image_folder, frames, bboxes, scale=1.1)
    joints, moments = [], []
    sel = torch.as_tensor(np.asarray(netspec.SPIN2_TO_KINECTV2), dtype=torch.long, device=device) if on_device else None
    for batch in ds.batches(batch_size or max(len(frames), MAX_SEQLEN), model=model):
        x = torch.as_tensor(batch, dtype=torch.float32).unsqueeze(0).to(device)
        out = model(x)[-1]
        if body:
            verts = out["verts"].detach().reshape(-1, netspec.NUM_VERTS, 3)
            if body_on_host or not hasattr(model, "mesh_moments"):
                rows = torch.as_tensor(mesh_moments(verts.cpu().numpy(), model.faces), dtype=torch.float64, device=device)
            else:
                rows = model.mesh_moments(verts)
            moments.append(rows if on_device else rows.cpu().numpy())
        if on_device:
            joints.append(out["kp_3d"].detach().squeeze(0).index_select(1, sel).to(torch.float32))
            continue
        j = out["kp_3d"].detach().cpu().squeeze(0).numpy()
        joints.append(spin2_to_kinectv2(j).astype(np.float32))
    if on_device:
        made = {"kp_3d": torch.cat(joints, 0) if joints else torch.zeros(0, 25, 3, dtype=torch.float32, device=device)}
        if body:
            made["body"] = torch.cat(moments, 0) if moments else torch.zeros(0, 11, dtype=torch.float64, device=device)
        return made
    made = {"kp_3d": np.concatenate(joints, 0) if joints else np.zeros((0, 25, 3), np.float32)}
    if body:
        made["body"] = np.concatenate(moments, 0) if moments else np.zeros((0, 11))
    return made


class BatchDb:
    """The joblib 'json' database of batch_generation.py:226-243,265-284: flushed every 50 videos."""

    def __init__(self, outpath):
        if not outpath.endswith(".json"):
            raise AssertionError("outpath must end with .json (batch_generation.py:236)")
        self.outpath, self.out_ind, self.db, self.written = outpath, 0, defaultdict(list), []

    def add(self, vid_name, bboxes, joints3d, **extra):
        """extra: further per-frame arrays of n rows (batch_generation.py --trajectory: trans, trans_status, reproj), every video or none."""
        n = bboxes.shape[0]
        self.db["vid_name"].extend([vid_name] * n)
        self.db["bbox"].append(np.asarray(bboxes).reshape(n, 4))
        self.db["joints3D"].append(np.asarray(joints3d).reshape(n, 25, 3))
        for name, rows in extra.items():
            assert np.asarray(rows).shape[0] == n, (name, np.asarray(rows).shape, n)
            self.db[name].append(np.asarray(rows))

    def flush(self):
        import joblib
        if not len(self.db):
            return None
        def stacked(v):                                        # floats as float32, as the reference stores them; integer columns keep their type
            a = np.concatenate(v, 0)
            return a if a.dtype.kind in "iu" else a.astype(np.float32)
        db = {k: (stacked(v) if isinstance(v[0], np.ndarray) else np.array(v)) for k, v in self.db.items()}
        outfp = self.outpath[:-5] + f"_{self.out_ind}.json"
        joblib.dump(db, outfp)
        self.written.append(outfp)
        self.out_ind += 1
        self.db = defaultdict(list)
        return outfp
