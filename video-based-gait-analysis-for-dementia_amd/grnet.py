"""Host-side mirror of the reference's model interface for the per-frame path.

``GRNet`` keeps the constructor signature, ``load_state_dict`` / ``eval`` / ``to`` surface and the
``forward(features, bbox=None, cimg=None, J_regressor=None) -> [dict]`` contract of
``lib/models/grnet.py:25-175`` (output keys per ``lib/models/pare.py:78-84``), but every FLOP runs
in libgrnet_hip.so on the MI355X.  PyTorch is used only as the tensor container (``data_ptr()``),
for the current HIP stream and for reading checkpoints.

Differences from the reference that are deliberate: no ``sys.exit`` on a missing PARE
checkpoint (weights arrive through ``load_state_dict`` / ``load_pare_dict``) and ``torch.load`` uses
``map_location='cpu'``.  ``use_gait_feat=True`` runs the temporal branch of ``grnet.py:154-173`` with the
names the reference's FeatCorrector leaves undefined bound as DESIGN.md records (feature_correction.py:40-62,144);
``featcorr`` must describe the one configuration the class can run in (configs/config_grnet.yaml).

``J_regressor`` (the evaluation path, pare.py:70-76) replaces ``kp_3d`` by the joints the caller's table takes from the FINAL
vertices (grnet_regress_joints, csrc/joint_regress.hip); ``theta``, ``verts``, ``kp_2d`` (29 joints) and ``rotmat`` are untouched.
harness.py's pose record and the entry points keep the 29 joints: demo.py and batch_generation.py never pass a regressor.
"""
import ctypes as C
import logging
from collections import namedtuple

import numpy as np
import torch

from . import _lib, netspec

logger = logging.getLogger(__name__)
_IncompatibleKeys = namedtuple("_IncompatibleKeys", ["missing_keys", "unexpected_keys"])

SMPL_PREFIX = "regressor.smpl.smpl."
_SMPL_KEYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights", "parents", "J_regressor_extra")
_TOLERATED_SMPL_KEYS = ("vertex_joint_selector.extra_joints_idxs", "betas", "global_orient",
                        "body_pose", "transl")


def _i32p(a):
    """The int32 numpy array `a` as the C ABI takes a `const int32_t*`."""
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _np32(t):
    if torch.is_tensor(t):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(t), dtype=np.float32)


def reference_selection(rows):
    """The rows VPRegressor.forward keeps of a table of ``rows`` rows (pare.py:73-75): H36M_TO_J14 below 24 rows, else all (None)."""
    if rows >= 24:
        return None
    if rows <= max(netspec.H36M_TO_J14):
        raise ValueError(f"a J_regressor of {rows} rows cannot be indexed with H36M_TO_J14 (needs >= 17 rows; pare.py:73-74)")
    return list(netspec.H36M_TO_J14)


def resolve_joint_regressor(J, select="reference"):
    """Argument checks of GRNet.set_joint_regressor that need no handle: J (rows,6890) tensor / array -> (contiguous f32 array, row
    indices or None).  select "reference": what VPRegressor.forward does (pare.py:70-76) -- netspec.H36M_TO_J14 when rows < 24, all rows
    otherwise; fewer than 17 rows raise ValueError there (the reference's indexing fails with an IndexError); None: all rows; or a
    sequence of row indices applied after the product."""
    W = _np32(J)
    if W.ndim != 2 or W.shape[1] != netspec.NUM_VERTS or W.shape[0] < 1:
        raise ValueError(f"J_regressor must be (rows,{netspec.NUM_VERTS}), got {tuple(W.shape)}")
    rows = W.shape[0]
    if isinstance(select, str):
        if select != "reference":
            raise ValueError("select must be 'reference', None or a sequence of row indices")
        return W, reference_selection(rows)
    if select is None:
        return W, None
    sel = [int(i) for i in select]
    if not sel or min(sel) < 0 or max(sel) >= rows:
        raise ValueError(f"select must hold row indices in [0, {rows})")
    return W, sel


_GAIT_JOINT_NAMES = "pelvis, spine-shoulder, left / right hip, ankle, foot"
_KIN_JOINT_NAMES = "pelvis, spine-shoulder, left / right hip, knee, ankle, foot, shoulder, elbow, wrist"
_ARENA_FIELDS = ("bytes", "full_bytes", "lower_bound_bytes", "tensors", "shared_tensors")


def arena_query(dtype="f32", max_frames=64, compact=False):
    """The arena GRNet(dtype=, max_frames=, compact_arena=) would allocate, computed on the host -- no GPU, no handle (grnet_arena_query):
    dict(bytes, full_bytes, lower_bound_bytes, tensors, shared_tensors)."""
    if dtype not in ("f32", "bf16"):
        raise ValueError("dtype must be 'f32' or 'bf16'")
    info = (C.c_int64 * 5)()
    rc = _lib.load().grnet_arena_query(_lib.PRECISION_BF16 if dtype == "bf16" else _lib.PRECISION_F32, int(max_frames),
                                       _lib.CREATE_COMPACT_ARENA if compact else 0, info)
    if rc != 0:
        raise _lib.GrnetError(f"grnet_arena_query failed with code {rc} (max_frames is 1 .. 2048)")
    return dict(zip(_ARENA_FIELDS, (int(v) for v in info)))


def arena_layout(dtype="f32", max_frames=64, compact=False):
    """The layout as text (grnet_arena_layout): tensor / op / group lines."""
    lib = _lib.load()
    args = (_lib.PRECISION_BF16 if dtype == "bf16" else _lib.PRECISION_F32, int(max_frames), _lib.CREATE_COMPACT_ARENA if compact else 0)
    need = lib.grnet_arena_layout(*args, None, 0)
    if need < 0:
        raise _lib.GrnetError(f"grnet_arena_layout failed with code {need}")
    buf = C.create_string_buffer(need)
    n = lib.grnet_arena_layout(*args, buf, need)
    if n < 0:
        raise _lib.GrnetError(f"grnet_arena_layout failed with code {n}")
    return buf.value.decode()


class GRNet:
    is_demo = False

    def __init__(self, num_joints=24, num_input_features=480, num_features_pare=128, num_features_smpl=64,
                 backbone='hrnet_w32', focal_length=5000., img_res=224, pretrained_pare=None, writer=None, seqlen=50,
                 pretrained_hrnet=None, use_gait_feat=False, featcorr=None, use_pose_encoder=False,
                 use_shpcam_encoder=False, max_frames=64, device_id=0, dtype="f32", compact_arena=False):
        if (num_joints, num_input_features, num_features_pare, num_features_smpl) != (24, 480, 128, 64) \
                or backbone != 'hrnet_w32' or focal_length != 5000. or img_res != 224:
            raise ValueError("the HIP path implements the reference's fixed configuration "
                             "(24 joints, hrnet_w32 -> 480 features, PARE 128/64, f=5000, 224 px)")
        self.use_gait_feat = bool(use_gait_feat)
        if use_gait_feat and featcorr is not None:
            want = dict(AVG_DIM=3, ESTIM_PHASE=True, NUM_LAYERS=1, H_SIZE=1024, NUM_HEADS=4, USE_JWFF=True)
            get = (lambda k: featcorr[k]) if isinstance(featcorr, dict) else (lambda k: getattr(featcorr, k))
            got = {k: get(k) for k in want}
            if got != want:
                raise ValueError(f"MODEL.FEAT_CORR {got}: the HIP path implements configs/config_grnet.yaml's {want} -- the only "
                                 "configuration in which FeatCorrector's reshapes are consistent (feature_correction.py:92,144)")
        self._lib = _lib.load()
        self.max_frames = int(max_frames)
        self.device = torch.device("cuda", device_id)
        h = C.c_void_p()
        if dtype not in ("f32", "bf16"):
            raise ValueError("dtype must be 'f32' (the reference's precision) or 'bf16' (bf16 storage, fp32 accumulation; BASELINE configs 3/5)")
        self.dtype = dtype
        # compact_arena: intermediates whose lifetimes cannot overlap share memory (grnet_create_ex; same launches, bit-identical outputs, 13.7 instead
        # of 103.8 MB per frame in fp32); debug_tensor then serves only the tensors nothing is placed over.  The default keeps every intermediate readable.
        self.compact_arena = bool(compact_arena)
        rc = self._lib.grnet_create_ex(C.byref(h), device_id, _lib.PRECISION_BF16 if dtype == "bf16" else _lib.PRECISION_F32, self.max_frames,
                                       _lib.CREATE_COMPACT_ARENA if self.compact_arena else 0)
        if rc != 0:
            raise _lib.GrnetError(f"grnet_create failed with code {rc} (is a GPU visible?)")
        self._h = h
        self._finalized = False
        self._smpl_loaded = False
        self.faces = None                 # host copy of the (F,3) int32 face table render() draws (load_faces)
        self._loaded = set()
        self._jreg = None                 # (host copy of the table, selection, the object it came from, its version) of the table on the device
        self.joint_regressor_uploads = 0  # tables handed to grnet_set_joint_regressor so far
        self.seqlen = seqlen
        self.training = False
        self.focal_length = focal_length
        if pretrained_pare:
            self.load_pare_dict(pretrained_pare)

    def _stream(self, device=None):
        """The current stream of `device` (None: the handle's) as the C ABI takes it."""
        if device is None:
            return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    # ------------------------------------------------------------------ weights
    def _load_tensor(self, key, value):
        if torch.is_tensor(value):
            value = value.detach().cpu().numpy()
        value = np.asarray(value)
        if value.dtype.kind in "iu":
            dtype, arr = _lib.DTYPE_I64, np.ascontiguousarray(value, dtype=np.int64)
        else:
            dtype, arr = _lib.DTYPE_F32, np.ascontiguousarray(value, dtype=np.float32)
        shape = (C.c_int64 * max(arr.ndim, 1))(*arr.shape)
        rc = self._lib.grnet_load_tensor(self._h, key.encode(), arr.ctypes.data_as(C.c_void_p), shape, arr.ndim, dtype)
        _lib.check(self._lib, self._h, rc, f"grnet_load_tensor({key})")
        self._loaded.add(key)

    def load_smpl(self, tables):
        """SMPL buffers (smplx.SMPL tables + J_regressor_extra, lib/models/smpl.py:97-106)."""
        arrs = [_np32(tables[k]) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights")]
        parents = np.ascontiguousarray(np.asarray(tables["parents"]).astype(np.int32))
        parents[0] = -1
        extra = _np32(tables["J_regressor_extra"])
        want = [netspec.SMPL_TABLE_SHAPES[k] for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights")]
        for a, w, k in zip(arrs, want, _SMPL_KEYS):
            if int(np.prod(a.shape)) != int(np.prod(w)):
                raise ValueError(f"SMPL table {k} has shape {a.shape}, expected {w}")
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = self._lib.grnet_load_smpl(self._h, ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), ptr(arrs[3]), ptr(arrs[4]),
                                       ptr(parents), ptr(extra))
        _lib.check(self._lib, self._h, rc, "grnet_load_smpl")
        self._smpl_loaded = True
        if "f" in tables:                    # SMPL_NEUTRAL.npz carries the face table the overlay draws
            self.load_faces(tables["f"])

    def load_faces(self, faces):
        """The (F,3) face table of the 6890-vertex mesh (smplx's faces_tensor, 'f' of SMPL_NEUTRAL.npz) for render(); before or after
        finalize(), a second table replaces the first (grnet_load_faces)."""
        if torch.is_tensor(faces):
            faces = faces.detach().cpu().numpy()
        f = np.asarray(faces)
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or f.dtype.kind not in "iu":
            raise ValueError(f"faces must be an integer (F,3) table, got {f.dtype} {f.shape}")
        f = np.ascontiguousarray(f.astype(np.int64).clip(-1, 2**31 - 1), dtype=np.int32)     # an index that does not fit stays out of range
        _lib.check(self._lib, self._h, self._lib.grnet_load_faces(self._h, f.ctypes.data_as(C.c_void_p), f.shape[0]), "grnet_load_faces")
        self.faces = f

    def load_state_dict(self, state_dict, strict=True):
        """Reference key names (demo.py:116-122; batch_generation.py:214-218)."""
        if self._finalized:
            raise RuntimeError("weights are already finalized on the device")
        spec = netspec.grnet_spec()
        unexpected, smpl, faces = [], {}, None
        for k, v in state_dict.items():
            if k.startswith(SMPL_PREFIX):
                name = k[len(SMPL_PREFIX):]
                if name in _SMPL_KEYS:
                    smpl[name] = v
                elif name == "faces_tensor":
                    faces = v
                elif name not in _TOLERATED_SMPL_KEYS:
                    unexpected.append(k)
            elif k in spec or k.startswith(("pfeat_corrector.", "gru.", "tsattn.")):
                want = spec.get(k)
                if want is not None and tuple(np.shape(v)) != tuple(want[0]):
                    raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(np.shape(v))} vs model {tuple(want[0])}")
                self._load_tensor(k, v)
            else:
                unexpected.append(k)
        if len(smpl) == len(_SMPL_KEYS):
            self.load_smpl(smpl)
        missing = [k for k in spec if k not in self._loaded]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for GRNet: missing {missing[:5]}{'...' if len(missing) > 5 else ''}"
                               f" unexpected {unexpected[:5]}{'...' if len(unexpected) > 5 else ''}")
        if faces is not None:                # after the checks above: a state dict they reject leaves the handle's face table as it was
            self.load_faces(faces)
        return _IncompatibleKeys(missing, unexpected)

    def load_pare_dict(self, pretrained_pare):
        """PARE head weights re-keyed from 'model.head.*' (grnet.py:93-109; utils.py:185-196)."""
        ckpt = torch.load(pretrained_pare, map_location="cpu")["state_dict"]
        if "model.head.init_pose" not in ckpt or "model.head.init_shape" not in ckpt:
            raise KeyError(f"Checkpoint at {pretrained_pare} does not match VPARE implementation.")
        sd = {"head." + k[len("model.head."):]: v for k, v in ckpt.items() if k.startswith("model.head.")}
        return self.load_state_dict(sd, strict=False)

    def finalize(self):
        if not self._finalized:
            if not self._smpl_loaded:
                raise RuntimeError("SMPL tables were not loaded (regressor.smpl.smpl.* keys or load_smpl())")
            _lib.check(self._lib, self._h, self._lib.grnet_finalize_weights(self._h), "grnet_finalize_weights")
            self._finalized = True
        return self

    # torch.nn.Module surface used by the entry points
    def to(self, device=None):
        return self

    def eval(self):
        return self

    def set_option(self, option, value):
        _lib.check(self._lib, self._h, self._lib.grnet_set_option(self._h, option, value), "grnet_set_option")

    # ------------------------------------------------------------------ J_regressor override (pare.py:70-76)
    def set_joint_regressor(self, J, select="reference"):
        """Upload the (rows,6890) table regress_joints uses; see resolve_joint_regressor for ``select``.  ``J=None`` clears it."""
        if J is None:
            _lib.check(self._lib, self._h, self._lib.grnet_set_joint_regressor(self._h, None, 0, None, 0), "grnet_set_joint_regressor")
            self._jreg = None
            return self
        W, sel = resolve_joint_regressor(J, select)
        self._upload_joint_regressor(W, sel, J)
        return self

    def _upload_joint_regressor(self, W, sel, src):
        self._jreg = None                                        # a refused table leaves the earlier one on the device; it is then re-sent on its next use
        arr = (C.c_int32 * len(sel))(*sel) if sel is not None else None
        rc = self._lib.grnet_set_joint_regressor(self._h, W.ctypes.data_as(C.c_void_p), W.shape[0], arr, len(sel) if sel is not None else 0)
        _lib.check(self._lib, self._h, rc, "grnet_set_joint_regressor")
        self.joint_regressor_uploads += 1
        self._jreg = (W.copy(), sel, src, getattr(src, "_version", None))

    def _use_joint_regressor(self, J):
        """forward's J_regressor argument: upload only when the table, or the reference's selection for its row count, differs from what
        the handle holds.  The same tensor object, unmodified, costs nothing; any other object is brought to the host (a device-to-host copy
        for a CUDA tensor) and compared with the kept copy -- so an evaluation loop passes the SAME object every time, or calls
        set_joint_regressor once and regress_joints on the vertices, rather than a fresh ``J.to(device)`` per batch."""
        cur = self._jreg
        if cur is not None and cur[2] is J and cur[3] == getattr(J, "_version", None) and torch.is_tensor(J) \
                and cur[1] == reference_selection(cur[0].shape[0]):        # the table on the device may carry another selection (set_joint_regressor)
            return
        W, sel = resolve_joint_regressor(J, "reference")
        if cur is not None and cur[1] == sel and cur[0].shape == W.shape and np.array_equal(cur[0], W):
            self._jreg = (cur[0], sel, J, getattr(J, "_version", None))
            return
        self._upload_joint_regressor(W, sel, J)

    def joint_regressor_rows(self):
        return self._lib.grnet_joint_regressor_rows(self._h)

    def regress_joints(self, verts):
        """verts (n,6890,3) or (b,t,6890,3) on the handle's device -> (n,Jout,3) / (b,t,Jout,3): the set table's (selected) rows times the
        vertices, fp32, bit-identical per frame whatever the call size (grnet_regress_joints)."""
        if verts.dim() not in (3, 4) or tuple(verts.shape[-2:]) != (netspec.NUM_VERTS, 3):
            raise ValueError(f"verts must be (n,6890,3) or (b,t,6890,3), got {tuple(verts.shape)}")
        if verts.device != self.device:
            raise RuntimeError(f"verts live on {verts.device} but this model's handle is bound to {self.device}")
        lead = tuple(verts.shape[:-2])
        v = verts.to(torch.float32).reshape(-1, netspec.NUM_VERTS, 3).contiguous()
        n = v.shape[0]
        jout = max(self.joint_regressor_rows(), 0)
        out = torch.empty(n, jout, 3, dtype=torch.float32, device=self.device)
        stream = self._stream()
        for s in range(0, max(n, 1), self.max_frames):
            m = min(self.max_frames, n - s)
            rc = self._lib.grnet_regress_joints(self._h, v[s:s + m].data_ptr(), m, out[s:s + m].data_ptr() if jout else None, stream)
            _lib.check(self._lib, self._h, rc, "grnet_regress_joints")
        return out.reshape(*lead, jout, 3)

    # ------------------------------------------------------------------ forward
    def forward(self, features, bbox=None, cimg=None, J_regressor=None, extras=()):
        if features.dim() == 5:
            batch_size, seqlen, nc, h, w = features.shape
            features = features.reshape(-1, nc, h, w)
        elif features.dim() == 4:
            batch_size = 1
            seqlen, nc, h, w = features.shape
        else:
            raise ValueError(f"Wrong feature dimension: {features.dim()}.")
        if (nc, h, w) != (3, 224, 224):
            raise ValueError(f"expected frames of shape (3,224,224), got {(nc, h, w)}")
        if J_regressor is not None:
            self._use_joint_regressor(J_regressor)              # checked (and uploaded, if it is a new table) before anything is enqueued
        if self.use_gait_feat:
            assert (bbox is not None) and (cimg is not None)                     # grnet.py:133
            if bbox.dim() == 2:
                bbox = bbox.unsqueeze(0)
            if cimg.dim() == 2:
                cimg = cimg.unsqueeze(0)
            extras = tuple(extras) + tuple(k for k in ("point_local_feat", "cam_shape_feats") if k not in extras)
        if not features.is_cuda:
            raise RuntimeError("frames must live in HBM (features.to('cuda')); the HIP path has no CPU fallback")
        if features.device != self.device:
            raise RuntimeError(f"frames live on {features.device} but this model's handle is bound to {self.device}")
        self.finalize()
        x = features.to(torch.float32).contiguous()
        n = x.shape[0]
        dev = x.device
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        out = {"theta": new(n, 85), "verts": new(n, 6890, 3), "kp_2d": new(n, 29, 2), "kp_3d": new(n, 29, 3),
               "rotmat": new(n, 24, 3, 3)}
        shapes = {"point_local_feat": (128, 24), "cam_shape_feats": (64, 24), "pred_rot6d": (24, 6),
                  "features": (480, 56, 56), "part_attn": (25, 56, 56), "smpl_feats": (128, 56, 56)}
        for k in extras:
            out[k] = new(n, *shapes[k])
        stream = self._stream(dev)
        for s in range(0, n, self.max_frames):
            m = min(self.max_frames, n - s)
            o = _lib.Outputs()
            for k, t in out.items():
                setattr(o, k, t[s:s + m].data_ptr())
            rc = self._lib.grnet_forward(self._h, C.c_void_p(x[s:s + m].data_ptr()), m, C.byref(o), stream)
            _lib.check(self._lib, self._h, rc, "grnet_forward")
        res = {"theta": out["theta"].reshape(batch_size, seqlen, 85),
               "verts": out["verts"].reshape(batch_size, seqlen, 6890, 3),
               "kp_2d": out["kp_2d"].reshape(batch_size, seqlen, 29, 2),
               "kp_3d": out["kp_3d"].reshape(batch_size, seqlen, 29, 3),
               "rotmat": out["rotmat"].reshape(batch_size, seqlen, 24, 3, 3)}
        for k in extras:
            res[k] = out[k]
        if self.use_gait_feat:                                 # grnet.py:154-173: FeatCorrector, second head pass, regressor
            g = self.gait_correct(out["point_local_feat"], out["cam_shape_feats"], out["theta"], bbox, cimg, batch_size, seqlen)
            for k in ("theta", "verts", "kp_2d", "kp_3d", "rotmat"):
                res[k] = g[k].reshape(res[k].shape)
            res["pred_avg"], res["pred_phase"] = g["pred_avg"], g["pred_phase"]
            res["pred_cparam"] = g["pred_cparam"]
            res["point_local_feat"] = g["point_local_feat"]
        if J_regressor is not None:                            # pare.py:70-76 on the FINAL vertices (grnet.py:171)
            res["kp_3d"] = self.regress_joints(res["verts"])
        return [res]

    __call__ = forward

    def gait_correct(self, point_local_feat, cam_shape_feats, theta_or_cam, bbox, cimg, b, t):
        """grnet.py:154-173 on the first pass's results for whole clips: (b*t,128,24), (b*t,64,24), theta (b*t,85) or pred_cam
        (b*t,3), bbox (b,t,4), cimg (b,t,2) -> dict(theta, verts, kp_2d, kp_3d, rotmat, pred_avg (b,3), pred_phase (b,t,4),
        pred_cparam (b*t,3), point_local_feat (b*t,128,24) corrected)."""
        self.finalize()
        dev, m = self.device, b * t
        f = lambda x, *shape: x.to(dev, torch.float32).reshape(*shape).contiguous()
        plf, csf = f(point_local_feat, m, 128, 24), f(cam_shape_feats, m, 64, 24)
        cam = f(theta_or_cam, m, -1)
        bb, ci = f(bbox, m, 4), f(cimg, m, 2)
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        out = {"theta": new(m, 85), "verts": new(m, 6890, 3), "kp_2d": new(m, 29, 2), "kp_3d": new(m, 29, 3), "rotmat": new(m, 24, 3, 3)}
        gait = {"pred_avg": new(b, 3), "pred_phase": new(b, t, 4), "pred_cparam": new(m, 3), "point_local_feat": new(m, 128, 24)}
        o, g = _lib.Outputs(), _lib.GaitOutputs()
        for k, v in out.items():
            setattr(o, k, v.data_ptr())
        for k, v in gait.items():
            setattr(g, k, v.data_ptr())
        stream = self._stream(dev)
        rc = self._lib.grnet_gait_correct(self._h, plf.data_ptr(), csf.data_ptr(), cam.data_ptr(), cam.shape[1], bb.data_ptr(), ci.data_ptr(),
                                          b, t, C.byref(o), C.byref(g), stream)
        _lib.check(self._lib, self._h, rc, "grnet_gait_correct")
        out.update(gait)
        return out

    def tune(self, n_frames, level=1, cache=None):
        """Measure-and-pick launch configurations for calls of ``n_frames`` frames (see grnet_tune).

        ``cache``: path of a text file holding a previously measured table; applied if present, written after tuning."""
        self.finalize()
        import os
        if cache and os.path.isfile(cache):
            with open(cache) as f:
                rc = self._lib.grnet_set_tuning(self._h, int(n_frames), f.read().encode())
            if rc == 0:
                return self
        stream = self._stream()
        _lib.check(self._lib, self._h, self._lib.grnet_tune(self._h, int(n_frames), stream, int(level)), "grnet_tune")
        if cache:
            buf = C.create_string_buffer(1 << 16)
            if self._lib.grnet_get_tuning(self._h, int(n_frames), buf, len(buf)) > 0:
                os.makedirs(os.path.dirname(os.path.abspath(cache)), exist_ok=True)
                with open(cache, "w") as f:
                    f.write(buf.value.decode())
        return self

    def tuned_mode(self, n_frames):
        """Schedule chosen by tune(): dict(measured_table, eager) or None if not tuned for n_frames."""
        buf = C.create_string_buffer(1 << 16)
        if self._lib.grnet_get_tuning(self._h, int(n_frames), buf, len(buf)) <= 0:
            return None
        mode = int(buf.value.decode().split("\n", 1)[0].split()[1])
        return {"measured_table": bool(mode & 1), "eager": bool(mode & 4)}

    # ------------------------------------------------------------------ introspection (bench / tests)
    def num_kernel_launches(self):
        return self._lib.grnet_num_kernel_launches(self._h)

    def num_conv_launches(self):
        return self._lib.grnet_num_conv_launches(self._h)

    def plan_counts(self):
        """Cross-lane hand-offs of the lane schedule (grnet_plan_counts): waits / recorded events over all edges and the kept ones, lanes used / joined."""
        c = (C.c_int64 * len(_lib.PLAN_COUNTS))()
        _lib.check(self._lib, self._h, self._lib.grnet_plan_counts(self._h, c), "grnet_plan_counts")
        return dict(zip(_lib.PLAN_COUNTS, (int(v) for v in c)))

    def conv_flops_per_frame(self):
        return self._lib.grnet_conv_flops_per_frame(self._h)

    def conv_executed_flops_per_frame(self, n_frames=None):
        """Winograd F(4x4,3x3) layers counted at the 1/4 of their multiplies they execute (x the tile padding on 14x14 / 7x7 maps), for a
        call of n_frames frames (default: the handle's latest forward).  Reporting only."""
        self.finalize()
        if n_frames is None:
            return self._lib.grnet_conv_executed_flops_per_frame(self._h)
        return self._lib.grnet_conv_executed_flops_per_frame_n(self._h, int(n_frames))

    def kernel_table(self, n_frames, reps=20):
        """Per kernel (family<shape>) of the conv-class launches of one forward of n_frames frames: launches, time of each distinct layer
        shape measured ALONE (grnet_time_conv: HIP events around `reps` back-to-back launches), algorithmic and executed FLOPs.
        Returns a list of dicts sorted by total time: name, launches, total_us, avg_us, gflop (algorithmic, per step), executed_gflop."""
        self.finalize()
        stream = self._stream()
        convs = self.describe_convs()
        timed, rows = {}, {}
        for pos, c in enumerate(convs):
            name, ex = C.create_string_buffer(96), C.c_double()
            _lib.check(self._lib, self._h, self._lib.grnet_conv_kernel_info(self._h, pos, int(n_frames), name, 96, C.byref(ex)), "grnet_conv_kernel_info")
            key = (name.value, c["cin"], c["cout"], c["ks"], c["stride"], c["hin"], c["n_add"], c["macs"])
            if key not in timed:
                us = C.c_float()
                _lib.check(self._lib, self._h, self._lib.grnet_time_conv(self._h, pos, int(n_frames), int(reps), stream, C.byref(us)), "grnet_time_conv")
                timed[key] = us.value
            member = name.value.endswith(b"+")              # a convolution inside a conv_bf16_chain launch: its FLOPs count, it has no launch of its own
            row = name.value.decode().rstrip("+")
            r = rows.setdefault(row, {"name": row, "launches": 0, "total_us": 0.0, "gflop": 0.0, "executed_gflop": 0.0})
            r["launches"] += 0 if member else 1
            r["total_us"] += timed[key]
            r["gflop"] += 2.0 * c["macs"] * n_frames / 1e9
            r["executed_gflop"] += 2.0 * ex.value * n_frames / 1e9
        out = sorted(rows.values(), key=lambda r: -r["total_us"])
        for r in out:
            r["avg_us"] = r["total_us"] / r["launches"]
        return out

    def conv_kernels(self, n_frames):
        """Per convolution-class launch of the plan, in launch order: (weight key of its first segment, kernel family<shape> that runs it in a call of
        n_frames frames) -- grnet_conv_kernel_info.  A name ending in '+' runs inside the launch of its group's first member."""
        self.finalize()
        out = []
        for pos, c in enumerate(self.describe_convs()):
            name = C.create_string_buffer(96)
            _lib.check(self._lib, self._h, self._lib.grnet_conv_kernel_info(self._h, pos, int(n_frames), name, 96, None), "grnet_conv_kernel_info")
            out.append((c["name"], name.value.decode()))
        return out

    def conv_launch_forms(self, n_frames):
        """fp32 handles, per convolution-class launch of the plan in launch order: (weight key of its first segment, launch form as a dict, tuning
        index) for a call of n_frames frames under the tile hints in effect -- grnet_conv_launch_form.  The dict holds "family" (direct, wino4,
        wino4w, wino4s, pw, stem, fuse_up) and the integer fields of that family; the tuning index is the one grnet_set_tuning's table uses (-1: none).
        A layer whose hint in effect is not valid for it raises GrnetError."""
        self.finalize()
        out = []
        for pos, c in enumerate(self.describe_convs()):
            out.append((c["name"],) + self.conv_launch_form(pos, n_frames))
        return out

    def conv_launch_form(self, pos, n_frames):
        """(launch form dict, tuning index) of the pos-th launch (see conv_launch_forms)."""
        buf, idx = C.create_string_buffer(256), C.c_int(-1)
        _lib.check(self._lib, self._h, self._lib.grnet_conv_launch_form(self._h, int(pos), int(n_frames), buf, len(buf), C.byref(idx)), "grnet_conv_launch_form")
        fam, *kv = buf.value.decode().split()
        form = {"family": fam}
        form.update((k, int(v)) for k, v in (t.split("=") for t in kv))
        return form, idx.value

    def describe_convs(self):
        """The convolution launches of one forward in launch order: list of dicts (shape, fused addends, weight key, MACs per frame).
        An entry with cin == 0 is the grouped launch of an HR module's 1x1 fuse terms (csrc/hr_fuse.hip)."""
        self.finalize()
        keys = ("cin", "cout", "ks", "stride", "hin", "win", "hout", "wout", "n_add", "relu", "lane", "add_elems")
        out = []
        for pos in range(self.num_conv_launches()):
            info, name = (C.c_int32 * 12)(), C.create_string_buffer(160)
            _lib.check(self._lib, self._h, self._lib.grnet_describe_conv(self._h, pos, info, name, 160), "grnet_describe_conv")
            d = dict(zip(keys, list(info)))
            d["name"] = name.value.decode()
            d["macs"] = int(self._lib.grnet_describe_conv_macs(self._h, pos))
            out.append(d)
        return out

    def op_timeline(self, frames):
        """Diagnostic (grnet_op_timeline): [(index, lane, start_us, end_us, label)] of one eager forward on `frames` (n,3,224,224)."""
        self.finalize()
        x = frames.to(self.device, torch.float32).contiguous()
        buf = C.create_string_buffer(1 << 18)
        stream = self._stream()
        rc = self._lib.grnet_op_timeline(self._h, x.data_ptr(), x.shape[0], stream, buf, len(buf))
        if rc < 0:
            _lib.check(self._lib, self._h, rc, "grnet_op_timeline")
        rows = []
        for line in buf.value.decode().splitlines():
            i, lane, a, b, label = line.split(" ", 4)
            rows.append((int(i), int(lane), float(a), float(b), label))
        return rows

    def time_convs(self, n_frames):
        ms = C.c_float()
        stream = self._stream()
        _lib.check(self._lib, self._h, self._lib.grnet_time_convs(self._h, n_frames, stream, C.byref(ms)), "grnet_time_convs")
        return ms.value

    def smpl_forward(self, betas, rotmat, cam=None, J_regressor=None):
        """SMPL LBS on the GPU: betas (n,10), rotmat (n,24,3,3) [, cam (n,3)] -> verts, kp_3d (29 spin2 joints) [, kp_2d].
        J_regressor (rows,6890): kp_3d is replaced as VPRegressor.forward replaces it (pare.py:70-76); verts and kp_2d are not touched."""
        self.finalize()
        if J_regressor is not None:
            self._use_joint_regressor(J_regressor)
        n = betas.shape[0]
        dev = self.device
        b = betas.to(dev, torch.float32).contiguous()
        r = rotmat.to(dev, torch.float32).reshape(n, 24, 9).contiguous()
        c = cam.to(dev, torch.float32).contiguous() if cam is not None else None
        verts = torch.empty(n, 6890, 3, dtype=torch.float32, device=dev)
        kp3d = torch.empty(n, 29, 3, dtype=torch.float32, device=dev)
        kp2d = torch.empty(n, 29, 2, dtype=torch.float32, device=dev) if cam is not None else None
        stream = self._stream(dev)
        for s0 in range(0, n, self.max_frames):
            m = min(self.max_frames, n - s0)
            rc = self._lib.grnet_smpl_forward(self._h, b[s0:].data_ptr(), r[s0:].data_ptr(), c[s0:].data_ptr() if c is not None else None,
                                              m, verts[s0:].data_ptr(), kp3d[s0:].data_ptr(),
                                              kp2d[s0:].data_ptr() if kp2d is not None else None, stream)
            _lib.check(self._lib, self._h, rc, "grnet_smpl_forward")
        if J_regressor is not None:
            kp3d = self.regress_joints(verts)
        return verts, kp3d, kp2d

    def crop_normalise(self, images, bboxes, scale=1.0, bgr=False, mode="cv2"):
        """uint8 frames (n,H,W,3) [or one (H,W,3) frame] + boxes (n,4) -> (n,3,224,224) normalised crops, on the GPU.
        mode "cv2" (default): OpenCV's fixed-point warpAffine arithmetic (grnet_crop_normalise_cv_maps; the maps are computed on the
        host as the reference's gen_trans_from_patch_cv / getAffineTransform / warpAffine do -- pipeline.cv_crop_maps; a box with
        w != h takes the reference's two-warp, aspect-preserving branch, img_utils.py:97-106);
        mode "ideal": exact bilinear sampling in float (grnet_crop_normalise), kept for A/B."""
        shared = images.dim() == 3
        if images.dtype != torch.uint8 or images.shape[-1] != 3 or not images.is_cuda:
            raise ValueError("images must be a uint8 CUDA tensor (n,H,W,3) or (H,W,3)")
        images = images.contiguous()
        bb_host = bboxes.detach().cpu().numpy() if torch.is_tensor(bboxes) else np.asarray(bboxes)
        n = bb_host.shape[0]
        if bb_host.shape != (n, 4) or (not shared and images.shape[0] != n):
            raise ValueError("bboxes must be (n,4) and match the number of frames")
        hgt, wid = images.shape[-3], images.shape[-2]
        out = torch.empty(n, 3, 224, 224, dtype=torch.float32, device=images.device)
        stream = self._stream(images.device)
        if mode == "cv2":
            from .pipeline import cv_crop_maps
            maps = torch.from_numpy(cv_crop_maps(bb_host, scale)).to(images.device, non_blocking=True)
            rc = self._lib.grnet_crop_normalise_cv_maps(self._h, images.data_ptr(), n, hgt, wid, int(shared), maps.data_ptr(), int(bgr),
                                                        out.data_ptr(), stream)
            _lib.check(self._lib, self._h, rc, "grnet_crop_normalise_cv_maps")
            return out
        if mode != "ideal":
            raise ValueError("mode must be 'cv2' or 'ideal'")
        bb = torch.as_tensor(bb_host).to(device=images.device, dtype=torch.float32).contiguous()
        rc = self._lib.grnet_crop_normalise(self._h, images.data_ptr(), n, hgt, wid, int(shared), bb.data_ptr(), float(scale),
                                            int(bgr), out.data_ptr(), stream)
        _lib.check(self._lib, self._h, rc, "grnet_crop_normalise")
        return out

    def debug_tensor(self, name, n_frames):
        """Named intermediate of the last forward as an (n,C,H,W) tensor (see grnet_debug_tensor)."""
        shp = (C.c_int64 * 3)()
        stream = self._stream()
        _lib.check(self._lib, self._h, self._lib.grnet_debug_tensor(self._h, name.encode(), n_frames, None, shp, stream),
                   "grnet_debug_tensor")
        out = torch.empty(n_frames, shp[0], shp[1], shp[2], dtype=torch.float32, device=self.device)
        _lib.check(self._lib, self._h, self._lib.grnet_debug_tensor(self._h, name.encode(), n_frames, out.data_ptr(), shp,
                                                                     stream), "grnet_debug_tensor")
        return out

    def arena_info(self):
        """The handle's activation arena (grnet_arena_info): dict(bytes, full_bytes, lower_bound_bytes, tensors, shared_tensors)."""
        info = (C.c_int64 * 5)()
        _lib.check(self._lib, self._h, self._lib.grnet_arena_info(self._h, info), "grnet_arena_info")
        return dict(zip(_ARENA_FIELDS, (int(v) for v in info)))

    def arena_fill(self, pattern):
        """Diagnostic: fill the arena behind its zero block with a 32-bit pattern on the current stream (grnet_arena_fill)."""
        stream = self._stream()
        _lib.check(self._lib, self._h, self._lib.grnet_arena_fill(self._h, int(pattern) & 0xffffffff, stream), "grnet_arena_fill")

    def tsattn_plan(self, n):
        """What the attention block does with a clip of n frames on this device (grnet_tsattn_plan):
        dict(kernel 'per_query' | 'blocked', parts, key_blocks, lds_bytes)."""
        plan = (C.c_int32 * 4)()
        _lib.check(self._lib, self._h, self._lib.grnet_tsattn_plan(self._h, int(n), plan), "grnet_tsattn_plan")
        return {"kernel": "blocked" if plan[0] else "per_query", "parts": plan[1], "key_blocks": plan[2], "lds_bytes": plan[3]}

    def arm_temporal_taps(self, buf):
        """Arm the taps of the NEXT gru_forward / tsattn_forward / gait_correct (grnet_temporal_taps): ``buf`` is a float32 device
        tensor that receives a copy of every launch's output; read it with temporal_taps() after the call.  None disarms."""
        if buf is None:
            _lib.check(self._lib, self._h, self._lib.grnet_temporal_taps(self._h, None, 0), "grnet_temporal_taps")
            return
        if buf.dtype != torch.float32 or not buf.is_contiguous() or buf.device.type != "cuda":
            raise ValueError("the tap buffer must be a contiguous float32 device tensor")
        _lib.check(self._lib, self._h, self._lib.grnet_temporal_taps(self._h, buf.data_ptr(), buf.numel()), "grnet_temporal_taps")

    def temporal_tap_layout(self):
        """(taps, gemms) of the last armed call: taps {name: (offset, shape)} in launch order, gemms [(M, N, K, slices)]."""
        need = self._lib.grnet_temporal_tap_layout(self._h, None, 0)
        text = C.create_string_buffer(max(need, 1))
        rc = self._lib.grnet_temporal_tap_layout(self._h, text, need)
        if rc < 0:
            _lib.check(self._lib, self._h, rc, "grnet_temporal_tap_layout")
        taps, gemms = {}, []
        for line in text.value.decode().splitlines():
            f = line.split()
            if f[0] == "tap":
                taps[f[1]] = (int(f[2]), tuple(int(v) for v in f[3:]))
            elif f[0] == "gemm":
                gemms.append(tuple(int(v) for v in f[1:5]))
        return taps, gemms

    def temporal_taps(self, buf):
        """Views into ``buf`` of everything the last armed call copied: {name: tensor of the tap's shape}."""
        taps, _ = self.temporal_tap_layout()
        flat = buf.reshape(-1)
        out = {}
        for name, (off, shape) in taps.items():
            count = 1
            for d in shape:
                count *= d
            out[name] = flat[off:off + count].reshape(shape)
        return out

    def gru_forward(self, x, cparams):
        """BidirectionalModel.forward on this handle's GRU weights (keys gru.* / pfeat_corrector.featnet.*)."""
        self.finalize()
        b, t, f = x.shape
        if f != 3072 or tuple(cparams.shape) != (b, t, 3):
            raise ValueError("x must be (b,T,3072) and cparams (b,T,3)")
        x = x.to(torch.float32).contiguous()
        cp = cparams.to(torch.float32).contiguous()
        y = torch.empty(b, 3, dtype=torch.float32, device=x.device)
        ph = torch.empty(b, t, 4, dtype=torch.float32, device=x.device)
        xc = torch.empty(b, t, 3072, dtype=torch.float32, device=x.device)
        stream = self._stream(x.device)
        rc = self._lib.grnet_gru_forward(self._h, x.data_ptr(), cp.data_ptr(), b, t, y.data_ptr(), ph.data_ptr(),
                                         xc.data_ptr(), stream)
        _lib.check(self._lib, self._h, rc, "grnet_gru_forward")
        return y, ph, xc

    def tsattn_forward(self, x, xs):
        """TSAttnBlock.forward (attention_utils.py:261-270) on this handle's attention-block weights
        (keys tsattn.* / pfeat_corrector.featTencoder.0.*): x (b,n,128,24), xs (b,n,128,25) -> (b,n,3072)."""
        self.finalize()
        if x.dim() != 4 or tuple(x.shape[2:]) != (128, 24) or tuple(xs.shape) != (x.shape[0], x.shape[1], 128, 25):
            raise ValueError("x must be (b,n,128,24) and xs (b,n,128,25)")
        b, n = x.shape[:2]
        x = x.to(torch.float32).contiguous()
        xs = xs.to(torch.float32).contiguous()
        y = torch.empty(b, n, 3072, dtype=torch.float32, device=x.device)
        stream = self._stream(x.device)
        rc = self._lib.grnet_tsattn_forward(self._h, x.data_ptr(), xs.data_ptr(), b, n, y.data_ptr(), stream)
        _lib.check(self._lib, self._h, rc, "grnet_tsattn_forward")
        return y

    def head_forward(self, point_local_feat, cam_shape_feats):
        """PareHead.forward + VPRegressor.forward from given pooled features (pare.py:271-303,52-91): (n,128,24), (n,64,24) ->
        dict(theta (n,85), verts, kp_2d, kp_3d, rotmat, pred_rot6d).  The second head pass of the use_gait_feat branch."""
        self.finalize()
        n = point_local_feat.shape[0]
        if tuple(point_local_feat.shape) != (n, 128, 24) or tuple(cam_shape_feats.shape) != (n, 64, 24):
            raise ValueError("point_local_feat must be (n,128,24) and cam_shape_feats (n,64,24)")
        dev = self.device
        plf = point_local_feat.to(dev, torch.float32).contiguous()
        csf = cam_shape_feats.to(dev, torch.float32).contiguous()
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        out = {"theta": new(n, 85), "verts": new(n, 6890, 3), "kp_2d": new(n, 29, 2), "kp_3d": new(n, 29, 3),
               "rotmat": new(n, 24, 3, 3), "pred_rot6d": new(n, 24, 6)}
        stream = self._stream(dev)
        for s0 in range(0, n, self.max_frames):
            m = min(self.max_frames, n - s0)
            o = _lib.Outputs()
            for k, t in out.items():
                setattr(o, k, t[s0:s0 + m].data_ptr())
            rc = self._lib.grnet_head_forward(self._h, plf[s0:].data_ptr(), csf[s0:].data_ptr(), m, C.byref(o), stream)
            _lib.check(self._lib, self._h, rc, "grnet_head_forward")
        return out

    def op_rot6d_to_rotmat(self, x):
        x = x.to(self.device, torch.float32).reshape(-1, 6).contiguous()
        out = torch.empty(x.shape[0], 3, 3, dtype=torch.float32, device=self.device)
        stream = self._stream()
        _lib.check(self._lib, self._h, self._lib.grnet_op_rot6d_to_rotmat(self._h, x.data_ptr(), x.shape[0], out.data_ptr(), stream),
                   "grnet_op_rot6d_to_rotmat")
        return out

    def op_rotmat_to_aa(self, R):
        R = R.to(self.device, torch.float32).reshape(-1, 9).contiguous()
        out = torch.empty(R.shape[0], 3, dtype=torch.float32, device=self.device)
        stream = self._stream()
        _lib.check(self._lib, self._h, self._lib.grnet_op_rotmat_to_aa(self._h, R.data_ptr(), R.shape[0], out.data_ptr(), stream),
                   "grnet_op_rotmat_to_aa")
        return out

    # ------------------------------------------------------------------ --smooth on the device (smooth_pose.py:28-116)
    def _pose_rows(self, x, what):
        """(T,72) or (T,85) theta, host or device -> (tensor kept alive, pointer to the first pose column, row stride in floats).  A
        device float32 tensor whose rows are contiguous is read in place (a theta is entered at column 3), whatever its row stride."""
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32))
        if x.dim() != 2 or x.shape[0] < 1:
            raise ValueError(f"{what} must be (T,72) or a (T,85) theta with T >= 1, got {tuple(x.shape)}")
        if x.shape[1] == 96:
            raise ValueError(f"{what} is 96 wide: quaternion poses (24 x 4) are not implemented on the device -- the filter and SMPL "
                             "run on axis-angle poses (T,72), the only form the reference's entry points pass to smooth_pose")
        if x.shape[1] not in (72, 85):
            raise ValueError(f"{what} must be (T,72) or a (T,85) theta, got {tuple(x.shape)}")
        x = x.to(self.device, torch.float32)
        if x.stride(1) != 1 or x.stride(0) < 72:
            x = x.contiguous()
        off = 3 if x.shape[1] == 85 else 0
        return x, x.data_ptr() + 4 * off, x.stride(0)

    def one_euro(self, x, min_cutoff=0.004, beta=0.7, d_cutoff=1.0):
        """The reference's OneEuroFilter over a sequence (grnet_op_one_euro): x (T,72), or a (T,85) theta whose pose columns are filtered
        in place -> (T,72) device tensor, bit-identical to the reference's float32 numpy arithmetic."""
        x, ptr, ld = self._pose_rows(x, "x")
        out = torch.empty(x.shape[0], 72, dtype=torch.float32, device=self.device)
        stream = self._stream()
        _lib.check(self._lib, self._h, self._lib.grnet_op_one_euro(self._h, ptr, ld, x.shape[0], min_cutoff, beta, d_cutoff, out.data_ptr(), stream),
                   "grnet_op_one_euro")
        return out

    def aa_to_rotmat(self, aa):
        """Axis-angle (...,3) -> (m,3,3), smplx's batch_rodrigues (grnet_op_aa_to_rotmat)."""
        aa = torch.as_tensor(aa).to(self.device, torch.float32).reshape(-1, 3).contiguous()
        out = torch.empty(aa.shape[0], 3, 3, dtype=torch.float32, device=self.device)
        stream = self._stream()
        _lib.check(self._lib, self._h, self._lib.grnet_op_aa_to_rotmat(self._h, aa.data_ptr(), aa.shape[0], out.data_ptr(), stream),
                   "grnet_op_aa_to_rotmat")
        return out

    _JOINT_KINDS = {"spin49": (_lib.JOINTS_SPIN49, 49), "spin2": (_lib.JOINTS_SPIN2, 29), "kinectv2": (_lib.JOINTS_KINECTV2, 25)}

    def smooth_pose(self, pose, betas, min_cutoff=0.004, beta=0.7, joints="spin49", return_verts=True):
        """smooth_pose.py:28-116 on the device (grnet_smooth_pose): One-Euro filter over the pose, SMPL with the betas of frame 0, the joints
        in the skeleton asked for.  pose (T,72) or a (T,85) theta (read in place), betas (T,10) -- host or device; T is not limited by
        max_frames.  Returns device tensors (verts (T,6890,3) or None, pose_hat (T,72), joints (T,49|29|25,3)); nothing synchronises."""
        if joints not in self._JOINT_KINDS:
            raise ValueError(f"joints must be one of {sorted(self._JOINT_KINDS)}, got {joints!r}")
        self.finalize()
        kind, nj = self._JOINT_KINDS[joints]
        x, ptr, ld = self._pose_rows(pose, "pose")
        T = x.shape[0]
        b = torch.as_tensor(betas).to(self.device, torch.float32)
        if b.dim() != 2 or b.shape[1] != 10 or b.shape[0] < 1:
            raise ValueError(f"betas must be (T,10), got {tuple(b.shape)}")
        b0 = b[0].contiguous()
        pose_hat = torch.empty(T, 72, dtype=torch.float32, device=self.device)
        verts = torch.empty(T, 6890, 3, dtype=torch.float32, device=self.device) if return_verts else None
        out = torch.empty(T, nj, 3, dtype=torch.float32, device=self.device)
        stream = self._stream()
        rc = self._lib.grnet_smooth_pose(self._h, ptr, ld, b0.data_ptr(), T, min_cutoff, beta, kind, pose_hat.data_ptr(),
                                         verts.data_ptr() if return_verts else None, out.data_ptr(), stream)
        _lib.check(self._lib, self._h, rc, "grnet_smooth_pose")
        return verts, pose_hat, out

    # ------------------------------------------------------------------ the mesh overlay (demo.py --mesh_render)
    SIDE_VIEW = (0.0, 0.0, -1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0)      # the reference's --sideview: rotation by 270 degrees about y (demo.py:351-352)

    RENDER_WIREFRAME = 1            # GRNET_RENDER_WIREFRAME

    def render(self, images, verts, cams, colours, image_index, M=None, rgb=True, wireframe=False):
        """Draw n meshes into uint8 device images (F,H,W,3) IN PLACE and return them (grnet_render_meshes_ex; the rules: DESIGN.md 4.5).  verts
        (n,6890,3) and cams (n,4) rows [sx,sy,tx,ty] -- host or device; colours (n,3): the (r,g,b) triples the reference hands to
        Renderer.render; image_index (n): the image each mesh is drawn into.  Meshes of one image are drawn in the order given, later over
        earlier.  M: 9 floats, None for the main view, GRNet.SIDE_VIEW for --sideview.  Nothing synchronises; n is not limited by max_frames.
        rgb: the reference writes its (r,g,b) triple into a BGR image (cv2) WITHOUT swapping, so what it shows is (b,g,r) of the triple.
        pipeline keeps frames in RGB, so the triple goes down reversed to put the same colour on the screen; rgb=False: BGR frames, as is.
        wireframe: the reference's --wireframe -- nothing filled, the three edges of every front face as 1-pixel lines, shaded alike."""
        if not torch.is_tensor(images) or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or not images.is_cuda \
                or not images.is_contiguous():
            raise ValueError("images must be a contiguous uint8 (F,H,W,3) tensor on the device")
        F, H, W = images.shape[:3]
        v = torch.as_tensor(verts).to(self.device, torch.float32).contiguous()
        if v.dim() != 3 or tuple(v.shape[1:]) != (6890, 3):
            raise ValueError(f"verts must be (n,6890,3), got {tuple(v.shape)}")
        n = v.shape[0]
        c = torch.as_tensor(cams).to(self.device, torch.float32).reshape(-1, 4).contiguous()
        col = np.ascontiguousarray(np.asarray(colours, np.float32).reshape(-1, 3)[:, ::-1] if rgb else np.asarray(colours, np.float32).reshape(-1, 3))
        idx = np.ascontiguousarray(np.asarray(image_index, np.int64).reshape(-1).clip(-1, 2**31 - 1), dtype=np.int32)
        if not (c.shape[0] == col.shape[0] == idx.shape[0] == n):
            raise ValueError(f"verts, cams, colours and image_index disagree on n: {n}, {c.shape[0]}, {col.shape[0]}, {idx.shape[0]}")
        Mh = None if M is None else np.ascontiguousarray(np.asarray(M, np.float32).reshape(9))
        stream = self._stream()
        rc = self._lib.grnet_render_meshes_ex(self._h, v.data_ptr(), n, c.data_ptr(), col.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p),
                                              Mh.ctypes.data_as(C.c_void_p) if Mh is not None else None, images.data_ptr(), F, H, W,
                                              self.RENDER_WIREFRAME if wireframe else 0, stream)
        _lib.check(self._lib, self._h, rc, "grnet_render_meshes_ex")
        return images

    def op_raster_setup(self, verts, faces, cam, H, W, M=None):
        """verts (V,3), faces (F,3), cam (4) -> (xy (V,2) int32 snapped window coordinates, z (V), unit vertex normals (V,3)) on the device
        (grnet_op_raster_setup)."""
        v = torch.as_tensor(verts).to(self.device, torch.float32).reshape(-1, 3).contiguous()
        f = np.ascontiguousarray(np.asarray(faces).reshape(-1, 3), dtype=np.int32)
        c = torch.as_tensor(cam).to(self.device, torch.float32).reshape(4).contiguous()
        Mh = None if M is None else np.ascontiguousarray(np.asarray(M, np.float32).reshape(9))
        V = v.shape[0]
        xy = torch.empty(V, 2, dtype=torch.int32, device=self.device)
        z = torch.empty(V, dtype=torch.float32, device=self.device)
        nrm = torch.empty(V, 3, dtype=torch.float32, device=self.device)
        stream = self._stream()
        rc = self._lib.grnet_op_raster_setup(self._h, v.data_ptr(), V, f.ctypes.data_as(C.c_void_p), f.shape[0], c.data_ptr(),
                                             Mh.ctypes.data_as(C.c_void_p) if Mh is not None else None, H, W, xy.data_ptr(), z.data_ptr(), nrm.data_ptr(),
                                             stream)
        _lib.check(self._lib, self._h, rc, "grnet_op_raster_setup")
        return xy, z, nrm

    def _op_raster(self, entry, xy, z, faces, H, W):
        xy = torch.as_tensor(xy).to(self.device, torch.int32).reshape(-1, 2).contiguous()
        z = torch.as_tensor(z).to(self.device, torch.float32).reshape(-1).contiguous()
        f = np.ascontiguousarray(np.asarray(faces).reshape(-1, 3), dtype=np.int32)
        out = torch.empty(H, W, dtype=torch.int32, device=self.device)
        stream = self._stream()
        rc = getattr(self._lib, entry)(self._h, xy.data_ptr(), z.data_ptr(), xy.shape[0], f.ctypes.data_as(C.c_void_p), f.shape[0], H, W, out.data_ptr(),
                                       stream)
        _lib.check(self._lib, self._h, rc, entry)
        return out

    def op_raster(self, xy, z, faces, H, W):
        """Snapped vertices xy (V,2) int32 and z (V) -> the winning face per pixel (H,W) int32 in image rows, -1 where uncovered (grnet_op_raster)."""
        return self._op_raster("grnet_op_raster", xy, z, faces, H, W)

    def op_raster_lines(self, xy, z, faces, H, W):
        """op_raster for the wireframe: 3 face + k of the winning edge per pixel, k = 0: v0->v1, 1: v1->v2, 2: v2->v0 (grnet_op_raster_lines)."""
        return self._op_raster("grnet_op_raster_lines", xy, z, faces, H, W)

    # ------------------------------------------------------------------ boxes from 2D joints (batch_generation.py:39-93)
    @staticmethod
    def _sequence_offsets(rows, lengths, what):
        """n_seq + 1 int32 offsets of sequences of `lengths` rows lying back to back (None: one sequence of all rows).  Which lengths the
        device takes is the C ABI's to say."""
        lengths = [int(rows)] if lengths is None else [int(v) for v in lengths]
        if sum(lengths) != rows or sum(lengths) > 2**31 - 1:
            raise ValueError(f"lengths sum to {sum(lengths)}, {what} has {rows} rows")
        off = np.zeros(len(lengths) + 1, np.int32)
        off[1:] = np.cumsum(np.asarray(lengths, np.int64))
        return off

    def _rows_input(self, x, what, trailing, dtype, finite=False):
        """`x` (numpy or torch) as a contiguous device tensor of `dtype` and shape (n,) + trailing with n >= 1; a None in `trailing` stands for any
        size >= 1 (how many joints a call takes is the C ABI's to say).  finite: ValueError on a NaN or an infinity."""
        t = torch.as_tensor(x)
        if t.dim() != 1 + len(trailing) or t.shape[0] < 1 or any(have < 1 if want is None else have != want for have, want in zip(t.shape[1:], trailing)):
            shape = ",".join(["n"] + ["K" if want is None else str(want) for want in trailing])
            raise ValueError(f"{what} must be ({shape}{',' if not trailing else ''}) with n >= 1, got {tuple(t.shape)}")
        if finite and not bool(torch.isfinite(t).all()):
            raise ValueError(f"{what} has a non-finite entry")
        return t.to(self.device, dtype).contiguous()

    @staticmethod
    def _whole_frames(**values):
        """ValueError unless every named value (window, min_stride, max_stride) is a whole number of frames."""
        for name, v in values.items():
            if int(v) != v:
                raise ValueError(f"{name} {v} must be a whole number of frames")

    def bbox_from_joints2d(self, joints2d, lengths=None, threshold=0.1, return_index=False):
        """One box per sequence from 2D joints, get_bbox_from_joints2d(smooth=False) on the device (grnet_bbox_from_joints2d).
        joints2d (T,K,3) rows (x, y, score) in pixels, or (sum T,K,3) with the sequences' `lengths` -- numpy or torch, taken as float64.
        Returns a float64 device tensor (n_seq,4) = [cx, cy, nw, nh]; return_index: also the medoids' indices (n_seq,) int32 into their
        sequences' T K points.  Works before finalize(): no weight is read.  ValueError on non-finite input."""
        j = self._rows_input(joints2d, "joints2d", (None, 3), torch.float64, finite=True)
        off = self._sequence_offsets(j.shape[0], lengths, "joints2d")
        n_seq = len(off) - 1
        box = torch.empty(n_seq, 4, dtype=torch.float64, device=self.device)
        index = torch.empty(n_seq, dtype=torch.int32, device=self.device) if return_index else None
        stream = self._stream()
        rc = self._lib.grnet_bbox_from_joints2d(self._h, j.data_ptr(), j.shape[1], _i32p(off), n_seq, float(threshold),
                                                box.data_ptr(), index.data_ptr() if return_index else None, stream)
        _lib.check(self._lib, self._h, rc, "grnet_bbox_from_joints2d")
        return (box, index) if return_index else box

    def op_medoid(self, points, lengths=None, splits=0):
        """The exact 1-medoid alone (grnet_op_medoid): points (n,3) or (n,4) float32 rows (x, y, s[, pad]), one sequence or `lengths` of them;
        splits: column splits of the row sums, 0 = the library's choice.  Returns (index (n_seq,) int32, cost (n_seq,) float64) on the device:
        each sequence's row of least summed distance, lowest index on ties, and that sum."""
        p = torch.as_tensor(points).to(self.device, torch.float32)
        if p.dim() != 2 or p.shape[1] not in (3, 4) or p.shape[0] < 1:
            raise ValueError(f"points must be (n,3) or (n,4) with n >= 1, got {tuple(p.shape)}")
        p4 = torch.zeros(p.shape[0], 4, dtype=torch.float32, device=self.device)
        p4[:, :3] = p[:, :3]
        off = self._sequence_offsets(p.shape[0], lengths, "points")
        n_seq = len(off) - 1
        index = torch.empty(n_seq, dtype=torch.int32, device=self.device)
        cost = torch.empty(n_seq, dtype=torch.float64, device=self.device)
        stream = self._stream()
        rc = self._lib.grnet_op_medoid(self._h, p4.data_ptr(), _i32p(off), n_seq, int(splits), index.data_ptr(),
                                       cost.data_ptr(), stream)
        _lib.check(self._lib, self._h, rc, "grnet_op_medoid")
        return index, cost

    # ------------------------------------------------------------------ pose metrics
    def pose_metrics(self, pred_joints, gt_joints, lengths=None, root=None, select=None, pred_verts=None, gt_verts=None, unit=1000.0,
                     return_transform=False):
        """MPJPE, PA-MPJPE, PVE, acceleration and acceleration error on the device (grnet_pose_metrics; the definitions: DESIGN 4.8).
        pred_joints, gt_joints (n,J,3), J <= 64, one sequence or `lengths` of them lying back to back -- numpy or torch, taken as float32 and
        widened to float64 on the device.  root: joint indices whose mean is subtracted per frame (H36M-14: [2, 3]; kinectv2: [0]; None:
        nothing); select: the joint indices that enter the metrics (None: all); pred_verts, gt_verts (n,V,3): both or neither; unit multiplies
        every metric (1000: metres -> millimetres).  Returns a dict of float64 device tensors: per_frame (n,5) = [mpjpe, pa_mpjpe, pve, accel,
        accel_err] with NaN where an entry is undefined by structure (the accelerations at a sequence's ends, pve without vertices),
        per_sequence (n_seq,5) and total (5,): the means over the defined entries; return_transform: also transform (n,13) = [s, R row-major,
        t] of the Procrustes alignment, in the inputs' units.  Works before finalize(): no weight is read.  Nothing synchronises.  ValueError
        on non-finite input."""
        p = self._rows_input(pred_joints, "pred_joints", (None, 3), torch.float32, finite=True)
        g = self._rows_input(gt_joints, "gt_joints", (None, 3), torch.float32, finite=True)
        if p.shape != g.shape:
            raise ValueError(f"pred_joints and gt_joints differ in shape: {tuple(p.shape)}, {tuple(g.shape)}")
        if (pred_verts is None) != (gt_verts is None):
            raise ValueError("pred_verts and gt_verts go together")
        n, J = p.shape[:2]
        pv = gv = None
        V = 0
        if pred_verts is not None:
            pv = self._rows_input(pred_verts, "pred_verts", (None, 3), torch.float32, finite=True)
            gv = self._rows_input(gt_verts, "gt_verts", (None, 3), torch.float32, finite=True)
            if pv.shape != gv.shape or pv.shape[0] != n:
                raise ValueError(f"pred_verts and gt_verts must both be ({n},V,3), got {tuple(pv.shape)} and {tuple(gv.shape)}")
            V = pv.shape[1]
        off = self._sequence_offsets(n, lengths, "pred_joints")
        n_seq = len(off) - 1

        def indices(v):                                       # int32 for the C ABI, which says which indices it takes
            return np.ascontiguousarray(np.asarray(v, np.int64).reshape(-1).clip(-1, 2**31 - 1), dtype=np.int32)
        sel_keep = None if select is None else indices(select)
        root_keep = None if root is None or len(root) == 0 else indices(root)
        out = {"per_frame": torch.empty(n, 5, dtype=torch.float64, device=self.device),
               "per_sequence": torch.empty(n_seq, 5, dtype=torch.float64, device=self.device),
               "total": torch.empty(5, dtype=torch.float64, device=self.device)}
        if return_transform:
            out["transform"] = torch.empty(n, 13, dtype=torch.float64, device=self.device)
        stream = self._stream()
        rc = self._lib.grnet_pose_metrics(self._h, p.data_ptr(), g.data_ptr(), J, _i32p(off), n_seq,
                                          _i32p(sel_keep) if sel_keep is not None else None, 0 if sel_keep is None else sel_keep.shape[0],
                                          _i32p(root_keep) if root_keep is not None else None, 0 if root_keep is None else root_keep.shape[0],
                                          pv.data_ptr() if pv is not None else None, gv.data_ptr() if gv is not None else None, V, float(unit),
                                          out["per_frame"].data_ptr(), out["per_sequence"].data_ptr(), out["total"].data_ptr(),
                                          out["transform"].data_ptr() if return_transform else None, stream)
        _lib.check(self._lib, self._h, rc, "grnet_pose_metrics")
        return out

    def op_procrustes(self, K):
        """The Procrustes rotation alone (grnet_op_procrustes): K (k,3,3) or (3,3) float64 -> (R (k,3,3) the proper rotation that maximises
        trace(R K), sigma (k,3) the singular values of K, descending) on the device."""
        k = torch.as_tensor(K).to(self.device, torch.float64).reshape(-1, 9).contiguous()
        if k.shape[0] < 1:
            raise ValueError("K must hold at least one 3x3 matrix")
        R = torch.empty(k.shape[0], 9, dtype=torch.float64, device=self.device)
        sigma = torch.empty(k.shape[0], 3, dtype=torch.float64, device=self.device)
        stream = self._stream()
        rc = self._lib.grnet_op_procrustes(self._h, k.data_ptr(), k.shape[0], R.data_ptr(), sigma.data_ptr(), stream)
        _lib.check(self._lib, self._h, rc, "grnet_op_procrustes")
        return R.reshape(-1, 3, 3), sigma

    # ------------------------------------------------------------------ the camera-space trajectory
    def fit_translation(self, joints3d, joints2d, pairs, lengths=None, focal_length=5000.0, centre=(112.0, 112.0), conf_threshold=0.1, min_joints=4,
                        root=0, fill=True):
        """The translation that makes the 3D joints project onto the 2D detections, per frame, on the device (grnet_fit_translation: SPIN's
        weighted least squares, the reference's estimate_translation_np; the rules: DESIGN 4.9).  joints3d (n,K3,3) and joints2d (n,K2,3) =
        (x, y, confidence) in pixels, one sequence or `lengths` of them lying back to back -- numpy or torch, taken as float32 and widened to
        float64 on the device; pairs (P,2), P <= 64, of (3D index, 2D index); focal_length: one number or one per sequence; centre: (cx, cy) or
        (n_seq,2).  Returns a dict of float64 device tensors: per_frame (n,6) = [tx, ty, tz, reproj_px, n_used, status] with status 0 fitted,
        1 fewer than min_joints pairs above conf_threshold, 2 degenerate (t and reproj NaN for 1 and 2), 3 filled (fill: linear between fitted
        frames, the nearest fitted t outside them); per_sequence (n_seq,4) = [fitted, filled, mean reproj, path length of joint `root`].
        Non-finite values are not refused: a dead confidence drops the pair, anything else ends in status 2.  Works before finalize(): no
        weight is read.  Nothing synchronises."""
        j3 = self._rows_input(joints3d, "joints3d", (None, 3), torch.float32)
        j2 = self._rows_input(joints2d, "joints2d", (None, 3), torch.float32)
        n = j3.shape[0]
        if j2.shape[0] != n:
            raise ValueError(f"joints3d has {n} frames and joints2d {j2.shape[0]}")
        off = self._sequence_offsets(n, lengths, "joints3d")
        n_seq = len(off) - 1
        table = np.asarray(pairs, np.int64)
        if table.ndim != 2 or table.shape[1] != 2:
            raise ValueError(f"pairs must be (P,2) of (3D index, 2D index), got {table.shape}")
        table = np.ascontiguousarray(table.clip(-1, 2**31 - 1), dtype=np.int32)       # which indices and how many the device takes is the C ABI's to say
        cam = np.empty((n_seq, 3), np.float64)
        try:
            cam[:, 0] = np.asarray(focal_length, np.float64)
            cam[:, 1:] = np.asarray(centre, np.float64)
        except ValueError:
            raise ValueError(f"focal_length must be one number or {n_seq} of them, centre (cx, cy) or ({n_seq},2)") from None
        out = {"per_frame": torch.empty(n, 6, dtype=torch.float64, device=self.device),
               "per_sequence": torch.empty(n_seq, 4, dtype=torch.float64, device=self.device)}
        stream = self._stream()
        rc = self._lib.grnet_fit_translation(self._h, j3.data_ptr(), j3.shape[1], j2.data_ptr(), j2.shape[1], n, _i32p(off), n_seq,
                                             _i32p(table), table.shape[0], cam.ctypes.data_as(C.POINTER(C.c_double)),
                                             float(conf_threshold), int(min_joints), int(root), int(bool(fill)), out["per_frame"].data_ptr(),
                                             out["per_sequence"].data_ptr(), stream)
        _lib.check(self._lib, self._h, rc, "grnet_fit_translation")
        return out

    # ------------------------------------------------------------------ per-frame boxes from 2D joints
    def track_boxes(self, joints2d, lengths=None, vis_thresh=0.3, kernel_size=1, sigma=0.0, pad="zero"):
        """One box per frame from 2D joints on the device (grnet_track_boxes: the reference's lib/utils/smooth_bbox.py and the box of
        lib/dataset/inference.py:57-66; the rules: DESIGN 4.10).  joints2d (T,K,3) rows (x, y, score) in pixels, or (sum T,K,3) with the sequences'
        `lengths` -- numpy or torch, taken as float64; a joint counts where score > vis_thresh.  kernel_size (odd, 1 .. 31; 1: none) and sigma
        (0: none, else <= 16) are the median and the Gaussian of smooth_bbox_params (the reference: 11 and 3 or 8); pad "zero" (scipy's) or
        "edge".  Returns a dict of device tensors: boxes (n,4) float64 [cx, cy, h, h]; status (n,) int32 -- 0 detected, 1 interpolated,
        2 outside [start, end), 3 inside but without a positive finite smoothed scale (2 and 3: a box of zeros); range (n_seq,2) int32
        [start, end), [-1, 0) without any detection.  Non-finite joints are not refused: their frame counts as undetected.  Works before
        finalize(): no weight is read.  Nothing synchronises."""
        j = self._rows_input(joints2d, "joints2d", (None, 3), torch.float64)
        if pad not in _lib.TRACK_PAD:
            raise ValueError(f"pad must be 'zero' or 'edge', got {pad!r}")
        n = j.shape[0]
        off = self._sequence_offsets(n, lengths, "joints2d")
        n_seq = len(off) - 1
        out = {"boxes": torch.empty(n, 4, dtype=torch.float64, device=self.device), "status": torch.empty(n, dtype=torch.int32, device=self.device),
               "range": torch.empty(n_seq, 2, dtype=torch.int32, device=self.device)}
        stream = self._stream()
        rc = self._lib.grnet_track_boxes(self._h, j.data_ptr(), j.shape[1], _i32p(off), n_seq, float(vis_thresh), int(kernel_size),
                                         float(sigma), _lib.TRACK_PAD[pad], out["boxes"].data_ptr(), out["status"].data_ptr(), out["range"].data_ptr(), stream)
        _lib.check(self._lib, self._h, rc, "grnet_track_boxes")
        return out

    def _op_filter1d(self, x, lengths):
        x = self._rows_input(x, "x", (), torch.float64)
        off = self._sequence_offsets(x.shape[0], lengths, "x")
        return x, off, torch.empty_like(x), self._stream()

    def op_median1d(self, x, lengths=None, kernel_size=11, pad="zero"):
        """The median of track_boxes alone (grnet_op_median1d): x (n,) float64, one column or `lengths` of them lying back to back -> (n,) on the device."""
        x, off, out, stream = self._op_filter1d(x, lengths)
        rc = self._lib.grnet_op_median1d(self._h, x.data_ptr(), _i32p(off), len(off) - 1, int(kernel_size), _lib.TRACK_PAD[pad],
                                         out.data_ptr(), stream)
        _lib.check(self._lib, self._h, rc, "grnet_op_median1d")
        return out

    def op_gauss1d(self, x, lengths=None, sigma=3.0):
        """The Gaussian of track_boxes alone (grnet_op_gauss1d): x (n,) float64, one column or `lengths` of them lying back to back -> (n,) on the device."""
        x, off, out, stream = self._op_filter1d(x, lengths)
        rc = self._lib.grnet_op_gauss1d(self._h, x.data_ptr(), _i32p(off), len(off) - 1, float(sigma), out.data_ptr(), stream)
        _lib.check(self._lib, self._h, rc, "grnet_op_gauss1d")
        return out

    # ------------------------------------------------------------------ what the gait calls take alike: the joint table, events, trans
    @staticmethod
    def _joint_table(joints, default, names):
        table = np.asarray(default if joints is None else joints, np.int32).reshape(-1)
        if table.size != len(default):
            raise ValueError(f"joints must name {len(default)} joints ({names}), got {table.size}")
        return table

    def _events_input(self, n, events):
        ev = torch.as_tensor(events).to(self.device, torch.int32).contiguous()
        if tuple(ev.shape) != (n,):
            raise ValueError(f"events must be ({n},), got {tuple(ev.shape)}")
        return ev

    def _trans_input(self, n, trans):
        if trans is None:
            return None
        t = torch.as_tensor(trans).to(self.device, torch.float64).contiguous()
        if tuple(t.shape) != (n, 3):
            raise ValueError(f"trans must be ({n},3), got {tuple(t.shape)}")
        return t

    def _exclude_input(self, n, exclude):
        if exclude is None:
            return None
        ex = torch.as_tensor(exclude).to(self.device, torch.int32).contiguous()
        if tuple(ex.shape) != (n,):
            raise ValueError(f"exclude must be ({n},), got {tuple(ex.shape)}")
        return ex

    # ------------------------------------------------------------------ gait events and parameters from the 3D joints
    def gait_parameters(self, joints3d, lengths=None, trans=None, fps=20.0, sigma=2.0, window=5, min_excursion=0.05, joints=_lib.GAIT_JOINTS_KINECTV2):
        """Heel strikes, toe-offs and the gait parameters of every sequence on the device (grnet_gait_parameters; the rules and the columns: DESIGN
        4.11, pipeline.GAIT_COLUMNS).  joints3d (T,J,3) in the camera frame of the SMPL stage, metres, or (sum T,J,3) with the sequences' `lengths` --
        numpy or torch, taken as float32; joints: the 8 indices pelvis, spine-shoulder, left and right hip, ankle, foot (default: kinectv2,
        pipeline.GAIT_JOINTS_KINECTV2); trans (sum T,3): the camera-space translation of every frame (fit_translation's per_frame[:, :3]; NaN rows
        allowed), taken as float64.  sigma (frames; 0: none, <= 16) smooths the four signals, window (1 .. 32 frames) and min_excursion (metres) rule the
        events.  Returns a dict of device tensors: per_frame (n,7) float64 [hL, hR, tL, tR, wd, step_length, step_width]; events (n,) int32, bit 0 heel
        strike left, 1 heel strike right, 2 toe-off left, 3 toe-off right; per_sequence (n_seq,18) float64.  Nothing is refused on the data: a
        degenerate frame has NaN signals and no events near it.  Works before finalize(): no weight is read.  Nothing synchronises."""
        j = self._rows_input(joints3d, "joints3d", (None, 3), torch.float32)
        n = j.shape[0]
        table = self._joint_table(joints, _lib.GAIT_JOINTS_KINECTV2, _GAIT_JOINT_NAMES)
        t = self._trans_input(n, trans)
        self._whole_frames(window=window)
        off = self._sequence_offsets(n, lengths, "joints3d")
        n_seq = len(off) - 1
        out = {"per_frame": torch.empty(n, 7, dtype=torch.float64, device=self.device), "events": torch.empty(n, dtype=torch.int32, device=self.device),
               "per_sequence": torch.empty(n_seq, 18, dtype=torch.float64, device=self.device)}
        stream = self._stream()
        rc = self._lib.grnet_gait_parameters(self._h, j.data_ptr(), j.shape[1], _i32p(off), n_seq, _i32p(table),
                                             None if t is None else t.data_ptr(), float(fps), float(sigma), int(window), float(min_excursion),
                                             out["per_frame"].data_ptr(), out["events"].data_ptr(), out["per_sequence"].data_ptr(), stream)
        _lib.check(self._lib, self._h, rc, "grnet_gait_parameters")
        return out

    def op_gait_events(self, signals, lengths=None, window=5, min_excursion=0.05):
        """The events rule of gait_parameters alone (grnet_op_gait_events): signals (n,4) float64 [hL, hR, tL, tR], one sequence or `lengths` of them
        lying back to back -> (n,) int32 events on the device."""
        x = self._rows_input(signals, "signals", (4,), torch.float64)
        self._whole_frames(window=window)
        off = self._sequence_offsets(x.shape[0], lengths, "signals")
        out = torch.empty(x.shape[0], dtype=torch.int32, device=self.device)
        rc = self._lib.grnet_op_gait_events(self._h, x.data_ptr(), _i32p(off), len(off) - 1, int(window), float(min_excursion),
                                            out.data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_op_gait_events")
        return out

    # ------------------------------------------------------------------ joint-angle kinematics per gait cycle
    def gait_kinematics(self, joints3d, events, lengths=None, sigma=2.0, min_stride=8, max_stride=60, joints=_lib.KINEMATICS_JOINTS_KINECTV2):
        """Joint angles over time and per gait cycle of every sequence on the device (grnet_gait_kinematics; the rules, channels and columns: DESIGN
        4.12, pipeline.KINEMATICS_CHANNELS, pipeline.KINEMATICS_COLUMNS).  joints3d (T,J,3) in the camera frame of the SMPL stage, metres, or
        (sum T,J,3) with the sequences' `lengths` -- numpy or torch, taken as float32; events (sum T,): what gait_parameters returned, taken as int32;
        joints: the 16 indices pelvis, spine-shoulder, then left and right hip, knee, ankle, foot, shoulder, elbow, wrist (default: kinectv2,
        pipeline.KINEMATICS_JOINTS_KINECTV2).  sigma (frames; 0: none, <= 16) smooths the 13 angle columns; a stride of min_stride .. max_stride frames
        (1 <= min <= max <= 4096) on which a channel is finite is used for it.  Returns a dict of device tensors: per_frame (n,13) float64 degrees;
        curves (n_seq,13,101,2) float64, mean and SD of the cycle curve; per_sequence (n_seq,13,6) float64.  Channel 12 assumes a level camera.
        Nothing is refused on the data.  Works before finalize(): no weight is read.  Nothing synchronises."""
        j = self._rows_input(joints3d, "joints3d", (None, 3), torch.float32)
        n = j.shape[0]
        ev = self._events_input(n, events)
        table = self._joint_table(joints, _lib.KINEMATICS_JOINTS_KINECTV2, _KIN_JOINT_NAMES)
        self._whole_frames(min_stride=min_stride, max_stride=max_stride)
        off = self._sequence_offsets(n, lengths, "joints3d")
        n_seq = len(off) - 1
        out = {"per_frame": torch.empty(n, 13, dtype=torch.float64, device=self.device),
               "curves": torch.empty(n_seq, 13, 101, 2, dtype=torch.float64, device=self.device),
               "per_sequence": torch.empty(n_seq, 13, 6, dtype=torch.float64, device=self.device)}
        stream = self._stream()
        rc = self._lib.grnet_gait_kinematics(self._h, j.data_ptr(), j.shape[1], _i32p(off), n_seq, _i32p(table),
                                             ev.data_ptr(), float(sigma), int(min_stride), int(max_stride), out["per_frame"].data_ptr(), out["curves"].data_ptr(),
                                             out["per_sequence"].data_ptr(), stream)
        _lib.check(self._lib, self._h, rc, "grnet_gait_kinematics")
        return out

    def op_gait_cycles(self, angles, events, lengths=None, min_stride=8, max_stride=60):
        """The cycle stage of gait_kinematics alone (grnet_op_gait_cycles): angles (n,13) float64 and events (n,) int32, one sequence or `lengths` of
        them lying back to back -> {curves (n_seq,13,101,2), per_sequence (n_seq,13,6)} on the device."""
        x = self._rows_input(angles, "angles", (13,), torch.float64)
        ev = self._events_input(x.shape[0], events)
        self._whole_frames(min_stride=min_stride, max_stride=max_stride)
        off = self._sequence_offsets(x.shape[0], lengths, "angles")
        n_seq = len(off) - 1
        out = {"curves": torch.empty(n_seq, 13, 101, 2, dtype=torch.float64, device=self.device),
               "per_sequence": torch.empty(n_seq, 13, 6, dtype=torch.float64, device=self.device)}
        rc = self._lib.grnet_op_gait_cycles(self._h, x.data_ptr(), ev.data_ptr(), _i32p(off), n_seq, int(min_stride), int(max_stride),
                                            out["curves"].data_ptr(), out["per_sequence"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_op_gait_cycles")
        return out

    # ------------------------------------------------------------------ turns and straight-walking gait parameters
    def _turn_inputs(self, n, events, gait_rows, min_frames, max_frames, max_turns):
        ev = self._events_input(n, events)
        rows = torch.as_tensor(gait_rows).to(self.device, torch.float64).contiguous()
        if tuple(rows.shape) != (n, 7):
            raise ValueError(f"gait_rows must be ({n},7), got {tuple(rows.shape)}")
        self._whole_frames(min_frames=min_frames, max_frames=max_frames, max_turns=max_turns)
        if not 1 <= int(max_turns) <= 64:
            raise ValueError(f"max_turns {max_turns} outside [1, 64]")      # the turn table is allocated here: a size the C ABI would refuse is refused first
        return ev, rows

    def _turn_outputs(self, n, n_seq, max_turns):
        return {"phase": torch.empty(n, dtype=torch.int32, device=self.device),
                "turns": torch.empty(n_seq, int(max_turns), 7, dtype=torch.float64, device=self.device),
                "per_sequence": torch.empty(n_seq, 24, dtype=torch.float64, device=self.device)}

    def gait_turns(self, joints3d, events, gait_rows, lengths=None, fps=20.0, sigma=8.0, edge_rate=5.0, peak_rate=15.0, min_angle=45.0, min_frames=10,
                   max_frames=200, max_turns=8, joints=_lib.GAIT_JOINTS_KINECTV2):
        """Turns and the gait parameters of straight walking of every sequence on the device (grnet_gait_turns; the rules and the columns: DESIGN 4.13,
        pipeline.TURN_COLUMNS).  Called after gait_parameters on the same joints3d, lengths and joints, with its `events` (taken as int32) and its
        `per_frame` as gait_rows (sum T,7), taken as float64.  The yaw rate (degrees a second, positive towards the subject's left) is smoothed by sigma
        frames (0: none, <= 16); a run of it beyond +-edge_rate is a turn where it peaks at peak_rate or more, covers min_angle degrees or more and
        lasts min_frames .. max_frames frames.  The defaults follow El-Gohary et al. 2014 and are unvalidated on the model's output; the heading
        assumes a level camera.  Returns a dict of device tensors: per_frame (n,2) float64 [yaw step, yaw rate]; phase (n,) int32 -- 0 straight, 1 left
        turn, 2 right turn, 3 unknown; turns (n_seq,max_turns,7) float64; per_sequence (n_seq,24) float64.  Works before finalize(): no weight is read.
        Nothing synchronises."""
        j = self._rows_input(joints3d, "joints3d", (None, 3), torch.float32)
        n = j.shape[0]
        table = self._joint_table(joints, _lib.GAIT_JOINTS_KINECTV2, _GAIT_JOINT_NAMES)
        ev, rows = self._turn_inputs(n, events, gait_rows, min_frames, max_frames, max_turns)
        off = self._sequence_offsets(n, lengths, "joints3d")
        n_seq = len(off) - 1
        out = self._turn_outputs(n, n_seq, max_turns)
        out["per_frame"] = torch.empty(n, 2, dtype=torch.float64, device=self.device)
        rc = self._lib.grnet_gait_turns(self._h, j.data_ptr(), j.shape[1], _i32p(off), n_seq, _i32p(table), ev.data_ptr(), rows.data_ptr(), float(fps),
                                        float(sigma), float(edge_rate), float(peak_rate), float(min_angle), int(min_frames), int(max_frames), int(max_turns),
                                        out["per_frame"].data_ptr(), out["phase"].data_ptr(), out["turns"].data_ptr(), out["per_sequence"].data_ptr(),
                                        self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_gait_turns")
        return out

    def op_gait_turn_runs(self, rates, events, gait_rows, lengths=None, fps=20.0, edge_rate=5.0, peak_rate=15.0, min_angle=45.0, min_frames=10, max_frames=200,
                          max_turns=8):
        """Rules 4 to 7 of gait_turns alone (grnet_op_gait_turn_runs): rates (n,2) float64 [yaw step, yaw rate], events (n,) and gait_rows (n,7), one
        sequence or `lengths` of them lying back to back -> {phase, turns, per_sequence} on the device."""
        x = self._rows_input(rates, "rates", (2,), torch.float64)
        n = x.shape[0]
        ev, rows = self._turn_inputs(n, events, gait_rows, min_frames, max_frames, max_turns)
        off = self._sequence_offsets(n, lengths, "rates")
        n_seq = len(off) - 1
        out = self._turn_outputs(n, n_seq, max_turns)
        rc = self._lib.grnet_op_gait_turn_runs(self._h, x.data_ptr(), ev.data_ptr(), rows.data_ptr(), _i32p(off), n_seq, float(fps), float(edge_rate),
                                               float(peak_rate), float(min_angle), int(min_frames), int(max_frames), int(max_turns), out["phase"].data_ptr(),
                                               out["turns"].data_ptr(), out["per_sequence"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_op_gait_turn_runs")
        return out

    # ------------------------------------------------------------------ foot contact phases and double support
    def _contact_inputs(self, n, events, reach, max_frames, max_runs):
        ev = self._events_input(n, events)
        self._whole_frames(reach=reach, max_frames=max_frames, max_runs=max_runs)
        if not 1 <= int(max_runs) <= 512:
            raise ValueError(f"max_runs {max_runs} outside [1, 512]")      # the run table is allocated here: a size the C ABI would refuse is refused first
        return ev

    def _contact_outputs(self, n, n_seq, max_runs):
        return {"phase": torch.empty(n, dtype=torch.int32, device=self.device),
                "runs": torch.empty(n_seq, int(max_runs), 6, dtype=torch.float64, device=self.device),
                "per_sequence": torch.empty(n_seq, 20, dtype=torch.float64, device=self.device)}

    def gait_contacts(self, joints3d, events, lengths=None, fps=20.0, sigma=0.0, fraction=0.25, speed=0.0, reach=2, max_frames=20, max_runs=128,
                      joints=_lib.GAIT_JOINTS_KINECTV2):
        """Foot contact phases and double support of every sequence on the device (grnet_gait_contacts; the rules and the columns: DESIGN 4.14,
        pipeline.CONTACT_COLUMNS).  Called after gait_parameters on the same joints3d, lengths and joints, with its `events` (taken as int32).  The
        speed s of the vector from the right ankle to the left one (metres a second; its three columns smoothed by sigma frames first, 0: none,
        <= 16) is about zero while both feet stand; an interval is static where s < fraction * mean s (or < speed, where speed > 0), a maximal run
        of static intervals whose edges lie inside the sequence is closed, and a closed run of at most max_frames intervals is a double support led
        by the foot whose heel strike alone lies within reach frames of it.  The thresholds are unvalidated on the model's output; smoothing
        shortens the runs.  Returns a dict of device tensors: per_frame (n,4) float64 [s, d_x, d_y, d_z]; phase (n,) int32 -- 0 moving, 1 left-led,
        2 right-led, 3 static and unattributed, 4 s is NaN; runs (n_seq,max_runs,6) float64; per_sequence (n_seq,20) float64.  Works before
        finalize(): no weight is read.  Nothing synchronises."""
        j = self._rows_input(joints3d, "joints3d", (None, 3), torch.float32)
        n = j.shape[0]
        table = self._joint_table(joints, _lib.GAIT_JOINTS_KINECTV2, _GAIT_JOINT_NAMES)
        ev = self._contact_inputs(n, events, reach, max_frames, max_runs)
        off = self._sequence_offsets(n, lengths, "joints3d")
        n_seq = len(off) - 1
        out = self._contact_outputs(n, n_seq, max_runs)
        out["per_frame"] = torch.empty(n, 4, dtype=torch.float64, device=self.device)
        rc = self._lib.grnet_gait_contacts(self._h, j.data_ptr(), j.shape[1], _i32p(off), n_seq, _i32p(table), ev.data_ptr(), float(fps), float(sigma),
                                           float(fraction), float(speed), int(reach), int(max_frames), int(max_runs), out["per_frame"].data_ptr(),
                                           out["phase"].data_ptr(), out["runs"].data_ptr(), out["per_sequence"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_gait_contacts")
        return out

    def op_gait_contact_runs(self, speeds, events, lengths=None, fps=20.0, fraction=0.25, speed=0.0, reach=2, max_frames=20, max_runs=128):
        """Rules 3 to 9 of gait_contacts alone (grnet_op_gait_contact_runs): speeds (n,) float64 (the last entry of every sequence is not read) and
        events (n,), one sequence or `lengths` of them lying back to back -> {phase, runs, per_sequence} on the device."""
        x = self._rows_input(speeds, "speeds", (), torch.float64)
        n = x.shape[0]
        ev = self._contact_inputs(n, events, reach, max_frames, max_runs)
        off = self._sequence_offsets(n, lengths, "speeds")
        n_seq = len(off) - 1
        out = self._contact_outputs(n, n_seq, max_runs)
        rc = self._lib.grnet_op_gait_contact_runs(self._h, x.data_ptr(), ev.data_ptr(), _i32p(off), n_seq, float(fps), float(fraction), float(speed), int(reach),
                                                  int(max_frames), int(max_runs), out["phase"].data_ptr(), out["runs"].data_ptr(),
                                                  out["per_sequence"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_op_gait_contact_runs")
        return out

    # ------------------------------------------------------------------ gait regularity and symmetry from the autocorrelation
    def _regularity_call(self, n, lengths, exclude, max_lag, min_lag, min_pairs, what):
        """(exclude on the device or None, offsets, the acf and per_sequence tensors) of gait_regularity and its hook."""
        self._whole_frames(max_lag=max_lag, min_lag=min_lag, min_pairs=min_pairs)
        if not 8 <= int(max_lag) <= 255:                           # the size of acf is made of it here
            raise ValueError(f"max_lag {max_lag} outside [8, 255]")
        ex = self._exclude_input(n, exclude)
        off = self._sequence_offsets(n, lengths, what)
        n_seq = len(off) - 1
        out = {"acf": torch.empty(n_seq, 4, int(max_lag) + 1, dtype=torch.float64, device=self.device),
               "per_sequence": torch.empty(n_seq, 4, 10, dtype=torch.float64, device=self.device)}
        return ex, off, out

    def gait_regularity(self, joints3d, lengths=None, trans=None, exclude=None, fps=20.0, sigma=0.0, max_lag=60, min_lag=4, min_peak=0.25, min_pairs=20,
                        joints=_lib.GAIT_JOINTS_KINECTV2):
        """Gait regularity and symmetry of every sequence WITHOUT EVENTS, on the device (grnet_gait_regularity; the rules, channels and columns: DESIGN
        4.15, pipeline.REGULARITY_CHANNELS, pipeline.REGULARITY_COLUMNS).  joints3d, lengths, trans and joints as gait_parameters takes them (the
        foot entries are not read).  Four signals per frame -- the ankles' separation along the facing (sep) and along the trunk (lift), the trunk's
        lean against the hip line (sway), the pelvis' height in the camera frame (bob, with trans alone) -- each smoothed by sigma frames (0: none,
        <= 16), then per (sequence, channel) the unbiased autocorrelation over the lags 0 .. max_lag (8 .. 255) of the frames that count: those
        whose signal is finite and whose `exclude` entry (sum T, taken as int32; gait_turns' phase: only straight walking counts) is 0, in pairs
        that no other frame lies between.  The first local maximum of at least min_peak from min_lag on is the stride (odd channels) or the step
        (bob); a lag with fewer than min_pairs pairs is undefined.  Returns a dict of device tensors: per_frame (n,4) float64; acf
        (n_seq,4,max_lag+1) float64; per_sequence (n_seq,4,10) float64.  The defaults are unvalidated on the model's output.  Nothing is refused
        on the data.  Works before finalize(): no weight is read.  Nothing synchronises."""
        j = self._rows_input(joints3d, "joints3d", (None, 3), torch.float32)
        n = j.shape[0]
        table = self._joint_table(joints, _lib.GAIT_JOINTS_KINECTV2, _GAIT_JOINT_NAMES)
        t = self._trans_input(n, trans)
        ex, off, out = self._regularity_call(n, lengths, exclude, max_lag, min_lag, min_pairs, "joints3d")
        out["per_frame"] = torch.empty(n, 4, dtype=torch.float64, device=self.device)
        rc = self._lib.grnet_gait_regularity(self._h, j.data_ptr(), j.shape[1], _i32p(off), len(off) - 1, _i32p(table), None if t is None else t.data_ptr(),
                                             None if ex is None else ex.data_ptr(), float(fps), float(sigma), int(max_lag), int(min_lag), float(min_peak),
                                             int(min_pairs), out["per_frame"].data_ptr(), out["acf"].data_ptr(), out["per_sequence"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_gait_regularity")
        return out

    def op_gait_autocorr(self, signals, lengths=None, exclude=None, fps=20.0, max_lag=60, min_lag=4, min_peak=0.25, min_pairs=20):
        """Rules 4 to 8 of gait_regularity alone (grnet_op_gait_autocorr): signals (n,4) float64 and exclude (n,) or None, one sequence or `lengths`
        of them lying back to back -> {acf, per_sequence} on the device."""
        x = self._rows_input(signals, "signals", (4,), torch.float64)
        ex, off, out = self._regularity_call(x.shape[0], lengths, exclude, max_lag, min_lag, min_pairs, "signals")
        rc = self._lib.grnet_op_gait_autocorr(self._h, x.data_ptr(), None if ex is None else ex.data_ptr(), _i32p(off), len(off) - 1, float(fps), int(max_lag),
                                              int(min_lag), float(min_peak), int(min_pairs), out["acf"].data_ptr(), out["per_sequence"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_op_gait_autocorr")
        return out

    # ------------------------------------------------------------------ harmonic ratios per stride
    def _harmonics_call(self, n, events, lengths, exclude, n_harmonics, derivative, min_stride, max_stride, max_strides, what):
        """(events and exclude on the device, offsets, the strides, spectrum and per_sequence tensors) of gait_harmonics and its hook."""
        ev = self._events_input(n, events)
        self._whole_frames(n_harmonics=n_harmonics, derivative=derivative, min_stride=min_stride, max_stride=max_stride, max_strides=max_strides)
        if not 2 <= int(n_harmonics) <= 32 or int(n_harmonics) % 2:        # the sizes of spectrum and strides are made of these here
            raise ValueError(f"n_harmonics {n_harmonics} must be even and within [2, 32]")
        if not 1 <= int(max_strides) <= 512:
            raise ValueError(f"max_strides {max_strides} outside [1, 512]")
        ex = self._exclude_input(n, exclude)
        off = self._sequence_offsets(n, lengths, what)
        n_seq = len(off) - 1
        out = {"strides": torch.empty(n_seq, 4, int(max_strides), 6, dtype=torch.float64, device=self.device),
               "spectrum": torch.empty(n_seq, 4, int(n_harmonics), 2, dtype=torch.float64, device=self.device),
               "per_sequence": torch.empty(n_seq, 4, 12, dtype=torch.float64, device=self.device)}
        return ev, ex, off, out

    def gait_harmonics(self, joints3d, events, lengths=None, trans=None, exclude=None, fps=20.0, sigma=0.0, n_harmonics=20, derivative=2, min_stride=8,
                       max_stride=60, max_strides=128, joints=_lib.GAIT_JOINTS_KINECTV2):
        """Harmonic ratios per stride of every sequence on the device (grnet_gait_harmonics; the rules, channels and columns: DESIGN 4.16,
        pipeline.HARMONICS_CHANNELS, HARMONICS_COLUMNS, HARMONICS_STRIDE_COLUMNS).  Called after gait_parameters on the same joints3d, lengths, trans and
        joints, with its `events` (taken as int32); exclude as gait_regularity takes it.  The four signals of gait_regularity, smoothed by sigma
        frames (0: none, the default, since a Gaussian damps the harmonics it is about to report; <= 16), are cut at consecutive heel strikes of one
        foot; a stride of min_stride .. max_stride (6 .. 255) frames that is finite and not excluded throughout is detrended, its first H <=
        n_harmonics (even, 2 .. 32) harmonics below Nyquist are weighted by k^derivative (2: the acceleration the papers measure) and summed over the
        even and the odd k.  HR is odd / even on sep, lift and sway and even / odd on bob; iHR its bounded form in percent.  Returns a dict of device
        tensors: per_frame (n,4) float64; strides (n_seq,4,max_strides,6); spectrum (n_seq,4,n_harmonics,2); per_sequence (n_seq,4,12).  The
        defaults are unvalidated on the model's output.  Nothing is refused on the data.  Works before finalize(): no weight is read.  Nothing
        synchronises."""
        j = self._rows_input(joints3d, "joints3d", (None, 3), torch.float32)
        n = j.shape[0]
        table = self._joint_table(joints, _lib.GAIT_JOINTS_KINECTV2, _GAIT_JOINT_NAMES)
        t = self._trans_input(n, trans)
        ev, ex, off, out = self._harmonics_call(n, events, lengths, exclude, n_harmonics, derivative, min_stride, max_stride, max_strides, "joints3d")
        out["per_frame"] = torch.empty(n, 4, dtype=torch.float64, device=self.device)
        rc = self._lib.grnet_gait_harmonics(self._h, j.data_ptr(), j.shape[1], _i32p(off), len(off) - 1, _i32p(table), None if t is None else t.data_ptr(),
                                            ev.data_ptr(), None if ex is None else ex.data_ptr(), float(fps), float(sigma), int(n_harmonics), int(derivative),
                                            int(min_stride), int(max_stride), int(max_strides), out["per_frame"].data_ptr(), out["strides"].data_ptr(),
                                            out["spectrum"].data_ptr(), out["per_sequence"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_gait_harmonics")
        return out

    def op_gait_stride_dft(self, signals, events, lengths=None, exclude=None, fps=20.0, n_harmonics=20, derivative=2, min_stride=8, max_stride=60,
                           max_strides=128):
        """Rules 3 to 8 of gait_harmonics alone (grnet_op_gait_stride_dft): signals (n,4) float64, events (n,) and exclude (n,) or None, one sequence or
        `lengths` of them lying back to back -> {strides, spectrum, per_sequence} on the device."""
        x = self._rows_input(signals, "signals", (4,), torch.float64)
        ev, ex, off, out = self._harmonics_call(x.shape[0], events, lengths, exclude, n_harmonics, derivative, min_stride, max_stride, max_strides, "signals")
        rc = self._lib.grnet_op_gait_stride_dft(self._h, x.data_ptr(), ev.data_ptr(), None if ex is None else ex.data_ptr(), _i32p(off), len(off) - 1, float(fps),
                                                int(n_harmonics), int(derivative), int(min_stride), int(max_stride), int(max_strides), out["strides"].data_ptr(),
                                                out["spectrum"].data_ptr(), out["per_sequence"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_op_gait_stride_dft")
        return out

    # ------------------------------------------------------------------ sample entropy at several scales
    def _entropy_call(self, n, lengths, exclude, m, derivative, scales, what):
        """(exclude on the device or None, offsets, the counts and per_sequence tensors) of gait_entropy and its hook."""
        self._whole_frames(m=m, derivative=derivative, scales=scales)
        if not 1 <= int(scales) <= 8:                              # the size of counts is made of it here
            raise ValueError(f"scales {scales} outside [1, 8]")
        ex = self._exclude_input(n, exclude)
        off = self._sequence_offsets(n, lengths, what)
        n_seq = len(off) - 1
        out = {"counts": torch.empty(n_seq, 4, int(scales), 3, dtype=torch.int64, device=self.device),
               "per_sequence": torch.empty(n_seq, 4, 4, dtype=torch.float64, device=self.device)}
        return ex, off, out

    def gait_entropy(self, joints3d, lengths=None, trans=None, exclude=None, sigma=0.0, m=2, fraction=0.2, derivative=2, scales=3,
                     joints=_lib.GAIT_JOINTS_KINECTV2):
        """The counts behind the sample entropy of every sequence at several scales, on the device (grnet_gait_entropy; the rules, channels and
        columns: DESIGN 4.17, pipeline.ENTROPY_CHANNELS, ENTROPY_COLUMNS, ENTROPY_COUNTS).  joints3d, lengths, trans, exclude and joints as
        gait_regularity takes them.  Its four signals, smoothed by sigma frames (0: none, the default; <= 16), are differenced `derivative` times
        (0 .. 2; 2: the acceleration the papers measure); r = fraction (in (0, 10]) times the SD of the frames that count; for every scale tau = 1
        .. scales (<= 8) the signal is averaged over tau frames (Costa's coarse-graining, r kept) and every pair of templates of m + 1 values (m in
        1 .. 4) is compared: B counts the pairs whose first m values lie within r of each other, A those whose next value does too.  A sequence
        has at most 32 768 frames: the work is quadratic in them.  Returns a dict of device tensors: per_frame (n,4) float64, gait_regularity's
        bits; counts (n_seq,4,scales,3) int64 = (valid templates, B, A); per_sequence (n_seq,4,4) float64 = (n, mu, SD, r).  The logarithm is
        pipeline.entropy_rows(counts), on the host.  The defaults are unvalidated on the model's output.  Nothing is refused on the data.  Works
        before finalize(): no weight is read.  Nothing synchronises."""
        j = self._rows_input(joints3d, "joints3d", (None, 3), torch.float32)
        n = j.shape[0]
        table = self._joint_table(joints, _lib.GAIT_JOINTS_KINECTV2, _GAIT_JOINT_NAMES)
        t = self._trans_input(n, trans)
        ex, off, out = self._entropy_call(n, lengths, exclude, m, derivative, scales, "joints3d")
        out["per_frame"] = torch.empty(n, 4, dtype=torch.float64, device=self.device)
        rc = self._lib.grnet_gait_entropy(self._h, j.data_ptr(), j.shape[1], _i32p(off), len(off) - 1, _i32p(table), None if t is None else t.data_ptr(),
                                          None if ex is None else ex.data_ptr(), float(sigma), int(m), float(fraction), int(derivative), int(scales),
                                          out["per_frame"].data_ptr(), out["counts"].data_ptr(), out["per_sequence"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_gait_entropy")
        return out

    def op_gait_sampen(self, signals, lengths=None, exclude=None, m=2, fraction=0.2, derivative=2, scales=3):
        """Rules 2 to 7 of gait_entropy alone (grnet_op_gait_sampen): signals (n,4) float64 and exclude (n,) or None, one sequence or `lengths` of
        them lying back to back -> {counts, per_sequence} on the device."""
        x = self._rows_input(signals, "signals", (4,), torch.float64)
        ex, off, out = self._entropy_call(x.shape[0], lengths, exclude, m, derivative, scales, "signals")
        rc = self._lib.grnet_op_gait_sampen(self._h, x.data_ptr(), None if ex is None else ex.data_ptr(), _i32p(off), len(off) - 1, int(m), float(fraction),
                                            int(derivative), int(scales), out["counts"].data_ptr(), out["per_sequence"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_op_gait_sampen")
        return out

    # ------------------------------------------------------------------ local dynamic stability
    def _stability_call(self, n, lengths, exclude, derivative, dim, lag, theiler, horizon, what):
        """(exclude on the device or None, offsets, the nn, pairs and mant tensors) of gait_stability and its hook."""
        self._whole_frames(derivative=derivative, dim=dim, lag=lag, theiler=theiler, horizon=horizon)
        if not 1 <= int(horizon) <= 63:                            # the size of pairs and mant is made of it here
            raise ValueError(f"horizon {horizon} outside [1, 63]")
        ex = self._exclude_input(n, exclude)
        off = self._sequence_offsets(n, lengths, what)
        n_seq = len(off) - 1
        out = {"nn": torch.empty(n, 4, dtype=torch.int32, device=self.device),
               "pairs": torch.empty(n_seq, 4, int(horizon) + 1, 2, dtype=torch.int64, device=self.device),
               "mant": torch.empty(n_seq, 4, int(horizon) + 1, dtype=torch.float64, device=self.device)}
        return ex, off, out

    def gait_stability(self, joints3d, lengths=None, trans=None, exclude=None, sigma=0.0, derivative=1, dim=5, lag=2, theiler=20, horizon=20,
                       joints=_lib.GAIT_JOINTS_KINECTV2):
        """The integers behind the local dynamic stability of every sequence, on the device (grnet_gait_stability; the rules and channels: DESIGN
        4.18, pipeline.STABILITY_CHANNELS, STABILITY_PAIRS).  joints3d, lengths, trans, exclude and joints as gait_regularity takes them.  Its four
        signals, smoothed by sigma frames (0: none, the default; <= 16), are differenced `derivative` times (0 .. 2; 1, velocities, is this
        project's choice) and embedded with `dim` (2 .. 8) delays of `lag` (1 .. 16) frames; every point that can be followed for `horizon`
        (1 .. 63) frames gets its nearest neighbour among those more than `theiler` (0 .. 4096) frames away, and for k = 0 .. horizon the squared
        distances of the pairs k frames later are multiplied up as a mantissa P with an exponent S.  A sequence has at most 32 768 frames: the
        work is quadratic in them.  Returns a dict of device tensors: per_frame (n,4) float64, gait_regularity's bits; nn (n,4) int32,
        sequence-relative, -1 where there is none; pairs (n_seq,4,horizon+1,2) int64 = (n, S); mant (n_seq,4,horizon+1) float64 = P.  The
        logarithm and the slope are pipeline.stability_rows(pairs, mant), on the host.  The papers use a trunk sensor and 100+ strides; the
        defaults are unvalidated on the model's output, and on noisy joints the slope mostly measures the noise.  Nothing is refused on the data.
        Works before finalize(): no weight is read.  Nothing synchronises."""
        j = self._rows_input(joints3d, "joints3d", (None, 3), torch.float32)
        n = j.shape[0]
        table = self._joint_table(joints, _lib.GAIT_JOINTS_KINECTV2, _GAIT_JOINT_NAMES)
        t = self._trans_input(n, trans)
        ex, off, out = self._stability_call(n, lengths, exclude, derivative, dim, lag, theiler, horizon, "joints3d")
        out["per_frame"] = torch.empty(n, 4, dtype=torch.float64, device=self.device)
        rc = self._lib.grnet_gait_stability(self._h, j.data_ptr(), j.shape[1], _i32p(off), len(off) - 1, _i32p(table), None if t is None else t.data_ptr(),
                                            None if ex is None else ex.data_ptr(), float(sigma), int(derivative), int(dim), int(lag), int(theiler), int(horizon),
                                            out["per_frame"].data_ptr(), out["nn"].data_ptr(), out["pairs"].data_ptr(), out["mant"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_gait_stability")
        return out

    def op_gait_divergence(self, signals, lengths=None, exclude=None, derivative=1, dim=5, lag=2, theiler=20, horizon=20):
        """Rules 1 (from the differencing on) to 6 of gait_stability alone (grnet_op_gait_divergence): signals (n,4) float64 and exclude (n,) or None,
        one sequence or `lengths` of them lying back to back -> {nn, pairs, mant} on the device."""
        x = self._rows_input(signals, "signals", (4,), torch.float64)
        ex, off, out = self._stability_call(x.shape[0], lengths, exclude, derivative, dim, lag, theiler, horizon, "signals")
        rc = self._lib.grnet_op_gait_divergence(self._h, x.data_ptr(), None if ex is None else ex.data_ptr(), _i32p(off), len(off) - 1, int(derivative), int(dim),
                                                int(lag), int(theiler), int(horizon), out["nn"].data_ptr(), out["pairs"].data_ptr(), out["mant"].data_ptr(),
                                                self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_op_gait_divergence")
        return out

    # ------------------------------------------------------------------ recurrence quantification
    def _recurrence_call(self, n, lengths, exclude, derivative, dim, lag, theiler, what):
        """(exclude on the device or None, offsets, the per_sequence, hist and counts tensors) of gait_recurrence and its hook."""
        self._whole_frames(derivative=derivative, dim=dim, lag=lag, theiler=theiler)
        ex = self._exclude_input(n, exclude)
        off = self._sequence_offsets(n, lengths, what)
        n_seq = len(off) - 1
        out = {"per_sequence": torch.empty(n_seq, 4, 5, dtype=torch.float64, device=self.device),
               "hist": torch.empty(n_seq, 4, 255, dtype=torch.int64, device=self.device),
               "counts": torch.empty(n_seq, 4, 6, dtype=torch.int64, device=self.device)}
        return ex, off, out

    def gait_recurrence(self, joints3d, lengths=None, trans=None, exclude=None, sigma=0.0, derivative=1, dim=5, lag=2, theiler=8, radius=0.8,
                        joints=_lib.GAIT_JOINTS_KINECTV2):
        """The integers behind the recurrence quantification of every sequence, on the device (grnet_gait_recurrence; the rules, channels and
        columns: DESIGN 4.20, pipeline.RECURRENCE_CHANNELS, RECURRENCE_COLUMNS, RECURRENCE_COUNTS, RECURRENCE_BINS).  joints3d, lengths, trans,
        exclude and joints as gait_regularity takes them.  Its four signals, smoothed by sigma frames (0: none, the default; <= 16), are
        differenced `derivative` times (0 .. 2; 1, velocities, as gait_stability) and embedded with `dim` (2 .. 8) delays of `lag` (1 .. 16)
        frames; every pair of valid points more than `theiler` (0 .. 4096) frames apart is comparable, and recurrent where its squared distance
        is at most eps2 = (radius SD)^2 dim (radius in (0, 10], SD of the frames that count); along every diagonal the runs of recurrent pairs
        are lines, counted by their length.  A sequence has at most 32 768 frames: the work is quadratic in them.  Returns a dict of device
        tensors: per_frame (n,4) float64, gait_regularity's bits; per_sequence (n_seq,4,5) float64 = (n, mu, SD, r, eps2); hist (n_seq,4,255)
        int64, the lines of length 1 .. 255; counts (n_seq,4,6) int64 = (points, comparable, recurrent, long_lines, long_points, longest).  The
        line threshold, the rates and the logarithm are pipeline.recurrence_rows(counts, hist), on the host.  The papers use a trunk sensor and
        minutes of walking; the radius rule is this project's and the defaults are unvalidated on the model's output.  Nothing is refused on the
        data.  Works before finalize(): no weight is read.  Nothing synchronises."""
        j = self._rows_input(joints3d, "joints3d", (None, 3), torch.float32)
        n = j.shape[0]
        table = self._joint_table(joints, _lib.GAIT_JOINTS_KINECTV2, _GAIT_JOINT_NAMES)
        t = self._trans_input(n, trans)
        ex, off, out = self._recurrence_call(n, lengths, exclude, derivative, dim, lag, theiler, "joints3d")
        out["per_frame"] = torch.empty(n, 4, dtype=torch.float64, device=self.device)
        rc = self._lib.grnet_gait_recurrence(self._h, j.data_ptr(), j.shape[1], _i32p(off), len(off) - 1, _i32p(table), None if t is None else t.data_ptr(),
                                             None if ex is None else ex.data_ptr(), float(sigma), int(derivative), int(dim), int(lag), int(theiler), float(radius),
                                             out["per_frame"].data_ptr(), out["per_sequence"].data_ptr(), out["hist"].data_ptr(), out["counts"].data_ptr(),
                                             self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_gait_recurrence")
        return out

    def op_gait_recurrence_counts(self, signals, lengths=None, exclude=None, derivative=1, dim=5, lag=2, theiler=8, radius=0.8):
        """Rules 1 (from the differencing on) to 6 of gait_recurrence alone (grnet_op_gait_recurrence_counts): signals (n,4) float64 and exclude
        (n,) or None, one sequence or `lengths` of them lying back to back -> {per_sequence, hist, counts} on the device."""
        x = self._rows_input(signals, "signals", (4,), torch.float64)
        ex, off, out = self._recurrence_call(x.shape[0], lengths, exclude, derivative, dim, lag, theiler, "signals")
        rc = self._lib.grnet_op_gait_recurrence_counts(self._h, x.data_ptr(), None if ex is None else ex.data_ptr(), _i32p(off), len(off) - 1, int(derivative),
                                                       int(dim), int(lag), int(theiler), float(radius), out["per_sequence"].data_ptr(), out["hist"].data_ptr(),
                                                       out["counts"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_op_gait_recurrence_counts")
        return out

    # ------------------------------------------------------------------ the Welch spectrum
    def _spectrum_call(self, n, lengths, exclude, derivative, segment, hop, nfft, min_segments, what):
        """(exclude on the device or None, offsets, hop, the psd and per_sequence tensors) of gait_spectrum and its hook."""
        if hop is None:
            hop = segment // 2 if int(segment) == segment else segment
        self._whole_frames(derivative=derivative, segment=segment, hop=hop, nfft=nfft, min_segments=min_segments)
        if not 8 <= int(nfft) <= 1024 or int(nfft) % 2:             # the size of psd is made of it here
            raise ValueError("nfft must be even and within [segment, 1024]")
        ex = self._exclude_input(n, exclude)
        off = self._sequence_offsets(n, lengths, what)
        n_seq = len(off) - 1
        out = {"psd": torch.empty(n_seq, 4, int(nfft) // 2 + 1, dtype=torch.float64, device=self.device),
               "per_sequence": torch.empty(n_seq, 4, 13, dtype=torch.float64, device=self.device)}
        return ex, off, int(hop), out

    def gait_spectrum(self, joints3d, lengths=None, trans=None, exclude=None, fps=20.0, sigma=0.0, derivative=2, segment=64, hop=None, nfft=256, f_lo=0.5,
                      f_hi=3.0, min_segments=2, joints=_lib.GAIT_JOINTS_KINECTV2):
        """The Welch power spectral density of every sequence's four body signals, on the device (grnet_gait_spectrum; the rules, channels and
        columns: DESIGN 4.19, pipeline.SPECTRUM_CHANNELS, SPECTRUM_COLUMNS).  joints3d, lengths, trans, exclude and joints as gait_regularity takes
        them.  Its four signals, smoothed by sigma frames (0: none, the default; <= 16), are differenced `derivative` times (0 .. 2; 2: the
        acceleration the papers measure); inside every run of frames that count, segments of `segment` frames (even, 8 .. 256) are laid `hop` apart
        (segment / 8 .. segment; None: segment / 2), each has its mean taken off, is weighted by a periodic Hann window and zero-padded to `nfft`
        (even, segment .. 1024), and the squared magnitudes of its transform are averaged over the segments, as scipy.signal.welch scales a
        density; fewer than min_segments segments give NaN.  The row reads the band [f_lo, f_hi] Hz (0 < f_lo < f_hi <= fps / 2): its power, the
        dominant peak's bin, refined frequency, height and width at half height, the share of the three bins round it, the centroid, the 95 % edge
        and a cadence (120 or 60 times the peak's frequency by channel).  A sequence has at most 32 768 frames.  Returns a dict of device tensors:
        per_frame (n,4) float64, gait_regularity's bits; psd (n_seq,4,nfft/2+1) float64; per_sequence (n_seq,4,13) float64.  The spectral entropy
        is pipeline.spectrum_rows(psd, per_sequence), on the host.  The papers use a trunk accelerometer; the peak's width has a floor set by
        `segment` (about 0.45 Hz at 20 fps and 64 frames), and the defaults are unvalidated on the model's output.  Nothing is refused on the
        data.  Works before finalize(): no weight is read.  Nothing synchronises."""
        j = self._rows_input(joints3d, "joints3d", (None, 3), torch.float32)
        n = j.shape[0]
        table = self._joint_table(joints, _lib.GAIT_JOINTS_KINECTV2, _GAIT_JOINT_NAMES)
        t = self._trans_input(n, trans)
        ex, off, hop, out = self._spectrum_call(n, lengths, exclude, derivative, segment, hop, nfft, min_segments, "joints3d")
        out["per_frame"] = torch.empty(n, 4, dtype=torch.float64, device=self.device)
        rc = self._lib.grnet_gait_spectrum(self._h, j.data_ptr(), j.shape[1], _i32p(off), len(off) - 1, _i32p(table), None if t is None else t.data_ptr(),
                                           None if ex is None else ex.data_ptr(), float(fps), float(sigma), int(derivative), int(segment), hop, int(nfft),
                                           float(f_lo), float(f_hi), int(min_segments), out["per_frame"].data_ptr(), out["psd"].data_ptr(),
                                           out["per_sequence"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_gait_spectrum")
        return out

    def op_gait_welch(self, signals, lengths=None, exclude=None, fps=20.0, derivative=2, segment=64, hop=None, nfft=256, f_lo=0.5, f_hi=3.0, min_segments=2):
        """Rules 1 (from the differencing on) to 5 of gait_spectrum alone (grnet_op_gait_welch): signals (n,4) float64 and exclude (n,) or None, one
        sequence or `lengths` of them lying back to back -> {psd, per_sequence} on the device."""
        x = self._rows_input(signals, "signals", (4,), torch.float64)
        ex, off, hop, out = self._spectrum_call(x.shape[0], lengths, exclude, derivative, segment, hop, nfft, min_segments, "signals")
        rc = self._lib.grnet_op_gait_welch(self._h, x.data_ptr(), None if ex is None else ex.data_ptr(), _i32p(off), len(off) - 1, float(fps), int(derivative),
                                           int(segment), hop, int(nfft), float(f_lo), float(f_hi), int(min_segments), out["psd"].data_ptr(),
                                           out["per_sequence"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_op_gait_welch")
        return out

    # ------------------------------------------------------------------ movement smoothness
    @staticmethod
    def smoothness_slots(lengths, segment=64, hop=None):
        """The prefix sums of the slots of sequences of `lengths` frames (grnet_gait_smoothness_slots' formula): a sequence of T frames has
        (T - segment) // hop + 1 slots, 0 where T < segment.  (n_seq + 1,) int64."""
        if hop is None:
            hop = segment // 2
        at = np.zeros(len(lengths) + 1, np.int64)
        at[1:] = np.cumsum([(int(T) - int(segment)) // int(hop) + 1 if int(T) >= int(segment) else 0 for T in lengths])
        return at

    def _smoothness_call(self, n, lengths, exclude, fps, derivative, segment, hop, nfft, f_cut, min_segments, what):
        """(exclude on the device or None, offsets, hop, f_cut, the per_segment and per_sequence tensors, slot_offsets) of gait_smoothness and its hook."""
        if hop is None:
            hop = segment // 2 if int(segment) == segment else segment
        if f_cut is None:
            f_cut = min(10.0, float(fps) / 2.0)
        self._whole_frames(derivative=derivative, segment=segment, hop=hop, nfft=nfft, min_segments=min_segments)
        if not 8 <= int(segment) <= 256 or int(segment) % 2:        # the size of per_segment is made of these here
            raise ValueError("segment must be even and within [8, 256]")
        if not int(segment) // 8 <= int(hop) <= int(segment):
            raise ValueError("hop outside [segment / 8, segment]")
        ex = self._exclude_input(n, exclude)
        off = self._sequence_offsets(n, lengths, what)
        n_seq = len(off) - 1
        slots = self.smoothness_slots(np.diff(off), int(segment), int(hop))
        out = {"per_segment": torch.empty(int(slots[-1]), 4, 8, dtype=torch.float64, device=self.device),
               "per_sequence": torch.empty(n_seq, 4, 10, dtype=torch.float64, device=self.device), "slot_offsets": slots}
        return ex, off, int(hop), float(f_cut), out

    def gait_smoothness(self, joints3d, lengths=None, trans=None, exclude=None, fps=20.0, sigma=0.0, derivative=1, segment=64, hop=None, nfft=1024, f_cut=None,
                        amplitude=0.05, min_segments=2, joints=_lib.GAIT_JOINTS_KINECTV2):
        """The movement smoothness of every sequence's four body signals, per segment of ongoing walking, on the device (grnet_gait_smoothness; the
        rules, channels and columns: DESIGN 4.24, pipeline.SMOOTHNESS_CHANNELS, SMOOTHNESS_SEGMENT_COLUMNS, SMOOTHNESS_COLUMNS).  joints3d, lengths,
        trans, exclude and joints as gait_regularity takes them.  Its four signals, smoothed by sigma frames (0: none, the default; <= 16), are
        differenced `derivative` times (0 .. 2; 1: the speed profile the measure is defined on); inside every run of frames that count, segments of
        `segment` frames (even, 8 .. 256) are laid `hop` apart (segment / 8 .. segment; None: segment / 2).  Each segment, with no mean taken off
        and no window, is zero-padded to `nfft` (even, segment .. 4096) and the magnitudes of its transform up to f_cut Hz (0 < f_cut <= fps / 2;
        None: min(10, fps / 2)) are divided by the largest; the spectral arc length (SPARC; Balasubramanian et al. 2015) is minus the length of that
        curve between the first and the last bin at or above `amplitude` (in (0, 1]), the band's width scaled to 1.  The dimensionless jerk of the
        same frames of the undifferenced signal stands beside it; its logarithm (LDLJ) is pipeline.smoothness_rows', on the host.  Fewer than
        min_segments segments give a NaN row; the segment rows are written whatever it is.  A sequence has at most 32 768 frames.  Returns a dict:
        per_frame (n,4) float64, gait_regularity's bits; per_segment (slots,4,8) float64, the sequences' slots back to back, NaN behind each one's
        candidates; per_sequence (n_seq,4,10) float64 -- device tensors -- and slot_offsets (n_seq+1,) int64 numpy.  THE INPUTS ARE JOINT
        POSITIONS OF A POSE MODEL AT 20 FPS, where 10 Hz is the Nyquist frequency; A SEGMENT'S RECTANGULAR WINDOW ALONE gives a noiseless sinusoid
        SPARC = -3.96 +- 0.30 at 64 frames, and with 5 mm of joint noise a good part of the number is the noise; THE DEFAULTS ARE UNVALIDATED on the
        model's output.  Nothing is refused on the data.  Works before finalize(): no weight is read.  Nothing synchronises."""
        j = self._rows_input(joints3d, "joints3d", (None, 3), torch.float32)
        n = j.shape[0]
        table = self._joint_table(joints, _lib.GAIT_JOINTS_KINECTV2, _GAIT_JOINT_NAMES)
        t = self._trans_input(n, trans)
        ex, off, hop, f_cut, out = self._smoothness_call(n, lengths, exclude, fps, derivative, segment, hop, nfft, f_cut, min_segments, "joints3d")
        out["per_frame"] = torch.empty(n, 4, dtype=torch.float64, device=self.device)
        rc = self._lib.grnet_gait_smoothness(self._h, j.data_ptr(), j.shape[1], _i32p(off), len(off) - 1, _i32p(table), None if t is None else t.data_ptr(),
                                             None if ex is None else ex.data_ptr(), float(fps), float(sigma), int(derivative), int(segment), hop, int(nfft),
                                             f_cut, float(amplitude), int(min_segments), out["per_frame"].data_ptr(), out["per_segment"].data_ptr() or None,
                                             out["per_sequence"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_gait_smoothness")
        return out

    def op_gait_sparc(self, signals, lengths=None, exclude=None, fps=20.0, derivative=1, segment=64, hop=None, nfft=1024, f_cut=None, amplitude=0.05,
                      min_segments=2):
        """Rules 1 (from the differencing on) to 7 of gait_smoothness alone (grnet_op_gait_sparc): signals (n,4) float64 and exclude (n,) or None, one
        sequence or `lengths` of them lying back to back -> {per_segment, per_sequence} on the device and slot_offsets."""
        x = self._rows_input(signals, "signals", (4,), torch.float64)
        ex, off, hop, f_cut, out = self._smoothness_call(x.shape[0], lengths, exclude, fps, derivative, segment, hop, nfft, f_cut, min_segments, "signals")
        rc = self._lib.grnet_op_gait_sparc(self._h, x.data_ptr(), None if ex is None else ex.data_ptr(), _i32p(off), len(off) - 1, float(fps), int(derivative),
                                           int(segment), hop, int(nfft), f_cut, float(amplitude), int(min_segments), out["per_segment"].data_ptr() or None,
                                           out["per_sequence"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_op_gait_sparc")
        return out

    # ------------------------------------------------------------------ arm swing and inter-limb coordination
    def _coordination_call(self, n, lengths, exclude, derivative, segment, hop, nfft, min_segments, what):
        """(exclude on the device or None, offsets, hop, the auto, cross, limbs and pairs tensors) of gait_coordination and its hook."""
        if hop is None:
            hop = segment // 2 if int(segment) == segment else segment
        self._whole_frames(derivative=derivative, segment=segment, hop=hop, nfft=nfft, min_segments=min_segments)
        if not 8 <= int(nfft) <= 1024 or int(nfft) % 2:             # the sizes of auto and cross are made of it here
            raise ValueError("nfft must be even and within [segment, 1024]")
        ex = self._exclude_input(n, exclude)
        off = self._sequence_offsets(n, lengths, what)
        n_seq, bins = len(off) - 1, int(nfft) // 2 + 1
        out = {"auto": torch.empty(n_seq, 4, bins, dtype=torch.float64, device=self.device),
               "cross": torch.empty(n_seq, 6, bins, 2, dtype=torch.float64, device=self.device),
               "limbs": torch.empty(n_seq, 4, 13, dtype=torch.float64, device=self.device),
               "pairs": torch.empty(n_seq, 6, 10, dtype=torch.float64, device=self.device)}
        return ex, off, int(hop), out

    def gait_coordination(self, joints3d, lengths=None, exclude=None, fps=20.0, sigma=0.0, derivative=0, segment=64, hop=None, nfft=256, f_lo=0.5, f_hi=3.0,
                          min_segments=4, joints=_lib.KINEMATICS_JOINTS_KINECTV2):
        """Arm swing and inter-limb coordination of every sequence, on the device (grnet_gait_coordination; the rules, channels, pairs and columns:
        DESIGN 4.21, pipeline.COORDINATION_CHANNELS, COORDINATION_PAIRS, COORDINATION_LIMB_COLUMNS, COORDINATION_PAIR_COLUMNS).  joints3d, lengths,
        exclude and joints (16 indices) as gait_kinematics and gait_spectrum take them.  The shoulder flexion left / right and the hip flexion left /
        right in degrees, gait_kinematics's bits at the same sigma (0: none, the default; <= 16), are differenced `derivative` times (0 .. 2; 0:
        amplitudes are degrees); a frame counts iff all four values are finite, so every limb and pair is estimated on the same segments, laid,
        windowed and transformed as gait_spectrum's (`segment`, `hop`, `nfft`); fewer than min_segments (2 .. 2^20) give NaN, and one segment is
        refused because its coherence is 1 whatever the signals are.  Returns a dict of device tensors: per_frame (n,4) float64; auto
        (n_seq,4,nfft/2+1) densities; cross (n_seq,6,nfft/2+1,2), real and imaginary part of conj(X_a) X_b, scipy.signal.csd(a, b)'s sign: a
        positive phase means b leads a; limbs (n_seq,4,13), gait_spectrum's columns with cadence = 120 peak_hz; pairs (n_seq,6,10): at the bin of
        [f_lo, f_hi] with the largest cross magnitude its frequency, magnitude, coherence (not clamped), phase in degrees, the phase's deviation
        from the expected 0 or 180, the lag in seconds, and the band's mean coherence.  The amplitudes and asymmetries are
        pipeline.coordination_rows(limbs, pairs), on the host.  With K segments the coherence of unrelated signals is about 1 / K (0.09 at the 11
        segments of 400 frames), not 0; the defaults are unvalidated on the model's output, and the numbers are reported, never judged.  A sequence
        has at most 32 768 frames.  Nothing is refused on the data.  Works before finalize(): no weight is read.  Nothing synchronises."""
        j = self._rows_input(joints3d, "joints3d", (None, 3), torch.float32)
        n = j.shape[0]
        table = self._joint_table(joints, _lib.KINEMATICS_JOINTS_KINECTV2, _KIN_JOINT_NAMES)
        ex, off, hop, out = self._coordination_call(n, lengths, exclude, derivative, segment, hop, nfft, min_segments, "joints3d")
        out["per_frame"] = torch.empty(n, 4, dtype=torch.float64, device=self.device)
        rc = self._lib.grnet_gait_coordination(self._h, j.data_ptr(), j.shape[1], _i32p(off), len(off) - 1, _i32p(table), None if ex is None else ex.data_ptr(),
                                               float(fps), float(sigma), int(derivative), int(segment), hop, int(nfft), float(f_lo), float(f_hi),
                                               int(min_segments), out["per_frame"].data_ptr(), out["auto"].data_ptr(), out["cross"].data_ptr(),
                                               out["limbs"].data_ptr(), out["pairs"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_gait_coordination")
        return out

    def op_gait_cross_welch(self, signals, lengths=None, exclude=None, fps=20.0, derivative=0, segment=64, hop=None, nfft=256, f_lo=0.5, f_hi=3.0,
                            min_segments=4):
        """Rules 2 to 7 of gait_coordination alone (grnet_op_gait_cross_welch): signals (n,4) float64 and exclude (n,) or None, one sequence or
        `lengths` of them lying back to back -> {auto, cross, limbs, pairs} on the device."""
        x = self._rows_input(signals, "signals", (4,), torch.float64)
        ex, off, hop, out = self._coordination_call(x.shape[0], lengths, exclude, derivative, segment, hop, nfft, min_segments, "signals")
        rc = self._lib.grnet_op_gait_cross_welch(self._h, x.data_ptr(), None if ex is None else ex.data_ptr(), _i32p(off), len(off) - 1, float(fps),
                                                 int(derivative), int(segment), hop, int(nfft), float(f_lo), float(f_hi), int(min_segments),
                                                 out["auto"].data_ptr(), out["cross"].data_ptr(), out["limbs"].data_ptr(), out["pairs"].data_ptr(),
                                                 self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_op_gait_cross_welch")
        return out

    # ------------------------------------------------------------------ footprints, centre of mass and margin of stability
    def _balance_call(self, n, lengths, events, window, settle, max_step, max_steps, what):
        """(events on the device, offsets, the three output tensors) of gait_balance and its hook."""
        ev = self._events_input(n, events)
        self._whole_frames(window=window, settle=settle, max_step=max_step, max_steps=max_steps)
        if not 1 <= int(max_steps) <= 1024:
            raise ValueError(f"max_steps {max_steps} outside [1, 1024]")      # the step table is allocated here: a size the C ABI would refuse is refused first
        off = self._sequence_offsets(n, lengths, what)
        n_seq = len(off) - 1
        out = {"per_frame": torch.empty(n, 8, dtype=torch.float64, device=self.device),
               "steps": torch.empty(n_seq, int(max_steps), 15, dtype=torch.float64, device=self.device),
               "per_sequence": torch.empty(n_seq, 24, dtype=torch.float64, device=self.device)}
        return ev, off, out

    def gait_balance(self, joints3d, events, lengths=None, fps=20.0, gravity=9.81, window=4, settle=1, max_step=30, max_steps=256,
                     segments=None, joints=_lib.GAIT_JOINTS_KINECTV2, com=None):
        """Footprints on the floor, the centre of mass over them and the margin of stability at foot placement of every sequence on the device
        (grnet_gait_balance; the rules and the columns: DESIGN 4.22, pipeline.BALANCE_COLUMNS).  Called after gait_parameters on the same joints3d,
        lengths and joints, with its `events` (taken as int32).  segments: rows of (proximal joint, distal joint, mass, the COM's fraction from the
        proximal joint), at most 16.  A foot on the ground stands still in the world: the vector between the ankles `settle` frames after a heel
        strike is a footprint-to-footprint vector, and the COM relative to the planted ankle, fitted over the last `window` + 1 frames of a step,
        gives its velocity.  THE FLOOR IS THE x-z PLANE OF A LEVEL, FIXED CAMERA; the segment layout is unvalidated; a margin of a few centimetres
        carries about two of noise per step.  Returns a dict of device tensors: per_frame (n,8) float64 [c, W, stance side, chain]; steps
        (n_seq,max_steps,15) float64; per_sequence (n_seq,24) float64.  Works before finalize(): no weight is read.  Nothing synchronises.
        segments: None stands for BALANCE_SEGMENTS_KINECTV2.  com (n,3), taken as float64 on the device: the centre of mass of every frame in
        place of the segment table's -- columns 1 to 3 of mesh_moments' rows (grnet_gait_balance_com); together with segments it is refused."""
        j = self._rows_input(joints3d, "joints3d", (None, 3), torch.float32)
        n = j.shape[0]
        table = self._joint_table(joints, _lib.GAIT_JOINTS_KINECTV2, _GAIT_JOINT_NAMES)
        if com is not None:
            if segments is not None:
                raise ValueError("segments and com are two sources of the centre of mass: give one")
            c = self._rows_input(com, "com", (3,), torch.float64)
            if c.shape[0] != n:
                raise ValueError(f"com must be ({n},3), got {tuple(c.shape)}")
            ev, off, out = self._balance_call(n, lengths, events, window, settle, max_step, max_steps, "joints3d")
            rc = self._lib.grnet_gait_balance_com(self._h, j.data_ptr(), j.shape[1], _i32p(off), len(off) - 1, _i32p(table), ev.data_ptr(), c.data_ptr(), float(fps),
                                                  float(gravity), int(window), int(settle), int(max_step), int(max_steps), out["per_frame"].data_ptr(),
                                                  out["steps"].data_ptr(), out["per_sequence"].data_ptr(), self._stream())
            _lib.check(self._lib, self._h, rc, "grnet_gait_balance_com")
            return out
        seg = np.asarray(_lib.BALANCE_SEGMENTS_KINECTV2 if segments is None else segments, np.float64)
        if seg.ndim != 2 or seg.shape[1] != 4 or seg.shape[0] < 1 or not np.array_equal(seg[:, :2], np.floor(seg[:, :2])) or np.abs(seg[:, :2]).max() >= 2**31:
            raise ValueError(f"segments must be rows of (proximal joint, distal joint, mass, fraction), got shape {seg.shape}")
        pairs, weights = np.ascontiguousarray(seg[:, :2], np.int32), np.ascontiguousarray(seg[:, 2:])
        ev, off, out = self._balance_call(n, lengths, events, window, settle, max_step, max_steps, "joints3d")
        rc = self._lib.grnet_gait_balance(self._h, j.data_ptr(), j.shape[1], _i32p(off), len(off) - 1, _i32p(table), ev.data_ptr(), _i32p(pairs),
                                          weights.ctypes.data_as(C.POINTER(C.c_double)), int(seg.shape[0]), float(fps), float(gravity), int(window),
                                          int(settle), int(max_step), int(max_steps), out["per_frame"].data_ptr(), out["steps"].data_ptr(),
                                          out["per_sequence"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_gait_balance")
        return out

    def op_gait_balance_steps(self, rel, events, lengths=None, fps=20.0, gravity=9.81, window=4, settle=1, max_step=30, max_steps=256):
        """Rules 2 to 8 of gait_balance alone (grnet_op_gait_balance_steps): rel (n,9) float64 = [c, rL, rR] and events (n,), one sequence or
        `lengths` of them lying back to back -> {per_frame, steps, per_sequence} on the device."""
        x = self._rows_input(rel, "rel", (9,), torch.float64)
        ev, off, out = self._balance_call(x.shape[0], lengths, events, window, settle, max_step, max_steps, "rel")
        rc = self._lib.grnet_op_gait_balance_steps(self._h, x.data_ptr(), ev.data_ptr(), _i32p(off), len(off) - 1, float(fps), float(gravity), int(window),
                                                   int(settle), int(max_step), int(max_steps), out["per_frame"].data_ptr(), out["steps"].data_ptr(),
                                                   out["per_sequence"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_op_gait_balance_steps")
        return out

    # ------------------------------------------------------------------ mesh volume, centre of mass and second moments
    def faces_closed(self):
        """How many directed edges of the loaded face table are duplicated, lack their reverse edge or join a vertex to itself
        (grnet_faces_closed; host only, counted once per load_faces): 0 for a closed, consistently oriented surface, the only kind mesh_moments takes."""
        count = C.c_int(-1)
        _lib.check(self._lib, self._h, self._lib.grnet_faces_closed(self._h, C.byref(count)), "grnet_faces_closed")
        return int(count.value)

    def mesh_moments(self, verts, return_sums=False, form=None):
        """Volume, centre of mass, central second moments per unit volume and area of the closed mesh of every frame on the device
        (grnet_mesh_moments; the rules and the columns: DESIGN 4.25, pipeline.MESH_MOMENT_COLUMNS).  verts (n,6890,3), any float dtype, taken as
        float32 on the device: what forward() returned as 'verts'.  Needs load_faces (load_smpl loads the table of SMPL_NEUTRAL.npz).  Returns
        rows (n,11) float64 on the device; with return_sums (rows, sums (n,11)).  Where the signed volume is not positive the nine columns of the
        centre and the moments are NaN.  UNIFORM DENSITY IS AN ASSUMPTION; the mesh is a statistical body shape, not the subject's.  form: None,
        or 0 / 1 to name the kernel's gather (grnet_op_mesh_moments: the same bits).  Works before finalize().  Nothing synchronises."""
        v = torch.as_tensor(verts)
        if v.dim() != 3 or v.shape[0] < 1 or tuple(v.shape[1:]) != (netspec.NUM_VERTS, 3) or not v.dtype.is_floating_point:
            raise ValueError(f"verts must be a float (n,{netspec.NUM_VERTS},3) tensor with n >= 1, got {v.dtype} {tuple(v.shape)}")
        v = v.to(self.device, torch.float32).contiguous()
        n = v.shape[0]
        rows = torch.empty(n, 11, dtype=torch.float64, device=self.device)
        sums = torch.empty(n, 11, dtype=torch.float64, device=self.device) if return_sums else None
        sums_ptr = sums.data_ptr() if return_sums else None
        if form is None:
            rc, what = self._lib.grnet_mesh_moments(self._h, v.data_ptr(), n, rows.data_ptr(), sums_ptr, self._stream()), "grnet_mesh_moments"
        else:
            rc, what = self._lib.grnet_op_mesh_moments(self._h, v.data_ptr(), n, rows.data_ptr(), sums_ptr, int(form), self._stream()), "grnet_op_mesh_moments"
        _lib.check(self._lib, self._h, rc, what)
        return (rows, sums) if return_sums else rows

    # ------------------------------------------------------------------ step and stride tables, bootstrap intervals
    def gait_step_tables(self, events, per_frame, lengths=None, fps=20.0, max_rows=256, phase=None, straight_only=False):
        """The samples behind gait_parameters' step and stride columns of every sequence on the device (grnet_gait_step_tables; DESIGN 4.23,
        pipeline.STEP_TABLE_COLUMNS, pipeline.STRIDE_TABLE_COLUMNS).  events (sum T,) and per_frame (sum T,7): what gait_parameters returned, taken
        as int32 and float64; phase (sum T,): gait_turns' phase, with straight_only the steps and strides its straight columns count are listed
        alone.  Returns a dict of device tensors: steps (n_seq,max_rows,6) float64 [t_prev, t, landing foot, step time, step length, step width];
        strides (n_seq,max_rows,4) float64 [t0, t1, foot, stride time], the left foot's first; counts (n_seq,2) int32 -- rows past max_rows are
        counted, not stored, rows past the count are NaN.  Works before finalize(): no weight is read.  Nothing synchronises."""
        rows = self._rows_input(per_frame, "per_frame", (7,), torch.float64)
        n = rows.shape[0]
        ev = self._events_input(n, events)
        ph = None
        if phase is not None:
            ph = torch.as_tensor(phase).to(self.device, torch.int32).contiguous()
            if tuple(ph.shape) != (n,):
                raise ValueError(f"phase must be ({n},), got {tuple(ph.shape)}")
        if straight_only and ph is None:
            raise ValueError("straight_only needs a phase")
        self._whole_frames(max_rows=max_rows)
        if not 1 <= int(max_rows) <= 1024:
            raise ValueError(f"max_rows {max_rows} outside [1, 1024]")      # the tables are allocated here: a size the C ABI would refuse is refused first
        off = self._sequence_offsets(n, lengths, "per_frame")
        n_seq = len(off) - 1
        out = {"steps": torch.empty(n_seq, int(max_rows), 6, dtype=torch.float64, device=self.device),
               "strides": torch.empty(n_seq, int(max_rows), 4, dtype=torch.float64, device=self.device),
               "counts": torch.empty(n_seq, 2, dtype=torch.int32, device=self.device)}
        rc = self._lib.grnet_gait_step_tables(self._h, ev.data_ptr(), rows.data_ptr(), _i32p(off), n_seq, float(fps), int(max_rows),
                                              None if ph is None else ph.data_ptr(), int(bool(straight_only)), out["steps"].data_ptr(),
                                              out["strides"].data_ptr(), out["counts"].data_ptr(), self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_gait_step_tables")
        return out

    def bootstrap_table(self, table, counts, cols, B=2000, block=1, seed=0, stream=0, quantiles=(250, 5000, 9750), return_replicates=False):
        """Bootstrap of mean, SD and CV of columns of a per-step table on the device (grnet_bootstrap_table; the generator, the resampling, the
        statistics and the selection: DESIGN 4.23).  table (n_seq,max_rows,C) float64 with C <= 16 -- gait_step_tables' steps or strides,
        gait_balance's steps; counts (n_seq,) int32: the rows of each sequence (above max_rows: max_rows); cols: at most 8 columns; B in [1, 4096]
        replicates of rows drawn in circular blocks of `block`; quantiles in basis points, at most 5.  Returns a dict of device tensors: out
        (n_seq,n_cols,3,2 + n_q) float64, per statistic (mean, SD, CV) [the sample's own, the count f of replicates that are not NaN, the quantiles];
        with return_replicates, replicates (n_seq,n_cols,3,B).  Two sequences with equal counts get equal indices; a sequence has the same bits alone
        or among others.  A percentile interval from some 15 strides under-covers.  Works before finalize().  Nothing synchronises."""
        t = torch.as_tensor(table)
        if t.dim() != 3 or min(t.shape) < 1:
            raise ValueError(f"table must be (n_seq,max_rows,C), got {tuple(t.shape)}")
        t = t.to(self.device, torch.float64).contiguous()
        n_seq, max_rows, width = t.shape
        cnt = torch.as_tensor(counts).to(self.device, torch.int32).contiguous()
        if tuple(cnt.shape) != (n_seq,):
            raise ValueError(f"counts must be ({n_seq},), got {tuple(cnt.shape)}")
        pick, q = np.asarray(cols, np.int64).reshape(-1), np.asarray(quantiles, np.int64).reshape(-1)
        self._whole_frames(B=B, block=block, seed=seed, stream=stream)
        if not 1 <= pick.size <= 8 or q.size > 5 or not 1 <= int(B) <= 4096:
            raise ValueError(f"cols must name 1 to 8 columns, quantiles at most 5 and B lie in [1, 4096], got {pick.size}, {q.size} and {B}")      # the outputs are allocated here
        if np.abs(pick).max() >= 2**31 or (q.size and np.abs(q).max() >= 2**31) or not 0 <= int(seed) < 2**64 or abs(int(stream)) >= 2**31 or abs(int(block)) >= 2**31:
            raise ValueError("cols, quantiles, stream and block must fit 32 bits and seed 64")
        pick, q = np.ascontiguousarray(pick, np.int32), np.ascontiguousarray(q, np.int32)
        out = {"out": torch.empty(n_seq, pick.size, 3, 2 + q.size, dtype=torch.float64, device=self.device)}
        if return_replicates:
            out["replicates"] = torch.empty(n_seq, pick.size, 3, int(B), dtype=torch.float64, device=self.device)
        rc = self._lib.grnet_bootstrap_table(self._h, t.data_ptr(), cnt.data_ptr(), n_seq, max_rows, width, _i32p(pick), int(pick.size), int(B), int(block),
                                             int(seed), int(stream), _i32p(q) if q.size else None, int(q.size), out["out"].data_ptr(),
                                             out["replicates"].data_ptr() if return_replicates else None, self._stream())
        _lib.check(self._lib, self._h, rc, "grnet_bootstrap_table")
        return out

    # ------------------------------------------------------------------ the 3D skeleton view (demo.py --skeleton_view)
    def spin_joints(self, joints29, verts, joints="spin49"):
        """The joints of smooth_pose without the filter and without an SMPL pass (grnet_spin_joints): joints29 (n,29,3) and verts (n,6890,3) as a
        forward returns them, host or device -> (n,49|29|25,3) device tensor, bit-identical to smooth_pose's joints for the same vertices.
        n is not limited by max_frames; nothing synchronises."""
        if joints not in self._JOINT_KINDS:
            raise ValueError(f"joints must be one of {sorted(self._JOINT_KINDS)}, got {joints!r}")
        kind, nj = self._JOINT_KINDS[joints]
        kp = torch.as_tensor(joints29).to(self.device, torch.float32).contiguous()
        v = torch.as_tensor(verts).to(self.device, torch.float32).contiguous()
        if kp.dim() != 3 or tuple(kp.shape[1:]) != (29, 3) or v.dim() != 3 or tuple(v.shape[1:]) != (6890, 3) or kp.shape[0] != v.shape[0]:
            raise ValueError(f"joints29 must be (n,29,3) and verts (n,6890,3), got {tuple(kp.shape)} and {tuple(v.shape)}")
        out = torch.empty(kp.shape[0], nj, 3, dtype=torch.float32, device=self.device)
        stream = self._stream()
        rc = self._lib.grnet_spin_joints(self._h, kp.data_ptr(), v.data_ptr(), kp.shape[0], kind, out.data_ptr(), stream)
        _lib.check(self._lib, self._h, rc, "grnet_spin_joints")
        return out

    @staticmethod
    def _segment_view(view, R):
        """(proj (16) float64, window (4) float64, R (9) float32 or None), contiguous, for the C ABI; view=None: pipeline.skeleton_view()."""
        if view is None:
            from . import pipeline
            view = pipeline.skeleton_view()
        proj = np.ascontiguousarray(np.asarray(view[0], np.float64).reshape(16))
        window = np.ascontiguousarray(np.asarray(view[1], np.float64).reshape(4))
        Rh = None if R is None else np.ascontiguousarray(np.asarray(R, np.float32).reshape(9))
        return proj, window, Rh

    @staticmethod
    def _segment_table(segments, widths):
        seg = np.ascontiguousarray(np.asarray(segments, np.int64).reshape(-1, 2).clip(-1, 2**31 - 1), dtype=np.int32)
        wid = np.ascontiguousarray(np.asarray(widths, np.int64).reshape(-1).clip(-1, 2**31 - 1), dtype=np.int32)
        if wid.shape[0] != seg.shape[0]:
            raise ValueError(f"segments and widths disagree on S: {seg.shape[0]}, {wid.shape[0]}")
        return seg, wid

    def render_segments(self, images, points, segments, colours, widths, image_index, R=None, view=None, rgb=True):
        """Draw n skeletons as wide line segments into uint8 device images (F,H,W,3) IN PLACE and return them (grnet_render_segments; the rules:
        DESIGN.md 4.6).  points (n,P,3), host or device; segments (S,2) point indices, colours (S,3) uint8 (r,g,b), widths (S) pixels in [1,16];
        image_index (n): the image each skeleton is drawn into -- all skeletons of an image share ONE depth buffer, the nearer segment wins,
        at equal depth the one drawn first.  R: the 3x3 body rotation applied to the points first (None: identity); view: (P 4x4, window
        (x0,x1,y0,y1)), None for pipeline.skeleton_view().  rgb: the images are RGB (pipeline's frames) and a pixel gets (r,g,b) as given;
        rgb=False: BGR images, the triple goes down reversed so that the screen shows the same colour.  The C call only enqueues (the host-side
        tables given as numpy arrays are read before it returns); n is not limited by max_frames."""
        if not torch.is_tensor(images) or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or not images.is_cuda \
                or not images.is_contiguous():
            raise ValueError("images must be a contiguous uint8 (F,H,W,3) tensor on the device")
        F, H, W = images.shape[:3]
        p = torch.as_tensor(points).to(self.device, torch.float32).contiguous()
        if p.dim() != 3 or p.shape[2] != 3:
            raise ValueError(f"points must be (n,P,3), got {tuple(p.shape)}")
        n, P = p.shape[:2]
        seg, wid = self._segment_table(segments, widths)
        col = np.asarray(colours).reshape(-1, 3)
        if col.shape[0] != seg.shape[0] or col.size and (col.min() < 0 or col.max() > 255):
            raise ValueError(f"colours must be (S,3) bytes with S = {seg.shape[0]}, got {col.shape} in [{col.min() if col.size else 0}, {col.max() if col.size else 0}]")
        col = np.ascontiguousarray(col if rgb else col[:, ::-1], dtype=np.uint8)
        idx = np.ascontiguousarray(np.asarray(image_index, np.int64).reshape(-1).clip(-1, 2**31 - 1), dtype=np.int32)
        if idx.shape[0] != n:
            raise ValueError(f"points and image_index disagree on n: {n}, {idx.shape[0]}")
        proj, window, Rh = self._segment_view(view, R)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        stream = self._stream()
        rc = self._lib.grnet_render_segments(self._h, p.data_ptr(), n, P, ptr(seg), seg.shape[0], ptr(col), ptr(wid), ptr(idx),
                                             ptr(Rh) if Rh is not None else None, ptr(proj), ptr(window), images.data_ptr(), F, H, W, stream)
        _lib.check(self._lib, self._h, rc, "grnet_render_segments")
        return images

    def op_segments_setup(self, points, H, W, R=None, view=None):
        """points (P,3) -> (xy (P,2) int32 snapped window coordinates, INT32_MIN in both for an invalid point; depth (P)) on the device
        (grnet_op_segments_setup)."""
        p = torch.as_tensor(points).to(self.device, torch.float32).reshape(-1, 3).contiguous()
        proj, window, Rh = self._segment_view(view, R)
        P = p.shape[0]
        xy = torch.empty(P, 2, dtype=torch.int32, device=self.device)
        d = torch.empty(P, dtype=torch.float32, device=self.device)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        stream = self._stream()
        rc = self._lib.grnet_op_segments_setup(self._h, p.data_ptr(), P, ptr(Rh) if Rh is not None else None, ptr(proj), ptr(window), H, W,
                                               xy.data_ptr(), d.data_ptr(), stream)
        _lib.check(self._lib, self._h, rc, "grnet_op_segments_setup")
        return xy, d

    def op_raster_segments(self, xy, depth, segments, widths, H, W):
        """Snapped points xy (P,2) int32 and depth (P) -> the winning segment per pixel (H,W) int32 in image rows, -1 where uncovered
        (grnet_op_raster_segments)."""
        xy = torch.as_tensor(xy).to(self.device, torch.int32).reshape(-1, 2).contiguous()
        d = torch.as_tensor(depth).to(self.device, torch.float32).reshape(-1).contiguous()
        seg, wid = self._segment_table(segments, widths)
        out = torch.empty(H, W, dtype=torch.int32, device=self.device)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        stream = self._stream()
        rc = self._lib.grnet_op_raster_segments(self._h, xy.data_ptr(), d.data_ptr(), xy.shape[0], ptr(seg), seg.shape[0], ptr(wid), H, W,
                                                out.data_ptr(), stream)
        _lib.check(self._lib, self._h, rc, "grnet_op_raster_segments")
        return out

    # single-op hooks for kernel parity tests
    def op_conv2d(self, x, w, bias=None, stride=1, relu=False, add=None, tile_hint=0):
        n, cin, h, wd = x.shape
        cout, _, ks, _ = w.shape
        pad = ks // 2
        ho, wo = (h + 2 * pad - ks) // stride + 1, (wd + 2 * pad - ks) // stride + 1
        out = torch.empty(n, cout, ho, wo, dtype=torch.float32, device=x.device)
        wn = _np32(w)
        bn = _np32(bias) if bias is not None else None
        stream = self._stream(x.device)
        rc = self._lib.grnet_op_conv2d(self._h, x.data_ptr(), n, cin, h, wd, wn.ctypes.data_as(C.c_void_p),
                                       bn.ctypes.data_as(C.c_void_p) if bn is not None else None, cout, ks, stride,
                                       int(relu), add.data_ptr() if add is not None else None, out.data_ptr(),
                                       tile_hint, stream)
        _lib.check(self._lib, self._h, rc, "grnet_op_conv2d")
        return out

    def op_conv2d_adds(self, x, w, bias=None, stride=1, relu=False, adds=(), tile_hint=0):
        """bf16 handles: op_conv2d with up to three addends, each (tensor (n,ctot,ho>>shift,wo>>shift) f32, channel offset, shift): the launch adds
        channels offset .. offset+cout-1 of it, nearest-upsampled by 2**shift (grnet_op_conv2d_adds)."""
        n, cin, h, wd = x.shape
        cout, _, ks, _ = w.shape
        pad = ks // 2
        ho, wo = (h + 2 * pad - ks) // stride + 1, (wd + 2 * pad - ks) // stride + 1
        out = torch.empty(n, cout, ho, wo, dtype=torch.float32, device=x.device)
        wn = _np32(w)
        bn = _np32(bias) if bias is not None else None
        k = len(adds)
        tens = [a[0].contiguous() for a in adds]
        ptrs = (C.c_void_p * max(k, 1))(*[t.data_ptr() for t in tens])
        ctot = (C.c_int * max(k, 1))(*[t.shape[1] for t in tens])
        coff = (C.c_int * max(k, 1))(*[int(a[1]) for a in adds])
        shift = (C.c_int * max(k, 1))(*[int(a[2]) for a in adds])
        stream = self._stream(x.device)
        rc = self._lib.grnet_op_conv2d_adds(self._h, x.data_ptr(), n, cin, h, wd, wn.ctypes.data_as(C.c_void_p),
                                            bn.ctypes.data_as(C.c_void_p) if bn is not None else None, cout, ks, stride, int(relu), k, ptrs, ctot, coff,
                                            shift, out.data_ptr(), tile_hint, stream)
        _lib.check(self._lib, self._h, rc, "grnet_op_conv2d_adds")
        return out

    def op_conv_chain(self, x, ws, bs, reps=0):
        """bf16 handles: ONE conv_bf16_chain launch over the BasicBlock chain ws = [(c,c,3,3)] * nconv, bs = [(c,)] * nconv on x (n,c,w,w) f32.
        Returns the output (n,c,w,w) f32 (bf16 values), or (output, us per launch) with reps > 0."""
        n, c, h, wd = x.shape
        out = torch.empty_like(x, dtype=torch.float32)
        wn = np.ascontiguousarray(np.stack([_np32(w) for w in ws]))
        bn = np.ascontiguousarray(np.stack([_np32(b) for b in bs]))
        us = C.c_float(0.0)
        stream = self._stream(x.device)
        rc = self._lib.grnet_op_conv_chain(self._h, x.data_ptr(), n, c, wd, len(ws), wn.ctypes.data_as(C.c_void_p), bn.ctypes.data_as(C.c_void_p),
                                           out.data_ptr(), int(reps), C.byref(us), stream)
        _lib.check(self._lib, self._h, rc, "grnet_op_conv_chain")
        return (out, us.value) if reps else out

    def op_bilinear2x(self, x):
        n, c, h, w = x.shape
        out = torch.empty(n, c, 2 * h, 2 * w, dtype=torch.float32, device=x.device)
        stream = self._stream(x.device)
        rc = self._lib.grnet_op_bilinear2x(self._h, x.data_ptr(), n, c, h, w, out.data_ptr(), stream)
        _lib.check(self._lib, self._h, rc, "grnet_op_bilinear2x")
        return out

    def op_attention_pool(self, heat, feat_a, feat_b):
        """The attention pooling alone, through the forward's pooling kernel and the merge at the front of the tail (grnet_op_attention_pool):
        heat (n,25,56,56), feat_a (n,128,56,56), feat_b (n,64,56,56) f32 -> (point_local_feat (n,128,24), cam_shape_feats (n,64,24)) f32."""
        n = heat.shape[0]
        assert tuple(heat.shape) == (n, 25, 56, 56) and tuple(feat_a.shape) == (n, 128, 56, 56) and tuple(feat_b.shape) == (n, 64, 56, 56)
        heat, feat_a, feat_b = (t.to(torch.float32).contiguous() for t in (heat, feat_a, feat_b))
        plf = torch.empty(n, 128, 24, dtype=torch.float32, device=heat.device)
        csf = torch.empty(n, 64, 24, dtype=torch.float32, device=heat.device)
        stream = self._stream(heat.device)
        rc = self._lib.grnet_op_attention_pool(self._h, heat.data_ptr(), feat_a.data_ptr(), feat_b.data_ptr(), n, plf.data_ptr(), csf.data_ptr(), stream)
        _lib.check(self._lib, self._h, rc, "grnet_op_attention_pool")
        return plf, csf

    def close(self):
        if getattr(self, "_h", None):
            self._lib.grnet_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def build_synthetic_model(max_frames=64, device_id=0, with_gru=True, with_tsattn=False, dtype="f32", use_gait_feat=False, compact_arena=False):
    """GRNet with the seed-defined weights / SMPL tables of synth.py (no checkpoint exists offline).  use_gait_feat: the whole
    pose-feature corrector under its checkpoint keys (pfeat_corrector.*: GRU, gait-token MLPs, BatchNorm1d, attention block)."""
    from . import synth
    m = GRNet(max_frames=max_frames, device_id=device_id, dtype=dtype, use_gait_feat=use_gait_feat, compact_arena=compact_arena,
              featcorr=dict(AVG_DIM=3, ESTIM_PHASE=True, NUM_LAYERS=1, H_SIZE=1024, NUM_HEADS=4, USE_JWFF=True) if use_gait_feat else None)
    sd = synth.make_state_dict()
    if use_gait_feat:
        sd.update(synth.make_featcorr_state_dict())
        with_gru = with_tsattn = False
    if with_gru:
        sd.update({"gru." + k: v for k, v in synth.make_gru_state_dict().items()})
    if with_tsattn:
        sd.update({"tsattn." + k: v for k, v in synth.make_tsattn_state_dict().items()})
    m.load_state_dict(sd, strict=True)
    m.load_smpl(synth.make_smpl_tables())
    m.load_faces(synth.make_faces())
    return m.finalize()
