"""The --smooth step on the device (csrc/smooth_kernels.hip, grnet_op_one_euro / grnet_op_aa_to_rotmat / grnet_smooth_pose): the filter
bit for bit against the reference's float32 arithmetic (a build that lets the compiler contract its multiply-adds fails items 1-3), Rodrigues
against float64, SMPL and the 49 / 29 / 25 joints against the float64 composition and the host path, refusals, and demo.py --smooth.

B below is the filter's LDS staging block (kOneEuroBlock in csrc/kernels.h, tests/test_smooth_checks_cpu.py pins it): sequence lengths
sit on and around its multiples, where the kernel changes buffers, takes its unrolled path (whole blocks after the first) or its tail."""
import ctypes as C
import importlib
import os
import sys

import joblib
import numpy as np
import pytest
import torch

from .conftest import CALL_SIZE_NOISE, ROOT, rel_err
from .helpers import smooth_checks as sc

pytestmark = pytest.mark.gpu

B = 32
SEAM_T = (1, 2, 3, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, 5 * B + 7)
PARAMS = ((0.004, 0.7), (0.004, 1.5), (1.0, 0.0))


@pytest.fixture(scope="module")
def m8(pkg):
    m = pkg.build_synthetic_model(max_frames=8, with_gru=False)
    yield m
    m.close()


@pytest.fixture(scope="module")
def step(m8, synth_smpl):
    """One run of the whole step at T = 20 (chunks 8 + 8 + 4), shared by the tests that read it; nothing below modifies it."""
    T = 20
    pose, _ = sc.random_walk(T, seed=17)
    g = np.random.Generator(np.random.Philox(key=[18, 18]))
    betas = (g.standard_normal((T, 10)) * 0.5).astype(np.float32)
    verts, pose_hat, j49 = m8.smooth_pose(pose, betas)
    torch.cuda.synchronize()
    return dict(T=T, pose=pose, betas=betas, verts=verts.cpu().numpy(), pose_hat=pose_hat.cpu().numpy(), j49=j49.cpu().numpy())


def _golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "one_euro.npz"))
    return g["seq"], g["hat"]


def test_golden_bit_for_bit(m8):
    seq, hat = _golden()
    got = m8.one_euro(seq.reshape(40, 72), 0.004, 0.7).cpu().numpy()
    assert np.array_equal(got, hat.reshape(40, 72)), int((got != hat.reshape(40, 72)).sum())


@pytest.mark.parametrize("ld", (72, 85))
@pytest.mark.parametrize("min_cutoff,beta", PARAMS)
def test_block_seams_bit_for_bit(m8, ld, min_cutoff, beta):
    """Every length around the staging block, dense rows and theta rows (whose 13 other columns are NaN and must never be read)."""
    for T in SEAM_T:
        x, dev_in = sc.random_walk(T, seed=100 + T, ld=ld)
        got = m8.one_euro(dev_in, min_cutoff, beta).cpu().numpy()
        want = sc.one_euro_strict_f32(x, min_cutoff, beta)
        assert got.shape == (T, 72)
        assert np.array_equal(got, want), (T, ld, int((got != want).sum()))
    assert np.array_equal(got[0], x[0])                       # the filter starts at the first frame


def test_constant_and_jump_sequences(m8):
    T = 3 * B
    const = np.tile(np.linspace(-2.0, 2.0, 72, dtype=np.float32)[None], (T, 1))
    got = m8.one_euro(const, 0.004, 0.7).cpu().numpy()
    assert np.array_equal(got, sc.one_euro_strict_f32(const, 0.004, 0.7))
    # a constant is NOT reproduced exactly by a x + (1 - a) x in float32: the reference drifts by an ulp here and there, and so must the kernel
    jump, _ = sc.random_walk(T, seed=7)
    jump[B + B // 2:, 0::2] += np.float32(3.0)                # a step in the middle block, up on even channels ...
    jump[B + B // 2:, 1::2] -= np.float32(3.0)                # ... down on odd ones
    for min_cutoff, beta in PARAMS:
        got = m8.one_euro(jump, min_cutoff, beta).cpu().numpy()
        assert np.array_equal(got, sc.one_euro_strict_f32(jump, min_cutoff, beta)), (min_cutoff, beta)


def test_causality(m8):
    """Frame t depends on frames 0..t only: a prefix run alone gives the same bits."""
    x, _ = sc.random_walk(5 * B + 7, seed=3)
    whole = m8.one_euro(x, 0.004, 0.7).cpu().numpy()
    for k in (B, 2 * B + 1):
        part = m8.one_euro(x[:k].copy(), 0.004, 0.7).cpu().numpy()
        assert np.array_equal(part, whole[:k]), k


def test_output_is_exactly_t_by_72(m8):
    """The C entry point writes (T,72) and not a float more: a guard row behind it keeps its bit pattern; theta rows are read in place."""
    lib, h = m8._lib, m8._h
    stream = C.c_void_p(torch.cuda.current_stream(m8.device).cuda_stream)
    for T in (1, B - 1, B, 2 * B + 1):
        x, full = sc.random_walk(T, seed=50 + T, ld=85)
        theta = torch.from_numpy(full).cuda()
        out = torch.full((T + 1, 72), float("nan"), dtype=torch.float32, device="cuda")
        out.view(torch.int32)[T].fill_(0x5A5A5A5A)
        rc = lib.grnet_op_one_euro(h, theta.data_ptr() + 12, 85, T, 0.004, 0.7, 1.0, out.data_ptr(), stream)
        assert rc == 0, lib.grnet_last_error(h)
        torch.cuda.synchronize()
        assert np.array_equal(out[:T].cpu().numpy(), sc.one_euro_strict_f32(x, 0.004, 0.7)), T
        assert bool((out.view(torch.int32)[T] == 0x5A5A5A5A).all()), T


def test_aa_to_rotmat(m8, pkg):
    """Stage policy: 8 x the error the plain fp32 numpy statement makes against float64 on the same inputs, never above 1e-5."""
    g = np.random.Generator(np.random.Philox(key=[9, 9]))
    axis = g.standard_normal((3, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    special = np.concatenate([np.zeros((1, 3)), [[1e-6, 0, 0]], axis * np.array([[3.1], [np.pi], [4.0]]),
                              [[3.1, 0, 0], [0, np.pi, 0], [0, 0, 4.0]]])
    aa = np.concatenate([special, g.standard_normal((2000, 3)) * 1.5]).astype(np.float32)
    ref = sc.rodrigues_f64(aa)
    host_err = float(np.abs(pkg.pipeline.rodrigues(aa).astype(np.float64) - ref).max())
    bar = min(8 * host_err, 1e-5)
    got = m8.aa_to_rotmat(aa).cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"aa_to_rotmat: device err {err:.3e}, host fp32 err {host_err:.3e}, bar {bar:.3e}")
    assert got.shape == (aa.shape[0], 3, 3) and got.dtype == np.float32
    assert host_err > 0 and err <= bar, (err, bar)
    assert np.array_equal(got[0], np.eye(3, dtype=np.float32))                 # the zero vector: d = 0 / |1e-8| = 0
    g64 = got.astype(np.float64)
    assert np.allclose(g64 @ g64.transpose(0, 2, 1), np.eye(3), atol=1e-5) and np.allclose(np.linalg.det(g64), 1, atol=1e-5)


def test_whole_step_against_float64(m8, pkg, oracle, synth_smpl, step):
    T, netspec = step["T"], pkg.netspec
    assert step["verts"].shape == (T, 6890, 3) and step["pose_hat"].shape == (T, 72) and step["j49"].shape == (T, 49, 3)
    want_pose = sc.one_euro_strict_f32(step["pose"], 0.004, 0.7)
    assert np.array_equal(step["pose_hat"], want_pose)
    R = sc.rodrigues_f64(step["pose_hat"].reshape(-1, 3)).reshape(T, 24, 3, 3)
    v_ref, j24 = oracle.smpl_lbs(np.repeat(step["betas"][:1], T, 0), R, synth_smpl)
    assert rel_err(step["verts"], v_ref) < 1e-4
    v64 = v_ref.astype(np.float64)
    extra = np.einsum("jv,nvk->njk", np.asarray(synth_smpl["J_regressor_extra"], np.float64), v64)
    j54 = np.concatenate([j24.astype(np.float64), v64[:, netspec.SMPL_EXTRA_VERT_IDS], extra], 1)
    assert j54.shape == (T, 54, 3)
    j49_ref = j54[:, netspec.SPIN49_FROM_54]
    assert rel_err(step["j49"], j49_ref) < 1e-4
    assert set(netspec.SPIN49_FROM_54) >= set(range(45, 54))  # all nine rows of J_regressor_extra are in the 49: the device list holds nine


def test_whole_step_skeletons_and_options(m8, pkg, step):
    T, netspec = step["T"], pkg.netspec
    pose, betas = step["pose"], step["betas"]
    _, ph2, spin2 = m8.smooth_pose(pose, betas, joints="spin2")
    assert spin2.shape == (T, 29, 3) and np.array_equal(ph2.cpu().numpy(), step["pose_hat"])
    rot = m8.aa_to_rotmat(step["pose_hat"]).reshape(T, 24, 3, 3)
    _, kp29, _ = m8.smpl_forward(torch.from_numpy(np.repeat(betas[:1], T, 0)), rot)
    assert rel_err(spin2.cpu().numpy(), kp29.cpu().numpy()) < CALL_SIZE_NOISE
    _, _, kin = m8.smooth_pose(pose, betas, joints="kinectv2")
    assert kin.shape == (T, 25, 3)
    assert np.array_equal(kin.cpu().numpy(), spin2.cpu().numpy()[:, netspec.SPIN2_TO_KINECTV2])
    # only row 0 of betas is used (smooth_pose.py:97)
    other = betas.copy()
    other[1:] = other[1:][::-1] * 3.0 + 1.0
    v2, p2, j2 = m8.smooth_pose(pose, other)
    assert np.array_equal(v2.cpu().numpy(), step["verts"]) and np.array_equal(j2.cpu().numpy(), step["j49"])
    assert np.array_equal(p2.cpu().numpy(), step["pose_hat"])
    # without vertices for the caller: the same joints
    v3, p3, j3 = m8.smooth_pose(pose, betas, return_verts=False)
    assert v3 is None and np.array_equal(j3.cpu().numpy(), step["j49"]) and np.array_equal(p3.cpu().numpy(), step["pose_hat"])
    # a theta is read in place: cam | pose | betas
    theta = torch.from_numpy(np.concatenate([np.full((T, 3), np.nan, np.float32), pose, betas], 1)).cuda()
    v4, p4, j4 = m8.smooth_pose(theta, theta[:, 75:])
    assert np.array_equal(v4.cpu().numpy(), step["verts"]) and np.array_equal(j4.cpu().numpy(), step["j49"])
    assert np.array_equal(p4.cpu().numpy(), step["pose_hat"])


@pytest.mark.parametrize("kinectv2", (False, True))
def test_against_the_host_path(m8, pkg, synth_smpl, step, kinectv2):
    pipe = pkg.pipeline
    hv, hp, hj = pipe.smooth_pose(m8, step["pose"], step["betas"], kinectv2=kinectv2, smpl_tables=synth_smpl)
    dv, dp, dj = pipe.smooth_pose_device(m8, step["pose"], step["betas"], kinectv2=kinectv2)
    for a, b in ((dv, hv), (dp, hp), (dj, hj)):
        assert type(a) is type(b) is np.ndarray and a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert dj.shape == ((step["T"], 25, 3) if kinectv2 else (step["T"], 49, 3))
    assert np.allclose(dp, hp, rtol=1e-6, atol=1e-7)          # the host filter's own bar against the golden
    assert rel_err(dv, hv) < 1e-4 and rel_err(dj, hj) < 1e-4


def test_run_twice_and_call_size(pkg, m8, step):
    a = m8.smooth_pose(step["pose"], step["betas"])
    b = m8.smooth_pose(step["pose"], step["betas"])
    for u, v, k in zip(a, b, ("verts", "pose_hat", "j49")):
        assert np.array_equal(u.cpu().numpy(), v.cpu().numpy()) and np.array_equal(u.cpu().numpy(), step[k]), k
    m32 = pkg.build_synthetic_model(max_frames=32, with_gru=False)         # T = 20 in ONE chunk
    v, p, j = m32.smooth_pose(step["pose"], step["betas"])
    assert np.array_equal(p.cpu().numpy(), step["pose_hat"])
    assert rel_err(v.cpu().numpy(), step["verts"]) < CALL_SIZE_NOISE and rel_err(j.cpu().numpy(), step["j49"]) < CALL_SIZE_NOISE
    m32.close()


def test_refusals_leave_the_handle_usable(m8, pkg, step):
    lib, h, EINVAL = m8._lib, m8._h, pkg._lib.EINVAL
    stream = C.c_void_p(torch.cuda.current_stream(m8.device).cuda_stream)
    T = 4
    pose = torch.from_numpy(step["pose"][:T].copy()).cuda()
    betas = torch.from_numpy(step["betas"][:T].copy()).cuda()
    ph = torch.empty(T, 72, device="cuda")
    jt = torch.empty(T, 49, 3, device="cuda")

    def call(pose_ptr=pose.data_ptr(), ld=72, n=T, beta=0.7, kind=0, min_cutoff=0.004):
        return lib.grnet_smooth_pose(h, pose_ptr, ld, betas.data_ptr(), n, min_cutoff, beta, kind, ph.data_ptr(), None, jt.data_ptr(), stream)

    for what, kw in (("T", dict(n=0)), ("stride", dict(ld=71)), ("null", dict(pose_ptr=None)), ("joints_kind", dict(kind=7)),
                     ("finite", dict(beta=float("nan"))), ("finite", dict(min_cutoff=float("inf")))):
        assert call(**kw) == EINVAL, kw
        msg = lib.grnet_last_error(h).decode()
        assert "grnet_smooth_pose" in msg and what in msg, (kw, msg)
    assert lib.grnet_op_one_euro(h, pose.data_ptr(), 71, T, 0.004, 0.7, 1.0, ph.data_ptr(), stream) == EINVAL
    assert lib.grnet_op_one_euro(h, pose.data_ptr(), 72, 0, 0.004, 0.7, 1.0, ph.data_ptr(), stream) == EINVAL
    assert lib.grnet_op_one_euro(h, None, 72, T, 0.004, 0.7, 1.0, ph.data_ptr(), stream) == EINVAL
    assert lib.grnet_op_one_euro(h, pose.data_ptr(), 72, T, 0.004, float("nan"), 1.0, ph.data_ptr(), stream) == EINVAL
    assert lib.grnet_last_error(h).decode()
    with pytest.raises(ValueError, match="quaternion"):
        m8.smooth_pose(np.zeros((T, 96), np.float32), step["betas"][:T])
    with pytest.raises(ValueError):
        m8.smooth_pose(step["pose"][:T], step["betas"][:T], joints="coco")
    with pytest.raises(ValueError):
        m8.one_euro(np.zeros((0, 72), np.float32))
    # the handle still works
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(ph.cpu().numpy(), sc.one_euro_strict_f32(step["pose"][:T], 0.004, 0.7))
    v, p, j = m8.smooth_pose(step["pose"], step["betas"])
    assert np.array_equal(j.cpu().numpy(), step["j49"])


def test_arena_accounting_is_untouched(m8, pkg, step):
    """The rotation / betas / kp workspace of grnet_smooth_pose lives outside the activation arena."""
    assert m8.arena_info() == pkg.grnet.arena_query("f32", 8, compact=False)


def test_demo_smooth(pkg, tmp_path):
    sys.path.insert(0, ROOT)
    demo = importlib.import_module("demo")
    frames = pkg.synth.make_frames(30)
    img_dir = str(tmp_path / "vid")
    os.makedirs(img_dir)
    for i, f in enumerate(frames):
        np.save(os.path.join(img_dir, f"{i:06d}.npy"), f)
    bbox = np.tile(np.array([[112.0, 112.0, 224.0, 224.0]], np.float32), (30, 1))
    tp = str(tmp_path / "tracking.pkl")
    joblib.dump({1: {"bbox": bbox, "frames": np.arange(30)}}, tp)
    base = ["--img_folder", img_dir, "--tracking_path", tp, "--output_folder", str(tmp_path / "out"), "--synthetic_weights",
            "--grnet_batch_size", "16", "--max_frames", "16"]
    run = lambda *extra: joblib.load(demo.main(demo.parser().parse_args(base + list(extra))))[1]
    plain, dev, host = run(), run("--smooth"), run("--smooth", "--smooth_on_host")
    assert dev["joints3d"].shape == (30, 49, 3) and dev["verts"].shape == (30, 6890, 3) and dev["pose"].shape == (30, 72)
    assert set(dev) == set(plain) == set(host)
    for k in dev:
        assert isinstance(dev[k], np.ndarray) and dev[k].shape == host[k].shape and dev[k].dtype == host[k].dtype, k
    assert np.array_equal(dev["pose"][0], plain["pose"][0])   # the filter starts at the first pose
    assert np.array_equal(dev["pose"], sc.one_euro_strict_f32(plain["pose"], 0.004, 0.7))
    for k in ("pred_cam", "betas", "orig_cam", "joints2d"):   # what smoothing does not touch
        assert np.array_equal(dev[k], plain[k]), k
    assert np.allclose(dev["pose"], host["pose"], rtol=1e-6, atol=1e-7)
    assert rel_err(dev["verts"], host["verts"]) < 1e-4 and rel_err(dev["joints3d"], host["joints3d"]) < 1e-4
    kin = run("--smooth", "--joint_type", "kinectv2")
    assert kin["joints3d"].shape == (30, 25, 3)
