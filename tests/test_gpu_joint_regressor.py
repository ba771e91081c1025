"""The J_regressor override on the GPU (grnet_set_joint_regressor / grnet_regress_joints, csrc/joint_regress.hip): exact integer sums,
the textbook rounding bound on real vertices, independence of the call size, the reference's VPRegressor outputs
(tests/golden/vp_jreg.npz), GRNet.forward / smpl_forward with the argument, the temporal branch, a bf16 handle, state and errors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from .conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu
MAXF = 67
V = 6890


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=MAXF)
    yield m
    m.close()


@pytest.fixture(scope="module")
def jreg_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "vp_jreg.npz"))


@pytest.fixture(scope="module")
def real_verts(model, pkg):
    """Vertices left by a real 16-frame forward."""
    out = model(torch.from_numpy(pkg.synth.make_frames(16)).cuda())[-1]
    torch.cuda.synchronize()
    return out["verts"].reshape(16, V, 3).clone()


def table_of(pkg, recipe):
    rows, nnz, signed, seed = (int(v) for v in recipe)
    return pkg.synth.make_joint_regressor(rows, nnz=None if nnz < 0 else nnz, signed=bool(signed), seed=seed)


def f64_joints(W, verts, select=None):
    full = np.einsum("jv,nvk->njk", np.asarray(W, np.float64), np.asarray(verts, np.float64))
    return full if select is None else full[:, select]


def int_case(rows, n, seed):
    g = np.random.Generator(np.random.Philox(key=[seed, rows * 1000 + n]))
    W = g.integers(-4, 5, (rows, V)).astype(np.float32)
    verts = g.integers(-64, 65, (n, V, 3)).astype(np.float32)
    return W, verts


def exact_check(m, rows, select, n, seed=11):
    W, verts = int_case(rows, n, seed)
    m.set_joint_regressor(W, select=select)
    jout = rows if select is None else len(select)
    assert m.joint_regressor_rows() == jout
    got = m.regress_joints(torch.from_numpy(verts).cuda()).cpu().numpy()
    full = np.einsum("jv,nvk->njk", W.astype(np.int64), verts.astype(np.int64))
    want = full if select is None else full[:, select]
    assert got.shape == (n, jout, 3)
    assert np.abs(want).max() < 2 ** 24
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32)), \
        (rows, n, int(np.abs(got - want).max()), int((got != want).sum()))


@pytest.mark.parametrize("n", [1, 5, 16, MAXF])
@pytest.mark.parametrize("rows,select", [(1, None), (17, "J14"), (24, None), (64, None)])
def test_exact_integer_sums(model, pkg, rows, select, n):
    """Integer tables in [-4,4] on integer vertices in [-64,64]: every partial sum is an integer below 6890*4*64 < 2^24, so any correct fp32
    summation order gives the int64 result exactly -- a dropped, doubled or misplaced vertex cannot hide in a tolerance."""
    exact_check(model, rows, list(pkg.netspec.H36M_TO_J14) if select == "J14" else None, n)


@pytest.mark.parametrize("rows,nnz,signed", [(17, 32, False), (17, 300, False), (17, None, False), (26, None, True)])
def test_rounding_bound_on_real_vertices(model, pkg, real_verts, rows, nnz, signed):
    """|gpu - f64| <= K 2^-24 (|W| @ |verts|) + one fp32 ulp of the result, K = non-zeros of the row: the bound of a length-K fp32 dot
    product in ANY order (zero terms add exactly).  A bf16 / TF32-like shortcut misses it by orders of magnitude."""
    W = pkg.synth.make_joint_regressor(rows, nnz=nnz, signed=signed, seed=77)
    model.set_joint_regressor(W, select=None)
    got = model.regress_joints(real_verts).cpu().numpy().astype(np.float64)
    v = real_verts.cpu().numpy()
    ref = f64_joints(W, v)
    K = (W != 0).sum(1).astype(np.float64)[None, :, None]
    bound = K * 2.0 ** -24 * f64_joints(np.abs(W), np.abs(v)) + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    ratio = np.abs(got - ref) / bound
    print(f"rows {rows} nnz {nnz} signed {signed}: worst |err| / bound = {ratio.max():.4f}")
    assert np.isfinite(got).all() and (np.abs(got - ref) <= bound).all(), float(ratio.max())


def test_value_of_a_frame_does_not_depend_on_the_call(model, pkg, real_verts):
    W = pkg.synth.make_joint_regressor(17, nnz=None, signed=True, seed=5)
    model.set_joint_regressor(W)
    g = torch.Generator().manual_seed(3)
    big = (torch.randn(MAXF, V, 3, generator=g) * 0.4).cuda()
    big[40] = real_verts[5]
    in16 = model.regress_joints(real_verts)
    again = model.regress_joints(real_verts)
    alone = model.regress_joints(real_verts[5:6])
    inbig = model.regress_joints(big)
    assert torch.equal(in16, again)
    assert torch.equal(in16[5], alone[0]) and torch.equal(in16[5], inbig[40])
    assert torch.equal(model.regress_joints(big[40:41])[0], inbig[40]) and torch.equal(model.regress_joints(big[60:])[6], inbig[66])
    # (b,t,6890,3) input and chunking by max_frames
    both = model.regress_joints(torch.cat([big, real_verts]).reshape(1, MAXF + 16, V, 3))
    assert both.shape == (1, MAXF + 16, 14, 3) and torch.equal(both[0, :MAXF], inbig) and torch.equal(both[0, MAXF:], in16)


def test_smpl_forward_matches_the_reference(model, pkg, golden, jreg_golden):
    g = golden["grnet_n4"]
    betas, rotmat, cam = (torch.from_numpy(g[k]).cuda() for k in ("pred_shape", "pred_rotmat", "pred_cam"))
    verts0, kp0, kp2d0 = model.smpl_forward(betas, rotmat, cam)
    assert kp0.shape == (4, 29, 3)
    for name, shape in (("a", (4, 14, 3)), ("b", (4, 14, 3)), ("c", (4, 26, 3)), ("d", (4, 24, 3))):
        W = table_of(pkg, jreg_golden[f"recipe_{name}"])
        verts, kp3d, kp2d = model.smpl_forward(betas, rotmat, cam, J_regressor=torch.from_numpy(W))
        err = rel_err(kp3d.cpu().numpy(), jreg_golden[f"kp_3d_{name}"])
        print(f"case {name}: rel_err vs reference {err:.2e}")
        assert tuple(kp3d.shape) == shape and err < 1e-4, (name, err)
        assert torch.equal(verts, verts0) and torch.equal(kp2d, kp2d0)
    assert rel_err(kp2d0.cpu().numpy(), jreg_golden["kp_2d_a"]) < 1e-4


def test_forward_with_and_without_the_argument(model, pkg, oracle, synth_weights, synth_smpl, jreg_golden):
    frames_np = pkg.synth.make_frames(4).reshape(2, 2, 3, 224, 224)
    frames = torch.from_numpy(frames_np).cuda()
    model.set_joint_regressor(None)
    plain = {k: v.clone() for k, v in model(frames)[-1].items()}
    launches = model.num_kernel_launches()
    J = torch.from_numpy(table_of(pkg, jreg_golden["recipe_a"]))
    uploads = model.joint_regressor_uploads
    out = model(frames, J_regressor=J)[-1]
    assert out["kp_3d"].shape == (2, 2, 14, 3)
    for k in ("theta", "verts", "kp_2d", "rotmat"):
        assert torch.equal(out[k], plain[k]), k
    assert torch.equal(out["kp_3d"], model.regress_joints(out["verts"]))
    ref = oracle.grnet_forward(frames_np, synth_weights, synth_smpl)
    want = f64_joints(J.numpy(), np.asarray(ref["verts"]).reshape(4, V, 3), pkg.netspec.H36M_TO_J14)
    err = rel_err(out["kp_3d"].cpu().numpy().reshape(4, 14, 3), want)
    print(f"kp_3d vs float64 product of the oracle's vertices: {err:.2e}")
    assert err < 1e-4, err
    # the same table again, as the same object and as an equal copy: one upload in all
    model(frames, J_regressor=J)
    model(frames, J_regressor=J.clone())
    model(frames, J_regressor=J.numpy().copy())
    assert model.joint_regressor_uploads == uploads + 1
    again = model(frames, J_regressor=None)[-1]
    assert again["kp_3d"].shape == (2, 2, 29, 3)
    for k in ("theta", "verts", "kp_2d", "kp_3d", "rotmat"):
        assert torch.equal(again[k], plain[k]), k
    assert model.num_kernel_launches() == launches


def test_forward_takes_the_reference_selection_whatever_was_set(model, pkg, golden, jreg_golden):
    """forward / smpl_forward promise the reference's [:, H36M_TO_J14] for a 17-row table even when the SAME tensor object sits on the device
    with another selection (all rows, or a custom list of the same length): one more upload, the selected rows bit for bit."""
    J14 = list(pkg.netspec.H36M_TO_J14)
    J = torch.from_numpy(table_of(pkg, jreg_golden["recipe_b"]))
    frames = torch.from_numpy(pkg.synth.make_frames(2)).cuda().reshape(1, 2, 3, 224, 224)
    model.set_joint_regressor(J, select=None)
    assert model.joint_regressor_rows() == 17
    uploads = model.joint_regressor_uploads
    out = model(frames, J_regressor=J)[-1]
    assert out["kp_3d"].shape == (1, 2, 14, 3) and model.joint_regressor_uploads == uploads + 1
    model(frames, J_regressor=J)
    assert model.joint_regressor_uploads == uploads + 1
    model.set_joint_regressor(J, select=None)
    all17 = model.regress_joints(out["verts"])
    assert all17.shape == (1, 2, 17, 3) and torch.equal(out["kp_3d"], all17[:, :, J14])
    model.set_joint_regressor(J, select=J14[::-1])                          # same length, other joints
    uploads = model.joint_regressor_uploads
    again = model(frames, J_regressor=J)[-1]
    assert model.joint_regressor_uploads == uploads + 1 and torch.equal(again["kp_3d"], out["kp_3d"])
    model.set_joint_regressor(J, select=None)
    g = golden["grnet_n4"]
    betas, rotmat = torch.from_numpy(g["pred_shape"]).cuda(), torch.from_numpy(g["pred_rotmat"]).cuda()
    verts, kp3d, _ = model.smpl_forward(betas, rotmat, J_regressor=J)
    model.set_joint_regressor(J, select=None)
    assert kp3d.shape == (4, 14, 3) and torch.equal(kp3d, model.regress_joints(verts)[:, J14])
    model.set_joint_regressor(None)


def test_temporal_branch_regresses_the_corrected_vertices(pkg, jreg_golden):
    m = pkg.build_synthetic_model(max_frames=8, use_gait_feat=True)
    try:
        frames = torch.from_numpy(pkg.synth.make_frames(8)).cuda().reshape(1, 8, 3, 224, 224)
        bbox, cimg = (torch.from_numpy(a).cuda() for a in pkg.synth.make_gait_boxes(1, 8))
        J = table_of(pkg, jreg_golden["recipe_b"])
        out = m(frames, bbox=bbox, cimg=cimg, J_regressor=J)[-1]
        plain = m(frames, bbox=bbox, cimg=cimg)[-1]
        assert out["kp_3d"].shape == (1, 8, 14, 3) and plain["kp_3d"].shape == (1, 8, 29, 3)
        assert torch.equal(out["verts"], plain["verts"]) and torch.equal(out["theta"], plain["theta"])
        assert torch.equal(out["kp_3d"], m.regress_joints(out["verts"]))
        m.use_gait_feat = False
        first = m(frames)[-1]
        assert not torch.equal(first["verts"], out["verts"])
        assert not torch.equal(m.regress_joints(first["verts"]), out["kp_3d"])
    finally:
        m.close()


def test_bf16_handle(pkg, jreg_golden):
    m = pkg.build_synthetic_model(max_frames=4, dtype="bf16")
    try:
        exact_check(m, 17, list(pkg.netspec.H36M_TO_J14), 4)
        frames = torch.from_numpy(pkg.synth.make_frames(4)).cuda().reshape(2, 2, 3, 224, 224)
        out = m(frames, J_regressor=table_of(pkg, jreg_golden["recipe_a"]))[-1]
        assert out["kp_3d"].shape == (2, 2, 14, 3) and out["kp_2d"].shape == (2, 2, 29, 2)
        assert torch.equal(out["kp_3d"], m.regress_joints(out["verts"]))
    finally:
        m.close()


def test_state_and_errors(model, pkg, real_verts):
    lib, E = pkg._lib, pkg._lib.GrnetError
    A = pkg.synth.make_joint_regressor(24, nnz=32, seed=1)
    B = pkg.synth.make_joint_regressor(49, nnz=None, signed=True, seed=2)
    v = real_verts.cpu().numpy()
    model.set_joint_regressor(A)
    ja = model.regress_joints(real_verts)
    model.set_joint_regressor(B)
    jb = model.regress_joints(real_verts)
    assert ja.shape == (16, 24, 3) and jb.shape == (16, 49, 3) and model.joint_regressor_rows() == 49
    assert rel_err(ja.cpu().numpy(), f64_joints(A, v)) < 1e-5 and rel_err(jb.cpu().numpy(), f64_joints(B, v)) < 1e-5
    model.set_joint_regressor(None)
    assert model.joint_regressor_rows() == 0
    with pytest.raises(E, match="code -1:.*table"):
        model.regress_joints(real_verts)
    model.set_joint_regressor(A)
    out = torch.empty(MAXF + 1, 24, 3, device="cuda")
    big = torch.zeros(MAXF + 1, V, 3, device="cuda")
    rc = model._lib.grnet_regress_joints(model._h, big.data_ptr(), MAXF + 1, out.data_ptr(), None)
    assert rc == lib.EINVAL and b"max_frames" in model._lib.grnet_last_error(model._h)
    assert model._lib.grnet_regress_joints(model._h, None, 1, out.data_ptr(), None) == lib.EINVAL
    with pytest.raises(E, match="limit of 64"):
        model.set_joint_regressor(np.zeros((lib.JOINT_REGRESSOR_MAX_ROWS + 1, V), np.float32))
    bad = A.copy()
    bad[3, 100] = np.nan
    with pytest.raises(E, match="non-finite"):
        model.set_joint_regressor(bad)
    bad[3, 100] = np.inf
    with pytest.raises(E, match="non-finite"):
        model.set_joint_regressor(bad)
    sel = (C.c_int32 * 2)(0, 24)
    rc = model._lib.grnet_set_joint_regressor(model._h, A.ctypes.data_as(C.c_void_p), 24, sel, 2)
    assert rc == lib.EINVAL and b"outside" in model._lib.grnet_last_error(model._h)
    assert model._lib.grnet_set_joint_regressor(model._h, A.ctypes.data_as(C.c_void_p), 0, None, 0) == lib.EINVAL
    # every refusal left the handle, and the table set before it, in working order
    assert model.joint_regressor_rows() == 24 and torch.equal(model.regress_joints(real_verts), ja)
    model.set_joint_regressor(None)
