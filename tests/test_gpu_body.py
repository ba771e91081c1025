"""Mesh volume, centre of mass and second moments on the GPU (grnet_mesh_moments, csrc/mesh_moments_kernels.hip) against the host
statement pipeline.mesh_moments.  The arithmetic is + - * / sqrt in float64 in fixed orders, so EVERY OUTPUT BIT IS EQUAL, NaN patterns included:
there is no tolerance anywhere in this file.  The face counts are the smallest at which the column logic can go wrong, all closed tables over a
subset of the 6890 vertices (tests/helpers/body_checks.py): 4 (1020 empty columns), 12, 1022 / 1024 / 1026 (the first column seam), 13 776 (SMPL's
count) and 13 780 (the synthetic table); 1, 3 and 17 frames; both forms of the gather; a frame alone; guard regions; the NaN rules and the flipped
mesh; scaling by powers of two; every refusal; gait_balance(com=...); WindowBody and run_on_frames(body=True) on a real handle."""
import ctypes as C
import functools
import importlib
import os

import numpy as np
import pytest
import torch

from .helpers import balance_checks as bal
from .helpers import body_checks as bc

pytestmark = pytest.mark.gpu
COUNTS = (4, 12, 1022, 1024, 1026, 13776, 13780)
FRAMES = (1, 3, 17)


@pytest.fixture(scope="module")
def model(pkg):
    """A handle of this module's own: its face table is replaced test by test.  No weights: the call reads none."""
    m = pkg.GRNet(max_frames=1)
    yield m
    m.close()


@functools.lru_cache(maxsize=None)
def statement(pkg_name, F):
    """(faces, verts of 17 frames, rows, sums) of a case, computed once and shared."""
    pipe = importlib.import_module(pkg_name).pipeline
    faces, verts = bc.case(F, n=max(FRAMES), seed=F)
    return (faces, verts) + pipe.mesh_moments(verts, faces, return_sums=True)


def device(model, verts, **kw):
    rows, sums = model.mesh_moments(torch.from_numpy(verts).cuda(), return_sums=True, **kw)
    assert rows.is_cuda and sums.is_cuda and rows.dtype == sums.dtype == torch.float64 and tuple(rows.shape) == tuple(sums.shape) == (len(verts), 11)
    return rows.cpu().numpy(), sums.cpu().numpy()


@pytest.mark.parametrize("F", COUNTS)
def test_rows_and_sums_equal_the_statement(model, pkg, F):
    faces, verts, rows, sums = statement(pkg.__name__, F)
    model.load_faces(faces)
    assert model.faces_closed() == 0
    for n in FRAMES:
        for form in (None, 0, 1):
            got = device(model, verts[:n], form=form)
            assert bc.same_bits(got[0], rows[:n]) and bc.same_bits(got[1], sums[:n]), (F, n, form)
    alone = device(model, verts[1:2])                             # frame 1 of 3 alone: the same bits
    assert bc.same_bits(alone[0], rows[1:2]) and bc.same_bits(alone[1], sums[1:2])
    only = model.mesh_moments(torch.from_numpy(verts[:3]).cuda())
    assert torch.is_tensor(only) and bc.same_bits(only.cpu().numpy(), rows[:3])
    half = model.mesh_moments(torch.from_numpy(verts[:2]).cuda().double())       # any float dtype: taken as float32
    assert bc.same_bits(half.cpu().numpy(), rows[:2])
    print(f"{F} faces: volumes {rows[:3, 0].tolist()}")
    assert (rows[:, 0] > 0).all() and np.isfinite(rows).all()


def test_guard_regions_stay_untouched(model, pkg):
    faces, verts, rows, sums = statement(pkg.__name__, 1026)
    model.load_faces(faces)
    lib, h = pkg._lib.load(), model._h
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for form in (0, 1):
        for n in (1, 3):
            v = torch.from_numpy(verts[:n]).cuda()
            out = torch.full((2, n + 2, 11), -7.0, dtype=torch.float64, device="cuda")
            assert lib.grnet_op_mesh_moments(h, v.data_ptr(), n, out[0, 1].data_ptr(), out[1, 1].data_ptr(), form, stream) == 0
            got = out.cpu().numpy()
            assert bc.same_bits(got[0, 1:n + 1], rows[:n]) and bc.same_bits(got[1, 1:n + 1], sums[:n])
            assert (got[:, 0] == -7.0).all() and (got[:, n + 1] == -7.0).all()
            out.fill_(-7.0)
            assert lib.grnet_op_mesh_moments(h, v.data_ptr(), n, out[0, 1].data_ptr(), None, form, stream) == 0       # without the sums
            got = out.cpu().numpy()
            assert bc.same_bits(got[0, 1:n + 1], rows[:n]) and (got[1] == -7.0).all() and (got[0, 0] == -7.0).all() and (got[0, n + 1] == -7.0).all()
    # a frame that does not begin on a 16-byte boundary: the staged form shifts its image (82 680 bytes a frame: every odd frame)
    v = torch.from_numpy(verts[:4]).cuda()
    got = model.mesh_moments(v[1:2], form=1)
    assert v[1:2].data_ptr() % 16 == 8 and bc.same_bits(got.cpu().numpy(), rows[1:2])
    flat = torch.zeros(3 * bc.V * 3 + 3, dtype=torch.float32, device="cuda")
    for lead in (1, 2, 3):                                       # ... and on every other 4-byte boundary
        flat[lead:lead + 2 * bc.V * 3] = v[:2].reshape(-1)
        shifted = flat[lead:lead + 2 * bc.V * 3].view(2, bc.V, 3)
        out = torch.empty(2, 11, dtype=torch.float64, device="cuda")
        assert lib.grnet_op_mesh_moments(h, shifted.data_ptr(), 2, out.data_ptr(), None, 1, stream) == 0
        assert shifted.data_ptr() % 16 == (4 * lead) % 16 and bc.same_bits(out.cpu().numpy(), rows[:2]), lead


def test_nan_rules_and_the_flipped_mesh(model, pkg):
    faces, verts, rows, sums = statement(pkg.__name__, 1026)
    model.load_faces(faces)
    three = verts[:3].copy()
    spare = bc.unreferenced(faces)
    three[:, spare[::7]] = np.nan
    three[1, spare[3]] = np.inf
    for form in (0, 1):
        got = device(model, three, form=form)
        assert bc.same_bits(got[0], rows[:3]) and bc.same_bits(got[1], sums[:3])          # an unreferenced vertex changes no bit
    three = verts[:3].copy()
    three[1, faces[700, 1], 2] = np.nan
    want = pkg.pipeline.mesh_moments(three, faces, return_sums=True)
    for form in (0, 1):
        got = device(model, three, form=form)
        assert np.isnan(got[0][1]).all() and np.isnan(got[1][1]).all()                    # a referenced one: its frame's row is NaN ...
        assert bc.same_bits(got[0], want[0]) and bc.same_bits(got[0][[0, 2]], rows[[0, 2]]) and bc.same_bits(got[1][[0, 2]], sums[[0, 2]])      # ... its neighbours are not
    model.load_faces(faces[:, ::-1])
    want = pkg.pipeline.mesh_moments(verts[:3], faces[:, ::-1], return_sums=True)
    got = device(model, verts[:3])
    assert bc.same_bits(got[0], want[0]) and bc.same_bits(got[1], want[1])
    assert (got[0][:, 0] < 0).all() and np.isnan(got[0][:, 1:10]).all() and np.isfinite(got[0][:, 10]).all()


def test_magnitudes_scale_exactly(model, pkg):
    """Vertices scaled by 2^-20 and 2^20: every operation scales exactly, so the sums are the unscaled ones times the power of their degree."""
    faces, verts, rows, sums = statement(pkg.__name__, 13776)
    model.load_faces(faces)
    degree = np.array([3, 4, 4, 4, 5, 5, 5, 5, 5, 5, 2])
    for e in (-20, 20):
        scaled = np.ldexp(verts[:2].astype(np.float64), e).astype(np.float32)
        assert np.array_equal(np.ldexp(scaled.astype(np.float64), -e), verts[:2].astype(np.float64))
        got = device(model, scaled)
        assert bc.same_bits(got[1], np.ldexp(sums[:2], e * degree)), e
        assert bc.same_bits(got[0], pkg.pipeline.mesh_moments(scaled, faces))
        assert bc.same_bits(got[0][:, 0], np.ldexp(rows[:2, 0], 3 * e)) and bc.same_bits(got[0][:, 4:10], np.ldexp(rows[:2, 4:10], 2 * e))


def test_refusals_leave_the_outputs_untouched(pkg):
    lib = pkg._lib.load()
    m = pkg.GRNet(max_frames=1)
    try:
        h = m._h
        faces, verts, rows, sums = statement(pkg.__name__, 1026)
        v = torch.from_numpy(verts[:2]).cuda()
        out = torch.full((2, 2, 11), -7.0, dtype=torch.float64, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        count = C.c_int(-7)

        def run(n=2, null=None, form=None):
            args = [h, v.data_ptr(), n, out[0].data_ptr(), out[1].data_ptr()] + ([] if form is None else [form]) + [stream]
            if null is not None:
                args[null] = None
            return (lib.grnet_mesh_moments if form is None else lib.grnet_op_mesh_moments)(*args)

        assert run() == pkg._lib.ESTATE and b"before grnet_load_faces" in lib.grnet_last_error(h)             # no faces loaded
        assert lib.grnet_faces_closed(h, C.byref(count)) == pkg._lib.ESTATE and count.value == -7
        with pytest.raises(pkg._lib.GrnetError, match="before grnet_load_faces"):
            m.mesh_moments(v)
        m.load_faces(faces[:-1])                                 # an open table: one face removed
        assert m.faces_closed() == 3
        assert run() == pkg._lib.EINVAL and lib.grnet_last_error(h).decode() == "grnet_mesh_moments: " + bc.OPEN_TEXT.format(3)
        m.load_faces(np.concatenate([faces, faces[5:6]]))        # a face twice
        assert m.faces_closed() == 6
        assert run(form=1) == pkg._lib.EINVAL and lib.grnet_last_error(h).decode() == "grnet_op_mesh_moments: " + bc.OPEN_TEXT.format(6)
        wrong = faces.copy()
        wrong[7, 2] = bc.V
        with pytest.raises(pkg._lib.GrnetError) as e:            # a refused table leaves the one loaded before in place
            m.load_faces(wrong)
        assert bc.INDEX_TEXT.format(7, bc.V, bc.V) in str(e.value) and m.faces_closed() == 6
        m.load_faces(faces)                                      # load_faces invalidates the count
        assert m.faces_closed() == 0 == pkg.pipeline.faces_closed(faces)
        for kw, word in ((dict(null=1), b"null"), (dict(null=3), b"null"), (dict(n=0), b"n 0 < 1"), (dict(n=-3), b"n -3 < 1"), (dict(form=2), b"form 2"), (dict(form=-1), b"form -1")):
            assert run(**kw) == pkg._lib.EINVAL, kw
            assert word in lib.grnet_last_error(h), (kw, lib.grnet_last_error(h))
        assert lib.grnet_faces_closed(h, None) == pkg._lib.EINVAL
        torch.cuda.synchronize()
        assert bool((out == -7.0).all())                         # nothing was written
        assert run(null=4) == 0                                  # only the sums may be NULL
        torch.cuda.synchronize()
        assert bc.same_bits(out[0].cpu().numpy(), rows[:2]) and bool((out[1] == -7.0).all())
        for bad in (v[0], v[:, :-1], v[:, :, :2], torch.zeros(0, bc.V, 3), torch.zeros(2, bc.V, 3, dtype=torch.int32)):      # wrong vertex count in Python
            with pytest.raises(ValueError, match="verts must be"):
                m.mesh_moments(bad)
    finally:
        m.close()


def test_gait_balance_with_a_given_com(pkg):
    """com set to rule 1's own c: every bit of the call without com.  A shifted com: every bit of pipeline.gait_balance(com=...)."""
    m = pkg.GRNet(max_frames=1)
    try:
        pipe = pkg.pipeline
        name, joints, par = bal.walker_cases(200)[0]
        lengths = [120, 80]
        events = pipe.gait_parameters(joints, lengths=lengths, fps=bal.FPS)["events"]
        com = pipe.balance_table_com(np.asarray(joints, np.float32).astype(np.float64))
        plain = {k: v.cpu().numpy() for k, v in m.gait_balance(joints, events, lengths=lengths, fps=bal.FPS).items()}
        given = m.gait_balance(joints, events, lengths=lengths, fps=bal.FPS, com=torch.from_numpy(com).cuda())
        assert all(v.is_cuda and v.dtype == torch.float64 for v in given.values()) and plain["per_sequence"][:, 1].min() >= 3
        for key in plain:
            assert bc.same_bits(given[key].cpu().numpy(), plain[key]), key
        shifted = com + np.array([0.01, 0.1, -0.02])
        shifted[57] = np.nan                                     # a frame without a centre of mass
        host = pipe.gait_balance(joints, events, lengths=lengths, fps=bal.FPS, com=shifted)
        got = m.gait_balance(joints, events, lengths=lengths, fps=bal.FPS, com=shifted)
        for key in plain:
            assert bc.same_bits(got[key].cpu().numpy(), host[key]), key
        assert not bc.same_bits(host["per_sequence"], plain["per_sequence"])
        with pytest.raises(ValueError, match="segments and com"):
            m.gait_balance(joints, events, lengths=lengths, fps=bal.FPS, com=com, segments=pipe.BALANCE_SEGMENTS_KINECTV2)
        with pytest.raises(ValueError, match="com must be"):
            m.gait_balance(joints, events, lengths=lengths, fps=bal.FPS, com=com[:-1])
        lib = pkg._lib.load()
        assert lib.grnet_gait_balance_com(m._h, None, 25, None, 1, None, None, None, 20.0, 9.81, 4, 1, 30, 256, None, None, None, None) == pkg._lib.EINVAL
        assert b"null pointer" in lib.grnet_last_error(m._h)
        with pytest.raises(pkg._lib.GrnetError, match="window"):
            m.gait_balance(joints, events, lengths=lengths, fps=bal.FPS, com=com, window=17)
    finally:
        m.close()


def test_window_body_and_run_on_frames_on_a_real_handle(pkg, tmp_path):
    """Shape and plumbing: the synthetic vertices are a point cloud, so a row has a centre exactly where its signed volume happens to be positive
    (rule 4) -- that, the shapes and the equality with the statement are asserted, not numbers."""
    import batch_generation as bg
    pipe = pkg.pipeline
    model = pkg.build_synthetic_model(max_frames=4, with_gru=False)
    try:
        assert model.faces_closed() == 0
        n = 6
        rng = np.random.default_rng(8)
        for k in range(n):
            np.save(os.path.join(str(tmp_path), f"{k:06d}.npy"), rng.standard_normal((3, 224, 224)).astype(np.float32))
        boxes = np.tile(np.array([[112.0, 112.0, 200.0, 200.0]], np.float32), (n, 1))
        made = pipe.run_on_frames(model, str(tmp_path), np.arange(n), boxes.copy(), device=model.device, batch_size=4, on_device=True, body=True)
        plain = pipe.run_on_frames(model, str(tmp_path), np.arange(n), boxes.copy(), device=model.device, batch_size=4, on_device=True)
        assert sorted(made) == ["body", "kp_3d"] and sorted(plain) == ["kp_3d"] and torch.equal(made["kp_3d"], plain["kp_3d"])
        rows = made["body"]
        assert rows.is_cuda and rows.dtype == torch.float64 and tuple(rows.shape) == (n, 11)
        host = pipe.run_on_frames(model, str(tmp_path), np.arange(n), boxes.copy(), device=model.device, batch_size=4, on_device=True, body=True, body_on_host=True)["body"]
        r = rows.cpu().numpy()
        assert bc.same_bits(r, host.cpu().numpy())
        has = r[:, 0] > 0
        print(f"volumes {r[:, 0].tolist()}: {int(has.sum())} of {n} frames have a centre")
        assert np.isfinite(r[:, [0, 10]]).all() and np.isnan(r[~has, 1:10]).all() and np.isfinite(r[has, 1:10]).all()
        w = bg.WindowBody(pipe, density=985.0)
        joints = made["kp_3d"].reshape(n, 75)
        out = w.add_window(["a", "b"], {0: joints[:4], 1: joints[4:]}, {0: rows[:4], 1: rows[4:]})
        assert [c.shape for c, v in out] == [(4, 3), (2, 3)] and [v.shape for c, v in out] == [(4,), (2,)] and all(c.dtype == v.dtype == np.float32 for c, v in out)
        assert w.com.is_cuda and tuple(w.com.shape) == (n, 3) and bc.same_bits(w.com.cpu().numpy(), r[:, 1:4])
        assert list(w.videos["a"]) == list(pipe.BODY_COLUMNS) + ["density"] and w.videos["a"]["frames"] == 4 and w.videos["a"]["frames_valid"] == int(has[:4].sum())
        assert (w.videos["a"]["volume_mean"] is None) == (has[:4].sum() == 0)
    finally:
        model.close()
