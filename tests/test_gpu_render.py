"""The mesh overlay on the device (csrc/render_kernels.hip; grnet_op_raster_setup / grnet_op_raster / grnet_load_faces / grnet_render_meshes;
the rules: DESIGN.md 4.5) against tests/helpers/raster_checks.py: vertex setup against float64, coverage bit for bit and the winning face
against the integer reference fed the device's own snapped vertices, shading against the float64 formula on the device's winner map, the
composite byte for byte, painter's order, chunking, refusals, and demo.py --mesh_render --sideview --save_obj."""
import ctypes as C
import importlib
import os
import sys

import joblib
import numpy as np
import pytest
import torch

from .conftest import ROOT
from .helpers import raster_checks as rc

pytestmark = pytest.mark.gpu

SCENES = rc.scenes()
COLOUR = (1.0, 0.55, 0.2)             # in the image's memory order


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=2, with_gru=False)
    yield m
    m.close()


def _draw(model, sc):
    """The stages alone on one scene, and the references they are held against.  The integer reference reads the DEVICE's snapped vertices and z."""
    xy, z, nrm = model.op_raster_setup(sc["verts"], sc["faces"], sc["cam"], sc["H"], sc["W"], M=sc["M"])
    winner = model.op_raster(xy, z, sc["faces"], sc["H"], sc["W"])
    xy, z, nrm, winner = xy.cpu().numpy(), z.cpu().numpy(), nrm.cpu().numpy(), winner.cpu().numpy()
    X64, Y64, z64, n64, q64 = rc.setup(sc["verts"], sc["faces"], sc["cam"], sc["M"], sc["H"], sc["W"])
    ref, d1, d2 = rc.rasterise(xy[:, 0], xy[:, 1], z, sc["faces"], sc["H"], sc["W"])
    return dict(xy=xy, z=z, nrm=nrm, winner=winner, X64=X64, Y64=Y64, z64=z64, n64=n64, q64=q64, ref=ref, d1=d1, d2=d2)


@pytest.fixture(scope="module")
def drawn(model):
    """Every scene drawn once by the stage hooks, shared by the tests below; nothing modifies it."""
    return {name: _draw(model, sc) for name, sc in SCENES.items()}


def _check_setup(sc, d):
    used = np.unique(sc["faces"])
    assert np.abs(d["xy"][:, 0] - d["X64"]).max() <= 1 and np.abs(d["xy"][:, 1] - d["Y64"]).max() <= 1
    assert (np.abs(d["z"] - d["z64"]) <= 4 * 2.0 ** -23 * np.maximum(1.0, np.abs(d["z64"]))).all()
    assert np.abs(d["nrm"][used] - d["n64"][used]).max() <= 1e-5
    unused = np.setdiff1d(np.arange(len(sc["verts"])), used)
    assert not d["nrm"][unused].any()


def _check_raster(d):
    rc.check_cover(d["winner"], d["ref"])
    return rc.check_winner(d["winner"], d["ref"], d["d1"], d["d2"])


def _render(model, sc, d, background_seed=5, guard=4096):
    """One scene through load_faces + render into a random image with a guard region behind it; every check of item 3."""
    H, W = sc["H"], sc["W"]
    g = np.random.Generator(np.random.Philox(key=[background_seed, H * W]))
    flat = torch.from_numpy(g.integers(0, 256, H * W * 3 + guard, dtype=np.uint8)).cuda()
    before = flat.cpu().numpy().copy()
    model.load_faces(sc["faces"])
    model.render(flat[:H * W * 3].view(1, H, W, 3), rc.pad_to_smpl(sc["verts"])[None], sc["cam"][None], [COLOUR], [0], M=sc["M"], rgb=False)
    after = flat.cpu().numpy()
    assert np.array_equal(after[H * W * 3:], before[H * W * 3:]), "the guard region behind the image changed"
    levels = rc.shade(d["q64"], d["n64"], d["xy"][:, 0], d["xy"][:, 1], sc["faces"], d["winner"], COLOUR)
    image, was = after[:H * W * 3].reshape(H, W, 3), before[:H * W * 3].reshape(H, W, 3)
    rc.check_image(image, was, levels)
    return image, was


# ------------------------------------------------------------------ 1. setup
@pytest.mark.parametrize("name", sorted(SCENES))
def test_setup_against_float64(drawn, name):
    _check_setup(SCENES[name], drawn[name])


def test_setup_snaps_pixel_centres_exactly(model):
    """x_ndc = (k + 1/2) / 32 - 1 at W = 64 is pixel k's centre exactly, in fp32 too: it must snap to 256 k + 128, not beside it."""
    k = np.arange(64)
    v = np.stack([(k + 0.5) / 32 - 1, -((k % 48 + 0.5) / 24 - 1), np.zeros(64)], 1).astype(np.float32)
    assert np.array_equal(v[:, 0].astype(np.float64), (k + 0.5) / 32 - 1)
    xy, _, _ = model.op_raster_setup(v, [(0, 1, 2)], (1.0, 1.0, 0.0, 0.0), 48, 64)
    xy = xy.cpu().numpy()
    assert np.array_equal(xy[:, 0], 256 * k + 128)
    assert np.array_equal(xy[:, 1], 256 * (k % 48) + 128)
    huge = np.array([[1e30, -1e30, 0], [np.nan, np.inf, 0], [0, 0, 0]], np.float32)        # clamped, never out of range
    xy, _, _ = model.op_raster_setup(huge, [(0, 1, 2)], (1.0, 1.0, 0.0, 0.0), 48, 64)
    assert np.abs(xy.cpu().numpy().astype(np.int64)).max() <= rc.LIMIT


# ------------------------------------------------------------------ 2. raster
@pytest.mark.parametrize("name", sorted(SCENES))
def test_raster_cover_and_winner(drawn, name):
    _check_raster(drawn[name])


def test_raster_rules_by_name(drawn):
    """What the scenes are for, read off the DEVICE's pictures."""
    H, W = 48, 64
    want = np.zeros((H, W), bool)
    want[7:30, 5:41] = True
    for name in ("split_rectangle", "split_rectangle_other"):
        assert np.array_equal(drawn[name]["winner"] >= 0, want)                             # [c0,c1) x [r0,r1), each pixel once
    assert (drawn["larger_than_image"]["winner"] == 0).all()
    assert set(np.unique(drawn["off_each_side"]["winner"])) == {-1, 0, 2, 4, 6, 8}
    assert set(np.unique(drawn["zero_area"]["winner"])) == {-1, 1}
    assert set(np.unique(drawn["back_facing"]["winner"])) == {-1, 1}
    for name in ("equal_depth", "equal_depth_swapped"):
        overlap = np.isfinite(drawn[name]["d2"])
        assert overlap.sum() > 100 and (drawn[name]["winner"][overlap] == 0).all()          # the lower index, whichever triangle carries it
    for name in ("crossing_far", "crossing_near"):
        cut = drawn[name]["winner"] >= 0
        assert cut.any() and not cut[:8].any()                                              # the end beyond the plane (the top of the image) is clipped
    assert drawn["triangle_1x1"]["winner"].tolist() == [[0]]


# ------------------------------------------------------------------ 3. shade and composite
@pytest.mark.parametrize("name", ("triangle_7x5", "triangle_97x61", "off_each_side", "equal_depth", "crossing_far", "torus_12x8", "torus_320x240",
                                  "torus_97x61_side", "negative_sx"))
def test_shade_and_composite(model, drawn, name):
    image, was = _render(model, SCENES[name], drawn[name])
    covered = drawn[name]["winner"] >= 0
    assert covered.any() and (image[covered] != was[covered]).any()


def test_colour_order(model, drawn):
    """rgb=True hands the triple down reversed (the reference writes (r,g,b) into a BGR image unswapped); rgb=False as it is."""
    sc, d = SCENES["triangle_64x48"], drawn["triangle_64x48"]
    model.load_faces(sc["faces"])
    pics = []
    for rgb, col in ((False, (0.9, 0.5, 0.1)), (True, (0.1, 0.5, 0.9))):
        img = torch.zeros(1, sc["H"], sc["W"], 3, dtype=torch.uint8, device="cuda")
        model.render(img, rc.pad_to_smpl(sc["verts"])[None], sc["cam"][None], [col], [0], rgb=rgb)
        pics.append(img.cpu().numpy())
    assert np.array_equal(pics[0], pics[1]) and (pics[0][0][d["winner"] >= 0] > 0).all()
    px = pics[0][0][d["winner"] >= 0][0].astype(int)
    assert px[0] > px[1] > px[2]


# ------------------------------------------------------------------ 4. painter's order, chunks, determinism
@pytest.fixture(scope="module")
def crowd(model):
    """24 tori (more than the 16 meshes of a launch group), tilted differently, each drawn ALONE into its own 97 x 61 image: the pictures the
    multi-mesh calls are held against, bit for bit."""
    n, H, W = 24, 61, 97
    verts = np.stack([rc.torus(65, 106, R=0.45, r=0.2, tilt=(0.3 * k, 0.5 + 0.2 * k))[0] for k in range(n)])
    faces = rc.torus(65, 106)[1]
    cams = np.stack([(0.8, 0.8 * W / H, 0.3 * np.cos(k), 0.2 * np.sin(k)) for k in range(n)]).astype(np.float32)
    g = np.random.Generator(np.random.Philox(key=[9, 9]))
    cols = g.uniform(0.2, 1.0, (n, 3)).astype(np.float32)
    back = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    model.load_faces(faces)
    alone, masks = [], []
    for k in range(n):
        img = torch.from_numpy(back[None].copy()).cuda()
        model.render(img, verts[k:k + 1], cams[k:k + 1], cols[k:k + 1], [0], rgb=False)
        alone.append(img.cpu().numpy()[0])
        xy, z, _ = model.op_raster_setup(verts[k], faces, cams[k], H, W)
        masks.append(model.op_raster(xy, z, faces, H, W).cpu().numpy() >= 0)
    model.load_faces(faces)
    return dict(n=n, H=H, W=W, verts=torch.from_numpy(verts).cuda(), faces=faces, cams=cams, cols=cols, back=back, alone=alone, masks=masks)


def _paint(back, layers):
    out = back.copy()
    for pic, mask in layers:
        out[mask] = pic[mask]
    return out


def test_painters_order_in_one_image(model, crowd):
    c = crowd
    model.load_faces(c["faces"])
    assert (c["masks"][0] & c["masks"][1]).sum() > 50
    for order in ((0, 1), (1, 0), (2, 0, 1, 0)):
        idx = list(order)
        img = torch.from_numpy(c["back"][None].copy()).cuda()
        model.render(img, c["verts"][idx], c["cams"][idx], c["cols"][idx], [0] * len(idx), rgb=False)
        want = _paint(c["back"], [(c["alone"][k], c["masks"][k]) for k in idx])
        assert np.array_equal(img.cpu().numpy()[0], want), order
    a = _paint(c["back"], [(c["alone"][k], c["masks"][k]) for k in (0, 1)])
    b = _paint(c["back"], [(c["alone"][k], c["masks"][k]) for k in (1, 0)])
    assert not np.array_equal(a, b)


def test_many_meshes_many_images_equal_one_call_each(pkg, model, crowd):
    """n = 24 + 24 + 3 meshes over 24 images in ONE call: four layers, the first two of two launch groups each (16 + 8); every image must be
    bit-identical to its meshes drawn one call each, and a second run to the first."""
    c = crowd
    model.load_faces(c["faces"])
    n = c["n"]
    mesh = list(range(n)) + [(k + 5) % n for k in range(n)] + [7, 8, 9]
    where = list(range(n)) + list(range(n))[::-1] + [3, 3, 20]
    runs = []
    for _ in range(2):
        imgs = torch.from_numpy(np.repeat(c["back"][None], n, 0).copy()).cuda()
        model.render(imgs, c["verts"][mesh], c["cams"][mesh], c["cols"][mesh], where, rgb=False)
        runs.append(imgs.cpu().numpy())
    assert np.array_equal(runs[0], runs[1])
    for f in range(n):
        layers = [(c["alone"][m], c["masks"][m]) for m, w in zip(mesh, where) if w == f]
        assert len(layers) >= 2
        assert np.array_equal(runs[0][f], _paint(c["back"], layers)), f
    assert model.arena_info() == pkg.grnet.arena_query("f32", 2, compact=False)


# ------------------------------------------------------------------ 5. refusals
def test_refusals_and_empty_call(pkg, model, crowd):
    c = crowd
    lib, L = model._lib, pkg._lib
    model.load_faces(c["faces"])
    img = torch.from_numpy(c["back"][None].copy()).cuda()
    cams = torch.from_numpy(c["cams"]).cuda()
    col = np.ascontiguousarray(c["cols"])
    idx = np.zeros(c["n"], np.int32)
    H, W = c["H"], c["W"]
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(n=1, verts=c["verts"].data_ptr(), cams_=cams.data_ptr(), col_=p(col), idx_=p(idx), images=img.data_ptr(), F=1, H_=H, W_=W, h=model._h):
        return lib.grnet_render_meshes(h, verts, n, cams_, col_, idx_, None, images, F, H_, W_, None)

    assert call(n=-1) == L.EINVAL and b"n -1" in lib.grnet_last_error(model._h)
    for bad in (dict(H_=0), dict(W_=0), dict(H_=4097), dict(W_=4097), dict(F=0)):
        assert call(**bad) == L.EINVAL, bad
    for bad in (dict(verts=None), dict(cams_=None), dict(col_=None), dict(idx_=None), dict(images=None)):
        assert call(**bad) == L.EINVAL, bad
    assert call(h=None) == L.EINVAL
    for wrong in (-1, 1):
        idx[0] = wrong
        assert call() == L.EINVAL and b"image_index" in lib.grnet_last_error(model._h)
    idx[0] = 0
    assert call(n=0, verts=None, cams_=None, col_=None, idx_=None) == 0                     # a no-op
    torch.cuda.synchronize()
    assert np.array_equal(img.cpu().numpy()[0], c["back"])
    bad_faces = np.array([[0, 1, 6890]], np.int32)
    assert lib.grnet_load_faces(model._h, p(bad_faces), 1) == L.EINVAL and b"6890" in lib.grnet_last_error(model._h)
    assert lib.grnet_load_faces(model._h, None, 1) == L.EINVAL and lib.grnet_load_faces(model._h, p(bad_faces), 0) == L.EINVAL
    with pytest.raises(ValueError):
        model.load_faces(np.zeros((3, 2), np.int32))
    with pytest.raises(ValueError):
        model.render(img.float(), c["verts"][:1], c["cams"][:1], c["cols"][:1], [0])
    one = np.zeros((1, 3), np.int32)
    out = torch.zeros(64, dtype=torch.int32, device="cuda")
    for V, F in ((0, 1), (3, 0)):                                                        # valid pointers, an empty mesh
        rc_ = lib.grnet_op_raster_setup(model._h, c["verts"].data_ptr(), V, p(one), F, cams.data_ptr(), None, 8, 8, out.data_ptr(), out.data_ptr(), out.data_ptr(), None)
        assert rc_ == L.EINVAL and b"V and F" in lib.grnet_last_error(model._h)
        assert lib.grnet_op_raster(model._h, out.data_ptr(), out.data_ptr(), V, p(one), F, 8, 8, out.data_ptr(), None) == L.EINVAL
    assert lib.grnet_op_raster(model._h, out.data_ptr(), out.data_ptr(), 3, p(one), 1, 8, 4097, out.data_ptr(), None) == L.EINVAL
    with pytest.raises(L.GrnetError, match="outside"):
        model.op_raster_setup(np.zeros((3, 3), np.float32), [(0, 1, 3)], (1, 1, 0, 0), 8, 8)
    # the failed calls left the table in place: the handle still draws
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(img.cpu().numpy()[0], c["alone"][0])
    # a handle without faces refuses to draw (before or after finalize)
    fresh = pkg.GRNet(max_frames=1)
    try:
        assert call(h=fresh._h) == L.ESTATE and b"grnet_load_faces" in lib.grnet_last_error(fresh._h)
        fresh.load_faces(c["faces"])                                                     # before finalize
        assert call(h=fresh._h) == 0
        torch.cuda.synchronize()
        assert np.array_equal(img.cpu().numpy()[0], c["alone"][0])
    finally:
        fresh.close()


# ------------------------------------------------------------------ 6. demo.py
def test_demo_mesh_render(pkg, model, tmp_path):
    from PIL import Image
    sys.path.insert(0, ROOT)
    demo = importlib.import_module("demo")
    H, W, T = 120, 160, 30
    g = np.random.Generator(np.random.Philox(key=[21, 21]))
    img_dir = str(tmp_path / "vid")
    os.makedirs(img_dir)
    frames = g.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(img_dir, f"{i:06d}.png"))
    box = lambda n, cx: np.tile(np.array([[cx, 60.0, 90.0, 90.0]], np.float32), (n, 1))
    tp = str(tmp_path / "tracking.pkl")
    # person 1: frames 0..25, person 2: frames 2..27 -- both in 2..25, nobody in 28, 29
    joblib.dump({1: {"bbox": box(26, 60.0), "frames": np.arange(0, 26)}, 2: {"bbox": box(26, 100.0), "frames": np.arange(2, 28)}}, tp)
    base = ["--img_folder", img_dir, "--tracking_path", tp, "--synthetic_weights", "--grnet_batch_size", "16", "--max_frames", "16", "--save_vid"]
    plain = demo.main(demo.parser().parse_args(base + ["--output_folder", str(tmp_path / "a")]))
    out = demo.main(demo.parser().parse_args(base + ["--output_folder", str(tmp_path / "b"), "--mesh_render", "--sideview", "--save_obj"]))
    res, ref = joblib.load(out), joblib.load(plain)
    assert set(res) == set(ref) == {1, 2}
    for pid in res:                                                                      # the pickle is what it is without --mesh_render
        assert set(res[pid]) == set(ref[pid])
        for k in res[pid]:
            assert np.array_equal(res[pid][k], ref[pid][k]) and res[pid][k].dtype == ref[pid][k].dtype, (pid, k)
    folder = out[:-len(".pkl")] + "_output"
    pngs = sorted(os.listdir(folder))
    assert pngs == [f"{i:06d}.png" for i in range(T)]
    pics = np.stack([np.asarray(Image.open(os.path.join(folder, p))) for p in pngs])
    assert pics.shape == (T, H, 2 * W, 3)                                                # the side view doubles the width
    for i in (28, 29):                                                                   # nobody there: the input, and black beside it
        assert np.array_equal(pics[i, :, :W], frames[i]) and not pics[i, :, W:].any()
    # a frame with one person or both differs from its input only inside the reference's mask.  The pickle holds exactly the fp32 vertices and
    # orig_cam the demo drew, so the mask is EXACT: the device's own snapped vertices of those rows through the integer reference, as in item 2
    faces = pkg.synth.make_faces()
    for i in (0, 10, 27):
        mask, side = np.zeros((H, W), bool), np.zeros((H, W), bool)
        for pid in res:
            for r in np.nonzero(res[pid]["frame_ids"] == i)[0]:
                for M, m in ((None, mask), (rc.SIDE_M, side)):
                    xy, z, _ = model.op_raster_setup(res[pid]["verts"][r], faces, res[pid]["orig_cam"][r], H, W, M=M)
                    xy, z = xy.cpu().numpy(), z.cpu().numpy()
                    m |= rc.rasterise(xy[:, 0], xy[:, 1], z, faces, H, W)[0] >= 0
        assert mask.sum() > 20 and side.sum() > 20, i
        changed, lit = (pics[i, :, :W] != frames[i]).any(-1), pics[i, :, W:].any(-1)
        assert not (changed & ~mask).any(), i
        # a covered pixel keeps its input only where all three shaded bytes equal the random frame's (2**-24 a pixel): none of a few thousand
        assert (mask & ~changed).sum() <= 1, i
        # on black every covered pixel is lit: shade >= 0.3 and the colour's least channel is 0.5 (HSV with s = 0.5, v = 1), so >= 38 levels
        assert np.array_equal(lit, side), i
    assert (len(os.listdir(os.path.join(os.path.dirname(out), "rendered", "0001"))), len(os.listdir(os.path.join(os.path.dirname(out), "rendered", "0002")))) == (26, 26)
    obj = open(os.path.join(os.path.dirname(out), "rendered", "0002", "000002.obj")).read().split("\n")
    v = np.array([l.split()[1:] for l in obj if l.startswith("v ")], np.float64)
    f = np.array([l.split()[1:] for l in obj if l.startswith("f ")], np.int64)
    assert np.allclose(v, res[2]["verts"][0].astype(np.float64) * [1, -1, -1], atol=1e-7) and np.array_equal(f, faces + 1)
    assert demo.refusal(demo.parser().parse_args(["--wireframe"])) and "line" in demo.refusal(demo.parser().parse_args(["--wireframe"]))
    assert demo.refusal(demo.parser().parse_args(["--display"])) and demo.refusal(demo.parser().parse_args(["--mesh_render"])) is None


# ------------------------------------------------------------------ 7. one production-size frame
def test_one_1080p_frame(model):
    sc = rc.scene_1080p()
    d = _draw(model, sc)
    _check_setup(sc, d)
    _check_raster(d)
    assert (d["winner"] >= 0).sum() > 100000
    _render(model, sc, d)
