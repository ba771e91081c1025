"""The wireframe on the device (raster_lines_cover_kernel / raster_resolve_kernel<true> of csrc/render_kernels.hip; grnet_op_raster_lines,
grnet_render_meshes_ex with GRNET_RENDER_WIREFRAME; the rule: DESIGN.md 4.5) against tests/helpers/line_checks.py: coverage bit for bit and the
winning edge against the integer reference fed the device's own snapped vertices, shading against the float64 formula on the device's winner
map, the composite byte for byte, flags = 0, painter's order and order independence, refusals, and demo.py --mesh_render --wireframe --sideview."""
import ctypes as C
import importlib
import os
import sys

import joblib
import numpy as np
import pytest
import torch

from .conftest import ROOT
from .helpers import line_checks as lc
from .helpers import raster_checks as rc

pytestmark = pytest.mark.gpu

SCENES = lc.all_scenes()
WINNER_SCENES = sorted(lc.winner_scenes())
COLOUR = (1.0, 0.55, 0.2)             # in the image's memory order


@pytest.fixture(scope="module")
def model(pkg):
    m = pkg.build_synthetic_model(max_frames=2, with_gru=False)
    yield m
    m.close()


def _draw(model, sc):
    """The line stage alone on one scene, and the reference it is held against: the integer rule on the DEVICE's snapped vertices and z."""
    xy, z, nrm = model.op_raster_setup(sc["verts"], sc["faces"], sc["cam"], sc["H"], sc["W"], M=sc["M"])
    winner = model.op_raster_lines(xy, z, sc["faces"], sc["H"], sc["W"])
    xy, z, winner = xy.cpu().numpy(), z.cpu().numpy(), winner.cpu().numpy()
    _, _, _, n64, q64 = rc.setup(sc["verts"], sc["faces"], sc["cam"], sc["M"], sc["H"], sc["W"])
    ref, d1, d2 = lc.rasterise_lines(xy[:, 0], xy[:, 1], z, sc["faces"], sc["H"], sc["W"])
    return dict(xy=xy, z=z, winner=winner, n64=n64, q64=q64, ref=ref, d1=d1, d2=d2)


@pytest.fixture(scope="module")
def drawn(model):
    """Every scene drawn once by the stage hooks, shared by the tests below; nothing modifies it."""
    return {name: _draw(model, sc) for name, sc in SCENES.items()}


def _render(model, sc, d, background_seed=5, guard=4096):
    """One scene through load_faces + render(wireframe=True) into a random image with a guard region behind it."""
    H, W = sc["H"], sc["W"]
    g = np.random.Generator(np.random.Philox(key=[background_seed, H * W]))
    flat = torch.from_numpy(g.integers(0, 256, H * W * 3 + guard, dtype=np.uint8)).cuda()
    before = flat.cpu().numpy().copy()
    model.load_faces(sc["faces"])
    model.render(flat[:H * W * 3].view(1, H, W, 3), rc.pad_to_smpl(sc["verts"])[None], sc["cam"][None], [COLOUR], [0], M=sc["M"], rgb=False, wireframe=True)
    after = flat.cpu().numpy()
    assert np.array_equal(after[H * W * 3:], before[H * W * 3:]), "the guard region behind the image changed"
    levels = lc.shade_lines(d["q64"], d["n64"], d["xy"][:, 0], d["xy"][:, 1], sc["faces"], d["winner"], COLOUR)
    image, was = after[:H * W * 3].reshape(H, W, 3), before[:H * W * 3].reshape(H, W, 3)
    rc.check_image(image, was, levels)                                     # covered: +-1 level; every other byte as before
    return image, was


# ------------------------------------------------------------------ 1. coverage and the winning edge
@pytest.mark.parametrize("name", sorted(SCENES))
def test_cover(drawn, name):
    rc.check_cover(drawn[name]["winner"], drawn[name]["ref"])


@pytest.mark.parametrize("name", WINNER_SCENES)
def test_winner(drawn, name):
    d = drawn[name]
    rc.check_winner(d["winner"], d["ref"], d["d1"], d["d2"])


def test_line_rules_by_name(drawn):
    """What the scenes are for, read off the DEVICE's pictures."""
    want = np.zeros((48, 64), bool)
    want[7, 5:29] = want[31, 5:29] = want[8:32, 5] = want[8:32, 29] = True
    k = np.arange(24)
    want[31 - k, 5 + k] = True
    square = drawn["square_outline"]["winner"]
    assert want.sum() == 118 and np.array_equal(square >= 0, want)
    inner = want.copy()
    inner[[7, 31], :] = False
    inner[:, [5, 29]] = False
    assert (square[inner] == 2).all()                                      # the shared diagonal: face 0's edge 2 -> 0, not face 1's 0 -> 2
    through = drawn["through_image"]["winner"] >= 0
    assert (through.sum(0) >= 1).all() and through.sum() == 64             # an edge through all 64 columns, both ends far outside: the wave's walk
    assert drawn["triangle_1x1"]["winner"].shape == (1, 1)
    assert set(np.unique(drawn["sub_pixel"]["winner"]) // 3) == {-1, 0}
    assert set(np.unique(drawn["back_facing"]["winner"]) // 3) == {-1, 1} and set(np.unique(drawn["zero_area"]["winner"]) // 3) == {-1, 1}
    assert not (drawn["larger_than_image"]["winner"] >= 0).any()           # nothing is filled: its edges pass outside
    boundary = drawn["on_pixel_boundaries"]["winner"] >= 0
    assert boundary[47 - 10, 10:40].all() and not boundary[47 - 9].any() and not boundary[:, 9].any()
    for name in ("equal_depth", "equal_depth_swapped"):
        sc = SCENES[name]
        masks = [lc.rasterise_lines(drawn[name]["xy"][:, 0], drawn[name]["xy"][:, 1], drawn[name]["z"], sc["faces"][f:f + 1], 48, 64)[0] >= 0 for f in (0, 1)]
        cross = masks[0] & masks[1]
        assert cross.sum() >= 4 and (drawn[name]["winner"][cross] // 3 == 0).all()           # the lower face, whichever triangle carries it
    for name in ("crossing_far", "crossing_near"):
        cut = drawn[name]["winner"] >= 0
        assert cut.any() and not cut[:8].any()                             # the end beyond the plane (the top of the image) is clipped


# ------------------------------------------------------------------ 2. shade and composite
@pytest.mark.parametrize("name", ("triangle_1x1", "triangle_7x5", "triangle_97x61", "fan_16", "through_image", "off_each_side", "crossing_far",
                                  "torus_12x8", "negative_sx_12x8", "torus_320x240", "torus_97x61_side"))
def test_shade_and_composite(model, drawn, name):
    image, was = _render(model, SCENES[name], drawn[name])
    covered = drawn[name]["winner"] >= 0
    assert covered.any() and (image[covered] != was[covered]).any()


# ------------------------------------------------------------------ 3. flags, painter's order, determinism
@pytest.fixture(scope="module")
def crowd(model):
    """5 tori, tilted differently, each drawn ALONE as a wireframe into its own 97 x 61 image: what the multi-mesh call is held against."""
    n, H, W = 5, 61, 97
    verts = np.stack([rc.torus(65, 106, R=0.45, r=0.2, tilt=(0.3 * k, 0.5 + 0.2 * k))[0] for k in range(n)])
    faces = rc.torus(65, 106)[1]
    cams = np.stack([(0.8, 0.8 * W / H, 0.3 * np.cos(k), 0.2 * np.sin(k)) for k in range(n)]).astype(np.float32)
    g = np.random.Generator(np.random.Philox(key=[9, 10]))
    cols = g.uniform(0.2, 1.0, (n, 3)).astype(np.float32)
    back = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    model.load_faces(faces)
    alone, masks = [], []
    for k in range(n):
        img = torch.from_numpy(back[None].copy()).cuda()
        model.render(img, verts[k:k + 1], cams[k:k + 1], cols[k:k + 1], [0], rgb=False, wireframe=True)
        alone.append(img.cpu().numpy()[0])
        xy, z, _ = model.op_raster_setup(verts[k], faces, cams[k], H, W)
        masks.append(model.op_raster_lines(xy, z, faces, H, W).cpu().numpy() >= 0)
    return dict(n=n, H=H, W=W, verts=torch.from_numpy(verts).cuda(), faces=faces, cams=cams, cols=cols, back=back, alone=alone, masks=masks)


def _paint(back, layers):
    out = back.copy()
    for pic, mask in layers:
        out[mask] = pic[mask]
    return out


def test_five_meshes_three_images_equal_one_call_each(model, crowd):
    c = crowd
    model.load_faces(c["faces"])
    mesh, where = [0, 1, 2, 3, 4], [0, 1, 0, 2, 1]                         # images 0 and 1 hold two meshes
    assert (c["masks"][0] & c["masks"][2]).sum() > 20 and (c["masks"][1] & c["masks"][4]).sum() > 20
    runs = []
    for _ in range(2):
        imgs = torch.from_numpy(np.repeat(c["back"][None], 3, 0).copy()).cuda()
        model.render(imgs, c["verts"][mesh], c["cams"][mesh], c["cols"][mesh], where, rgb=False, wireframe=True)
        runs.append(imgs.cpu().numpy())
    assert np.array_equal(runs[0], runs[1])
    # one call per mesh, in the same order, into the same images
    each = torch.from_numpy(np.repeat(c["back"][None], 3, 0).copy()).cuda()
    for m, w in zip(mesh, where):
        model.render(each, c["verts"][m:m + 1], c["cams"][m:m + 1], c["cols"][m:m + 1], [w], rgb=False, wireframe=True)
    assert np.array_equal(runs[0], each.cpu().numpy())
    # and each image is its meshes' own pictures painted over one another through the line masks
    for f in range(3):
        layers = [(c["alone"][m], c["masks"][m]) for m, w in zip(mesh, where) if w == f]
        assert np.array_equal(runs[0][f], _paint(c["back"], layers)), f
    # the other order in image 0 is another picture: later over earlier
    a = _paint(c["back"], [(c["alone"][k], c["masks"][k]) for k in (0, 2)])
    b = _paint(c["back"], [(c["alone"][k], c["masks"][k]) for k in (2, 0)])
    assert not np.array_equal(a, b)


def test_flags_and_refusals(pkg, model, crowd):
    c = crowd
    lib, L = model._lib, pkg._lib
    model.load_faces(c["faces"])
    cams = torch.from_numpy(c["cams"]).cuda()
    col = np.ascontiguousarray(c["cols"])
    idx = np.zeros(c["n"], np.int32)
    H, W = c["H"], c["W"]
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def draw(entry, *flags):
        img = torch.from_numpy(c["back"][None].copy()).cuda()
        rc_ = getattr(lib, entry)(model._h, c["verts"].data_ptr(), 2, cams.data_ptr(), p(col), p(idx), None, img.data_ptr(), 1, H, W, *flags, None)
        torch.cuda.synchronize()
        return rc_, img.cpu().numpy()[0]

    rc0, plain = draw("grnet_render_meshes")
    rc1, ex0 = draw("grnet_render_meshes_ex", 0)
    rc2, wire = draw("grnet_render_meshes_ex", 1)
    assert (rc0, rc1, rc2) == (0, 0, 0)
    assert np.array_equal(plain, ex0) and not np.array_equal(plain, c["back"])                # flags = 0 is grnet_render_meshes
    assert np.array_equal(wire, _paint(c["back"], [(c["alone"][k], c["masks"][k]) for k in (0, 1)])) and not np.array_equal(wire, plain)
    for bad in (2, 3, 1 << 31):
        rc_, img = draw("grnet_render_meshes_ex", bad)
        assert rc_ == L.EINVAL and b"flags" in lib.grnet_last_error(model._h) and np.array_equal(img, c["back"]), bad
    # the hook validates as grnet_op_raster does
    one = np.zeros((1, 3), np.int32)
    out = torch.zeros(64, dtype=torch.int32, device="cuda")
    for V, F in ((0, 1), (3, 0)):
        assert lib.grnet_op_raster_lines(model._h, out.data_ptr(), out.data_ptr(), V, p(one), F, 8, 8, out.data_ptr(), None) == L.EINVAL
        assert b"grnet_op_raster_lines: V and F" in lib.grnet_last_error(model._h)
    assert lib.grnet_op_raster_lines(model._h, out.data_ptr(), out.data_ptr(), 3, p(one), 1, 8, 4097, out.data_ptr(), None) == L.EINVAL
    assert lib.grnet_op_raster_lines(model._h, None, out.data_ptr(), 3, p(one), 1, 8, 8, out.data_ptr(), None) == L.EINVAL
    assert lib.grnet_op_raster_lines(None, out.data_ptr(), out.data_ptr(), 3, p(one), 1, 8, 8, out.data_ptr(), None) == L.EINVAL
    with pytest.raises(L.GrnetError, match="outside"):
        model.op_raster_lines(np.zeros((3, 2), np.int32), np.zeros(3, np.float32), [(0, 1, 3)], 8, 8)
    # a point and a lone vertex pair draw nothing or a line, never a fault: every vertex the same
    assert not (model.op_raster_lines(np.full((3, 2), 1000, np.int32), np.zeros(3, np.float32), [(0, 1, 2)], 8, 8).cpu().numpy() >= 0).any()


# ------------------------------------------------------------------ 4. demo.py
def test_demo_wireframe(pkg, model, tmp_path):
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
    out = demo.main(demo.parser().parse_args(base + ["--output_folder", str(tmp_path / "b"), "--mesh_render", "--wireframe", "--sideview"]))
    res, ref = joblib.load(out), joblib.load(plain)
    assert set(res) == set(ref) == {1, 2}
    for pid in res:                                                                      # the pickle is what it is without the flags
        assert set(res[pid]) == set(ref[pid])
        for k in res[pid]:
            assert np.array_equal(res[pid][k], ref[pid][k]) and res[pid][k].dtype == ref[pid][k].dtype, (pid, k)
    folder = out[:-len(".pkl")] + "_output"
    pngs = sorted(os.listdir(folder))
    assert pngs == [f"{i:06d}.png" for i in range(T)]
    pics = np.stack([np.asarray(Image.open(os.path.join(folder, p))) for p in pngs])
    assert pics.shape == (T, H, 2 * W, 3)
    for i in (28, 29):                                                                   # nobody there: the input, and black beside it
        assert np.array_equal(pics[i, :, :W], frames[i]) and not pics[i, :, W:].any()
    faces = pkg.synth.make_faces()
    for i in (0, 10, 27):
        mask, side = np.zeros((H, W), bool), np.zeros((H, W), bool)
        for pid in res:
            for r in np.nonzero(res[pid]["frame_ids"] == i)[0]:
                for M, m in ((None, mask), (rc.SIDE_M, side)):
                    xy, z, _ = model.op_raster_setup(res[pid]["verts"][r], faces, res[pid]["orig_cam"][r], H, W, M=M)
                    xy, z = xy.cpu().numpy(), z.cpu().numpy()
                    m |= lc.rasterise_lines(xy[:, 0], xy[:, 1], z, faces, H, W)[0] >= 0
        assert mask.sum() > 20 and side.sum() > 20, i
        changed, lit = (pics[i, :, :W] != frames[i]).any(-1), pics[i, :, W:].any(-1)
        assert not (changed & ~mask).any(), i                                            # frames change only inside the line reference's mask
        assert (mask & ~changed).sum() <= 1, i                                           # a line pixel keeps its input with probability 2**-24
        assert np.array_equal(lit, side), i                                              # on black every line pixel is lit (>= 38 levels), no other


# ------------------------------------------------------------------ 5. one production-size frame
def test_one_1080p_frame(model):
    sc = rc.scene_1080p()
    d = _draw(model, sc)
    rc.check_cover(d["winner"], d["ref"])
    rc.check_winner(d["winner"], d["ref"], d["d1"], d["d2"])
    assert (d["winner"] >= 0).sum() > 100000
    filled = model.op_raster(d["xy"], d["z"], sc["faces"], sc["H"], sc["W"]).cpu().numpy() >= 0
    assert (filled & ~(d["winner"] >= 0)).sum() > 100000                  # lines, not the filled overlay
    _render(model, sc, d)
