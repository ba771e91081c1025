"""A compact-arena handle (grnet_create_ex + GRNET_CREATE_COMPACT_ARENA: tensors whose lifetimes cannot overlap share memory) against a default handle
with the same weights and frames: every output equal BY BITS, for every call size, launch form and schedule; nothing leaks between tenants or
between forwards; grnet_debug_tensor serves exactly the tensors nothing is placed over.  The layout's safety proof is tests/test_arena_cpu.py."""
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

OUTPUTS = ("theta", "verts", "kp_2d", "kp_3d", "rotmat", "point_local_feat", "cam_shape_feats", "pred_rot6d", "features", "part_attn", "smpl_feats")
EXTRAS = OUTPUTS[5:]
FILL = struct.unpack("<I", struct.pack("<f", 1e30))[0]          # finite on purpose: a zero-weighted pad lane still contributes exactly 0
ALL_GROUPS = 1023                                               # GRNET_OPT_BF16_CHAIN: every kernel group


def _frames(pkg, n, start=0):
    """n distinct frames: the 8 seed-defined frames from `start`, tiled, each copy scaled by its own factor."""
    base = torch.from_numpy(pkg.synth.make_frames(8, start=start)).cuda()
    idx = torch.arange(n, device="cuda")
    return (base[idx % 8] * (1.0 + 0.001 * (idx // 8).float()).reshape(n, 1, 1, 1)).contiguous()


_PAIRS = {}


def _pair(pkg, dtype, max_frames):
    """(full handle, compact handle) with the same synthetic weights; kept for the module (the 400-frame full arena is 41 GB: one at a time)."""
    key = (dtype, max_frames)
    if key not in _PAIRS:
        for k in [k for k in _PAIRS if k[1] >= 400 or max_frames >= 400]:
            for m in _PAIRS.pop(k):
                m.close()
        _PAIRS[key] = tuple(pkg.build_synthetic_model(max_frames=max_frames, with_gru=False, dtype=dtype, compact_arena=c) for c in (False, True))
        assert [m.compact_arena for m in _PAIRS[key]] == [False, True]
    return _PAIRS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_pairs():
    yield
    for pair in _PAIRS.values():
        for m in pair:
            m.close()
    _PAIRS.clear()


def _forward(m, x, repeats=1):
    out = None
    for _ in range(repeats):                                      # GRNET_OPT_USE_GRAPH: the first call of a size runs eagerly, the second captures, the third replays
        out = m(x, extras=EXTRAS)[-1]
    torch.cuda.synchronize()
    return {k: out[k] for k in OUTPUTS}


def _assert_same_bits(a, b, what):
    for k in OUTPUTS:
        assert a[k].shape == b[k].shape and torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{what}: {k} differs by bits"
        assert torch.isfinite(a[k]).all(), f"{what}: {k} is not finite"


def _set(pkg, models, graph=0, multi_lane=1, min_frames=0):
    L = pkg._lib
    for m in models:
        m.set_option(L.OPT_USE_GRAPH, graph)
        m.set_option(L.OPT_MULTI_LANE, multi_lane)
        if m.dtype == "bf16":
            m.set_option(L.OPT_BF16_CHAIN, ALL_GROUPS)
            m.set_option(L.OPT_BF16_MIN_FRAMES, min_frames)


# ---------------------------------------------------------------------------------------------------- 5. bit identity
@pytest.mark.parametrize("graph,multi_lane", [(0, 1), (1, 1), (0, 0), (1, 0)])
@pytest.mark.parametrize("max_frames,n", [(64, 1), (64, 16), (64, 50), (400, 400)])
def test_f32_outputs_are_bit_identical(pkg, max_frames, n, graph, multi_lane):
    full, comp = _pair(pkg, "f32", max_frames)
    _set(pkg, (full, comp), graph, multi_lane)
    x = _frames(pkg, n)
    _assert_same_bits(_forward(comp, x, 3 if graph else 1), _forward(full, x, 3 if graph else 1), f"f32 n={n} graph={graph} multi_lane={multi_lane}")
    assert comp.num_kernel_launches() == full.num_kernel_launches() and comp.num_conv_launches() == full.num_conv_launches()


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("n,min_frames", [(4, 0), (64, 0), (65, 0), (256, 0), (4, 1)])
def test_bf16_outputs_are_bit_identical(pkg, n, min_frames, graph):
    full, comp = _pair(pkg, "bf16", 256)
    _set(pkg, (full, comp), graph, 1, min_frames)
    x = _frames(pkg, n)
    _assert_same_bits(_forward(comp, x, 3 if graph else 1), _forward(full, x, 3 if graph else 1), f"bf16 n={n} min_frames={min_frames} graph={graph}")
    assert comp.num_kernel_launches() == full.num_kernel_launches() and comp.num_conv_launches() == full.num_conv_launches()
    assert comp.conv_kernels(n) == full.conv_kernels(n)
    if n >= 64 or min_frames:
        assert any("chain" in str(k) for k in comp.conv_kernels(n)), "the grouped launches did not run"


# ---------------------------------------------------------------------------------------------------- 6. nothing leaks
@pytest.mark.parametrize("dtype,max_frames,n,min_frames", [("f32", 64, 16, 0), ("f32", 64, 50, 0), ("bf16", 256, 64, 0), ("bf16", 256, 4, 1), ("bf16", 256, 4, 0)])
def test_no_leak_between_tenants_or_forwards(pkg, dtype, max_frames, n, min_frames):
    _, comp = _pair(pkg, dtype, max_frames)
    _set(pkg, (comp,), 0, 1, min_frames)
    a, b = _frames(pkg, n), _frames(pkg, n, start=8)
    plain = _forward(comp, a)
    comp.arena_fill(FILL)
    _assert_same_bits(_forward(comp, a), plain, f"{dtype} n={n}: forward over an arena filled with 1e30")
    other = _forward(comp, b)
    assert not torch.equal(other["theta"], plain["theta"])
    _assert_same_bits(_forward(comp, a), plain, f"{dtype} n={n}: A after B")


# ---------------------------------------------------------------------------------------------------- 7. any schedule
def test_tuned_table_from_a_full_handle(pkg):
    full, comp = _pair(pkg, "f32", 64)
    _set(pkg, (full, comp), 0, 1)
    full.tune(16, level=1)
    import ctypes as C
    buf = C.create_string_buffer(1 << 16)
    assert full._lib.grnet_get_tuning(full._h, 16, buf, len(buf)) > 0
    assert comp._lib.grnet_set_tuning(comp._h, 16, buf.value) == 0
    x = _frames(pkg, 16)
    _assert_same_bits(_forward(comp, x), _forward(full, x), "f32 n=16 under the table tuned on the full handle")
    assert comp.num_kernel_launches() == full.num_kernel_launches() and comp.num_conv_launches() == full.num_conv_launches()
    assert comp.conv_launch_forms(16) == full.conv_launch_forms(16)


# ---------------------------------------------------------------------------------------------------- 8. grnet_debug_tensor
def _names(dtype):
    names = ["stem_conv1", "stem_conv2", "layer1", "transition1.0", "transition1.1", "transition2.2", "transition3.3"]
    names += [f"layer1.{k}{s}" for k in range(4) for s in ("", ".conv1", ".conv2")]
    for stage, mods, nb in (("stage2", 1, 2), ("stage3", 4, 3), ("stage4", 3, 4)):
        for m in range(mods):
            names += [f"{stage}.{m}.x{b}" for b in range(nb)] + [f"{stage}.{m}.y{b}" for b in range(nb)]
    for idx, layers in ((2, 1), (3, 2), (4, 3)):
        names += [f"up{idx}.{l}.{k}" for l in range(layers) for k in ("bilinear", "conv")]
    return names + ["cat", "head.first", "head.part_feats", "head.heat", "head.smpl_feats", "head.cam_shape"]


@pytest.mark.parametrize("dtype,max_frames,n", [("f32", 64, 16), ("bf16", 256, 16)])
def test_debug_tensor_serves_final_tenants_only(pkg, dtype, max_frames, n):
    full, comp = _pair(pkg, dtype, max_frames)
    _set(pkg, (full, comp), 0, 1)
    x = _frames(pkg, n)
    _forward(full, x)
    _forward(comp, x)
    served, refused = [], []
    for name in _names(dtype):
        want = full.debug_tensor(name, n)
        try:
            got = comp.debug_tensor(name, n)
        except pkg._lib.GrnetError as e:
            assert "code -1" in str(e) and "compact" in str(e) and "GRNET_CREATE_COMPACT_ARENA" in str(e), str(e)      # GRNET_ESTATE, and what to do about it
            refused.append(name)
            continue
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), name
        served.append(name)
    # the concat buffer and its four writers, and the head's maps the pooling reads, are under nothing
    must = ["cat", "stage4.2.y0", "up2.0.conv", "up3.1.conv", "up4.2.conv", "head.heat", "head.smpl_feats", "head.cam_shape"]
    assert not [m for m in must if m not in served], (served, refused)
    # the big early tensors are what the memory is saved on
    assert all(f"layer1.{k}{s}" in refused for k in range(4) for s in (".conv1", ".conv2")), refused
    assert "stem_conv1" in refused and "transition1.0" in refused
    assert len(refused) > len(served)


# ---------------------------------------------------------------------------------------------------- 9. grnet_arena_info
@pytest.mark.parametrize("dtype,max_frames", [("f32", 64), ("bf16", 256)])
def test_arena_info_equals_the_query(pkg, dtype, max_frames):
    full, comp = _pair(pkg, dtype, max_frames)
    assert full.arena_info() == pkg.arena_query(dtype, max_frames, compact=False)
    assert comp.arena_info() == pkg.arena_query(dtype, max_frames, compact=True)
    assert comp.arena_info()["bytes"] < full.arena_info()["bytes"] == full.arena_info()["full_bytes"] == comp.arena_info()["full_bytes"]
    assert full.arena_info()["shared_tensors"] == 0 < comp.arena_info()["shared_tensors"]


# ---------------------------------------------------------------------------------------------------- 10. the rest of the library
def test_temporal_branch_and_smpl_do_not_depend_on_the_arena(pkg):
    t = 16
    x = _frames(pkg, t).reshape(1, t, 3, 224, 224)
    bbox, cimg = pkg.synth.make_gait_boxes(1, t)
    bbox, cimg = torch.from_numpy(bbox).cuda(), torch.from_numpy(cimg).cuda()
    W = torch.from_numpy(pkg.synth.make_joint_regressor(17, nnz=None, signed=True, seed=5))
    got = []
    for compact in (False, True):
        m = pkg.build_synthetic_model(max_frames=t, use_gait_feat=True, compact_arena=compact)
        try:
            first = m(x, bbox=bbox, cimg=cimg)[-1]                                   # forward + gait_correct (grnet.py:154-173)
            torch.cuda.synchronize()
            betas, rotmat, cam = first["theta"].reshape(t, 85)[:, 75:].contiguous(), first["rotmat"].reshape(t, 24, 3, 3), first["theta"].reshape(t, 85)[:, :3].contiguous()
            verts, kp3d, kp2d = m.smpl_forward(betas, rotmat, cam)
            m.set_joint_regressor(W)
            joints = m.regress_joints(verts)
            torch.cuda.synchronize()
            got.append({**{k: first[k] for k in ("theta", "verts", "kp_2d", "kp_3d", "rotmat", "pred_avg", "pred_phase", "pred_cparam", "point_local_feat")},
                        "smpl.verts": verts, "smpl.kp3d": kp3d, "smpl.kp2d": kp2d, "joints": joints})
        finally:
            m.close()
    for k in got[0]:
        assert torch.equal(got[0][k].view(torch.int32), got[1][k].view(torch.int32)), k
