"""tests/helpers/smpl_checks.py, the float64 yardstick of the SMPL stage and the regressor tail ("The bound of the SMPL stage"), checked without a GPU:

- the fp32 oracle (oracle.smpl_lbs, smpl_joints29, project: an independent fp32 implementation) stays within 1.5 roundings of the
  element's magnitude on every input of tests/test_gpu_smpl.py that uses the SMPL tree -- the measurement the accepted ratio rests on;
- the reference follows tables["parents"]: with a chain and with a star as the tree it equals a brute-force product of 4x4 matrices per joint;
- ten planted faults, each applied to the reference's own output rounded to fp32, are all flagged by the per-element check -- and the bar the
  stage had before (max |a - b| / max |b| < 1e-4 per tensor) lets some of them through: PLANTED_FAULTS records which;
- oracle.float64() reaches smpl_lbs, smpl_joints29, project and rot6d_to_rotmat, and outside it their fp32 results are bit for bit what they
  were (tests/golden/oracle_smpl_f32.npz: a copy of their outputs from before the switch existed)."""
import os

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import smpl_checks as sc

ORACLE_MAX_RATIO = 1.5


@pytest.fixture(scope="module")
def tables(synth_smpl):
    t = {"standard": sc.standard_table(synth_smpl)}
    t.update({kind: sc.variant_table(synth_smpl, kind) for kind in sc.VARIANTS})
    return t


@pytest.fixture(scope="module")
def cases(tables):
    c = {"standard": sc.make_case(tables["standard"], sc.STANDARD_FRAMES, sc.STANDARD_SEED)}
    c.update({kind: sc.make_case(tables[kind], sc.VARIANT_FRAMES, sc.VARIANT_SEED) for kind in sc.VARIANTS})
    return c


def test_tables_and_inputs_are_what_the_recipes_state(tables, cases, synth_smpl):
    std = tables["standard"]
    moved = np.flatnonzero((std["v_template"] != synth_smpl["v_template"]).any(1))
    assert set(sc.HAND_VERTS + sc.LAST_VERTS) <= set(moved.tolist()) and len(moved) <= 29
    for k in synth_smpl:
        if k != "v_template":
            assert np.array_equal(std[k], synth_smpl[k]), k
    nz = (tables["dense_skin"]["lbs_weights"] != 0).sum(1)
    assert nz.max() == 24 and nz.min() == 1 and (nz == 1).sum() >= 8 and set(range(1, 25)) == set(nz.tolist())
    assert np.allclose(tables["dense_skin"]["lbs_weights"].sum(1), 1.0, atol=1e-6)
    assert [int((tables[k]["J_regressor_extra"][5] != 0).sum()) for k in ("thorax700", "thorax1", "thorax0")] == [700, 1, 0]
    assert tables["chain"]["parents"].tolist() == list(range(-1, 23)) and tables["star"]["parents"].tolist() == [-1] + [0] * 23
    c = cases["standard"]
    R = c["rotmat"].astype(np.float64)
    err = np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3)).max((-1, -2))                       # (129, 24): distance from a rotation
    assert (err[[127, 126]] > 0.5).any(1).all() and (np.delete(err, [126, 127], 0) < 1e-6).all()
    assert (R[127] == 0).all((-1, -2)).sum() == 8
    ident = (R == np.eye(3)).all((-1, -2))
    half_turn = np.isclose(np.trace(R, axis1=-2, axis2=-1), -1.0, atol=1e-6) & (err < 1e-6)
    assert ident.sum() > 300 and half_turn.sum() > 600                                       # exactly pi and pi - 1e-3
    assert set(np.unique(c["cam"][:, 0]).tolist()) == set(np.float32(sc.SCALES).tolist())
    assert (c["betas"][0] == 0).all() and (c["betas"][1] == 5).all() and (c["betas"][2] == -5).all()


def test_fp32_oracle_is_within_a_rounding_and_a_half_of_the_reference(oracle, tables, cases):
    """Every SMPL-tree input of the GPU tests; the call sizes of the standard table one by one, as the GPU test takes its bar from them."""
    for kind in ("standard", "dense_skin", "thorax700", "thorax1", "thorax0"):
        got = sc.fp32_oracle(oracle, cases[kind], tables[kind])
        sizes = (1, 15, 16, 17, 33, 48, 49, 63, 64, 65, 80, 129) if kind == "standard" else (1, 5, 17)
        for m in sizes:
            f = sc.frames(cases[kind], m)
            r = sc.ratios({k: v[f] for k, v in got.items()}, cases[kind]["ref"], cases[kind]["mag"], f)
            if m == sizes[-1]:
                print(kind, m, {k: (round(v, 3), i) for k, (v, i) in r.items()})
            assert all(v <= ORACLE_MAX_RATIO for v, _ in r.values()), (kind, m, r)
    assert (sc.fp32_oracle(oracle, cases["thorax0"], tables["thorax0"])["kp_3d"][:, 28] == 0).all()
    assert (cases["thorax0"]["ref"]["kp_3d"][:, 28] == 0).all() and (cases["thorax0"]["mag"]["kp_3d"][:, 28] == 0).all()


def test_oracle_float64_mode_reaches_the_smpl_functions(oracle, tables, cases):
    """Under oracle.float64() the oracle is a second float64 statement of the stage (per-frame, per-joint loops against the helper's batched
    form): the two agree to 1e-6 of a rounding of fp32, on the SMPL tree, the chain and the star (smpl_lbs reads smpl["parents"])."""
    for kind in ("dense_skin", "thorax700", "chain", "star"):
        with oracle.float64():
            got = sc.fp32_oracle(oracle, cases[kind], tables[kind], dtype=np.float64)
        assert all(v.dtype == np.float64 for v in got.values())
        r = sc.ratios(got, cases[kind]["ref"], cases[kind]["mag"])
        assert all(v < 1e-6 for v, _ in r.values()), (kind, r)


def test_fp32_oracle_is_bit_for_bit_what_it_was(oracle, synth_smpl):
    g = np.load(os.path.join(ROOT, "tests", "golden", "oracle_smpl_f32.npz"))
    R = oracle.rot6d_to_rotmat(g["rot6d"])
    verts, j24 = oracle.smpl_lbs(g["betas"], R.reshape(-1, 24, 3, 3), synth_smpl)
    no_parents = {k: v for k, v in synth_smpl.items() if k != "parents"}                      # real-model files carry none: the SMPL tree
    verts2, j24b = oracle.smpl_lbs(g["betas"], R.reshape(-1, 24, 3, 3), no_parents)
    kp3d = oracle.smpl_joints29(verts, j24, synth_smpl)
    kp2d = oracle.project(kp3d, g["cam"])
    for name, a in (("rotmat", R), ("verts", verts), ("joints24", j24), ("kp_3d", kp3d), ("kp_2d", kp2d)):
        assert a.dtype == np.float32 and a.tobytes() == g[name].tobytes(), name
    assert verts2.tobytes() == verts.tobytes() and j24b.tobytes() == j24.tobytes()
    with oracle.float64():
        R64 = oracle.rot6d_to_rotmat(g["rot6d"])
    assert R64.dtype == np.float64 and np.abs(R64 - sc.gram_schmidt(g["rot6d"].reshape(-1, 6))[0]).max() < 1e-14


@pytest.mark.parametrize("kind", ["chain", "star", "standard"])
def test_reference_follows_the_parent_table(tables, cases, kind):
    """The posed joints and the vertices from 4x4 homogeneous matrices multiplied down each joint's own path to the root, joint by joint and
    vertex by vertex -- no level loop, no shared partial products."""
    t, c = tables[kind], cases[kind]
    n = 5
    f = sc.frames(c, n)
    betas, R = sc.widen(c["betas"][f]), sc.widen(c["rotmat"][f])
    v_shaped, J = sc.shape_stage(betas, t)
    v_posed = sc.pose_blend(v_shaped, sc.pose_feature(R), t)
    parents = [int(p) for p in t["parents"]]
    W = sc.widen(t["lbs_weights"])
    some = list(sc.HAND_VERTS) + [0, 1, 6868, 6869, 6889] + list(range(100, 6890, 97))
    worst = 0.0
    for i in range(n):
        G = []
        for j in range(24):
            path = [j]
            while parents[path[-1]] >= 0:
                path.append(parents[path[-1]])
            M = np.eye(4)
            for k in reversed(path):                                        # root first
                T = np.eye(4)
                T[:3, :3] = R[i, k]
                T[:3, 3] = J[i, k] - (J[i, parents[k]] if parents[k] >= 0 else 0.0)
                M = M @ T
            G.append(M)
            worst = max(worst, np.abs(M[:3, 3] - c["ref"]["joints24"][f][i, j]).max())
        for v in some:
            x = np.zeros(3)
            for j in range(24):
                if W[v, j] != 0:
                    x += W[v, j] * (G[j] @ np.append(v_posed[i, v] - J[i, j], 1.0))[:3]
            worst = max(worst, np.abs(x - c["ref"]["verts"][f][i, v]).max() / max(1.0, np.abs(x).max()))
    print(kind, "worst difference from the brute-force product", worst)
    assert worst < 1e-12
    depth = lambda j: 0 if parents[j] < 0 else 1 + depth(parents[j])
    assert max(map(depth, range(24))) == {"chain": 23, "star": 1, "standard": 8}[kind]


# --------------------------------------------------------------------------------------------------------------- planted faults
def _run(case, table, m, feat_edit=None, vposed_edit=None, skip_level=None, kp3d_edit=None, cam=None, weights=None, extra=None, posedirs=None):
    """The stages of the reference on the last m frames of the case with a fault planted between them; outputs rounded to fp32."""
    f = sc.frames(case, m)
    t = dict(table)
    if posedirs is not None:
        t["posedirs"] = posedirs
    if extra is not None:
        t["J_regressor_extra"] = extra
    betas, R = case["betas"][f], case["rotmat"][f]
    v_shaped, J = sc.shape_stage(betas, t)
    feat = sc.pose_feature(R)
    if feat_edit:
        feat_edit(feat)
    v_posed = sc.pose_blend(v_shaped, feat, t)
    if vposed_edit:
        vposed_edit(v_posed.reshape(m, -1))
    GR, Gt = sc.chain(R, J, t["parents"], skip_level=skip_level)
    verts = sc.skin(v_posed, GR, Gt, J, t["lbs_weights"] if weights is None else weights)
    kp3d = sc.joints29(verts, Gt, t)
    if kp3d_edit:
        kp3d_edit(kp3d, verts)
    kp2d = sc.project(kp3d, case["cam"][f] if cam is None else cam)
    return {k: a.astype(np.float32) for k, a in (("verts", verts), ("joints24", Gt), ("kp_3d", kp3d), ("kp_2d", kp2d))}


def _verdict(got, case, m, bar):
    """(flagged by the per-element check, flagged by the bar of before, worst ratio / accepted ratio, worst rel_err)"""
    f = sc.frames(case, m)
    r = sc.ratios(got, case["ref"], case["mag"], f)
    old = max(sc.rel_err(got[k], case["ref"][k][f]) for k in ("verts", "kp_3d", "kp_2d"))     # the three tensors the stage was checked on
    new = max(r[k][0] / bar[k] for k in r)
    return new > 1.0, not old < sc.OLD_BAR, new, old


# name -> does the bar of before (rel_err < 1e-4 on verts, kp_3d, kp_2d) flag it?  Measured by test_planted_faults, which asserts this table.
PLANTED_FAULTS = {
    "1 rows r and r+8 of a 16-row tile exchanged in one 64-column block": True,
    "2 the last 62 columns taken from column 0": True,
    "3 the 4th skinning weight dropped where it is below 1e-3": False,             # trace weights of 1e-6 .. 1e-4: at most 0.3 mm on a vertex
    "4 thorax entries beyond the first 256 dropped": True,
    "5 one hand vertex taken from its neighbour index": True,
    "6 pose feature of joint 23 with R instead of R - I on the diagonal": True,
    "7 posedirs rounded to bf16": True,
    "7 posedirs rounded to bf16, poses of at most 0.3 rad": False,               # the pose a walking person gives: |R - I| <= 0.3
    "8 the feat row of a 129-frame call left for frame 0 of a 1-frame call": True,
    "9 kp_2d with tz of the neighbouring frame, every frame": True,
    "9 kp_2d with tz of the neighbouring frame, the frame of scale 1e-6": False,   # its kp_2d is 1e-6 of the tensor's scale
    "10 one level of the chain tree skipped": True,
}


def test_planted_faults(oracle, tables, cases):
    """Each fault against the accepted ratio of its case (4 x the fp32 oracle's, at least 4; the chain takes the standard table's) and against
    the bar of before.  Every one must fail the per-element check; at least three must have passed the bar of before."""
    std, tstd = cases["standard"], tables["standard"]
    m = 17
    bar = {}
    for kind in ("standard", "dense_skin", "thorax700"):
        f = sc.frames(cases[kind], m)
        got = sc.fp32_oracle(oracle, cases[kind], tables[kind])
        bar[kind] = sc.bars(sc.ratios({k: v[f] for k, v in got.items()}, cases[kind]["ref"], cases[kind]["mag"], f))
        assert all(4.0 <= b <= 4 * ORACLE_MAX_RATIO for b in bar[kind].values())
    assert _verdict(_run(std, tstd, m), std, m, bar["standard"])[:2] == (False, False)           # the reference rounded to fp32 passes both
    seen = {}

    def plant(name, got, case, bar):
        seen[name] = _verdict(got, case, m if len(got["verts"]) == m else len(got["verts"]), bar)

    def mild_bar(case, table):
        r = sc.ratios(sc.fp32_oracle(oracle, case, table), case["ref"], case["mag"])
        assert all(v <= ORACLE_MAX_RATIO for v, _ in r.values()), r
        return sc.bars(r)

    names = iter(PLANTED_FAULTS)

    def swap(vp):
        vp[[3, 11], 6400:6464] = vp[[11, 3], 6400:6464]
    plant(next(names), _run(std, tstd, m, vposed_edit=swap), std, bar["standard"])

    def column0(vp):
        vp[:, 322 * 64:] = vp[:, :1]
    plant(next(names), _run(std, tstd, m, vposed_edit=column0), std, bar["standard"])

    W = tables["dense_skin"]["lbs_weights"].copy()
    fourth = np.sort(W, 1)[:, -4]
    hit = (fourth > 0) & (fourth < 1e-3)
    assert hit.sum() > 100
    W[hit[:, None] & (W == fourth[:, None])] = 0
    plant(next(names), _run(cases["dense_skin"], tables["dense_skin"], m, weights=W), cases["dense_skin"], bar["dense_skin"])

    extra = tables["thorax700"]["J_regressor_extra"].copy()
    extra[5, np.flatnonzero(extra[5])[256:]] = 0
    plant(next(names), _run(cases["thorax700"], tables["thorax700"], m, extra=extra), cases["thorax700"], bar["thorax700"])

    def neighbour(kp3d, verts):
        kp3d[:, 24] = verts[:, sc.HAND_VERTS[0] + 1]
    plant(next(names), _run(std, tstd, m, kp3d_edit=neighbour), std, bar["standard"])

    def diagonal(feat):
        feat[:, [22 * 9, 22 * 9 + 4, 22 * 9 + 8]] += 1.0
    plant(next(names), _run(std, tstd, m, feat_edit=diagonal), std, bar["standard"])

    bf16 = sc.round_bf16(tstd["posedirs"])
    assert 0 < np.abs(bf16 - tstd["posedirs"]).max() <= 2.0 ** -8 * np.abs(tstd["posedirs"]).max()
    plant(next(names), _run(std, tstd, m, posedirs=bf16), std, bar["standard"])
    mild = sc.make_case(tstd, m, sc.STANDARD_SEED, poses=sc.make_mild_poses)
    plant(next(names), _run(mild, tstd, m, posedirs=bf16), mild, mild_bar(mild, tstd))

    other = sc.pose_feature(sc.make_poses(sc.STANDARD_FRAMES, sc.OTHER_SEED)[1])[0]

    def stale(feat):
        feat[0] = other
    plant(next(names), _run(std, tstd, 1, feat_edit=stale), std, bar["standard"])

    f = sc.frames(std, m)
    cam = std["cam"][f].copy()
    cam[:, 0] = np.roll(cam[:, 0], -1)
    plant(next(names), _run(std, tstd, m, cam=cam), std, bar["standard"])
    cam = std["cam"][f].copy()
    tiny = int(np.flatnonzero(cam[:, 0] == np.float32(1e-6))[0])
    assert cam[tiny + 1, 0] == 0.0
    cam[tiny, 0] = cam[tiny + 1, 0]
    plant(next(names), _run(std, tstd, m, cam=cam), std, bar["standard"])

    plant(next(names), _run(cases["chain"], tables["chain"], m, skip_level=23), cases["chain"], bar["standard"])

    for name, (new, old, worst_new, worst_old) in seen.items():
        print(f"{name:80s} per-element {worst_new:10.3g} x accepted  {'FLAGGED' if new else 'passes '}   rel_err {worst_old:8.2g}  "
              f"{'flagged' if old else 'PASSES the bar of before'}")
    assert all(new for new, *_ in seen.values()), [k for k, v in seen.items() if not v[0]]
    assert {k: v[1] for k, v in seen.items()} == PLANTED_FAULTS
    assert sum(1 for new, old, *_ in seen.values() if new and not old) >= 3


# --------------------------------------------------------------------------------------------------------------- the check itself, the tail
def test_ratio_excludes_nothing():
    ref = np.array([[1.0, 0.0], [-2.0, 3.0]])
    mag = np.array([[1.0, 0.0], [8.0, 3.0]])
    assert sc.ratio(ref, ref, mag) == (0.0, (0, 0))
    got = ref.copy()
    got[1, 0] += 8 * sc.EPS * 2.5
    assert sc.ratio(got, ref, mag) == (2.5, (1, 0))
    got[0, 1] = 1e-30                                                     # magnitude 0: every term is 0, the element must be exactly 0
    assert sc.ratio(got, ref, mag) == (np.inf, (0, 1))
    got[0, 1], got[1, 1] = 0.0, np.nan
    assert sc.ratio(got, ref, mag) == (np.inf, (1, 1))
    assert sc.bars({"a": (0.9, (0,)), "b": (1.3, (0,)), "c": 0.0}) == {"a": 4.0, "b": 5.2, "c": 4.0}


def test_magnitude_of_the_quotient():
    """kp_2d's magnitude bounds what perturbing X by mag X and Z by mag Z (2^-24 each, the worst signs) does to X / Z, to first order."""
    g = np.random.default_rng(3)
    kp3d, mag3d = g.standard_normal((5, 29, 3)), np.abs(g.standard_normal((5, 29, 3))) + 1.0
    cam = sc.make_cameras(5, 3)
    out, mag = sc.project(kp3d, cam, mag3d)
    t = np.abs(sc.camera_translation(cam))[:, None]
    e = 1e-9
    for sx in (-1, 1):
        for sz in (-1, 1):
            moved = sc.project(kp3d + e * np.stack([sx * (mag3d + t)[..., 0], sx * (mag3d + t)[..., 1], sz * (mag3d + t)[..., 2]], -1), cam)
            assert (np.abs(moved - out) <= e * mag * (1 + 1e-6) + 1e-300).all()
    assert sc.ratio(out, out, mag)[0] == 0.0


def test_tail_reference_against_the_fp32_oracle(oracle, synth_weights):
    plf, csf = sc.make_features(17, sc.STANDARD_SEED)
    assert len({plf[i].tobytes() for i in range(17)}) == 17 and (plf > 0).any() and (plf < 0).any()
    a = np.abs(plf[plf != 0])
    assert np.quantile(a, 0.99) / np.quantile(a, 0.01) > 1e3
    ref, mag = sc.tail_reference(plf, csf, synth_weights)
    rot6d, shape, cam = oracle.head_tail(plf, csf, synth_weights)
    assert rot6d.dtype == np.float32
    r = sc.ratios({"pred_rot6d": rot6d, "shape": shape, "cam": cam}, ref, mag)
    print({k: (round(v, 3), i) for k, (v, i) in r.items()})
    # sums of 128 and of 1537 terms, added in whatever order numpy's einsum and matmul choose: within sqrt(terms) roundings of the magnitude
    assert r["pred_rot6d"][0] <= 128 ** 0.5 and r["shape"][0] <= 1537 ** 0.5 and r["cam"][0] <= 1537 ** 0.5, r
    with oracle.float64():
        rot6d, shape, cam = oracle.head_tail(plf, csf, synth_weights)
    r = sc.ratios({"pred_rot6d": rot6d, "shape": shape, "cam": cam}, ref, mag)
    assert all(v < 1e-6 for v, _ in r.values()), r
    # the seed of the features: the fp32 oracle's own axis-angle of its own rotations stays within the rule at the discontinuity at pi
    R = oracle.rot6d_to_rotmat(oracle.head_tail(plf, csf, synth_weights)[0])
    fell_back, worst, geo = sc.axis_angle_check(oracle.rotmat_to_aa(R), R)
    print("fp32 oracle on the tail's features:", fell_back, "rows at the discontinuity, worst element", worst, "worst geodesic", geo)
    assert fell_back <= sc.AA_MAX_FALLBACK and geo < sc.AA_GEODESIC_TOL
    bad = {"pred_rot6d": ref["pred_rot6d"].copy(), "shape": ref["shape"], "cam": ref["cam"]}
    bad["pred_rot6d"][3, 5, 2] = ref["pred_rot6d"][3, 5, 2] + 10 * sc.EPS * mag["pred_rot6d"][3, 5, 2]
    assert sc.ratios(bad, ref, mag)["pred_rot6d"] == (pytest.approx(10.0), (3, 5, 2))


def test_rotation_helpers(oracle):
    g = np.random.default_rng(5)
    x = g.standard_normal((400, 6)).astype(np.float32)
    x[:20, 1::2] = x[:20, 0::2] * 3 + 1e-3 * x[:20, 1::2]                 # a2 nearly parallel to a1: |u| << |a2|
    R, kappa = sc.gram_schmidt(x)
    assert (np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max((1, 2)) < 1e-15 * kappa[:, 0, 0]).all() and np.allclose(np.linalg.det(R), 1.0)
    assert kappa[:20].min() > 1e3 and kappa[20:].min() >= 2.0
    r32 = sc.ratio(oracle.rot6d_to_rotmat(x), R, kappa)
    print("fp32 Gram-Schmidt against float64, in roundings of the row's magnitude:", r32)
    assert r32[0] <= 4.0
    # axis-angle: every angle from 0 to pi, exactly 0 and exactly pi included, returns the rotation it was given
    axis = g.standard_normal((300, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = np.concatenate([[0.0, 1e-9, 1e-4, np.pi - 1e-3, np.pi - 1e-7, np.pi], g.uniform(0, np.pi, 294)])
    Rm = sc.rotvec_matrix(axis * angle[:, None])
    assert sc.geodesic(Rm, sc.rotvec_matrix(sc.axis_angle(Rm.astype(np.float32)))).max() < 1e-6
    assert np.abs(np.linalg.norm(sc.axis_angle(Rm.astype(np.float32)), axis=1) - angle).max() < 2e-3     # fp32 matrices near pi: sqrt(2^-24)
    aa32 = oracle.rotmat_to_aa(Rm.astype(np.float32))
    fell_back, worst, geo = sc.axis_angle_check(aa32, Rm.astype(np.float32))
    print("fp32 oracle axis-angle:", fell_back, "rows at the discontinuity, worst element", worst, "worst geodesic", geo)
    assert worst < sc.AA_TOL and geo < sc.AA_GEODESIC_TOL
    wrong = aa32.copy()
    wrong[10] *= 1.01
    assert sc.axis_angle_check(wrong, Rm.astype(np.float32))[2] > sc.AA_GEODESIC_TOL
