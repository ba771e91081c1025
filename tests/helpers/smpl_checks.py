"""The yardstick of the SMPL stage and of the regressor tail ("The bound of the SMPL stage"): plain numpy float64, written from the published algorithm (SMPL: shape
blend shapes, joint regression, pose blend shapes on R - I, the kinematic chain, linear blend skinning; the wrapper's 29 joints; the
weak-perspective camera turned into a translation and projected) -- it imports nothing from the package and nothing from the oracle.

Every stage exists twice: as the computation, and (mag=True) as its MAGNITUDE: every operand replaced by its absolute value and every
subtraction by an addition (the R - I of the pose feature, J_i - J_parent, t - G.J).  The magnitude of an element is the sum of the absolute
values of all the terms that make it up, so 2^-24 x magnitude is one fp32 rounding of the largest partial sum a summation order can meet:
the unit in which the error of ANY fp32 evaluation of that element is a small number, whatever cancels in it.

smpl_reference / smpl_magnitude    verts, the 24 posed joints, kp_3d (29), kp_2d of a call; inputs are the fp32 values the GPU was given, widened
ratio(got, ref, mag)               max |got - ref| / (2^-24 mag) and where; an element of magnitude 0 must be exactly the reference's
bars(oracle_ratios)                what a test accepts: 4 x the ratio an independent fp32 implementation reaches on the same inputs, never below 4
tail_reference                     the per-joint 128 -> 6 products and the two 1536-wide linears of the regressor tail, with magnitudes
gram_schmidt / axis_angle          float64 rot6d -> rotation matrix (with the conditioning of each row) and rotation matrix -> axis-angle
standard_table / variant_table     seeded SMPL tables: the synthetic model's with the hand vertices and the last 21 vertices moved far from their
                                   index neighbours; dense skinning weights; thorax rows of 700 / 1 / 0 entries; a chain and a star as the tree
make_poses / make_cameras          the seeded poses (identity, 1e-4 rad, uniform, pi - 1e-3, exactly pi; two frames that are no rotations) and cameras
make_case / frames / fp32_oracle   the inputs of a table with reference and magnitudes, computed once; the frames a call of m is given; the yardstick
make_features / make_mild_poses    lognormal pooled features for the tail; poses of at most 0.3 rad (the planted faults of tests/test_smpl_checks_cpu.py)
"""
import numpy as np

EPS = 2.0 ** -24
FACTOR = 4.0                                   # summation order: an MFMA chain adds 220 terms one after another, numpy adds pairwise
NUM_VERTS = 6890
HAND_VERTS = (2746, 2445, 6191, 5905)          # joints 24..27 of the 29: left thumb, left middle, right thumb, right middle finger tips
LAST_VERTS = tuple(range(6869, 6890))          # the vertices of the last, partial 64-column block of the blend GEMM (20670 = 322 * 64 + 62)
FOCAL, IMG_RES = 5000.0, 224.0
SCALES = (1.0, 0.05, -0.7, 1e-6, 0.0)
OUTPUTS = ("verts", "joints24", "kp_3d", "kp_2d")


def widen(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


def _inp(x, mag):
    x = widen(x)
    return np.abs(x) if mag else x


def _sub(a, b, mag):
    return a + b if mag else a - b


# ----------------------------------------------------------------------------------------------------------------- the stages
def shape_stage(betas, tables, mag=False):
    """v_shaped (n,V,3) = v_template + shapedirs . betas, and the rest joints J (n,24,3) = J_regressor . v_shaped."""
    b = _inp(betas, mag)
    v_shaped = _inp(tables["v_template"], mag)[None] + np.einsum("vkl,nl->nvk", _inp(tables["shapedirs"], mag).reshape(-1, 3, 10), b)
    return v_shaped, np.einsum("jv,nvk->njk", _inp(tables["J_regressor"], mag), v_shaped)


def pose_feature(rotmat, mag=False):
    """(R_1 .. R_23 - I) flattened: (n,207)."""
    R = _inp(rotmat, mag).reshape(-1, 24, 3, 3)
    return _sub(R[:, 1:], np.eye(3), mag).reshape(R.shape[0], 207)


def pose_blend(v_shaped, feat, tables, mag=False):
    return v_shaped + (feat @ _inp(tables["posedirs"], mag).reshape(207, -1)).reshape(v_shaped.shape)


def chain(rotmat, J, parents, mag=False, skip_level=None):
    """World transforms of the 24 joints along tables["parents"]: G_i = G_parent . [R_i | J_i - J_parent], as rotation parts (n,24,3,3) and
    translations (n,24,3).  skip_level: a planted fault -- the joints of that depth keep their parent's transform."""
    R = _inp(rotmat, mag).reshape(-1, 24, 3, 3)
    GR, Gt = np.empty_like(R), np.empty_like(J)
    depth = [0] * 24
    for i in range(24):
        p = int(parents[i])
        if i == 0:
            GR[:, 0], Gt[:, 0] = R[:, 0], J[:, 0]
            continue
        assert 0 <= p < i, "parents must be topologically ordered"
        depth[i] = depth[p] + 1
        if depth[i] == skip_level:
            GR[:, i], Gt[:, i] = GR[:, p], Gt[:, p]
            continue
        GR[:, i] = GR[:, p] @ R[:, i]
        Gt[:, i] = np.einsum("nab,nb->na", GR[:, p], _sub(J[:, i], J[:, p], mag)) + Gt[:, p]
    return GR, Gt


def skin(v_posed, GR, Gt, J, weights, mag=False):
    """verts = sum_j w_vj (G_j . (v_posed - J_j)) written as T_v . [v_posed; 1], T_v = sum_j w_vj [G_j | t_j - G_j . J_j]."""
    W = _inp(weights, mag)
    At = _sub(Gt, np.einsum("njab,njb->nja", GR, J), mag)
    n = GR.shape[0]
    TR = (W @ GR.reshape(n, 24, 9)).reshape(n, -1, 3, 3)
    return np.einsum("nvab,nvb->nva", TR, v_posed) + W @ At


def thorax_row(tables, mag=False):
    return _inp(np.asarray(tables["J_regressor_extra"])[5], mag)


def joints29(verts, Gt, tables, mag=False):
    """The wrapper's 29 joints: the 24 posed joints, the four finger-tip vertices, and row 5 ('Thorax (MPII)') of J_regressor_extra."""
    thorax = np.einsum("v,nvk->nk", thorax_row(tables, mag), verts)
    return np.concatenate([Gt, verts[:, list(HAND_VERTS)], thorax[:, None]], 1)


def camera_translation(cam):
    """(s, tx, ty) -> (tx, ty, 2 f / (224 s + 1e-9))."""
    c = widen(cam)
    return np.stack([c[:, 1], c[:, 2], 2 * FOCAL / (IMG_RES * c[:, 0] + 1e-9)], -1)


def project(kp3d, cam, mag_kp3d=None):
    """kp_2d = f (X / Z) / 112 of the translated joints.  With mag_kp3d: also its magnitude, propagated through the quotient,
    mag(X / Z) = (mag X + |X / Z| mag Z) / |Z|."""
    t = camera_translation(cam)[:, None, :]
    P = kp3d + t
    k = FOCAL / (IMG_RES / 2)
    out = k * P[..., :2] / P[..., 2:3]
    if mag_kp3d is None:
        return out
    M = mag_kp3d + np.abs(t)
    return out, k * (M[..., :2] + np.abs(P[..., :2] / P[..., 2:3]) * M[..., 2:3]) / np.abs(P[..., 2:3])


def _stages(betas, rotmat, tables, mag):
    v_shaped, J = shape_stage(betas, tables, mag)
    v_posed = pose_blend(v_shaped, pose_feature(rotmat, mag), tables, mag)
    GR, Gt = chain(rotmat, J, tables["parents"], mag)
    verts = skin(v_posed, GR, Gt, J, tables["lbs_weights"], mag)
    return verts, Gt, joints29(verts, Gt, tables, mag)


def smpl_reference(betas, rotmat, cam, tables):
    """dict(verts (n,6890,3), joints24 (n,24,3), kp_3d (n,29,3), kp_2d (n,29,2) or None without a camera), float64."""
    verts, Gt, kp3d = _stages(betas, rotmat, tables, False)
    return {"verts": verts, "joints24": Gt, "kp_3d": kp3d, "kp_2d": None if cam is None else project(kp3d, cam)}


def smpl_magnitude(betas, rotmat, cam, tables, ref=None):
    """The same dict of magnitudes.  kp_2d's needs the reference's own X / Z and Z: pass `ref` to save computing it again."""
    verts, Gt, kp3d = _stages(betas, rotmat, tables, True)
    out = {"verts": verts, "joints24": Gt, "kp_3d": kp3d, "kp_2d": None}
    if cam is not None:
        ref_kp3d = (ref or smpl_reference(betas, rotmat, None, tables))["kp_3d"]
        out["kp_2d"] = project(ref_kp3d, cam, kp3d)[1]
    return out


def min_abs_depth(ref, cam):
    """min |Z| over the joints of the call: the tests choose cameras so that it is >= 1 and no quotient needs special treatment."""
    return float(np.abs(ref["kp_3d"][..., 2] + camera_translation(cam)[:, None, 2]).min())


# ----------------------------------------------------------------------------------------------------------------- the check
def ratio(got, ref, mag):
    """(max |got - ref| / (2^-24 mag), index of the worst element).  No element is excluded: where the magnitude is 0 every term of the element
    is 0, and anything but the reference's exact value counts as infinitely wrong."""
    got, ref, mag = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(mag, np.float64)
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(mag > 0, d / (EPS * mag), np.where(d == 0, 0.0, np.inf))
    q = np.where(np.isnan(q), np.inf, q)
    i = int(np.argmax(q))
    return float(q.flat[i]), tuple(int(k) for k in np.unravel_index(i, q.shape))


def ratios(got, ref, mag, frames=slice(None)):
    """name -> (ratio, index) for every output `got` holds; `frames` selects the frames of ref / mag that the call was given."""
    return {k: ratio(np.asarray(got[k]).reshape(ref[k][frames].shape), ref[k][frames], mag[k][frames]) for k in got if got[k] is not None}


def bars(oracle_ratios):
    """name -> accepted ratio: FACTOR x what the independent fp32 implementation reaches on the same inputs, never below FACTOR."""
    return {k: max(FACTOR, FACTOR * (r[0] if isinstance(r, tuple) else r)) for k, r in oracle_ratios.items()}


def rel_err(a, b):
    """The bar the stage had before: max |a - b| / max |b| over the whole tensor, accepted below 1e-4."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


OLD_BAR = 1e-4


# ----------------------------------------------------------------------------------------------------------------- the tail
def tail_reference(plf, csf, sd, p="head."):
    """The regressor tail on given pooled features (n,128,24), (n,64,24): pred_rot6d[n,j,o] = sum_c plf[n,c,j] W[o,c,j]; shape and cam =
    Linear(1536) of csf flattened c * 24 + j.  Returns (reference, magnitude), dicts of pred_rot6d (n,24,6), shape (n,10), cam (n,3)."""
    ref, mag = {}, {}
    for m, out in ((False, ref), (True, mag)):
        x, y = _inp(plf, m), _inp(csf, m).reshape(len(csf), -1)
        wp = _inp(sd[p + "pose_mlp.weight"], m).reshape(6, 128, 24)
        out["pred_rot6d"] = np.einsum("ncj,ocj->njo", x, wp)
        for k in ("shape", "cam"):
            out[k] = y @ _inp(sd[p + k + "_mlp.weight"], m).T + _inp(sd[p + k + "_mlp.bias"], m)
    return ref, mag


def gram_schmidt(rot6d):
    """rot6d (m,6) viewed (3,2): a1 = elements 0,2,4, a2 = 1,3,5 -> (R (m,3,3) with columns b1 b2 b3, magnitude (m,3,3)).
    b2 = u / |u| with u = a2 - (b1.a2) b1 loses what cancels in u, so the rounding of an fp32 evaluation scales per row with
    1 + (|a2| + |b1.a2|) / |u|: the magnitude of every element of the row."""
    x = widen(rot6d).reshape(-1, 3, 2)
    a1, a2 = x[:, :, 0], x[:, :, 1]
    b1 = a1 / np.linalg.norm(a1, axis=1, keepdims=True)
    d = (b1 * a2).sum(1, keepdims=True)
    u = a2 - d * b1
    nu = np.linalg.norm(u, axis=1, keepdims=True)
    b2 = u / nu
    R = np.stack([b1, b2, np.cross(b1, b2)], -1)
    kappa = 1 + (np.linalg.norm(a2, axis=1, keepdims=True) + np.abs(d)) / nu
    return R, np.broadcast_to(kappa[:, :, None], R.shape).copy()


def axis_angle(R):
    """Rotation matrices (m,3,3) -> rotation vectors (m,3) with angle in [0, pi], float64.  The angle is atan2(|skew part|, trace - 1).  The axis
    comes from the skew part R - R^T = 2 sin(angle) [a]x below 1 rad and from the symmetric part (R + R^T) / 2 = cos I + (1 - cos) a a^T from
    there on, where the skew part vanishes (its sign from the skew part; at exactly pi either sign is the same rotation)."""
    R = widen(R).reshape(-1, 3, 3)
    w = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], -1)
    s2 = np.linalg.norm(w, axis=1)                                         # 2 sin
    angle = np.arctan2(s2, np.trace(R, axis1=1, axis2=2) - 1)
    out = np.zeros_like(w)
    for i in range(len(R)):
        if angle[i] < 1.0:
            if s2[i] > 0:
                out[i] = w[i] / s2[i] * angle[i]
            continue
        S = (R[i] + R[i].T) / 2 - np.cos(angle[i]) * np.eye(3)
        a = S[:, int(np.argmax(np.diag(S)))]
        a = a / np.linalg.norm(a)
        out[i] = (-a if a @ w[i] < 0 else a) * angle[i]
    return out


def rotvec_matrix(aa):
    """Rodrigues, float64: (m,3) -> (m,3,3)."""
    aa = np.asarray(aa, np.float64).reshape(-1, 3)
    th = np.linalg.norm(aa, axis=1)
    k = aa / np.where(th > 0, th, 1.0)[:, None]
    K = np.zeros((len(aa), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    s, c = np.sin(th)[:, None, None], np.cos(th)[:, None, None]
    return np.eye(3) + s * K + (1 - c) * (K @ K)


def geodesic(Ra, Rb):
    """The angle of Ra^T Rb, from the skew part as well as the trace (accurate near 0)."""
    D = np.swapaxes(Ra, 1, 2) @ Rb
    w = np.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], -1)
    return np.arctan2(np.linalg.norm(w, axis=1), np.trace(D, axis1=1, axis2=2) - 1)


AA_TOL, AA_GEODESIC_TOL, AA_MAX_FALLBACK = 1e-4, 2e-3, 4      # test_rotmat_to_axis_angle_all_branches_on_the_gpu's rule at the discontinuity at pi


def axis_angle_check(aa, R):
    """aa (m,3) against the float64 axis-angle of R.  Rows that differ element-wise by AA_TOL or more must be the same rotation within
    AA_GEODESIC_TOL (aa and -aa (2 pi - angle) / angle are one rotation).  Returns (rows that fell back, worst element-wise difference of the
    others, worst geodesic distance of those that fell back)."""
    aa = np.asarray(aa, np.float64).reshape(-1, 3)
    ref = axis_angle(R)
    d = np.abs(aa - ref).max(1)
    bad = ~(d < AA_TOL)                                                     # a NaN is bad
    geo = geodesic(rotvec_matrix(aa[bad]), rotvec_matrix(ref[bad])).max() if bad.any() else 0.0
    return int(bad.sum()), float(d[~bad].max()) if (~bad).any() else 0.0, float(geo)


# ----------------------------------------------------------------------------------------------------------------- tables
def _rng(seed, name):
    return np.random.default_rng([seed, *name.encode()])


def _far_vertices(tables):
    """The four finger-tip vertices and the vertices of the last 64-column block of the blend GEMM, every coordinate at least 5 cm from both
    index neighbours': a wrong index costs centimetres there."""
    vt = np.array(tables["v_template"], np.float32)
    step = np.array([0.11, 0.13, 0.07], np.float32)
    for k, v in enumerate(HAND_VERTS + LAST_VERTS):
        vt[v] = vt[v - 1] + step * (1 + k % 3) * (-1) ** k
        if v + 1 < NUM_VERTS and v + 1 not in LAST_VERTS and np.abs(vt[v + 1] - vt[v]).min() < 0.05:
            vt[v + 1] = vt[v] - step * (1 + (k + 1) % 3) * (-1) ** k
    for v in HAND_VERTS + LAST_VERTS:
        for u in (v - 1, v + 1):
            assert u >= NUM_VERTS or np.abs(vt[v] - vt[u]).min() >= 0.05, (v, u)
    return dict(tables, v_template=vt)


def standard_table(base):
    """`base`: the synthetic model's tables (synth.make_smpl_tables()).  Nothing else is drawn."""
    return _far_vertices({k: np.asarray(v) for k, v in base.items()})


VARIANTS = ("dense_skin", "thorax700", "thorax1", "thorax0", "chain", "star")


def variant_table(base, kind, seed=2026):
    """dense_skin: 1 .. 24 non-zero skinning weights per vertex (vertex 0 has 24, vertices 1 .. 8 have one): 1-4 of them uniform in 0.1 .. 1,
    the others log-uniform in 1e-6 .. 1e-5, before the rows are normalised; thorax700 / thorax1 / thorax0: row 5 of J_regressor_extra with 700, one and no entries;
    chain: parents[i] = i - 1; star: parents[i] = 0."""
    t = standard_table(base)
    g = _rng(seed, kind)
    if kind == "dense_skin":
        W = np.zeros((NUM_VERTS, 24), np.float64)
        count = g.integers(1, 25, NUM_VERTS)
        count[0], count[1:9], count[HAND_VERTS[0]], count[NUM_VERTS - 1] = 24, 1, 24, 24
        for v in range(NUM_VERTS):
            idx = g.choice(24, size=int(count[v]), replace=False)
            if count[v] == 24:
                idx = np.concatenate([[23], idx[idx != 23]])               # the 24th entry of a full list carries the vertex
            w = 10.0 ** g.uniform(-6.0, -5.0, len(idx))                     # trace weights, as fitted tables carry them ...
            main = int(g.integers(1, 5))
            w[:main] = g.uniform(0.1, 1.0, len(w[:main]))                   # ... next to the 1-4 weights that carry the vertex
            W[v, idx] = w / w.sum()
        t["lbs_weights"] = W.astype(np.float32)
        nz = (t["lbs_weights"] != 0).sum(1)
        assert nz.max() == 24 and nz[0] == 24 and (nz == 1).sum() >= 8 and nz.min() == 1
        assert t["lbs_weights"][t["lbs_weights"] > 0].min() < 2e-6
    elif kind.startswith("thorax"):
        nnz = int(kind[len("thorax"):])
        extra = np.array(t["J_regressor_extra"], np.float32)
        extra[5] = 0
        if nnz:
            idx = np.sort(g.choice(NUM_VERTS, size=nnz, replace=False))
            w = g.uniform(0.1, 1.0, nnz)
            extra[5, idx] = (w / w.sum()).astype(np.float32)
        assert (extra[5] != 0).sum() == nnz
        t["J_regressor_extra"] = extra
    elif kind == "chain":
        t["parents"] = np.arange(-1, 23, dtype=np.int32)
    elif kind == "star":
        t["parents"] = np.array([-1] + [0] * 23, np.int32)
    else:
        raise ValueError(kind)
    return t


# ----------------------------------------------------------------------------------------------------------------- poses, cameras
def _rodrigues(axis, angle):
    K = np.zeros(axis.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = (-axis[..., 2], axis[..., 1], axis[..., 2], -axis[..., 0],
                                                                                         -axis[..., 1], axis[..., 0])
    a = angle[..., None, None]
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def make_poses(n, seed):
    """betas (n,10) and rotmat (n,24,3,3), fp32.  Per joint a seeded choice of: the identity, 1e-4 rad, a uniform angle, pi - 1e-3, exactly pi
    (2 a a^T - I) about a random axis.  From 5 frames on, two frames are no rotations -- the stage is polynomial in the matrices --: frame n - 2
    has the zero matrix on eight joints, frame n - 3 diag(2, 0.5, 1) times the rotation on six.  Betas by frame: 0, +5, -5, N(0, 2^2)."""
    g = _rng(seed, f"poses{n}")
    kind = g.integers(0, 5, (n, 24))
    axis = g.standard_normal((n, 24, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    angle = np.choose(kind, [np.zeros((n, 24)), np.full((n, 24), 1e-4), g.uniform(0, np.pi, (n, 24)), np.full((n, 24), np.pi - 1e-3),
                             np.full((n, 24), np.pi)])
    R = _rodrigues(axis, angle)
    R[kind == 0] = np.eye(3)
    R[kind == 4] = (2 * axis[..., :, None] * axis[..., None, :] - np.eye(3))[kind == 4]
    if n >= 5:
        R[n - 2, g.choice(np.arange(1, 24), 8, replace=False)] = 0.0
        six = g.choice(24, 6, replace=False)
        R[n - 3, six] = np.diag([2.0, 0.5, 1.0]) @ R[n - 3, six]
    betas = np.zeros((n, 10))
    for f in range(n):
        betas[f] = (0.0, 5.0, -5.0, 0.0)[f % 4]
        if f % 4 == 3:
            betas[f] = 2.0 * g.standard_normal(10)
    return betas.astype(np.float32), R.astype(np.float32)


def make_mild_poses(n, seed):
    """betas N(0, 1) and rotations of at most 0.3 rad about random axes on every joint: the size of pose a walking person gives the stage."""
    g = _rng(seed, f"mild{n}")
    axis = g.standard_normal((n, 24, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    return g.standard_normal((n, 10)).astype(np.float32), _rodrigues(axis, g.uniform(0, 0.3, (n, 24))).astype(np.float32)


def make_cameras(n, seed):
    """(s, tx, ty) (n,3) fp32: s runs through SCALES frame by frame (large, small, negative, tiny, zero), tx, ty uniform in +-0.5."""
    g = _rng(seed, f"cameras{n}")
    s = np.array(SCALES)[np.arange(n) % len(SCALES)]
    return np.concatenate([s[:, None], g.uniform(-0.5, 0.5, (n, 2))], 1).astype(np.float32)


def make_features(n, seed):
    """Pooled features for the tail, (n,128,24) and (n,64,24) fp32: lognormal magnitudes (sigma 2: five decades between the 1st and the 99th
    percentile), both signs, every frame its own."""
    g = _rng(seed, f"features{n}")
    draw = lambda *s: (np.exp(2.0 * g.standard_normal(s)) * g.choice([-1.0, 1.0], s) * 0.05).astype(np.float32)
    return draw(n, 128, 24), draw(n, 64, 24)


def round_bf16(x):
    """fp32 -> nearest-even bf16 -> fp32."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


# ----------------------------------------------------------------------------------------------------------------- cases
STANDARD_FRAMES, VARIANT_FRAMES = 129, 17
STANDARD_SEED, OTHER_SEED, VARIANT_SEED = 1, 7, 2


def make_case(tables, n, seed, poses=make_poses):
    """The inputs of n frames with their reference and magnitudes, computed once; a call of m <= n frames is given the LAST m frames of the case
    (frames(case, m)), so that a frame sits at another place in every call size and the two frames that are no rotations are in every call of
    5 frames or more."""
    betas, rotmat = poses(n, seed)
    cam = make_cameras(n, seed)
    assert len({rotmat[f].tobytes() for f in range(n)}) == n, "all frames of a call are distinct"
    ref = smpl_reference(betas, rotmat, cam, tables)
    assert min_abs_depth(ref, cam) >= 1.0
    return {"n": n, "betas": betas, "rotmat": rotmat, "cam": cam, "ref": ref, "mag": smpl_magnitude(betas, rotmat, cam, tables, ref)}


def frames(case, m):
    return slice(case["n"] - m, case["n"])


def fp32_oracle(oracle, case, tables, dtype=np.float32):
    """The independent fp32 implementation (oracle.smpl_lbs and friends) on the inputs of the case: the yardstick of the accepted ratio."""
    verts, j24 = oracle.smpl_lbs(case["betas"], case["rotmat"], tables)
    kp3d = oracle.smpl_joints29(verts, j24, tables)
    out = {"verts": verts, "joints24": j24, "kp_3d": kp3d, "kp_2d": oracle.project(kp3d, case["cam"])}
    assert all(v.dtype == dtype for v in out.values())                      # float64 inside oracle.float64()
    return out
