"""The rasteriser's rules restated in numpy -- float64 for everything continuous, int64 for coverage -- and the scenes the
GPU tests draw.  Written from the rules, not from csrc/render_kernels.hip; tests/test_raster_checks_cpu.py proves it on its own (the fill
rule against a pixel set known in advance) and shows that each check fails a renderer that breaks the rule it checks.

Rules: q = M (x, -y, -z); x_ndc = sx (q.x + tx), y_ndc = sy (q.y - ty), z_ndc = -q.z; x_win = (x_ndc + 1) W / 2, y_win = (y_ndc + 1) H / 2 with
GL's origin at the bottom-left; X = floor(256 x_win + 0.5), clamped to +-2^28; the sample of pixel (i, j) is (256 i + 128, 256 j + 128); twice
the signed area A2 <= 0 is culled; a centre exactly on an edge belongs to the triangle only if the edge is a top or a left edge in image
space (y down); z from the barycentrics; z outside [-1, 1] is discarded; GL_LESS, the lower face index winning at equal depth; image row
r = H - 1 - j.

Near-ties: a pixel whose two nearest reference depths differ by less than NEAR_TIE, but are not EQUAL, is a near-tie: there the device's
fp32 depths may order the other way, and the winner is excused.  Equal reference depths are no near-tie -- the rule above decides them, and
the scene `equal_depth` (constant z, exact in fp32 too) checks that it does."""
import numpy as np

SUB = 256
HALF = 128
LIMIT = 1 << 28
NEAR_TIE = 1e-5
NEAR_TIE_CAP = 0.005
LIGHTS = np.array([[0.0, -1.0, 1.0], [0.0, 1.0, 1.0], [1.0, 1.0, 2.0]])
AMBIENT = 0.3
SIDE_M = np.array([0, 0, -1, 0, 1, 0, 1, 0, 0], np.float32)          # rotation by 270 degrees about y (renderer.py:88-90, demo.py:351-352)
N_SMPL = 6890


# ----------------------------------------------------------------------------- the rules
def transform(verts, cam, M=None):
    """verts (V,3), cam (sx,sy,tx,ty), M 9 or None -> q (V,3), x_win, y_win, z_ndc, all float64 (window coordinates still need H, W: see snap)."""
    v = np.asarray(verts, np.float64) * np.array([1.0, -1.0, -1.0])
    Mm = np.eye(3) if M is None else np.asarray(M, np.float64).reshape(3, 3)
    q = v @ Mm.T
    sx, sy, tx, ty = (float(c) for c in np.asarray(cam, np.float64))
    return q, sx * (q[:, 0] + tx), sy * (q[:, 1] - ty), -q[:, 2]


def snap(ndc, size):
    w = (np.asarray(ndc, np.float64) + 1.0) * size / 2.0
    return np.clip(np.floor(w * SUB + 0.5), -LIMIT, LIMIT).astype(np.int64)


def setup(verts, faces, cam, M, H, W):
    """The float64 statement of grnet_op_raster_setup: X, Y int64, z, unit vertex normals, q."""
    q, xn, yn, z = transform(verts, cam, M)
    return snap(xn, W), snap(yn, H), z, vertex_normals(q, faces), q


def vertex_normals(q, faces):
    """Normalised sum of the un-normalised face normals cross(q1 - q0, q2 - q0) over the faces at each vertex; 0 where there is none."""
    f = np.asarray(faces, np.int64)
    fn = np.cross(q[f[:, 1]] - q[f[:, 0]], q[f[:, 2]] - q[f[:, 0]])
    n = np.zeros_like(q)
    for k in range(3):
        np.add.at(n, f[:, k], fn)
    l = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(l > 0, n / np.where(l > 0, l, 1.0), 0.0)


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _top_left(ax, ay, bx, by):
    """Edge a -> b of a triangle counter-clockwise in GL window space (y up): its inside is on the left of a -> b.  Going down (dy < 0) the
    inside is at larger x: a left edge.  Horizontal and going towards smaller x the inside is below it on the screen: a top edge."""
    return by < ay or (by == ay and bx < ax)


def rasterise(X, Y, z, faces, H, W, fill="top_left", cull=True, depth="less"):
    """The z-buffer over integer coordinates.  Returns winner (H,W) int64 in IMAGE rows (-1: uncovered), d1 and d2 (H,W): the nearest and the
    second nearest depth (inf where there is none).  The wrong variants serve the discrimination tests only: fill="inclusive" keeps every centre
    on an edge, cull=False draws back faces too, depth="lequal" lets the later face win a tie."""
    X, Y, z = np.asarray(X, np.int64), np.asarray(Y, np.int64), np.asarray(z, np.float64)
    win = np.full((H, W), -1, np.int64)
    d1 = np.full((H, W), np.inf)
    d2 = np.full((H, W), np.inf)
    for fi, (a, b, c) in enumerate(np.asarray(faces, np.int64)):
        A2 = int(_edge(X[a], Y[a], X[b], Y[b], X[c], Y[c]))
        if A2 == 0 or (A2 < 0 and cull):
            continue
        if A2 < 0:
            b, c, A2 = c, b, -A2
        xs, ys = (int(X[a]), int(X[b]), int(X[c])), (int(Y[a]), int(Y[b]), int(Y[c]))
        i0, i1 = max(0, -((HALF - min(xs)) // SUB)), min(W - 1, (max(xs) - HALF) // SUB)
        j0, j1 = max(0, -((HALF - min(ys)) // SUB)), min(H - 1, (max(ys) - HALF) // SUB)
        if i0 > i1 or j0 > j1:
            continue
        px = (np.arange(i0, i1 + 1, dtype=np.int64) * SUB + HALF)[None, :]
        py = (np.arange(j0, j1 + 1, dtype=np.int64) * SUB + HALF)[:, None]
        inside = np.ones((j1 - j0 + 1, i1 - i0 + 1), bool)
        ws = []
        for (s, t) in ((b, c), (c, a), (a, b)):
            w = _edge(X[s], Y[s], X[t], Y[t], px, py)
            keep_zero = fill == "inclusive" or _top_left(X[s], Y[s], X[t], Y[t])
            inside &= (w >= 0) if keep_zero else (w > 0)
            ws.append(w)
        if not inside.any():
            continue
        zz = (ws[0] * z[a] + ws[1] * z[b] + ws[2] * z[c]) / A2
        inside &= (zz >= -1.0) & (zz <= 1.0)
        sl = (slice(j0, j1 + 1), slice(i0, i1 + 1))
        o1, o2, ow = d1[sl], d2[sl], win[sl]
        first = inside & ((zz <= o1) if depth == "lequal" else (zz < o1))
        second = inside & ~first
        o2[:] = np.where(first, o1, np.where(second, np.minimum(o2, zz), o2))
        o1[:] = np.where(first, zz, o1)
        ow[:] = np.where(first, fi, ow)
    return win[::-1].copy(), d1[::-1].copy(), d2[::-1].copy()


def near_ties(d1, d2):
    gap = np.where(np.isfinite(d2), d2, np.inf) - np.where(np.isfinite(d1), d1, 0.0)
    return np.isfinite(d1) & (gap < NEAR_TIE) & (gap > 0)


def shade(q, normals, X, Y, faces, winner, colour):
    """The float64 shading formula at the covered pixels of `winner` (image rows): (H,W,3) float64 levels BEFORE the final floor(. + 0.5), nan
    where uncovered.  Barycentrics from the integer edge values, exactly."""
    H, W = winner.shape
    out = np.full((H, W, 3), np.nan)
    r, i = np.nonzero(winner >= 0)
    if not len(r):
        return out
    f = np.asarray(faces, np.int64)[winner[r, i]]
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    px, py = i.astype(np.int64) * SUB + HALF, (H - 1 - r).astype(np.int64) * SUB + HALF
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    A2 = _edge(X[a], Y[a], X[b], Y[b], X[c], Y[c]).astype(np.float64)
    bar = np.stack([_edge(X[b], Y[b], X[c], Y[c], px, py), _edge(X[c], Y[c], X[a], Y[a], px, py), _edge(X[a], Y[a], X[b], Y[b], px, py)], 1) / A2[:, None]
    n = np.einsum("pk,pkd->pd", bar, normals[f])
    p = np.einsum("pk,pkd->pd", bar, q[f])
    l = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(l > 0, n / np.where(l > 0, l, 1.0), 0.0)
    s = np.full(len(r), AMBIENT)
    for L in LIGHTS:
        d = L[None, :] - p
        d2 = (d * d).sum(1)
        s += np.maximum(0.0, (n * d).sum(1) / np.sqrt(d2)) / (np.pi * d2)
    out[r, i] = 255.0 * np.minimum(1.0, np.asarray(colour, np.float64)[None, :] * s[:, None])
    return out


# ----------------------------------------------------------------------------- scenes
def torus(nu, nv, R=0.55, r=0.25, tilt=(0.0, 0.0)):
    """nu x nv vertices on a torus, closed: 2 nu nv faces, counter-clockwise seen from outside.  65 x 106 is 6890 vertices, 13 780 faces."""
    u = np.arange(nu) * 2 * np.pi / nu
    w = np.arange(nv) * 2 * np.pi / nv
    uu, ww = np.meshgrid(u, w, indexing="ij")
    p = np.stack([(R + r * np.cos(ww)) * np.cos(uu), (R + r * np.cos(ww)) * np.sin(uu), r * np.sin(ww)], -1).reshape(-1, 3)
    ax, ay = tilt
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    p = p @ (Ry @ Rx).T
    idx = np.arange(nu * nv).reshape(nu, nv)
    a, b = idx, np.roll(idx, -1, 0)
    c, d = np.roll(b, -1, 1), np.roll(idx, -1, 1)
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return p.astype(np.float32), faces.astype(np.int32)


def _from_window(pts, H, W, z=0.0):
    """Vertices that the identity view with cam (1,1,0,0) puts at the given window positions (x_win, y_win[, z_ndc]), in pixels, GL rows."""
    pts = np.asarray(pts, np.float64)
    zz = pts[:, 2] if pts.shape[1] == 3 else np.full(len(pts), z)
    return np.stack([pts[:, 0] * 2 / W - 1, -(pts[:, 1] * 2 / H - 1), zz], 1).astype(np.float32)      # x = x_ndc, -y = y_ndc, -(-z) ... z_ndc = z


def _scene(verts, faces, H, W, cam=(1.0, 1.0, 0.0, 0.0), M=None):
    return dict(verts=np.asarray(verts, np.float32), faces=np.asarray(faces, np.int32).reshape(-1, 3), cam=np.asarray(cam, np.float32),
                M=None if M is None else np.asarray(M, np.float32), H=int(H), W=int(W))


def split_rectangle(c0, c1, r0, r1, H, W, other_diagonal=False):
    """A rectangle with its corners on the centres of pixels (c0, r0) .. (c1, r1) in IMAGE rows, split along one diagonal: it must cover exactly
    the pixels [c0,c1) x [r0,r1), each once."""
    jt, jb = H - 1 - r0, H - 1 - r1                                       # GL rows of the top and the bottom side
    corners = [(c0 + 0.5, jb + 0.5), (c1 + 0.5, jb + 0.5), (c1 + 0.5, jt + 0.5), (c0 + 0.5, jt + 0.5)]      # counter-clockwise, y up
    faces = [(0, 1, 3), (1, 2, 3)] if other_diagonal else [(0, 1, 2), (0, 2, 3)]
    return _scene(_from_window(corners, H, W), faces, H, W)


def scenes():
    """name -> scene (verts float32, faces int32, cam, M, H, W): everything the GPU tests draw except the 1920 x 1080 frame (scene_1080p)."""
    out = {}
    for (W, H) in ((1, 1), (7, 5), (64, 48), (97, 61)):
        out[f"triangle_{W}x{H}"] = _scene(_from_window([(-0.3 * W, 0.1 * H), (1.2 * W, 0.3 * H), (0.4 * W, 1.1 * H)] if W == 1 else
                                                       [(0.11 * W, 0.13 * H), (0.93 * W, 0.32 * H), (0.41 * W, 0.89 * H)], H, W, z=0.25), [(0, 1, 2)], H, W)
    out["larger_than_image"] = _scene(_from_window([(-300.0, -200.0), (500.0, -100.0), (20.0, 700.0)], 48, 64), [(0, 1, 2)], 48, 64)
    W, H = 64, 48
    tri = np.array([(0.0, 0.0), (9.0, 1.5), (3.5, 8.0)])
    offs = [(-4.0, 20.0), (-30.0, 20.0), (W - 4.0, 10.0), (W + 20.0, 10.0), (25.0, -3.5), (25.0, -40.0), (30.0, H - 4.0), (30.0, H + 9.0), (-5.0, -4.0)]
    out["off_each_side"] = _scene(_from_window(np.concatenate([tri + o for o in offs]), H, W), np.arange(3 * len(offs)).reshape(-1, 3), H, W)
    out["zero_area"] = _scene(_from_window([(5.0, 10.0), (20.5, 10.0), (36.0, 10.0), (40.0, 8.0), (60.0, 9.0), (50.0, 30.0)], H, W), [(0, 1, 2), (3, 4, 5)], H, W)
    out["back_facing"] = _scene(_from_window([(4.0, 4.0), (30.0, 6.0), (12.0, 40.0), (34.0, 8.0), (60.0, 9.0), (50.0, 30.0)], H, W), [(0, 2, 1), (3, 4, 5)], H, W)
    out["split_rectangle"] = split_rectangle(5, 41, 7, 30, H, W)
    out["split_rectangle_other"] = split_rectangle(5, 41, 7, 30, H, W, other_diagonal=True)
    out["crossing_far"] = _scene(_from_window([(4.0, 4.0, 0.2), (60.0, 6.0, 0.6), (30.0, 44.0, 1.8)], H, W), [(0, 1, 2)], H, W)
    out["crossing_near"] = _scene(_from_window([(4.0, 4.0, -0.2), (60.0, 6.0, -0.6), (30.0, 44.0, -1.8)], H, W), [(0, 1, 2)], H, W)
    out["equal_depth"] = _scene(_from_window([(3.0, 3.0), (50.0, 8.0), (20.0, 40.0), (15.0, 2.0), (61.0, 20.0), (25.0, 45.0)], H, W, z=0.5), [(0, 1, 2), (3, 4, 5)], H, W)
    out["equal_depth_swapped"] = _scene(out["equal_depth"]["verts"], [(3, 4, 5), (0, 1, 2)], H, W)
    tv, tf = torus(12, 8, tilt=(0.9, 0.4))
    out["torus_12x8"] = _scene(tv, tf, 61, 97, cam=(0.9, 0.9 * 97 / 61, 0.05, -0.03))
    tv, tf = torus(65, 106, tilt=(0.9, 0.4))
    for (W, H) in ((97, 61), (320, 240)):
        cam = (0.9, 0.9 * W / H, 0.05, -0.03)
        out[f"torus_{W}x{H}"] = _scene(tv, tf, H, W, cam=cam)
        out[f"torus_{W}x{H}_side"] = _scene(tv, tf, H, W, cam=cam, M=SIDE_M)
    out["negative_sx"] = _scene(tv, tf, 61, 97, cam=(-0.9, 0.9 * 97 / 61, 0.05, -0.03))
    return out


def scene_1080p():
    tv, tf = torus(65, 106, tilt=(0.9, 0.4))
    return _scene(tv, tf, 1080, 1920, cam=(0.5, 0.5 * 1920 / 1080, 0.3, -0.1))


def pad_to_smpl(verts):
    """(V,3) -> (6890,3): the vertices grnet_render_meshes reads; those no face names sit at the origin."""
    out = np.zeros((N_SMPL, 3), np.float32)
    out[:len(verts)] = verts
    return out


# ----------------------------------------------------------------------------- the checks (shared by the CPU and the GPU file)
def check_cover(winner, ref_winner):
    """Coverage bit-exact."""
    a, b = winner >= 0, ref_winner >= 0
    assert np.array_equal(a, b), f"coverage differs at {int((a != b).sum())} of {int(b.sum())} covered pixels"


def check_winner(winner, ref_winner, d1, d2):
    """The winning face exact except at near-ties; the share of pixels actually excused stays under the cap.  Returns the excused mask."""
    bad = winner != ref_winner
    excused = bad & near_ties(d1, d2)
    assert not (bad & ~excused).any(), f"{int((bad & ~excused).sum())} pixels with the wrong face and no near-tie"
    covered = int((ref_winner >= 0).sum())
    assert excused.sum() <= NEAR_TIE_CAP * covered, f"{int(excused.sum())} of {covered} pixels excused"
    return excused


def check_near_tie_cap(ref_winner, d1, d2):
    covered, ties = int((ref_winner >= 0).sum()), int(near_ties(d1, d2).sum())
    assert ties <= NEAR_TIE_CAP * covered, f"{ties} near-ties among {covered} covered pixels"
    return ties, covered


def check_image(image, before, levels, excused=None):
    """image, before (H,W,3) uint8; levels from shade(): covered pixels within +-1 level of floor(level + 0.5), every other byte as before."""
    covered = ~np.isnan(levels[..., 0])
    assert np.array_equal(image[~covered], before[~covered]), "an uncovered pixel changed"
    want = np.floor(levels[covered] + 0.5)
    diff = np.abs(image[covered].astype(np.float64) - want)
    if excused is not None:
        diff = diff[~excused[covered]]
    assert diff.size == 0 or diff.max() <= 1, f"a covered pixel is {diff.max():.0f} levels off"
