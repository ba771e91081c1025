"""The wireframe's line rule ("Lines") restated in numpy -- int64 for coverage, float64 for depth and shading -- and the scenes
the GPU tests add for it.  Written from the rule, not from csrc/render_kernels.hip; tests/test_line_checks_cpu.py proves it on its own (a square's
outline against a pixel set known in advance) and shows that each check fails a renderer that breaks the rule it checks.  Vertex setup, the
shading constants, the scenes of the fill and the check_* functions are those of raster_checks.

The rule, on the snapped integers of setup (SUB = 256, pixel centre 256 i + 128): edges come from faces with doubled area A2 > 0 only, three
each, k = 0: v0 -> v1, 1: v1 -> v2, 2: v2 -> v0.  dx = dy = 0: nothing.  x-major if |dx| >= |dy|, else y-major; P the major, Q the minor
coordinate; the end points ordered P_lo < P_hi, and everything after that from (lo, hi) alone.  Major index m is covered iff
P_lo <= 256 m + 128 < P_hi, clamped to the viewport; minor index n = floor((Q_lo dP + (256 m + 128 - P_lo) dQ) / (256 dP)), dropped outside the
viewport; t = (256 m + 128 - P_lo) / dP, z = z_lo + t (z_hi - z_lo), dropped outside [-1, 1]; GL_LESS, at equal depth the lower 3 face + k
wins; pixel (i, j) = (m, n) if x-major else (n, m), image row H - 1 - j.  Normal and position of a fragment: lo + t (hi - lo)."""
import numpy as np

from . import raster_checks as rc

SUB, HALF = rc.SUB, rc.HALF


def _fragments(X, Y, z, faces, H, W, upper, cull, minor):
    """Every fragment of every edge, before the depth test: (pixel index in GL rows, z float64, id = 3 face + k)."""
    X, Y, z = np.asarray(X, np.int64), np.asarray(Y, np.int64), np.asarray(z, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    A2 = (X[b] - X[a]) * (Y[c] - Y[a]) - (Y[b] - Y[a]) * (X[c] - X[a])
    front = (A2 > 0) if cull else np.ones(len(f), bool)
    s = np.stack([a, b, c], 1).reshape(-1)                               # edge e = 3 face + k runs from s[e] to t[e]
    t = np.stack([b, c, a], 1).reshape(-1)
    ids = np.arange(3 * len(f), dtype=np.int64)
    dx, dy = X[t] - X[s], Y[t] - Y[s]
    live = np.repeat(front, 3) & ((dx != 0) | (dy != 0))
    s, t, ids, dx, dy = s[live], t[live], ids[live], dx[live], dy[live]
    xmaj = np.abs(dx) >= np.abs(dy)
    Ps, Pt = np.where(xmaj, X[s], Y[s]), np.where(xmaj, X[t], Y[t])
    Qs, Qt = np.where(xmaj, Y[s], X[s]), np.where(xmaj, Y[t], X[t])
    swap = Pt < Ps
    lo, hi = np.where(swap, t, s), np.where(swap, s, t)
    Plo, Phi, Qlo, Qhi = np.where(swap, Pt, Ps), np.where(swap, Ps, Pt), np.where(swap, Qt, Qs), np.where(swap, Qs, Qt)
    assert (Plo < Phi).all()
    n_major, n_minor = np.where(xmaj, W, H), np.where(xmaj, H, W)
    m0 = np.maximum(0, -((HALF - Plo) // SUB))                           # the first m with 256 m + 128 >= P_lo
    last = (Phi - HALF) // SUB if upper == "closed" else -((HALF - Phi) // SUB) - 1       # the last m with 256 m + 128 <= or < P_hi
    m1 = np.minimum(n_major - 1, last)
    count = np.maximum(0, m1 - m0 + 1)
    e = np.repeat(np.arange(len(s)), count)                              # the edge of each fragment
    m = m0[e] + (np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count))
    cP = m * SUB + HALF
    dP, dQ = (Phi - Plo)[e], (Qhi - Qlo)[e]
    num = Qlo[e] * dP + (cP - Plo[e]) * dQ
    D = SUB * dP
    n = num // D if minor == "floor" else -((-num) // D) - 1            # "half_down": a line exactly between two pixels goes to the lower one
    tt = (cP - Plo[e]).astype(np.float64) / dP.astype(np.float64)
    zz = z[lo[e]] + tt * (z[hi[e]] - z[lo[e]])
    keep = (n >= 0) & (n < n_minor[e]) & (zz >= -1.0) & (zz <= 1.0)
    i, j = np.where(xmaj[e], m, n), np.where(xmaj[e], n, m)
    return (j * W + i)[keep], zz[keep], ids[e][keep]


def rasterise_lines(X, Y, z, faces, H, W, upper="open", cull=True, tie="lower", minor="floor"):
    """The wireframe's z-buffer over integer coordinates.  Returns winner (H,W) int64 in IMAGE rows: 3 face + k, -1 where uncovered; d1: the
    nearest depth; d2: the nearest depth STRICTLY greater than d1 (inf where there is none) -- the two draws of a shared edge have equal depths,
    which the index rule decides and which are no near-tie.  The wrong variants serve the discrimination tests only: upper="closed" also covers
    a centre exactly on P_hi, cull=False draws back faces too, tie="higher" lets the higher index win, minor="half_down" rounds a line exactly
    between two pixels the other way."""
    pix, zz, ids = _fragments(X, Y, z, faces, H, W, upper, cull, minor)
    win = np.full(H * W, -1, np.int64)
    d1 = np.full(H * W, np.inf)
    d2 = np.full(H * W, np.inf)
    if len(pix):
        order = np.lexsort((ids if tie == "lower" else -ids, zz, pix))   # by pixel, then depth, then index
        pix, zz, ids = pix[order], zz[order], ids[order]
        start = np.nonzero(np.r_[True, pix[1:] != pix[:-1]])[0]
        group = np.cumsum(np.r_[True, pix[1:] != pix[:-1]]) - 1
        win[pix[start]] = ids[start]
        d1[pix[start]] = zz[start]
        d2[pix[start]] = np.minimum.reduceat(np.where(zz > zz[start][group], zz, np.inf), start)
    flip = lambda v: v.reshape(H, W)[::-1].copy()
    return flip(win), flip(d1), flip(d2)


def shade_lines(q, normals, X, Y, faces, winner, colour):
    """The float64 shading at the covered pixels of `winner` (image rows, 3 face + k): (H,W,3) levels BEFORE the final floor(. + 0.5), nan where
    uncovered.  t from the pixel's major index; normal (renormalised) and position are lo + t (hi - lo)."""
    H, W = winner.shape
    out = np.full((H, W, 3), np.nan)
    r, i = np.nonzero(winner >= 0)
    if not len(r):
        return out
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ids = winner[r, i]
    s, t = f[ids // 3, ids % 3], f[ids // 3, (ids % 3 + 1) % 3]
    xmaj = np.abs(X[t] - X[s]) >= np.abs(Y[t] - Y[s])
    Ps, Pt = np.where(xmaj, X[s], Y[s]), np.where(xmaj, X[t], Y[t])
    lo, hi = np.where(Pt < Ps, t, s), np.where(Pt < Ps, s, t)
    cP = np.where(xmaj, i, H - 1 - r).astype(np.int64) * SUB + HALF
    Plo, Phi = np.minimum(Ps, Pt), np.maximum(Ps, Pt)
    tt = ((cP - Plo) / (Phi - Plo).astype(np.float64))[:, None]
    n = normals[lo] + tt * (normals[hi] - normals[lo])
    p = q[lo] + tt * (q[hi] - q[lo])
    l = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(l > 0, n / np.where(l > 0, l, 1.0), 0.0)
    sh = np.full(len(r), rc.AMBIENT)
    for L in rc.LIGHTS:
        d = L[None, :] - p
        d2 = (d * d).sum(1)
        sh += np.maximum(0.0, (n * d).sum(1) / np.sqrt(d2)) / (np.pi * d2)
    out[r, i] = 255.0 * np.minimum(1.0, np.asarray(colour, np.float64)[None, :] * sh[:, None])
    return out


# ----------------------------------------------------------------------------- scenes
def line_scenes():
    """name -> scene: what the wireframe tests draw beyond raster_checks.scenes()."""
    out = {}
    W, H = 64, 48
    ang = np.arange(16) * np.pi / 8
    rim = np.stack([32.5 + 20 * np.cos(ang), 24.5 + 20 * np.sin(ang)], 1)       # one depth: where the spokes meet, the index rule decides
    fan = [(0, 1 + k, 1 + (k + 1) % 16) for k in range(16)]              # counter-clockwise with y up
    out["fan_16"] = rc._scene(rc._from_window(np.concatenate([[(32.5, 24.5)], rim]), H, W), fan, H, W)
    out["square_outline"] = rc.split_rectangle(5, 29, 7, 31, H, W)
    out["through_image"] = rc._scene(rc._from_window([(-300.0, 10.0), (500.0, 40.0), (20.0, 700.0)], H, W), [(0, 1, 2)], H, W)
    # the first holds the centre of pixel (10, 10) in GL rows, the second holds none
    out["sub_pixel"] = rc._scene(rc._from_window([(10.3, 10.3), (10.8, 10.4), (10.5, 10.9), (20.1, 20.1), (20.4, 20.15), (20.2, 20.4)], H, W),
                                 [(0, 1, 2), (3, 4, 5)], H, W)
    # corners on pixel CORNERS: a horizontal and a vertical edge that run exactly between two pixels, a hypotenuse through pixel corners
    out["on_pixel_boundaries"] = rc._scene(rc._from_window([(10.0, 10.0), (40.0, 10.0), (10.0, 30.0)], H, W), [(0, 1, 2)], H, W)
    tv, tf = rc.torus(12, 8, tilt=(0.9, 0.4))
    out["negative_sx_12x8"] = rc._scene(tv, tf, 61, 97, cam=(-0.9, 0.9 * 97 / 61, 0.05, -0.03))
    return out


COVER_ONLY = ("torus_97x61", "torus_97x61_side", "negative_sx")           # saturated blobs: near-ties at or close to the cap


def all_scenes():
    out = dict(rc.scenes())
    out.update(line_scenes())
    return out


def winner_scenes():
    """The scenes of the winner check: all but the 6890-vertex torus at 97 x 61, whose wireframe is a saturated blob with near-ties over the cap."""
    return {k: v for k, v in all_scenes().items() if k not in COVER_ONLY}
