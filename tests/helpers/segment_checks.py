"""The skeleton view's rules restated in numpy -- float64 for everything continuous, int64 for coverage -- and the scenes the
GPU tests draw.  Written from the rules, not from csrc/skeleton_kernels.hip; tests/test_segment_checks_cpu.py proves it on its own (pixel sets
written out by hand, the wireframe's rule at width 1) and shows that each check fails a renderer that breaks the rule it checks.  The near-tie
bar and the check_* functions are those of raster_checks.

Rules.  View: p' = R p; hom = P (p', 1); (xs, ys) = hom[0,1] / hom[3]; the window (x0, x1, y0, y1) maps onto the centred S x S square of the
H x W panel, S = min(H, W), in GL window coordinates (origin bottom-left): x_win = (W - S)/2 + S (xs - x0)/(x1 - x0), y likewise;
X = floor(256 x_win + 0.5); depth d = P[3,:3] . p'.  A point is invalid (X = Y = INT32_MIN) if p' is not finite, hom[3] <= 0 or |x_win| or |y_win|
exceeds 2^20.  Lines: a segment with an invalid end or of length 0 draws nothing; x-major if |dx| >= |dy|, else y-major; P the major, Q the minor
coordinate; ends ordered P0 < P1 and everything from (lo, hi) alone; major index m covered iff P0 <= 256 m + 128 < P1, clamped to the viewport;
the column n0 .. n0 + w - 1, n0 = floor((Q0 dP + (256 m + 128 - P0) dQ - (w - 1) 128 dP) / (256 dP)), cut by the viewport, all at
d = d_lo + t (d_hi - d_lo), t = (256 m + 128 - P0) / dP; no caps, no joins.  ONE depth buffer per image: GL_LESS on (d, id), id = r S + s with r the
skeleton's rank among those of the image and s the segment; at equal depth the lower id wins.  Pixel (i, j) = (m, n) if x-major else (n, m),
image row H - 1 - j; a covered pixel takes its segment's three colour bytes, every other byte stays."""
import numpy as np

from . import raster_checks as rc

SUB, HALF = rc.SUB, rc.HALF
SENTINEL = -2**31
WINDOW_LIMIT = 2.0**20


# ----------------------------------------------------------------------------- the rules
def window_coords(points, H, W, view, R=None):
    """points (N,3) -> (x_win, y_win, d, valid) in float64, before the snap."""
    P, (x0, x1, y0, y1) = np.asarray(view[0], np.float64), view[1]
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if R is not None:
        with np.errstate(invalid="ignore"):
            p = p @ np.asarray(R, np.float64).reshape(3, 3).T
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        hom = p @ P[:, :3].T + P[:, 3]
        S = min(H, W)
        xw = (W - S) / 2 + S * (hom[:, 0] / hom[:, 3] - x0) / (x1 - x0)
        yw = (H - S) / 2 + S * (hom[:, 1] / hom[:, 3] - y0) / (y1 - y0)
        d = p @ P[3, :3]
        valid = np.isfinite(p).all(1) & (hom[:, 3] > 0) & (np.abs(xw) <= WINDOW_LIMIT) & (np.abs(yw) <= WINDOW_LIMIT)
    return xw, yw, d, valid


def project(points, H, W, view, R=None):
    """The float64 statement of grnet_op_segments_setup: (xy (N,2) int64, SENTINEL in both for an invalid point; d (N) float64; valid (N))."""
    xw, yw, d, valid = window_coords(points, H, W, view, R)
    xy = np.full((len(d), 2), SENTINEL, np.int64)
    xy[valid, 0] = np.floor(xw[valid] * SUB + 0.5).astype(np.int64)
    xy[valid, 1] = np.floor(yw[valid] * SUB + 0.5).astype(np.int64)
    return xy, d, valid


def _fragments(xy, d, segments, widths, H, W, upper, offset):
    """Every fragment of one skeleton's segments, before the depth test: (pixel index in GL rows, depth float64, segment)."""
    xy, d = np.asarray(xy, np.int64), np.asarray(d, np.float64)
    seg = np.asarray(segments, np.int64).reshape(-1, 2)
    wid = np.asarray(widths, np.int64).reshape(-1)
    a, b = seg[:, 0], seg[:, 1]
    ids = np.arange(len(seg), dtype=np.int64)
    ok = (np.abs(xy[a]) <= rc.LIMIT).all(1) & (np.abs(xy[b]) <= rc.LIMIT).all(1)          # the sentinel is far below -LIMIT
    dx, dy = xy[b, 0] - xy[a, 0], xy[b, 1] - xy[a, 1]
    live = ok & ((dx != 0) | (dy != 0))
    a, b, ids, dx, dy, wid = a[live], b[live], ids[live], dx[live], dy[live], wid[live]
    xmaj = np.abs(dx) >= np.abs(dy)
    Pa, Pb = np.where(xmaj, xy[a, 0], xy[a, 1]), np.where(xmaj, xy[b, 0], xy[b, 1])
    Qa, Qb = np.where(xmaj, xy[a, 1], xy[a, 0]), np.where(xmaj, xy[b, 1], xy[b, 0])
    swap = Pb < Pa
    lo, hi = np.where(swap, b, a), np.where(swap, a, b)
    P0, P1, Q0, Q1 = np.where(swap, Pb, Pa), np.where(swap, Pa, Pb), np.where(swap, Qb, Qa), np.where(swap, Qa, Qb)
    n_major, n_minor = np.where(xmaj, W, H), np.where(xmaj, H, W)
    m0 = np.maximum(0, -((HALF - P0) // SUB))                            # the first m with 256 m + 128 >= P0
    last = (P1 - HALF) // SUB if upper == "closed" else -((HALF - P1) // SUB) - 1          # the last m with 256 m + 128 <= or < P1
    m1 = np.minimum(n_major - 1, last)
    count = np.maximum(0, m1 - m0 + 1)
    e = np.repeat(np.arange(len(a)), count)                              # the segment of each column
    m = m0[e] + (np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count))
    cP = m * SUB + HALF
    dP, dQ, w = (P1 - P0)[e], (Q1 - Q0)[e], wid[e]
    num = Q0[e] * dP + (cP - P0[e]) * dQ
    D = SUB * dP
    if offset == "gl":
        n0, cols = (num - (w - 1) * HALF * dP) // D, w
    elif offset == "up":                                                 # wrong: the half pixel of an even width rounded the other way
        n0, cols = (num - (w // 2) * SUB * dP) // D, w
    else:                                                                # wrong: "symmetric", n - w/2 .. n + w/2 about the 1-pixel line
        n0, cols = num // D - w // 2, 2 * (w // 2) + 1
    tt = (cP - P0[e]).astype(np.float64) / dP.astype(np.float64)
    zz = d[lo[e]] + tt * (d[hi[e]] - d[lo[e]])
    # a column of `cols` pixels each
    c = np.repeat(np.arange(len(e)), cols)
    n = n0[c] + (np.arange(cols.sum()) - np.repeat(np.cumsum(cols) - cols, cols))
    keep = (n >= 0) & (n < n_minor[e][c])
    i, j = np.where(xmaj[e][c], m[c], n), np.where(xmaj[e][c], n, m[c])
    return (j * W + i)[keep], zz[c][keep], ids[e][c][keep]


def _zbuffer(pix, zz, ids, H, W, tie):
    win = np.full(H * W, -1, np.int64)
    d1 = np.full(H * W, np.inf)
    d2 = np.full(H * W, np.inf)
    if len(pix):
        order = np.lexsort((ids if tie == "lower" else -ids, zz, pix))   # by pixel, then depth, then id
        pix, zz, ids = pix[order], zz[order], ids[order]
        first = np.r_[True, pix[1:] != pix[:-1]]
        start = np.nonzero(first)[0]
        group = np.cumsum(first) - 1
        win[pix[start]] = ids[start]
        d1[pix[start]] = zz[start]
        d2[pix[start]] = np.minimum.reduceat(np.where(zz > zz[start][group], zz, np.inf), start)
    return win, d1, d2


def rasterise_segments(xy, d, segments, widths, H, W, upper="open", offset="gl", tie="lower", buffers="shared"):
    """The z-buffer of ONE image over the skeletons aimed at it: xy (n,P,2) or (P,2) int64 snapped coordinates, d (n,P) or (P).  Returns winner
    (H,W) int64 in IMAGE rows: r S + s, -1 where uncovered; d1: the nearest depth; d2: the nearest depth STRICTLY greater than d1 (inf where there
    is none) -- equal depths are decided by the id rule and are no near-tie.  The wrong variants serve the discrimination tests only:
    upper="closed" also covers a centre exactly on P1; offset="up" rounds an even width's half pixel the other way; offset="symmetric" covers
    n - w/2 .. n + w/2; tie="higher" lets the later id win; buffers="per_skeleton" gives every skeleton a fresh depth buffer and paints later
    skeletons over earlier ones."""
    xy, d = np.asarray(xy, np.int64), np.asarray(d, np.float64)
    if xy.ndim == 2:
        xy, d = xy[None], d[None]
    S = len(np.asarray(segments).reshape(-1, 2))
    frags = [_fragments(xy[r], d[r], segments, widths, H, W, upper, offset) for r in range(len(xy))]
    if buffers == "shared":
        pix = np.concatenate([f[0] for f in frags]) if frags else np.zeros(0, np.int64)
        zz = np.concatenate([f[1] for f in frags]) if frags else np.zeros(0)
        ids = np.concatenate([f[2] + r * S for r, f in enumerate(frags)]) if frags else np.zeros(0, np.int64)
        win, d1, d2 = _zbuffer(pix, zz, ids, H, W, tie)
    else:
        win, d1, d2 = np.full(H * W, -1, np.int64), np.full(H * W, np.inf), np.full(H * W, np.inf)
        for r, (pix, zz, ids) in enumerate(frags):
            w, a, b = _zbuffer(pix, zz, ids + r * S, H, W, tie)
            on = w >= 0
            win[on], d1[on], d2[on] = w[on], a[on], b[on]
    flip = lambda v: v.reshape(H, W)[::-1].copy()
    return flip(win), flip(d1), flip(d2)


def compose(image, winner, colours):
    """image (H,W,3) uint8, winner from rasterise_segments, colours (S,3) uint8 in the image's memory order -> the image with every covered
    pixel in its segment's colour (segment = id modulo S), every other byte as it was."""
    colours = np.asarray(colours, np.uint8).reshape(-1, 3)
    out = np.array(image, np.uint8, copy=True)
    on = winner >= 0
    out[on] = colours[winner[on] % len(colours)]
    return out


# ----------------------------------------------------------------------------- scenes
def _scene(pts, segments, widths, H, W, d=None):
    """pts: window positions in pixels (x, y) in GL rows, snapped here; d per point (default 0.25)."""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    xy = np.floor(pts * SUB + 0.5).astype(np.int64)
    seg = np.asarray(segments, np.int64).reshape(-1, 2)
    wid = np.broadcast_to(np.asarray(widths, np.int64), (len(seg),)).copy()
    dd = np.full(len(pts), 0.25) if d is None else np.asarray(d, np.float64)
    return dict(xy=xy, d=dd.astype(np.float32).astype(np.float64), segments=seg, widths=wid, H=int(H), W=int(W))


def spin_points(key):
    """The seeded 49 joints of the SPIN-bone scenes."""
    g = np.random.Generator(np.random.Philox(key=list(key)))
    return (g.standard_normal((49, 3)) * (0.2, 0.3, 0.3)).astype(np.float32)


def _bones_scene(key, H, W, width, bones):
    return dict(points=spin_points(key), segments=np.asarray(bones, np.int64), widths=np.full(len(bones), width, np.int64), H=H, W=W)


def scenes(bones):
    """name -> scene: either snapped points (xy, d) or world points (points) that go through the setup first.  bones: the SPIN bone table."""
    out = {}
    W, H = 64, 48
    for name, (a, b) in dict(horizontal=((5.5, 20.5), (50.5, 20.5)), vertical=((30.25, 4.5), (30.25, 40.5)), diagonal=((10.5, 5.5), (45.5, 40.5)),
                             antidiagonal=((10.5, 40.5), (45.5, 5.5)), slanted=((3.2, 7.9), (58.7, 31.1))).items():
        out[name + "_fwd"] = _scene([a, b], [(0, 1)], 3, H, W, d=[0.1, 0.7])
        out[name + "_back"] = _scene([a, b], [(1, 0)], 3, H, W, d=[0.1, 0.7])
    out["zero_length"] = _scene([(10.5, 10.5), (10.5, 10.5), (20.0, 20.0), (30.0, 21.0)], [(0, 1), (2, 2), (2, 3)], 2, H, W)
    out["ends_on_centres"] = _scene([(4.5, 9.5), (20.5, 13.5), (40.5, 8.5), (40.5, 30.5)], [(0, 1), (2, 3)], [1, 2], H, W)
    out["through_image"] = _scene([(-300.0, 10.0), (500.0, 40.0), (20.0, -200.0), (45.0, 700.0), (-50.0, -40.0), (90.0, 100.0)], [(0, 1), (2, 3), (4, 5)], [2, 3, 1], H, W)
    out["wholly_outside"] = _scene([(-30.0, 10.0), (-5.0, 40.0), (10.0, 60.0), (50.0, 52.0), (70.0, 5.0), (66.0, 40.0), (5.0, -9.0), (60.0, -9.5)],
                                   [(0, 1), (2, 3), (4, 5), (6, 7)], [1, 2, 3, 2], H, W)
    out["widths_1_2_3_16"] = _scene([(3.3, 2.2), (60.1, 9.7), (3.3, 8.2), (60.1, 15.7), (3.3, 15.2), (60.1, 22.7), (3.3, 30.2), (60.1, 37.7),
                                     (5.2, 3.0), (9.9, 45.0), (14.2, 3.0), (18.9, 45.0)], [(0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, 11)], [1, 2, 3, 16, 2, 16], H, W,
                                    d=[0.5, 0.5, 0.4, 0.4, 0.3, 0.3, 0.2, 0.2, 0.6, 0.6, 0.1, 0.1])
    out["wide_at_edges"] = _scene([(-5.0, 2.3), (70.0, 3.1), (61.7, -4.0), (62.4, 55.0), (2.0, 46.9), (60.0, 44.0), (1.1, 3.0), (2.9, 44.0)],
                                  [(0, 1), (2, 3), (4, 5), (6, 7)], 16, H, W, d=[0.1, 0.1, 0.2, 0.2, 0.3, 0.3, 0.4, 0.4])
    out["crossing_gap"] = _scene([(5.0, 5.0), (58.0, 42.0), (6.0, 41.0), (57.0, 7.0)], [(0, 1), (2, 3)], 5, H, W, d=[0.4, 0.4, 0.3, 0.3])
    out["crossing_gap_swapped"] = _scene([(5.0, 5.0), (58.0, 42.0), (6.0, 41.0), (57.0, 7.0)], [(2, 3), (0, 1)], 5, H, W, d=[0.4, 0.4, 0.3, 0.3])
    out["coincident_equal_depth"] = _scene([(4.0, 6.0), (55.0, 33.0), (4.0, 6.0), (55.0, 33.0), (8.0, 40.0), (50.0, 4.0)], [(0, 1), (3, 2), (4, 5)], [3, 3, 2], H, W)
    out["one_pixel_1x1"] = _scene([(-3.0, 0.2), (4.0, 0.9), (0.5, -2.0), (0.5, 5.0)], [(0, 1), (2, 3)], [1, 16], 1, 1, d=[0.5, 0.5, 0.2, 0.2])
    out["slanted_7x5"] = _scene([(0.4, 0.3), (6.8, 4.1), (6.5, 0.5), (0.5, 4.5)], [(0, 1), (2, 3)], [2, 1], 5, 7, d=[0.2, 0.6, 0.5, 0.1])
    W, H = 97, 61
    out["long_97x61"] = _scene([(-2.0, 3.3), (99.0, 57.7), (48.2, -3.0), (50.9, 70.0), (0.5, 30.5), (96.5, 30.5)], [(0, 1), (2, 3), (4, 5)], [2, 5, 1], H, W,
                               d=[0.1, 0.9, 0.5, 0.5, 0.9, 0.1])
    out["spin_k0_64x48_w2"] = _bones_scene((0, 7), 48, 64, 2, bones)
    out["spin_k2_64x48_w1"] = _bones_scene((2, 7), 48, 64, 1, bones)
    out["spin_k0_97x61_w5"] = _bones_scene((0, 7), 61, 97, 5, bones)
    out["spin_k2_97x61_w3"] = _bones_scene((2, 7), 61, 97, 3, bones)
    out["spin_k1_97x61_w2"] = _bones_scene((1, 7), 61, 97, 2, bones)
    return out


COVER_ONLY = ("spin_k1_97x61_w2",)            # 1-2 near-ties among a few hundred pixels: over the cap, so coverage only


def winner_scenes(bones):
    return {k: v for k, v in scenes(bones).items() if k not in COVER_ONLY}


def scene_1080p(bones):
    """Four seeded skeletons as ONE point array of 4 x 49 points and 4 x 27 segments of width 13 (so the single-skeleton hook draws them into one
    depth buffer), spread over the panel."""
    bones = np.asarray(bones, np.int64)
    shift = np.array([(0.0, -0.45, 0.0), (0.0, -0.15, 0.1), (0.0, 0.15, -0.1), (0.0, 0.45, 0.0)])
    pts = np.concatenate([spin_points((k, 7)) + shift[k] for k in range(4)]).astype(np.float32)
    seg = np.concatenate([bones + 49 * k for k in range(4)])
    return dict(points=pts, segments=seg, widths=np.full(len(seg), 13, np.int64), H=1080, W=1920)


def resolve(scene, view):
    """(xy, d) of a scene by the float64 rules: what the CPU tests rasterise."""
    if "xy" in scene:
        return scene["xy"], scene["d"]
    xy, d, _ = project(scene["points"], scene["H"], scene["W"], view)
    return xy, d


def placed_skeleton(key, place):
    """The seeded joints of key (key, 7) moved to one of 5 places across the panel (place 2: the middle)."""
    return (spin_points((key, 7)) + np.array([0.0, (place - 2) * 0.22, 0.0])).astype(np.float32)


def many_images(n_images=24, per_image=5):
    """(points (n,49,3), image_index (n)): per_image skeletons side by side in each of n_images images -- more images than a launch group holds,
    and more skeletons in the first group than one launch takes -- listed image by image."""
    pts = np.stack([placed_skeleton((per_image * f + j) % 60, j) for f in range(n_images) for j in range(per_image)])
    return pts, np.repeat(np.arange(n_images), per_image)


def many_points(n_first=70, n_second=3, P=1024):
    """(points (n,P,3), image_index (n), segments (2,2), widths): skeletons of P points of which two short segments are drawn, n_first aimed at
    image 0 -- more points than the workspace holds at a time -- and n_second at image 1."""
    g = np.random.Generator(np.random.Philox(key=[5, 7]))
    n = n_first + n_second
    pts = (g.uniform(-1, 1, (n, P, 3)) * (0.5, 0.9, 0.9)).astype(np.float32)
    for a, b in ((0, P - 1), (P // 2 - 1, P // 2)):                      # the drawn pairs: short, so that the picture stays sparse
        pts[:, b] = pts[:, a] + (g.uniform(-1, 1, (n, 3)) * 0.12).astype(np.float32)
    return pts, np.r_[np.zeros(n_first, np.int64), np.ones(n_second, np.int64)], np.array([(0, P - 1), (P // 2 - 1, P // 2)], np.int64), np.array([2, 1], np.int64)
