"""The build's own specification of rag.clearance / rag.sample_points (csrc/dm_points.hip), in numpy.

The reference reads sample points and their `inner` / `object` window fields from a point shapefile written by external GIS
software and never defines them; this is the rule the build uses instead.  Everything is integer arithmetic, so the kernels must
equal this file bit for bit.

Input: labels int32 [H,W] (H*W < 2^31), S superpixel ids 0..S-1, k >= 1, max_window (default 384).  Ids outside [0,S) are never
sampled, but they are "another label" for their neighbours (raw ids are compared).

Clearance.  c(p) = Chebyshev distance from p to the nearest pixel that carries a different id or lies outside the raster, capped
at cap = (max_window + 1) // 2.  c >= 1, and the largest odd square centred on p inside p's superpixel has side 2c - 1.
`clearance_at` states it by brute force; `clearance` computes it for a whole raster through the identity "c - 1 = chessboard
distance to the nearest pixel that has an 8-neighbour of another id or sits on the raster edge" (tests/test_points_host.py
checks the identity against the brute force).

Points.  Superpixel s gets min(k, area(s)) points in rounds j = 0..k-1: round j takes the pixel of s that maximises
score_j(p) = min(c(p), Chebyshev distance from p to every point already chosen for s); ties go to the smallest linear index
y*W + x; a round yields a point only if its best score is >= 1 (chosen pixels score 0: no duplicates).  With the key
(score << 32) | (0xFFFFFFFF - linear) a round is one unsigned 64-bit max per superpixel.

Windows.  inner = 2 c(p) - 1; side = max(bbox width, bbox height) of s; obj = min(side, (max_window + 2 inner) // 3).
Then inner <= obj and 3 obj - 2 inner <= max_window.

Order.  Points sorted by (superpixel, round); ptr = exclusive scan of the counts; idx = arange(P).
"""
import numpy as np

MAX_WINDOW = 384
INT_MAX = 2 ** 31 - 1


def cap_of(max_window=MAX_WINDOW):
    return (max_window + 1) // 2


def clearance_at(labels, y, x, max_window=MAX_WINDOW):
    """The definition, for one pixel: grow the square until it meets another id or leaves the raster."""
    H, W = labels.shape
    cap = cap_of(max_window)
    for m in range(1, cap):
        if y - m < 0 or x - m < 0 or y + m >= H or x + m >= W:
            return m
        if (labels[y - m:y + m + 1, x - m:x + m + 1] != labels[y, x]).any():
            return m
    return cap


def clearance_brute(labels, max_window=MAX_WINDOW):
    H, W = labels.shape
    return np.array([[clearance_at(labels, y, x, max_window) for x in range(W)] for y in range(H)], np.uint16).reshape(H, W)


def boundary_pixels(labels):
    """True where a pixel has an 8-neighbour with another id or sits on the raster edge."""
    H, W = labels.shape
    lab = labels.astype(np.int64)
    pad = np.full((H + 2, W + 2), np.int64(1) << 40)             # no int32 id: the outside is "another label"
    pad[1:-1, 1:-1] = lab
    b = np.zeros((H, W), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            b |= pad[dy:dy + H, dx:dx + W] != lab
    return b


def clearance(labels, max_window=MAX_WINDOW):
    """uint16 [H,W] through the 8-neighbour-boundary identity: 1 + chessboard distance to the nearest boundary pixel, capped."""
    H, W = labels.shape
    cap = cap_of(max_window)
    reached = boundary_pixels(labels)
    c = np.full((H, W), cap, np.uint16)
    c[reached] = 1
    for d in range(1, cap - 1):                                   # distance d <-> clearance d + 1 <= cap - 1
        if reached.all():
            break
        pad = np.zeros((H + 2, W + 2), bool)
        pad[1:-1, 1:-1] = reached
        grown = np.zeros((H, W), bool)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                grown |= pad[dy:dy + H, dx:dx + W]
        c[grown & ~reached] = d + 1
        reached = grown
    return c


def sample_points(labels, S, k=3, max_window=MAX_WINDOW, clr=None):
    """dict: xy int32 [P,2] (x, y), label, inner, obj, round int32 [P], ptr int32 [S+1], idx int32 [P], bbox int32 [S,4],
    clearance uint16 [H,W]."""
    H, W = labels.shape
    assert H * W < 2 ** 31 and S >= 1 and k >= 1
    c = clearance(labels, max_window) if clr is None else clr
    lab = labels.reshape(-1).astype(np.int64)
    lin = np.arange(H * W, dtype=np.int64)
    ys, xs = lin // W, lin % W
    valid = (lab >= 0) & (lab < S)
    vl, vy, vx, vlin = lab[valid], ys[valid], xs[valid], lin[valid]
    bbox = np.empty((S, 4), np.int64)
    bbox[:, :2], bbox[:, 2:] = INT_MAX, -1
    np.minimum.at(bbox[:, 0], vl, vx); np.minimum.at(bbox[:, 1], vl, vy)
    np.maximum.at(bbox[:, 2], vl, vx); np.maximum.at(bbox[:, 3], vl, vy)
    score = c.reshape(-1).astype(np.int64)[valid]
    rows = []                                                     # (s, round, x, y, clearance at the point)
    for j in range(k):
        key = (score.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - vlin.astype(np.uint64))
        best = np.zeros(S, np.uint64)
        live = score >= 1
        np.maximum.at(best, vl[live], key[live])
        got = np.nonzero(best)[0]
        if got.size == 0:
            break
        plin = (np.uint64(0xFFFFFFFF) - (best[got] & np.uint64(0xFFFFFFFF))).astype(np.int64)
        py, px = plin // W, plin % W
        rows.append(np.stack((got, np.full(got.size, j), px, py, c.reshape(-1)[plin].astype(np.int64)), 1))
        at_x, at_y = np.full(S, -1, np.int64), np.full(S, -1, np.int64)
        at_x[got], at_y[got] = px, py
        has = at_x[vl] >= 0
        d = np.maximum(np.abs(vx - at_x[vl]), np.abs(vy - at_y[vl]))
        score = np.where(has, np.minimum(score, d), score)
    t = np.concatenate(rows) if rows else np.zeros((0, 5), np.int64)
    t = t[np.lexsort((t[:, 1], t[:, 0]))]
    counts = np.bincount(t[:, 0], minlength=S)
    ptr = np.zeros(S + 1, np.int64)
    ptr[1:] = np.cumsum(counts)
    inner = 2 * t[:, 4] - 1
    side = np.maximum(bbox[t[:, 0], 2] - bbox[t[:, 0], 0], bbox[t[:, 0], 3] - bbox[t[:, 0], 1]) + 1
    obj = np.minimum(side, (max_window + 2 * inner) // 3)
    i32 = np.int32
    return {"xy": np.ascontiguousarray(t[:, 2:4]).astype(i32), "label": t[:, 0].astype(i32), "inner": inner.astype(i32), "obj": obj.astype(i32),
            "round": t[:, 1].astype(i32), "ptr": ptr.astype(i32), "idx": np.arange(t.shape[0], dtype=i32), "bbox": bbox.astype(i32),
            "clearance": c}


def voronoi_labels(H, W, cell, seed):
    """Jittered-grid Voronoi labels (the geometry of workload.voronoi_raster): superpixel ny * gx + nx grows from grid cell (ny, nx)."""
    rng = np.random.default_rng(seed)
    gy, gx = (H + cell - 1) // cell, (W + cell - 1) // cell
    cy = (np.arange(gy)[:, None] + rng.uniform(0.2, 0.8, (gy, gx))) * cell
    cx = (np.arange(gx)[None, :] + rng.uniform(0.2, 0.8, (gy, gx))) * cell
    yy, xx = np.mgrid[0:H, 0:W]
    best = np.full((H, W), np.inf, dtype=np.float32)
    lab = np.zeros((H, W), np.int32)
    by, bx = yy // cell, xx // cell
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ny, nx = np.clip(by + dy, 0, gy - 1), np.clip(bx + dx, 0, gx - 1)
            d = ((yy - cy[ny, nx]) ** 2 + (xx - cx[ny, nx]) ** 2).astype(np.float32)
            upd = d < best
            best[upd] = d[upd]
            lab[upd] = (ny * gx + nx)[upd]
    return lab, gy * gx
