"""The build's own specification of rag.slic / rag.connected_labels (csrc/dm_slic.hip), in numpy.

The reference reads its over-segmentation from shapefiles written by external GIS software and never defines it; this is the rule
the build uses instead.  Everything is integer arithmetic and nothing depends on an order of evaluation, so the kernels must equal
this file bit for bit.  Pure numpy (tests/test_slic_host.py compares the component labelling with scipy where scipy exists).

Input: tile uint8 [bands,H,W] (the first nb = min(bands, 4) bands are used), H*W < 2^31, cell in 4..256, compactness in 0..255,
iters >= 0, min_size >= 1 (default max(1, cell*cell // 4)).

1. Centres.  gy = ceil(H / cell), gx = ceil(W / cell), K = gy*gx.  Centre c = j*gx + i starts at y = min(H-1, j*cell + cell//2),
   x = min(W-1, i*cell + cell//2), with the colour of the pixel there.
2. Assignment.  Pixel (y, x) of grid cell (j, i) = (y // cell, x // cell) considers the up to 9 centres of the grid cells
   (j+dj, i+di), dj, di in -1..1, inside the grid, and takes the one with the smallest
   D = cell^2 * sum_b (p_b - c_b)^2 + compactness^2 * ((y - c_y)^2 + (x - c_x)^2); ties go to the smaller centre id.
3. Update.  A centre with n >= 1 pixels becomes the rounded mean (2 sum + n) // (2 n) of their y, x and every band; a centre with
   none stays.  Sequence: assignment, then iters times (update, assignment).
4. Components.  4-connected components of equal label, numbered 0..n-1 by first pixel in raster-scan order.
5. Absorption, in rounds.  With areas and shared boundary lengths (pixel edges) as at the start of the round, every region with
   area < min_size that has a neighbour picks the neighbour with the longest shared boundary, ties to the smaller id; the picks are
   united (regions = connected components of the pick graph) and renumbered by first pixel; until no region picks.
6. Result: labels int32 [H,W] with ids 0..n-1, and n.
"""
import numpy as np


def default_min_size(cell):
    return max(1, cell * cell // 4)


# ---- union-find over index pairs, smallest index as the representative ---------------------------------------------------------
def _unite(n, a, b):
    """root int64 [n]: the smallest member of every connected component of the graph with edges (a[k], b[k])."""
    parent = np.arange(n, dtype=np.int64)
    while a.size:
        pa, pb = parent[a], parent[b]
        diff = pa != pb
        if not diff.any():
            break
        a, b, pa, pb = a[diff], b[diff], pa[diff], pb[diff]
        np.minimum.at(parent, np.maximum(pa, pb), np.minimum(pa, pb))
        while True:                                               # full compression: parents only point downwards
            pp = parent[parent]
            if (pp == parent).all():
                break
            parent = pp
    return parent


def connected_labels(raster, background=None):
    """(labels int32 [H,W], n): 4-connected components of equal values, numbered by first pixel in raster-scan order; pixels equal
    to `background` get -1 and belong to no component."""
    r = np.asarray(raster)
    H, W = r.shape
    lin = np.arange(H * W, dtype=np.int64).reshape(H, W)
    live = np.ones((H, W), bool) if background is None else r != background
    hz = (r[:, 1:] == r[:, :-1]) & live[:, 1:]
    vt = (r[1:, :] == r[:-1, :]) & live[1:, :]
    a = np.concatenate((lin[:, 1:][hz], lin[1:, :][vt]))
    b = np.concatenate((lin[:, :-1][hz], lin[:-1, :][vt]))
    root = _unite(H * W, a, b)
    is_root = (root == lin.reshape(-1)) & live.reshape(-1)        # the root is the component's first pixel
    dense = np.cumsum(is_root) - 1
    out = np.where(live.reshape(-1), dense[root], -1)
    return out.astype(np.int32).reshape(H, W), int(is_root.sum())


# ---- steps 1-3 -----------------------------------------------------------------------------------------------------------------
def initial_centres(tile, cell):
    """int64 [K,6] = y, x, band 0..3 (unused bands 0), and (gy, gx)."""
    bands, H, W = tile.shape
    nb = min(bands, 4)
    gy, gx = -(-H // cell), -(-W // cell)
    y = np.minimum(H - 1, np.arange(gy) * cell + cell // 2)
    x = np.minimum(W - 1, np.arange(gx) * cell + cell // 2)
    c = np.zeros((gy * gx, 6), np.int64)
    c[:, 0] = np.repeat(y, gx)
    c[:, 1] = np.tile(x, gy)
    c[:, 2:2 + nb] = tile[:nb][:, c[:, 0], c[:, 1]].T
    return c, (gy, gx)


def assign(tile, centres, cell, compactness, grid):
    """int64 [H,W]: the centre id every pixel takes (step 2).  D is evaluated in Python-width integers via uint64: it stays below
    256^2 * (4 * 255^2 + 18 * 255^2) < 2^37."""
    bands, H, W = tile.shape
    nb = min(bands, 4)
    gy, gx = grid
    px = tile[:nb].astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    jj, ii = yy // cell, xx // cell
    best = np.full((H, W), np.iinfo(np.int64).max, np.int64)
    lab = np.full((H, W), -1, np.int64)
    for dj in (-1, 0, 1):                                         # ascending centre id: a strict "<" keeps the smaller id on ties
        for di in (-1, 0, 1):
            cj, ci = jj + dj, ii + di
            ok = (cj >= 0) & (cj < gy) & (ci >= 0) & (ci < gx)
            c = np.where(ok, cj * gx + ci, 0)
            dc = sum((px[b] - centres[c, 2 + b]) ** 2 for b in range(nb))
            d = cell * cell * dc + compactness * compactness * ((yy - centres[c, 0]) ** 2 + (xx - centres[c, 1]) ** 2)
            upd = ok & (d < best)
            best[upd] = d[upd]
            lab[upd] = c[upd]
    return lab


def update(tile, lab, centres):
    """Step 3: the rounded means; centres without pixels stay."""
    bands, H, W = tile.shape
    nb = min(bands, 4)
    K = centres.shape[0]
    flat = lab.reshape(-1)
    n = np.bincount(flat, minlength=K).astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    cols = [yy.reshape(-1), xx.reshape(-1)] + [tile[b].reshape(-1) for b in range(nb)]
    out = centres.copy()
    has = n > 0
    for k, v in enumerate(cols):
        s = np.zeros(K, np.int64)
        np.add.at(s, flat, v.astype(np.int64))
        out[has, k] = (2 * s[has] + n[has]) // (2 * n[has])
    return out


def iterate(tile, cell, compactness=10, iters=10):
    """Steps 1-3: (centre id of every pixel int64 [H,W], final centres int64 [K,6])."""
    centres, grid = initial_centres(tile, cell)
    lab = assign(tile, centres, cell, compactness, grid)
    for _ in range(iters):
        centres = update(tile, lab, centres)
        lab = assign(tile, centres, cell, compactness, grid)
    return lab, centres


# ---- step 5 --------------------------------------------------------------------------------------------------------------------
def region_edges(labels, n):
    """(a, b, w): unique unordered 4-neighbour label pairs a < b with the number of shared pixel edges, sorted by (a, b)."""
    lab = labels.astype(np.int64)
    p = np.concatenate((lab[:, 1:].reshape(-1), lab[1:, :].reshape(-1)))
    q = np.concatenate((lab[:, :-1].reshape(-1), lab[:-1, :].reshape(-1)))
    d = p != q
    keys, w = np.unique(np.minimum(p[d], q[d]) * n + np.maximum(p[d], q[d]), return_counts=True)
    return keys // n, keys % n, w.astype(np.int64)


def absorb_round(labels, n, min_size):
    """One round of step 5: (labels, n, number of picks)."""
    area = np.bincount(labels.reshape(-1), minlength=n)
    a, b, w = region_edges(labels, n)
    src, dst, ww = np.concatenate((a, b)), np.concatenate((b, a)), np.concatenate((w, w))
    small = area[src] < min_size
    src, dst, ww = src[small], dst[small], ww[small]
    if src.size == 0:
        return labels, n, 0
    best = np.zeros(n, np.uint64)
    np.maximum.at(best, src, (ww.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - dst.astype(np.uint64)))
    who = np.nonzero(best)[0]
    pick = (np.uint64(0xFFFFFFFF) - (best[who] & np.uint64(0xFFFFFFFF))).astype(np.int64)
    root = _unite(n, who, pick)
    is_root = root == np.arange(n)
    dense = np.cumsum(is_root) - 1                                # a united region's first pixel is that of its smallest member
    return dense[root][labels].astype(np.int32), int(is_root.sum()), int(who.size)


def absorb(labels, n, min_size):
    """Step 5: (labels, n, rounds applied)."""
    rounds = 0
    while True:
        labels, n, picks = absorb_round(labels, n, min_size)
        if picks == 0:
            return labels, n, rounds
        rounds += 1


def slic(tile, cell=29, compactness=10, iters=10, min_size=None, return_rounds=False):
    """(labels int32 [H,W], n_labels)."""
    tile = np.asarray(tile)
    assert tile.dtype == np.uint8 and tile.ndim == 3 and tile.shape[1] * tile.shape[2] < 2 ** 31
    assert 4 <= cell <= 256 and 0 <= compactness <= 255 and iters >= 0
    min_size = default_min_size(cell) if min_size is None else min_size
    assert min_size >= 1
    lab, _ = iterate(tile, cell, compactness, iters)
    labels, n = connected_labels(lab)
    labels, n, rounds = absorb(labels, n, min_size)
    return (labels, n, rounds) if return_rounds else (labels, n)


# ---- test images ---------------------------------------------------------------------------------------------------------------
def block_image(bands, H, W, block, seed, noise=8):
    """Piecewise-constant blocks of side `block` with uniform noise of +-noise, uint8 [bands,H,W]."""
    rng = np.random.default_rng(seed)
    by, bx = -(-H // block), -(-W // block)
    base = rng.integers(noise, 256 - noise, (bands, by, bx))
    img = np.repeat(np.repeat(base, block, 1), block, 2)[:, :H, :W]
    return (img + rng.integers(-noise, noise + 1, (bands, H, W))).astype(np.uint8)


def noise_image(bands, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (bands, H, W), dtype=np.uint8)


def serpentine(H, W, gap=2):
    """A one-pixel-wide path (value 1 on 0) that runs along every `gap`-th row and turns at alternating ends."""
    r = np.zeros((H, W), np.int32)
    for k, y in enumerate(range(0, H, gap)):
        r[y, :] = 1
        if y + gap < H:
            r[y:y + gap, W - 1 if k % 2 == 0 else 0] = 1
    return r
