"""Spec (numpy, integers only) of rag.rasterize: closed polygon rings into a label raster, in two independent formulations.

The rule (include/deepmerge_hip.h and DESIGN.md 3.5.6 restate it):
  pixel-corner space, x right, y down; pixel (c, r) covers [c, c+1] x [r, r+1], its centre is (c + 1/2, r + 1/2).
  a float64 coordinate v becomes the fixed-point q = floor(256 v + 0.5).
  a ring is closed (the last vertex joins the first).  An edge with y0 == y1 contributes nothing; otherwise its ends are swapped so
  that y0 < y1, dy = y1 - y0, and it crosses pixel row r iff y0 <= Yc < y1 with Yc = 256 r + 128.  There num = x0 dy + (Yc - y0)
  (x1 - x0), the crossing is at X = num / dy, and the event's column is cx = ceil((num - 128 dy) / (256 dy)) clamped to [0, W]: the
  first column whose centre 256 c + 128 is not left of X.
  pixel (c, r) belongs to label l iff the number of events of all rings of l in row r with cx <= c is odd; a pixel inside several
  labels gets the greatest, a pixel inside none gets `fill`.
`rasterize` follows the events (ceiling division, a toggle per event, a running XOR along x).  `inside` asks every edge about every
pixel centre with the division-free comparison num <= Xc dy.  They share the row test and nothing else.
"""
from __future__ import annotations

import numpy as np

SUBPIXEL = 256
HALF = SUBPIXEL // 2


def quantise(v) -> np.ndarray:
    return np.floor(np.asarray(v, np.float64) * SUBPIXEL + 0.5).astype(np.int64)


def _ceil_div(a, b):
    return -((-a) // b)                                         # floor division rounds down for negatives too: exact


def edge_events(x0, y0, x1, y1, H, W):
    """(rows, cx) int64 arrays: the events of one fixed-point edge."""
    x0, y0, x1, y1 = int(x0), int(y0), int(x1), int(y1)
    none = np.zeros(0, np.int64)
    if y0 == y1:
        return none, none
    if y0 > y1:
        x0, y0, x1, y1 = x1, y1, x0, y0
    dy = y1 - y0
    rows = np.arange(H, dtype=np.int64)
    yc = SUBPIXEL * rows + HALF
    hit = (y0 <= yc) & (yc < y1)
    rows, yc = rows[hit], yc[hit]
    num = x0 * dy + (yc - y0) * (x1 - x0)
    assert abs(x0 * dy) < 1 << 60 and (np.abs(num) < 1 << 60).all()
    cx = np.clip(_ceil_div(num - HALF * dy, SUBPIXEL * dy), 0, W)
    return rows, cx


def _rings(ring_ptr, xy_fixed, ring_label):
    ring_ptr, xy = np.asarray(ring_ptr, np.int64), np.asarray(xy_fixed, np.int64).reshape(-1, 2)
    for r, l in enumerate(np.asarray(ring_label)):
        yield int(l), xy[ring_ptr[r]:ring_ptr[r + 1]]


def rasterize(ring_ptr, xy_fixed, ring_label, H, W, fill=-1) -> np.ndarray:
    """int32 [H,W] from fixed-point rings: the spec."""
    acc = {}
    for l, p in _rings(ring_ptr, xy_fixed, ring_label):
        a = acc.setdefault(l, np.zeros((H, W + 1), bool))
        for (x0, y0), (x1, y1) in zip(p, np.roll(p, -1, 0)):
            rows, cx = edge_events(x0, y0, x1, y1, H, W)
            a[rows, cx] ^= True                                  # an edge has one event per row
    out = np.full((H, W), fill, np.int32)
    for l in sorted(acc):                                       # ascending: the greatest label wins
        out[np.logical_xor.accumulate(acc[l], axis=1)[:, :W]] = l
    return out


def inside(Xc, Yc, ring) -> np.ndarray:
    """bool, the shape of Xc / Yc: is the fixed-point position (Xc, Yc) inside the ring (even-odd)?  Division-free: an edge counts
    iff y0 <= Yc < y1 and num <= Xc dy."""
    Xc, Yc = np.asarray(Xc, np.int64), np.asarray(Yc, np.int64)
    odd = np.zeros(np.broadcast(Xc, Yc).shape, bool)
    p = np.asarray(ring, np.int64).reshape(-1, 2)
    for (x0, y0), (x1, y1) in zip(p.tolist(), np.roll(p, -1, 0).tolist()):
        if y0 == y1:
            continue
        if y0 > y1:
            x0, y0, x1, y1 = x1, y1, x0, y0
        dy = y1 - y0
        odd ^= (y0 <= Yc) & (Yc < y1) & (x0 * dy + (Yc - y0) * (x1 - x0) <= Xc * dy)
    return odd


def rasterize_by_predicate(ring_ptr, xy_fixed, ring_label, H, W, fill=-1) -> np.ndarray:
    """The same raster from `inside` at every pixel centre."""
    Yc, Xc = np.meshgrid(SUBPIXEL * np.arange(H, dtype=np.int64) + HALF, SUBPIXEL * np.arange(W, dtype=np.int64) + HALF, indexing="ij")
    odd = {}
    for l, p in _rings(ring_ptr, xy_fixed, ring_label):
        odd[l] = odd.get(l, False) ^ inside(Xc, Yc, p)
    out = np.full((H, W), fill, np.int32)
    for l in sorted(odd):
        out[odd[l]] = l
    return out


def claims(ring_ptr, xy_fixed, ring_label, H, W) -> np.ndarray:
    """int [H,W]: how many labels claim every pixel."""
    n = np.zeros((H, W), np.int64)
    for l in np.unique(np.asarray(ring_label)):
        mine = [p for m, p in _rings(ring_ptr, xy_fixed, ring_label) if m == l]
        ptr = np.cumsum([0] + [len(p) for p in mine])
        n += rasterize(ptr, np.concatenate(mine), np.zeros(len(mine), np.int32), H, W) == 0
    return n


# ---- the general-polygon fixtures -------------------------------------------------------------------------------------------------------
def pack(polys):
    """[(label, [(x, y), ...]), ...] -> (ring_ptr int64 [R+1], xy float64 [V,2], ring_label int32 [R])."""
    ptr = np.cumsum([0] + [len(p) for _, p in polys]).astype(np.int64)
    xy = np.asarray([v for _, p in polys for v in p], np.float64).reshape(-1, 2)
    return ptr, xy, np.asarray([l for l, _ in polys], np.int32)


def _square(x0, y0, x1, y1, reverse=False):
    p = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    return p[::-1] if reverse else p


def random_polygons(n=300, H=150, W=170, seed=7, n_labels=100):
    """Triangles and quads on the 1/256 grid, about a third of their vertices outside the raster; the rings of a label are scattered."""
    rng = np.random.default_rng(seed)
    polys = []
    for _ in range(n):
        k = int(rng.integers(3, 5))
        centre = rng.uniform((-0.1 * W, -0.1 * H), (1.1 * W, 1.1 * H))
        v = centre + rng.uniform(-12.0, 12.0, (k, 2))
        polys.append((int(rng.integers(0, n_labels)), [tuple(c) for c in np.round(v * SUBPIXEL) / SUBPIXEL]))
    return polys


def cases():
    """name -> (rings = (ring_ptr, xy float64, ring_label), H, W)."""
    star = [(10 + 9 * np.sin(2 * np.pi * 2 * k / 5), 10 - 9 * np.cos(2 * np.pi * 2 * k / 5)) for k in range(5)]
    sq = _square(2, 3, 9, 8)
    sliver = [(0.3, -1.0), (5.6, 701.0), (0.9, 350.0)]
    out = {
        "fractional_triangle": ([(0, [(1.3, 0.7), (9.6, 2.2), (4.1, 8.9)])], 10, 12),
        "pentagram": ([(0, star)], 20, 20),
        "hole_same_orientation": ([(2, _square(1, 1, 11, 11)), (2, _square(4, 4, 8, 8))], 12, 13),
        "hole_opposite_orientation": ([(2, _square(1, 1, 11, 11)), (2, _square(4, 4, 8, 8, reverse=True))], 12, 13),
        "half_outside": ([(0, [(-5.5, -3.25), (6.5, 4.0), (3.0, 20.5)]), (1, [(7.0, 9.0), (25.5, 2.0), (30.0, 18.0)])], 12, 10),
        "entirely_outside": ([(0, [(-10.0, -10.0), (-2.0, -9.0), (-5.0, -1.0)]), (1, [(13.0, 2.0), (19.0, 3.0), (15.0, 8.0)]),
                              (2, [(2.0, 14.5), (8.0, 15.0), (4.0, 30.0)])], 12, 10),
        "vertex_on_centre_row": ([(0, [(5.5, 0.5), (9.25, 4.5), (5.5, 8.5), (1.25, 4.5)])], 10, 11),
        "horizontal_edge_on_centre_row": ([(0, _square(1, 2.5, 7, 6.5))], 9, 9),
        "diagonal_through_centres": ([(0, [(0.5, 0.5), (8.5, 8.5), (0.5, 8.5)]), (1, [(0.5, 0.5), (8.5, 0.5), (8.5, 8.5)])], 9, 9),
        "degenerate_rings": ([(0, []), (1, [(3.0, 3.0)]), (2, [(1.0, 1.0), (6.0, 5.0)]), (3, [(1.0, 1.0), (5.0, 3.0), (9.0, 5.0)]),
                              (4, [(1.0, 6.0), (4.0, 1.0), (7.0, 6.0), (4.0, 1.0)]), (0, []), (5, _square(6, 5, 9, 8))], 9, 10),
        "only_degenerate_rings": ([(0, []), (1, [(3.0, 3.0)]), (2, [(1.0, 1.0), (6.0, 5.0)]), (3, _square(1, 2.5, 7, 2.5))], 6, 8),
        "closing_vertex_repeated": ([(0, sq + sq[:1])], 10, 11),
        "overlap_ab": ([(3, _square(1, 1, 7, 7)), (5, _square(4, 3, 10, 9))], 10, 11),
        "overlap_ba": ([(5, _square(4, 3, 10, 9)), (3, _square(1, 1, 7, 7))], 10, 11),
        "abutting_slanted": ([(0, [(0.0, 0.0), (6.3, 0.0), (2.7, 12.0), (0.0, 12.0)]), (1, [(6.3, 0.0), (12.0, 0.0), (12.0, 12.0), (2.7, 12.0)])],
                             12, 12),
        "sliver_tall": ([(0, sliver)], 700, 6),
        "sliver_wide": ([(0, [(y, x) for x, y in sliver])], 6, 700),
        "random_300": (random_polygons(), 150, 170),
    }
    return {name: (pack(polys), H, W) for name, (polys, H, W) in out.items()}
