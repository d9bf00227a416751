"""Spec (numpy, integers only) of rag.polygons / rag.boundary_arcs: a label raster traced into closed rings and boundary arcs.

The definitions (include/deepmerge_hip.h and DESIGN.md 3.5.5 restate them):
  pixel (x, y) covers [x, x+1] x [y, y+1], y down.  A pixel has a dart on every side whose neighbour has another label or lies
  outside the raster (the dart's `other` label; -1 outside).  side 0 top runs east, 1 right runs south, 2 bottom runs west,
  3 left runs north: the pixel lies on the dart's right.  dart id = 4 (y W + x) + side.
  successor of a dart of label l ending at corner c, with the two pixels ahead of c seen along the dart: ahead-right is not l
  -> turn right (side + 1 of the same pixel); else ahead-left is not l -> straight (same side of ahead-right); else turn left
  (side + 3 of ahead-left).
  ring = cycle of the successor permutation, head = its smallest dart id; vertex dart = predecessor has another side; break dart
  = predecessor has another `other`.  The head of an outer ring is a vertex dart (the top side of the component's first pixel in
  raster order); the head of a hole need not be: the vertices then start at the first vertex dart behind it, and a closed arc
  starts at the head's start corner, which lies inside a straight run.
Everything here walks the cycles one dart at a time: slow and plain on purpose.
"""
from __future__ import annotations

import numpy as np

DX = (1, 0, -1, 0)          # direction of a dart of side 0..3
DY = (0, 1, 0, -1)
SX = (0, 1, 1, 0)           # start corner of a dart, relative to its pixel
SY = (0, 0, 1, 1)


def _label(L, x, y):
    H, W = L.shape
    return int(L[y, x]) if 0 <= x < W and 0 <= y < H else -1


def darts(labels: np.ndarray):
    """dict dart id -> (x, y, side, label, other) of every dart, in ascending id."""
    L = np.asarray(labels)
    H, W = L.shape
    out = {}
    for y in range(H):
        for x in range(W):
            l = int(L[y, x])
            for side in range(4):
                lx, ly = DY[side], -DX[side]                # the pixel across: to the dart's left
                o = _label(L, x + lx, y + ly)
                if o != l:
                    out[4 * (y * W + x) + side] = (x, y, side, l, o)
    return out


def successor(labels: np.ndarray, x: int, y: int, side: int) -> int:
    L = np.asarray(labels)
    W = L.shape[1]
    l = int(L[y, x])
    arx, ary = x + DX[side], y + DY[side]                   # ahead-right
    alx, aly = arx + DY[side], ary - DX[side]               # ahead-left
    if _label(L, arx, ary) != l:
        return 4 * (y * W + x) + ((side + 1) & 3)
    if _label(L, alx, aly) != l:
        return 4 * (ary * W + arx) + side
    return 4 * (aly * W + alx) + ((side + 3) & 3)


def successor_map(labels: np.ndarray):
    d = darts(labels)
    return d, {i: successor(labels, x, y, s) for i, (x, y, s, _, _) in d.items()}


def _start(d):
    x, y, s = d[0], d[1], d[2]
    return (x + SX[s], y + SY[s])


def _end(d):
    x, y, s = d[0], d[1], d[2]
    return (x + SX[s] + DX[s], y + SY[s] + DY[s])


def trace(labels: np.ndarray, n_labels: int):
    """Both results: a dict with region_ptr, ring_ptr, xy, ring_label, ring_area2, ring_head (polygons) and arc_ptr, arc_xy,
    left, right, arc_first (arcs), dtypes as rag.polygons / rag.boundary_arcs return them."""
    L = np.asarray(labels)
    H, W = L.shape
    if H * W > 1 << 28:
        raise ValueError("H * W must be at most 2^28")
    if L.min() < 0 or L.max() >= n_labels:
        raise ValueError("labels must be in 0..n_labels-1")
    d, nxt = successor_map(L)
    seen = set()
    rings = []                                              # (label, head, [dart ids in cycle order from the head])
    for i in sorted(d):
        if i in seen:
            continue
        cyc, j = [], i
        while j not in seen:
            seen.add(j)
            cyc.append(j)
            j = nxt[j]
        assert j == i, "the successor map is not a permutation"
        rings.append((d[i][3], i, cyc))
    rings.sort(key=lambda r: (r[0], r[1]))
    ring_ptr, xy, ring_label, ring_area2, ring_head = [0], [], [], [], []
    arcs = []                                               # (right, left, first dart, [vertices])
    for l, head, cyc in rings:
        n = len(cyc)
        vertex = [d[cyc[k]][2] != d[cyc[k - 1]][2] for k in range(n)]
        brk = [d[cyc[k]][4] != d[cyc[k - 1]][4] for k in range(n)]
        verts = [_start(d[cyc[k]]) for k in range(n) if vertex[k]]
        a2 = 0
        for k in range(len(verts)):
            (x0, y0), (x1, y1) = verts[k], verts[(k + 1) % len(verts)]
            a2 += x0 * y1 - x1 * y0
        xy += verts
        ring_ptr.append(len(xy))
        ring_label.append(l)
        ring_area2.append(a2)
        ring_head.append(head)
        starts = [k for k in range(n) if brk[k]] or [0]
        for a, k0 in enumerate(starts):
            k1 = starts[a + 1] if a + 1 < len(starts) else starts[0] + n      # one past the arc's last dart
            first = d[cyc[k0]]
            pts = [_start(first)] + [_start(d[cyc[k % n]]) for k in range(k0 + 1, k1) if vertex[k % n]] + [_end(d[cyc[(k1 - 1) % n]])]
            if first[4] == -1 or first[4] > l:
                arcs.append((l, first[4], cyc[k0], pts))
    arcs.sort(key=lambda a: a[:3])
    arc_ptr, arc_xy = [0], []
    for a in arcs:
        arc_xy += a[3]
        arc_ptr.append(len(arc_xy))
    region_ptr = np.zeros(n_labels + 1, np.int64)
    np.add.at(region_ptr, np.asarray(ring_label, np.int64) + 1, 1)
    return {"region_ptr": np.cumsum(region_ptr).astype(np.int32), "ring_ptr": np.asarray(ring_ptr, np.int64),
            "xy": np.asarray(xy, np.int32).reshape(-1, 2), "ring_label": np.asarray(ring_label, np.int32),
            "ring_area2": np.asarray(ring_area2, np.int64), "ring_head": np.asarray(ring_head, np.int64),
            "arc_ptr": np.asarray(arc_ptr, np.int64), "arc_xy": np.asarray(arc_xy, np.int32).reshape(-1, 2),
            "left": np.asarray([a[1] for a in arcs], np.int32), "right": np.asarray([a[0] for a in arcs], np.int32),
            "arc_first": np.asarray([a[2] for a in arcs], np.int64)}


def arc_edge(left: np.ndarray, right: np.ndarray, edges: np.ndarray) -> np.ndarray:
    """Row of (min, max) = (right, left) in `edges` (sorted by (a, b), as rag_edges returns them); -1 for left == -1."""
    out = np.full(left.shape[0], -1, np.int32)
    rows = {(int(a), int(b)): i for i, (a, b) in enumerate(np.asarray(edges))}
    for i, (lf, rt) in enumerate(zip(left, right)):
        if lf >= 0:
            out[i] = rows[(int(rt), int(lf))]
    return out


def path_length(xy: np.ndarray, ptr: np.ndarray, closed: bool) -> np.ndarray:
    """Length in unit segments of every ring (closed: back to its first vertex) or arc; all segments are axis-parallel."""
    out = np.zeros(len(ptr) - 1, np.int64)
    for r in range(len(ptr) - 1):
        p = np.asarray(xy[ptr[r]:ptr[r + 1]], np.int64)
        q = np.roll(p, -1, 0) if closed else p[1:]
        out[r] = np.abs(q - (p if closed else p[:-1])).sum()
    return out


def rasterise(t, H: int, W: int) -> np.ndarray:
    """The label raster back from the rings: +1 / -1 on the south / north unit darts of a label, cumulative sum along x."""
    out = np.full((H, W), -1, np.int64)
    labels = np.unique(t["ring_label"])
    for l in labels:
        acc = np.zeros((H, W + 1), np.int64)
        for r in np.nonzero(t["ring_label"] == l)[0]:
            p = np.asarray(t["xy"][t["ring_ptr"][r]:t["ring_ptr"][r + 1]], np.int64)
            for (x0, y0), (x1, y1) in zip(p, np.roll(p, -1, 0)):
                if x0 == x1 and y1 > y0:
                    acc[y0:y1, x0] += 1                     # south: a pixel's right side, the label ends in front of x0
                elif x0 == x1 and y1 < y0:
                    acc[y1:y0, x0] -= 1                     # north: a pixel's left side, the label starts at x0
        # summed along x from the right, pixel x is inside iff the sum over the corners x+1 .. W is 1
        inside = np.cumsum(acc[:, ::-1], 1)[:, ::-1][:, 1:]
        assert set(np.unique(inside)) <= {0, 1}
        assert (out[inside == 1] == -1).all(), "two labels claim a pixel"
        out[inside == 1] = l
    return out


# ---- the small rasters both test files trace ------------------------------------------------------------------------------------------
def comb_of_combs(n: int = 130) -> np.ndarray:
    """Two labels: label 1 is a spine down column 1 with a full row every fourth line and a tooth under every odd pixel of it.  It is
    simply connected, so it has ONE ring, with four vertices per tooth: 64 teeth on 32 rows, more than 8192 vertices, through every
    64x64 tile of the raster."""
    y, x = np.mgrid[0:n, 0:n]
    inside = (x >= 1) & (x <= n - 2) & (y >= 1) & (y <= n - 2)
    return (inside & ((x == 1) | (y % 4 == 1) | ((y % 4 == 2) & (x % 2 == 1)))).astype(np.int32)


def host_cases():
    """name -> (labels int32 [H,W], n_labels)."""
    y, x = np.mgrid[0:6, 0:6]
    frame = np.zeros((4, 5), np.int32)
    frame[1:3, 1:3] = 1
    holes = np.zeros((5, 5), np.int32)
    holes[1, 1] = holes[2, 2] = 1                               # one label in two pieces, the holes it leaves meet at a corner
    corner = np.full((5, 5), 2, np.int32)
    corner[0:3, 0:3] = 0
    corner[1, 1] = 1
    corner[2, 2] = 2                                            # the hole of label 0 meets label 0's outside at corner (2, 2)
    return {"one_pixel": (np.zeros((1, 1), np.int32), 1),
            "single_label": (np.zeros((5, 7), np.int32), 1),
            "parity": (((x + y) & 1).astype(np.int32), 2),
            "frame_island": (frame, 2),
            "diagonal_holes": (holes, 2),
            "hole_meets_outside": (corner, 3),
            "absent_ids": (frame * 3, 6)}                       # n_labels larger than the ids present
