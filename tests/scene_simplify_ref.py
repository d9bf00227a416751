"""Spec (numpy and Python ints) of the sparse form of `keep` behind scene.simplify_labels (csrc/dm_scene_simplify.hip, DESIGN.md
3.5.11).  The rule is tests/simplify_ref.py's, unchanged; a scene has no corner raster, so `keep` is held as
  node records   per tile: the scene corner ids y (W + 1) + x of the nodes among the corners the tile's core owns.  The tile is read
                 through the window scene_vector_ref reads (core + one pixel, clipped to the scene); corner (x, y) belongs to the
                 core that holds pixel (min(y, H - 1), min(x, W - 1)); outside the SCENE is -1.
  node_row       the tiles' records joined and sorted; node_col: the same nodes as x (H + 1) + y, sorted.
  arc_keep       uint8 per stored arc vertex: 2 where the vertex's corner is in node_row; the chain pass writes its 1s by position,
                 at stored vertex first + skip + (p mod len).
  kept_row       sorted: the nodes and the corners of the arc vertices with arc_keep == 1.
  rings          per ring vertex v: v itself iff it is in kept_row, then the nodes strictly inside the run to its successor, one
                 range of node_row (horizontal run) or node_col (vertical run), in the walk's direction.
Slow and plain on purpose.
"""
from __future__ import annotations

import bisect

import numpy as np

import simplify_ref as S
import vector_ref as V


def tile_nodes(window: np.ndarray, core, origin, scene_h: int, scene_w: int) -> np.ndarray:
    """int64, ascending: the scene corner ids of the nodes the core (cy0, cy1, cx0, cx1) of `window` owns (both in window
    coordinates), the window's first pixel at origin = (oy, ox) of a scene_h x scene_w scene."""
    L = np.asarray(window)
    wh, ww = L.shape
    cy0, cy1, cx0, cx1 = core
    oy, ox = int(origin[0]), int(origin[1])
    out = []
    for y in range(wh + 1):
        for x in range(ww + 1):
            Y, X = y + oy, x + ox
            py, px = min(Y, scene_h - 1) - oy, min(X, scene_w - 1) - ox          # the pixel that decides the owner
            if not (cy0 <= py < cy1 and cx0 <= px < cx1):
                continue
            a, b = V._label(L, x - 1, y - 1), V._label(L, x, y - 1)              # outside the window: -1; asked only outside the scene
            c, d = V._label(L, x - 1, y), V._label(L, x, y)
            degree = (a != b) + (c != d) + (a != c) + (b != d)
            if degree >= 3 or (X in (0, scene_w) and Y in (0, scene_h)):
                out.append(Y * (scene_w + 1) + X)
    return np.asarray(out, np.int64)


def windows(H: int, W: int, tile):
    """(core in window coordinates, window box in the scene) of every tile, row-major."""
    th, tw = tile
    for y0 in range(0, H, th):
        for x0 in range(0, W, tw):
            y1, x1 = min(H, y0 + th), min(W, x0 + tw)
            wy0, wy1, wx0, wx1 = max(0, y0 - 1), min(H, y1 + 1), max(0, x0 - 1), min(W, x1 + 1)
            yield (y0 - wy0, y1 - wy0, x0 - wx0, x1 - wx0), (wy0, wy1, wx0, wx1)


def scene_nodes(labels: np.ndarray, tile) -> np.ndarray:
    """node_row: the node records of every tile of `labels` cut into cores of `tile` = (th, tw), joined and sorted."""
    L = np.asarray(labels)
    H, W = L.shape
    parts = [tile_nodes(L[b[0]:b[1], b[2]:b[3]], core, (b[0], b[2]), H, W) for core, b in windows(H, W, tile)]
    return np.sort(np.concatenate(parts))


def node_columns(node_row: np.ndarray, H: int, W: int) -> np.ndarray:
    y, x = node_row // (W + 1), node_row % (W + 1)
    return np.sort(x * (H + 1) + y)


def arc_keep(arc_xy: np.ndarray, arc_ptr: np.ndarray, node_row: np.ndarray, W: int, q: int, limit: int = S.MAX_SIDE) -> np.ndarray:
    """uint8 [Va]: 2 at every stored vertex whose corner is a node, 1 where the chain pass keeps the vertex, 0 otherwise.  An arc whose
    bounding box is wider than `limit` on a side is left alone (the driver raises for it)."""
    xy = np.asarray(arc_xy, np.int64).reshape(-1, 2)
    ids = xy[:, 1] * (W + 1) + xy[:, 0]
    keep = np.where(np.isin(ids, node_row), 2, 0).astype(np.uint8)
    for a in range(len(arc_ptr) - 1):
        first, end = int(arc_ptr[a]), int(arc_ptr[a + 1])
        n = end - first
        pts = [tuple(int(c) for c in p) for p in xy[first:end]]
        closed = n >= 3 and pts[0] == pts[-1]
        ln, skip = (n - 1 if closed else n), 0
        if closed and keep[first] != 2 and S._collinear(pts[ln - 1], pts[0], pts[1]):
            skip, ln = 1, ln - 1
        if ln < 2:
            continue
        stored = lambda p: first + skip + p % ln
        box = xy[[stored(p) for p in range(ln)]]
        if (box.max(0) - box.min(0)).max() > limit:
            continue
        if closed:
            cuts = [p for p in range(ln) if keep[stored(p)] == 2]
            if cuts:
                s = cuts[0]
            else:                                                           # the anchor: smallest corner id, then smallest position
                s = min(range(ln), key=lambda p: (int(ids[stored(p)]), p))
                keep[stored(s)] = 1
            e = s + ln
        else:
            s, e = 0, ln - 1
        cut = [s] + [p for p in range(s + 1, e) if keep[stored(p)] == 2] + [e]
        for i, j in zip(cut[:-1], cut[1:]):
            chain = [pts[stored(p) - first] for p in range(i, j + 1)]
            for k in S.douglas_peucker(chain, q):
                assert keep[stored(i + k)] == 0
                keep[stored(i + k)] = 1
    return keep


def kept_rows(arc_xy: np.ndarray, keep: np.ndarray, node_row: np.ndarray, W: int) -> np.ndarray:
    xy = np.asarray(arc_xy, np.int64).reshape(-1, 2)
    ids = xy[:, 1] * (W + 1) + xy[:, 0]
    return np.sort(np.concatenate((node_row, ids[keep == 1])))


def arcs_out(arc_xy: np.ndarray, arc_ptr: np.ndarray, keep: np.ndarray):
    """(arc_ptr int64, arc_xy int32): the kept vertices of every arc in stored order, a closed arc without its repeated end and with
    its first kept vertex again at its end."""
    xy = np.asarray(arc_xy).reshape(-1, 2)
    ptr, out = [0], []
    for a in range(len(arc_ptr) - 1):
        first, end = int(arc_ptr[a]), int(arc_ptr[a + 1])
        closed = end - first >= 3 and tuple(xy[first]) == tuple(xy[end - 1])
        kept = [tuple(xy[i]) for i in range(first, end - 1 if closed else end) if keep[i]]
        out += kept + kept[:1] if closed else kept
        ptr.append(len(out))
    return np.asarray(ptr, np.int64), np.asarray(out, np.int32).reshape(-1, 2)


def run_vertices(p0, p1, node_row, node_col, kept_row, H: int, W: int):
    """The kept corners on the run from ring vertex p0 to its successor p1 (excluded), from the sorted lists."""
    (x0, y0), (x1, y1) = p0, p1
    assert (x0 == x1) != (y0 == y1)
    out = []
    k = bisect.bisect_left(kept_row, y0 * (W + 1) + x0)
    if k < len(kept_row) and kept_row[k] == y0 * (W + 1) + x0:
        out.append((x0, y0))
    if y0 == y1:
        base, lo, hi, nodes = y0 * (W + 1), min(x0, x1) + 1, max(x0, x1), node_row
    else:
        base, lo, hi, nodes = x0 * (H + 1), min(y0, y1) + 1, max(y0, y1), node_col
    inside = [int(v) - base for v in nodes[bisect.bisect_left(nodes, base + lo):bisect.bisect_left(nodes, base + hi)]]
    if (x1 < x0) or (y1 < y0):
        inside.reverse()
    return out + [(c, y0) if y0 == y1 else (x0, c) for c in inside]


def rings_out(xy: np.ndarray, ring_ptr: np.ndarray, node_row, node_col, kept_row, H: int, W: int):
    """(ring_ptr int64, xy int32, ring_area2 int64) from the sorted lists."""
    node_row, node_col, kept_row = (np.asarray(v).tolist() for v in (node_row, node_col, kept_row))
    ptr, out, area2 = [0], [], []
    for r in range(len(ring_ptr) - 1):
        pts = [tuple(int(c) for c in p) for p in xy[ring_ptr[r]:ring_ptr[r + 1]]]
        ring = []
        for p0, p1 in zip(pts, pts[1:] + pts[:1]):
            ring += run_vertices(p0, p1, node_row, node_col, kept_row, H, W)
        out += ring
        ptr.append(len(out))
        area2.append(S.area2(ring))
    return np.asarray(ptr, np.int64), np.asarray(out, np.int32).reshape(-1, 2), np.asarray(area2, np.int64)


def simplify(labels: np.ndarray, n_labels: int, tolerance, tile, t: dict = None) -> dict:
    """The sparse form end to end: the fields of simplify_ref.simplify (without the dense `keep`), and node_row, node_col, arc_keep,
    kept_row."""
    q = S.quantise(tolerance)
    L = np.asarray(labels)
    H, W = L.shape
    t = V.trace(L, n_labels) if t is None else t
    node_row = scene_nodes(L, tile)
    node_col = node_columns(node_row, H, W)
    keep = arc_keep(t["arc_xy"], t["arc_ptr"], node_row, W, q)
    kept_row = kept_rows(t["arc_xy"], keep, node_row, W)
    arc_ptr, arc_xy = arcs_out(t["arc_xy"], t["arc_ptr"], keep)
    ring_ptr, xy, ring_area2 = rings_out(t["xy"], t["ring_ptr"], node_row, node_col, kept_row, H, W)
    return {"arc_ptr": arc_ptr, "arc_xy": arc_xy, "left": t["left"], "right": t["right"], "region_ptr": t["region_ptr"], "ring_ptr": ring_ptr,
            "xy": xy, "ring_label": t["ring_label"], "ring_area2": ring_area2, "node_row": node_row, "node_col": node_col, "arc_keep": keep,
            "kept_row": kept_row}
