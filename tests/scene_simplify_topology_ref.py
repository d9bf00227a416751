"""Spec (numpy and Python ints) of what scene.simplify_labels_topology adds to tests/simplify_topology_ref.py and
tests/scene_simplify_ref.py (csrc/dm_scene_simplify_topology.hip).  No new geometry rule; two restatements:
  the grid       the flags of simplify_topology_ref.kinds computed the way the kernels search: a segment is registered in every cell
                 `walk_cells` gives for it, a fixed point in the cell of its coordinates >> log2; pairs are tested within a cell,
                 fixed points are taken from the cells under a sub-chain's bounding box.  The cell side is a parameter: the flags
                 must not depend on it.
  arc_keep       the dense keep [H+1, W+1] read per stored arc vertex, as the scene holds it, and the emit from it through
                 scene_simplify_ref's sorted lists.
Slow and plain on purpose."""
from __future__ import annotations

import numpy as np

import scene_simplify_ref as SR
import simplify_ref as S
import simplify_topology_ref as T

MAX_CELLS = 1 << 22


def walk_cells(x0: int, y0: int, x1: int, y1: int, log2: int):
    """dm_topo_walk_cells in Python ints: per cell column the segment crosses, the rows between its heights at the column's sides."""
    if x0 > x1:
        x0, y0, x1, y1 = x1, y1, x0, y0
    dx, dy = x1 - x0, y1 - y0
    out = []
    for cx in range(x0 >> log2, (x1 >> log2) + 1):
        if dx == 0:
            lo, hi = min(y0, y1), max(y0, y1)
        else:
            left = cx << log2
            right = left + (1 << log2)
            xa, xb = max(left, x0) - x0, min(right, x1) - x0
            ya, yb = y0 + (dy * xa) // dx, y0 + (dy * xb) // dx          # floor: dx > 0
            lo, hi = min(ya, yb), max(ya, yb)
        out += [(cx, cy) for cy in range(lo >> log2, (hi >> log2) + 1)]
    return out


def cells_of_points(x0: int, y0: int, x1: int, y1: int, log2: int):
    """The cell of every integer-parameter point of the closed segment, floored: what `walk_cells` has to cover."""
    dx, dy = x1 - x0, y1 - y0
    n = 2 * (abs(dx) + abs(dy)) + 1
    return {((x0 * n + dx * k) // n >> log2, (y0 * n + dy * k) // n >> log2) for k in range(n + 1)}


def grid_kinds(segments, fixed, log2: int) -> np.ndarray:
    """simplify_topology_ref.kinds through a grid of cells of 2^log2 corners."""
    ends = [(s["chain"][s["i"]], s["chain"][s["j"]]) for s in segments]
    kind = np.zeros(len(segments), np.uint8)
    cells = {}
    for n, (a, b) in enumerate(ends):
        if a == b:
            kind[n] |= T.MEETS
        else:
            for c in walk_cells(*a, *b, log2):
                cells.setdefault(c, []).append(n)
    box = np.array([[min(a[0], b[0]), min(a[1], b[1]), max(a[0], b[0]), max(a[1], b[1])] for a, b in ends], np.int64).reshape(-1, 4)
    for members in cells.values():                              # every pair of a cell (those whose boxes do not touch cannot meet)
        members = np.asarray(members)
        for m in members:
            b = box[members]
            near = members[(b[:, 0] <= box[m, 2]) & (b[:, 2] >= box[m, 0]) & (b[:, 1] <= box[m, 3]) & (b[:, 3] >= box[m, 1])]
            for n in near:
                if n > m and not (kind[m] & T.MEETS and kind[n] & T.MEETS) and T.meets(*ends[m], *ends[n]):
                    kind[m] |= T.MEETS
                    kind[n] |= T.MEETS
    points = {}
    for p in fixed:
        points.setdefault((p[0] >> log2, p[1] >> log2), []).append(p)
    for n, s in enumerate(segments):
        if s["j"] - s["i"] > 1:
            poly = s["chain"][s["i"]:s["j"] + 1]
            xs, ys = [p[0] for p in poly], [p[1] for p in poly]
            under = [p for cy in range(min(ys) >> log2, (max(ys) >> log2) + 1) for cx in range(min(xs) >> log2, (max(xs) >> log2) + 1)
                     for p in points.get((cx, cy), [])]
            if any(min(xs) <= p[0] <= max(xs) and min(ys) <= p[1] <= max(ys) and p != poly[0] and p != poly[-1] and T.inside(poly, p)
                   for p in under):
                kind[n] |= T.JUMPS
    return kind


def below_len(t: dict) -> np.ndarray:
    """bool [Va]: false at the repeated end of every closed arc, which is no position of the cyclic sequence."""
    out = np.ones(len(t["arc_xy"]), bool)
    for a in range(len(t["left"])):
        first, end = int(t["arc_ptr"][a]), int(t["arc_ptr"][a + 1])
        if end - first >= 3 and tuple(t["arc_xy"][first]) == tuple(t["arc_xy"][end - 1]):
            out[end - 1] = False
    return out


def arc_keep_of(t: dict, keep: np.ndarray, W: int) -> np.ndarray:
    """uint8 [Va]: the dense keep flags read per stored arc vertex; the repeated end of a closed arc holds a 2 or nothing."""
    xy = t["arc_xy"].astype(np.int64)
    out = keep.reshape(-1)[xy[:, 1] * (W + 1) + xy[:, 0]].astype(np.uint8)
    out[~below_len(t) & (out == 1)] = 0
    return out


def emit(labels: np.ndarray, t: dict, keep: np.ndarray, tile) -> dict:
    """The sparse emit of scene_simplify_ref from given dense flags: node lists from the tiles, the kept set from the flags per
    stored arc vertex, the arcs and rings from those."""
    L = np.asarray(labels)
    H, W = L.shape
    node_row = SR.scene_nodes(L, tile)
    node_col = SR.node_columns(node_row, H, W)
    arc_keep = arc_keep_of(t, keep, W)
    kept_row = SR.kept_rows(t["arc_xy"], arc_keep, node_row, W)
    arc_ptr, arc_xy = SR.arcs_out(t["arc_xy"], t["arc_ptr"], arc_keep)
    ring_ptr, xy, ring_area2 = SR.rings_out(t["xy"], t["ring_ptr"], node_row, node_col, kept_row, H, W)
    return {"arc_ptr": arc_ptr, "arc_xy": arc_xy, "left": t["left"], "right": t["right"], "region_ptr": t["region_ptr"], "ring_ptr": ring_ptr,
            "xy": xy, "ring_label": t["ring_label"], "ring_area2": ring_area2, "arc_keep": arc_keep, "kept_row": kept_row}


def cell_log2(H: int, W: int) -> int:
    """The smallest log2 >= 5 at which ((H >> log2) + 1) ((W >> log2) + 1) <= 2^22, by trying every one."""
    return next(l for l in range(5, 32) if ((H >> l) + 1) * ((W >> l) + 1) <= MAX_CELLS)


def quantise(tolerance) -> int:
    return S.quantise(tolerance)
