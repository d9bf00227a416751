"""Spec (numpy and Python ints) of rag.simplify: shared-boundary Douglas-Peucker on the rings and arcs of a label raster.

The definitions (include/deepmerge_hip.h and DESIGN.md 3.5.7 restate them), on top of tests/vector_ref.py:
  nodes: a corner (x, y), 0 <= x <= W, 0 <= y <= H, is a node iff at least three of its four unit grid edges are boundary edges (two
  different labels across, the outside is -1) or it is one of the four raster corners.  Nodes are never removed.  Every other
  corner on a boundary has two boundary edges: one chain passes through it, once, so a keep flag per corner is single-valued.
  chains: an arc of vector_ref.trace is cut at every vertex that is a node; an open arc also at its two ends (they are nodes).  A
  closed arc (first vertex == last) is a cyclic sequence: its stored start is dropped when it is no node and lies inside a
  straight run; with no node among its vertices the chain begins and ends at the vertex smallest in (y, x), which is kept.
  Douglas-Peucker on a chain v[0..n-1], ends kept: for a segment (i, j), j > i + 1, d_k = |cross(v[j] - v[i], v[k] - v[i])| if
  v[i] != v[j], else |v[k] - v[i]|^2; k* = arg-max, ties to the smallest k; with q = floor(256 t + 0.5), k* is kept and both halves
  are split further iff 65536 d^2 > q^2 |v[j] - v[i]|^2 (distinct ends) or 65536 d > q^2 (coinciding ends).
  keep[y (W+1) + x] = 2 node, 1 kept chain vertex, 0 otherwise.
  arcs: the kept vertices of every arc in stored order; a closed arc begins at its first kept vertex and repeats it at its end.
  rings: the kept corners met when walking from every ring vertex to the next, one unit step at a time (this inserts the nodes
  on a straight run of the ring); ring_area2 is the shoelace sum again.
Plain on purpose; only the arg-max over a segment is a numpy expression (int64; every value is below 2^32).
"""
from __future__ import annotations

import math

import numpy as np

import vector_ref as V

MAX_SIDE = 32768
MAX_Q = 1 << 20


def quantise(t) -> int:
    """q = floor(256 t + 0.5), as rasterize quantises coordinates; 0 <= q <= 2^20."""
    t = float(t)
    if not math.isfinite(t) or t < 0:
        raise ValueError("tolerance must be finite and >= 0")
    q = int(math.floor(256.0 * t + 0.5))
    if q > MAX_Q:
        raise ValueError("tolerance must quantise to at most 2^20 (4096 pixels)")
    return q


def nodes(labels: np.ndarray) -> np.ndarray:
    """uint8 [H+1, W+1]: 2 at every node, 0 elsewhere."""
    L = np.asarray(labels)
    H, W = L.shape
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError("H, W must be at most 32768")
    keep = np.zeros((H + 1, W + 1), np.uint8)
    for y in range(H + 1):
        for x in range(W + 1):
            a, b = V._label(L, x - 1, y - 1), V._label(L, x, y - 1)          # the four pixels around the corner
            c, d = V._label(L, x - 1, y), V._label(L, x, y)
            degree = (a != b) + (c != d) + (a != c) + (b != d)
            if degree >= 3 or (x in (0, W) and y in (0, H)):
                keep[y, x] = 2
    return keep


def exceeds(d: int, len2: int, q: int) -> bool:
    """The split test, in Python ints: len2 = |v[j] - v[i]|^2, 0 for coinciding ends (d is then a squared distance)."""
    return 65536 * d > q * q if len2 == 0 else 65536 * d * d > q * q * len2


def farthest(chain: np.ndarray, i: int, j: int):
    """(k*, d) of the segment (i, j) of chain int64 [n,2]."""
    a, b = chain[i], chain[j]
    rel = chain[i + 1:j] - a
    if (a == b).all():
        d = rel[:, 0] * rel[:, 0] + rel[:, 1] * rel[:, 1]
    else:
        e = b - a
        d = np.abs(e[0] * rel[:, 1] - e[1] * rel[:, 0])
    k = int(np.argmax(d))                                           # the first of equal maxima
    return i + 1 + k, int(d[k])


def douglas_peucker(chain, q: int):
    """Sorted interior indices of `chain` (a list of (x, y)) that are kept."""
    v = np.asarray(chain, np.int64).reshape(-1, 2)
    kept, todo = [], [(0, len(v) - 1)]
    while todo:
        i, j = todo.pop()
        if j <= i + 1:
            continue
        k, d = farthest(v, i, j)
        e = v[j] - v[i]
        if exceeds(d, int(e[0] * e[0] + e[1] * e[1]), q):
            kept.append(k)
            todo += [(i, k), (k, j)]
    return sorted(kept)


def _collinear(a, b, c) -> bool:
    return (b[0] - a[0]) * (c[1] - b[1]) == (b[1] - a[1]) * (c[0] - b[0])


def chains_of(pts, keep: np.ndarray):
    """The chains of one arc (a list of (x, y)), each a list of vertices from one cut to the next, and the anchor of a closed arc
    without a node (None otherwise)."""
    node = lambda p: keep[p[1], p[0]] == 2
    if pts[0] != pts[-1]:
        cuts = [0] + [i for i in range(1, len(pts) - 1) if node(pts[i])] + [len(pts) - 1]
        return [pts[a:b + 1] for a, b in zip(cuts[:-1], cuts[1:])], None
    cyc = pts[:-1]
    if not node(cyc[0]) and _collinear(cyc[-1], cyc[0], cyc[1]):
        cyc = cyc[1:]
    at = [i for i, p in enumerate(cyc) if node(p)]
    anchor = None
    if not at:
        anchor = min(cyc, key=lambda p: (p[1], p[0]))
        at = [cyc.index(anchor)]
    seq = cyc[at[0]:] + cyc[:at[0]] + [cyc[at[0]]]
    cuts = [i - at[0] for i in at] + [len(cyc)]
    return [seq[a:b + 1] for a, b in zip(cuts[:-1], cuts[1:])], anchor


def keep_flags(labels: np.ndarray, t: dict, q: int) -> np.ndarray:
    """uint8 [H+1, W+1] from the traced arcs t (vector_ref.trace)."""
    keep = nodes(labels)
    for a in range(len(t["left"])):
        pts = [tuple(int(c) for c in p) for p in t["arc_xy"][t["arc_ptr"][a]:t["arc_ptr"][a + 1]]]
        chains, anchor = chains_of(pts, keep)
        if anchor is not None:
            keep[anchor[1], anchor[0]] = 1
        for chain in chains:
            for k in douglas_peucker(chain, q):
                assert keep[chain[k][1], chain[k][0]] == 0, "a chain's interior vertex is a node or lies on two chains"
                keep[chain[k][1], chain[k][0]] = 1
    return keep


def area2(pts) -> int:
    return sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(pts, pts[1:] + pts[:1]))


def simplify(labels: np.ndarray, n_labels: int, tolerance, t: dict = None) -> dict:
    """keep uint8 [(H+1)(W+1)], the simplified arcs (arc_ptr, arc_xy, left, right) and rings (region_ptr, ring_ptr, xy, ring_label,
    ring_area2), dtypes as rag.simplify returns them.  t: vector_ref.trace(labels, n_labels) when the caller has it."""
    q = quantise(tolerance)
    L = np.asarray(labels)
    t = V.trace(L, n_labels) if t is None else t
    keep = keep_flags(L, t, q)
    arc_ptr, arc_xy = [0], []
    for a in range(len(t["left"])):
        pts = [tuple(int(c) for c in p) for p in t["arc_xy"][t["arc_ptr"][a]:t["arc_ptr"][a + 1]]]
        closed = pts[0] == pts[-1]
        kept = [p for p in (pts[:-1] if closed else pts) if keep[p[1], p[0]]]
        arc_xy += kept + kept[:1] if closed else kept
        arc_ptr.append(len(arc_xy))
    ring_ptr, xy, ring_area2 = [0], [], []
    for r in range(len(t["ring_label"])):
        pts = [tuple(int(c) for c in p) for p in t["xy"][t["ring_ptr"][r]:t["ring_ptr"][r + 1]]]
        out = []
        for (x0, y0), (x1, y1) in zip(pts, pts[1:] + pts[:1]):
            assert (x0 == x1) != (y0 == y1)
            sx, sy = int(np.sign(x1 - x0)), int(np.sign(y1 - y0))
            for s in range(abs(x1 - x0) + abs(y1 - y0)):
                c = (x0 + s * sx, y0 + s * sy)
                if keep[c[1], c[0]]:
                    out.append(c)
        xy += out
        ring_ptr.append(len(xy))
        ring_area2.append(area2(out))
    return {"keep": keep.reshape(-1), "arc_ptr": np.asarray(arc_ptr, np.int64), "arc_xy": np.asarray(arc_xy, np.int32).reshape(-1, 2),
            "left": t["left"], "right": t["right"], "region_ptr": t["region_ptr"], "ring_ptr": np.asarray(ring_ptr, np.int64),
            "xy": np.asarray(xy, np.int32).reshape(-1, 2), "ring_label": t["ring_label"], "ring_area2": np.asarray(ring_area2, np.int64)}


# ---- the rasters both test files simplify -------------------------------------------------------------------------------------------
def drawn_cases():
    """name -> (labels int32 [H,W], n_labels): hand-drawn rasters with known answers (tests/test_simplify_host.py states them)."""
    return {"stair": (np.array([[0, 1], [0, 0]], np.int32), 2),                  # 0|1 is (1,0) (1,1) (2,1): one step between two frame nodes
            "bump": (np.array([[0, 1, 0], [0, 0, 0]], np.int32), 2),             # 0|1 is (1,0) (1,1) (2,1) (2,0): two vertices tie
            "tee": (np.array([[0, 0], [1, 2]], np.int32), 3)}                    # (1,1) is a T-junction on label 0's bottom side


def _smooth(H: int, W: int, n: int, seed: int) -> np.ndarray:
    """n labels with wavy boundaries: the nearest of n seeded sites under a distance bent by two sines."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    x = x + 3.0 * np.sin(y / 5.0)
    y = y + 3.0 * np.sin(x / 7.0)
    sites = rng.uniform(0, 1, (n, 2)) * (W, H)
    d = (x[None] - sites[:, 0, None, None]) ** 2 + (y[None] - sites[:, 1, None, None]) ** 2
    return np.argmin(d, 0).astype(np.int32)


def extra_cases():
    """name -> (labels int32 [H,W], n_labels): the rasters beyond vector_ref.host_cases() / comb_of_combs()."""
    return {"flat_wide": (_smooth(5, 700, 40, 17), 40),
            "flat_tall": (_smooth(700, 6, 40, 19), 40),
            "random_4": (np.random.default_rng(23).integers(0, 4, (130, 130)).astype(np.int32), 4)}
