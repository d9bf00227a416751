"""Spec (numpy and Python ints) of rag.simplify(topology=True) and rag.simplify_conflicts: find the segments of a simplified scene
that meet another segment or jumped over a fixed point, and repair them by keeping more vertices (include/deepmerge_hip.h and
DESIGN.md 3.5.12 restate it).  On top of tests/simplify_ref.py and tests/vector_ref.py; integers only.

  orient(a, b, c) = (b.x - a.x)(c.y - a.y) - (b.y - a.y)(c.x - a.x); coordinates are at most 32768, so it is below 2^31.
  segments: for a keep array, every chain (simplify_ref.chains_of) is the sequence of its kept vertices; a segment is two
  consecutive kept vertices (v[i], v[j]) of one chain and its interior is v[i+1 .. j-1] of the traced chain.  Frame arcs take part.
  Order: by arc, then along the arc from its first kept vertex in stored order: segment s of an arc joins vertices s and s + 1 of
  the simplified arc simplify_ref.simplify emits.
  fixed points: every node (keep == 2) and the anchor of every closed arc without a node.
  kind bit 1, meets: the segment is degenerate (v[i] == v[j]), or it shares with another non-degenerate segment a point that is
  not an end of both: the same two ends, a proper crossing, or an end of one on the other that is not an end of that other.
  kind bit 2, jumps: the segment has interior vertices and a fixed point other than v[i], v[j] is inside the polygon v[i] .. v[j]
  closed by the segment, by the even-odd rule, half-open in y.
  repair: a round computes the kinds of all segments; every flagged segment with interior vertices keeps its arg-max k*
  (simplify_ref.farthest) and both halves are simplified by Douglas-Peucker at the same q; rounds repeat until no kind is set.
Plain on purpose: every pair of segments is tested, every fixed point against every segment."""
from __future__ import annotations

import numpy as np

import simplify_ref as S
import vector_ref as V

MEETS, JUMPS = 1, 2


def orient(a, b, c) -> int:
    return (int(b[0]) - int(a[0])) * (int(c[1]) - int(a[1])) - (int(b[1]) - int(a[1])) * (int(c[0]) - int(a[0]))


def _on(a, b, p) -> bool:
    """p lies on the closed segment (a, b)."""
    return (orient(a, b, p) == 0 and min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1]))


def meets(a, b, c, d) -> bool:
    """Two non-degenerate segments (a, b), (c, d) share a point that is not an end of both."""
    a, b, c, d = tuple(a), tuple(b), tuple(c), tuple(d)
    if {a, b} == {c, d}:
        return True
    o1, o2, o3, o4 = orient(a, b, c), orient(a, b, d), orient(c, d, a), orient(c, d, b)
    if ((o1 > 0 and o2 < 0) or (o1 < 0 and o2 > 0)) and ((o3 > 0 and o4 < 0) or (o3 < 0 and o4 > 0)):
        return True
    return ((_on(a, b, c) and c not in (a, b)) or (_on(a, b, d) and d not in (a, b)) or (_on(c, d, a) and a not in (c, d))
            or (_on(c, d, b) and b not in (c, d)))


def inside(poly, p) -> bool:
    """Even-odd, half-open in y: p against the closed polygon `poly` (a list of (x, y))."""
    n = 0
    for u, w in zip(poly, poly[1:] + poly[:1]):
        if (u[1] <= p[1]) != (w[1] <= p[1]):
            o = orient(u, w, p)
            if (w[1] > u[1] and o > 0) or (w[1] < u[1] and o < 0):
                n += 1
    return n % 2 == 1


def _arc_points(t: dict, a: int):
    return [tuple(int(c) for c in p) for p in t["arc_xy"][t["arc_ptr"][a]:t["arc_ptr"][a + 1]]]


def scene_of(t: dict, keep: np.ndarray):
    """(segments, fixed): segments in order, each {arc, chain (list of (x, y)), i, j}; fixed the set of fixed points."""
    segments = []
    fixed = {(int(x), int(y)) for y, x in zip(*np.nonzero(keep == 2))}
    for a in range(len(t["left"])):
        pts = _arc_points(t, a)
        chains, anchor = S.chains_of(pts, keep)
        if anchor is not None:
            fixed.add(anchor)
        mine, at = [], 0                                        # `at`: the position of a chain's start along the cut sequence
        for chain in chains:
            kept = [k for k, p in enumerate(chain) if keep[p[1], p[0]]]
            assert kept[0] == 0 and kept[-1] == len(chain) - 1
            mine += [(at + i, {"arc": a, "chain": chain, "i": i, "j": j}) for i, j in zip(kept[:-1], kept[1:])]
            at += len(chain) - 1
        if pts[0] == pts[-1]:                                   # a closed arc is emitted from its first kept vertex in stored order
            cyc = pts[:-1]
            if keep[cyc[0][1], cyc[0][0]] != 2 and S._collinear(cyc[-1], cyc[0], cyc[1]):
                cyc = cyc[1:]
            first = cyc.index(chains[0][0])
            mine = [((first + pos) % len(cyc), s) for pos, s in mine]
        segments += [s for _, s in sorted(mine, key=lambda m: m[0])]
    return segments, fixed


def kinds(segments, fixed) -> np.ndarray:
    """uint8 [n]: the kind of every segment."""
    ends = [(s["chain"][s["i"]], s["chain"][s["j"]]) for s in segments]
    kind = np.zeros(len(segments), np.uint8)
    live = [n for n, (a, b) in enumerate(ends) if a != b]
    for n, (a, b) in enumerate(ends):
        if a == b:
            kind[n] |= MEETS
    box = np.array([[min(a[0], b[0]), min(a[1], b[1]), max(a[0], b[0]), max(a[1], b[1])] for a, b in ends], np.int64).reshape(-1, 4)
    for m in live:                                              # every pair whose boxes touch
        near = np.nonzero((box[:, 0] <= box[m, 2]) & (box[:, 2] >= box[m, 0]) & (box[:, 1] <= box[m, 3]) & (box[:, 3] >= box[m, 1]))[0]
        for n in near:
            if n > m and ends[n][0] != ends[n][1] and meets(*ends[m], *ends[n]):
                kind[m] |= MEETS
                kind[n] |= MEETS
    points = sorted(fixed)
    for n, s in enumerate(segments):
        if s["j"] - s["i"] > 1:
            poly = s["chain"][s["i"]:s["j"] + 1]
            xs, ys = [p[0] for p in poly], [p[1] for p in poly]
            for p in points:
                if (min(xs) <= p[0] <= max(xs) and min(ys) <= p[1] <= max(ys) and p != poly[0] and p != poly[-1] and inside(poly, p)):
                    kind[n] |= JUMPS
                    break
    return kind


def _flagged(segments, kind) -> dict:
    hit = np.nonzero(kind)[0]
    return {"arc": np.asarray([segments[n]["arc"] for n in hit], np.int32),
            "xy": np.asarray([segments[n]["chain"][segments[n]["i"]] + segments[n]["chain"][segments[n]["j"]] for n in hit], np.int32).reshape(-1, 4),
            "kind": kind[hit], "n_segments": len(segments)}


def conflicts(labels: np.ndarray, n_labels: int, tolerance, t: dict = None, keep: np.ndarray = None) -> dict:
    """The flagged segments of `keep` (plain simplify's when None): arc int32 [n], xy int32 [n,4], kind uint8 [n], n_segments."""
    L = np.asarray(labels)
    t = V.trace(L, n_labels) if t is None else t
    if keep is None:
        keep = S.keep_flags(L, t, S.quantise(tolerance))
    segments, fixed = scene_of(t, keep)
    return _flagged(segments, kinds(segments, fixed))


def repair(labels: np.ndarray, t: dict, q: int, max_rounds: int = 64):
    """(keep uint8 [H+1, W+1], the flagged-segment count of every round; the last is 0, `conflicts` of the plain keep)."""
    keep = S.keep_flags(np.asarray(labels), t, q)
    flagged, first = [], None
    while True:
        segments, fixed = scene_of(t, keep)
        kind = kinds(segments, fixed)
        first = _flagged(segments, kind) if first is None else first
        flagged.append(int(np.count_nonzero(kind)))
        if flagged[-1] == 0:
            return keep, flagged, first
        if len(flagged) > max_rounds:
            raise RuntimeError(f"conflicts remain after {max_rounds} rounds")
        split = [s for s, k in zip(segments, kind) if k and s["j"] - s["i"] > 1]
        if not split:
            raise AssertionError("a conflict with nothing to split: the traced arcs are not conflict-free")
        for s in split:
            v = np.asarray(s["chain"], np.int64)
            k, _ = S.farthest(v, s["i"], s["j"])
            new = [k] + [s["i"] + m for m in S.douglas_peucker(s["chain"][s["i"]:k + 1], q)] + [k + m for m in S.douglas_peucker(s["chain"][k:s["j"] + 1], q)]
            for m in new:
                x, y = s["chain"][m]
                assert keep[y, x] == 0, "a segment's interior vertex is kept, a node, or lies on two segments"
                keep[y, x] = 1


def emit(t: dict, keep: np.ndarray) -> dict:
    """The arrays simplify_ref.simplify returns, from a given keep [H+1, W+1]."""
    arc_ptr, arc_xy = [0], []
    for a in range(len(t["left"])):
        pts = _arc_points(t, a)
        closed = pts[0] == pts[-1]
        kept = [p for p in (pts[:-1] if closed else pts) if keep[p[1], p[0]]]
        arc_xy += kept + kept[:1] if closed else kept
        arc_ptr.append(len(arc_xy))
    ring_ptr, xy, ring_area2 = [0], [], []
    for r in range(len(t["ring_label"])):
        pts = [tuple(int(c) for c in p) for p in t["xy"][t["ring_ptr"][r]:t["ring_ptr"][r + 1]]]
        out = []
        for (x0, y0), (x1, y1) in zip(pts, pts[1:] + pts[:1]):
            sx, sy = int(np.sign(x1 - x0)), int(np.sign(y1 - y0))
            out += [c for c in ((x0 + s * sx, y0 + s * sy) for s in range(abs(x1 - x0) + abs(y1 - y0))) if keep[c[1], c[0]]]
        xy += out
        ring_ptr.append(len(xy))
        ring_area2.append(S.area2(out))
    return {"keep": keep.reshape(-1), "arc_ptr": np.asarray(arc_ptr, np.int64), "arc_xy": np.asarray(arc_xy, np.int32).reshape(-1, 2),
            "left": t["left"], "right": t["right"], "region_ptr": t["region_ptr"], "ring_ptr": np.asarray(ring_ptr, np.int64),
            "xy": np.asarray(xy, np.int32).reshape(-1, 2), "ring_label": t["ring_label"], "ring_area2": np.asarray(ring_area2, np.int64)}


def simplify(labels: np.ndarray, n_labels: int, tolerance, t: dict = None, max_rounds: int = 64) -> dict:
    """simplify_ref.simplify with the repair: its arrays, plus `rounds` (repair rounds taken), `flagged` (per round) and
    `conflicts` (those of the plain keep, as `conflicts` returns them)."""
    L = np.asarray(labels)
    t = V.trace(L, n_labels) if t is None else t
    keep, flagged, first = repair(L, t, S.quantise(tolerance), max_rounds)
    out = emit(t, keep)
    out.update(rounds=len(flagged) - 1, flagged=flagged, conflicts=first)
    return out


# ---- the rasters both test files use ------------------------------------------------------------------------------------------------
def bay():
    L = np.zeros((5, 5), np.int32)
    L[4:] = 1
    L[1:4, 1:4] = 1
    L[2, 2] = 2
    return L, 3


def long_bay():
    L = np.zeros((7, 200), np.int32)
    L[5:] = 1
    L[1:5, 1:199] = 1
    L[2, 40] = 2
    L[2, 70:130] = 3
    L[3, 160] = 4
    return L, 5


def _noise(side: int, seed: int, n: int):
    return np.random.default_rng(seed).integers(0, n, (side, side)).astype(np.int32), n


def cases():
    """name -> (labels int32 [H,W], n_labels)."""
    out = dict(V.host_cases())
    out.update(S.drawn_cases())
    out.update(bay=bay(), long_bay=long_bay(), smooth=(S._smooth(64, 64, 30, 5), 30))
    extra = S.extra_cases()
    out.update(flat_wide=extra["flat_wide"], flat_tall=extra["flat_tall"])
    for side in (32, 48):
        for seed in (7, 11):
            out[f"noise{side}_{seed}"] = _noise(side, seed, 2)
    out["noise24_23"] = _noise(24, 23, 3)
    return out


TOLERANCES = (0, 1, 2.5, 20)
