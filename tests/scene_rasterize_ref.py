"""Spec (numpy, integers only) of polygon rasterisation on a scene: scene.RingSource / scene.rasterize_rings
(csrc/dm_scene_rasterize.hip).  The rule is tests/rasterize_ref.py's; this file restates its band and window
form step by step as the device runs it:

  band    the pixel rows [r0, r1) of the H x W scene.  An edge (ends swapped so that y0 < y1) has an event in row r of the band iff
          r0 <= r < r1 and y0 <= 256 r + 128 < y1; the event's column cx is the rule's, clamped to [0, W] scene-wide.
  key     (label (r1 - r0) + (r - r0)) (W + 1) + cx, with (largest label + 1) (r1 - r0) (W + 1) < 2^63: it names no window.
  sort    the band's keys ascending: closed rings give every (label, row) an even count, so keys 2j and 2j+1 bound a span.
  window  the columns [x0, x1).  out [r1 - r0, x1 - x0] is pre-set to fill; pair (a, b) writes max(label) over the columns
          [cx_a, cx_b) that lie in [x0, x1).  A pair that disagrees in (label, row), a negative key or a label above 2^31 - 2 is
          the error "rings not closed", for every window of the band.

`translated` is the other formulation: rasterize_ref.rasterize of the rings moved by (-256 x0, -256 r0) on a raster of the box's
size.  Translation by whole pixels is exact in the rule, and clamping cx to the window instead of the scene keeps the parity.
"""
from __future__ import annotations

import numpy as np

import rasterize_ref as Z

SUBPIXEL, HALF = Z.SUBPIXEL, Z.HALF
MAX_LABEL = (1 << 31) - 2


def _ceil_div(a, b):
    return -((-a) // b)


def edge_band_events(x0, y0, x1, y1, r0, r1, W):
    """(rows, cx) int64 arrays: the events of one fixed-point edge in the band [r0, r1).  The rows come from two ceiling divisions,
    not from a test of every row, so a band of a 2^20-row scene costs what it holds."""
    x0, y0, x1, y1 = int(x0), int(y0), int(x1), int(y1)
    none = np.zeros(0, np.int64)
    if y0 == y1:
        return none, none
    if y0 > y1:
        x0, y0, x1, y1 = x1, y1, x0, y0
    dy = y1 - y0
    lo, hi = max(r0, _ceil_div(y0 - HALF, SUBPIXEL)), min(r1 - 1, _ceil_div(y1 - HALF, SUBPIXEL) - 1)
    if hi < lo:
        return none, none
    rows = np.arange(lo, hi + 1, dtype=np.int64)
    yc = SUBPIXEL * rows + HALF
    num = x0 * dy + (yc - y0) * (x1 - x0)
    assert abs(x0 * dy) < 1 << 60 and (np.abs(num) < 1 << 60).all()
    return rows, np.clip(_ceil_div(num - HALF * dy, SUBPIXEL * dy), 0, W)


def band_keys(ring_ptr, xy_fixed, ring_label, H, W, r0, r1) -> np.ndarray:
    """int64 [N], SORTED: the keys of the band [r0, r1)."""
    assert 0 <= r0 < r1 <= H and W >= 1
    ring_ptr, xy = np.asarray(ring_ptr, np.int64), np.asarray(xy_fixed, np.int64).reshape(-1, 2)
    labels = np.asarray(ring_label, np.int64)
    rows_n = r1 - r0
    assert (int(labels.max()) + 1 if labels.size else 1) * rows_n * (W + 1) < 1 << 63
    keys = [np.zeros(0, np.int64)]
    for r, l in enumerate(labels.tolist()):
        p = xy[ring_ptr[r]:ring_ptr[r + 1]]
        for (ax, ay), (bx, by) in zip(p.tolist(), np.roll(p, -1, 0).tolist()):
            rows, cx = edge_band_events(ax, ay, bx, by, r0, r1, W)
            keys.append((l * rows_n + (rows - r0)) * (W + 1) + cx)
    return np.sort(np.concatenate(keys))


def fill_window(keys, r0, r1, W, x0, x1, fill=-1):
    """(int32 [r1 - r0, x1 - x0], error) from the SORTED keys of the band."""
    assert keys.size % 2 == 0 and 0 <= x0 < x1 <= W
    rows_n = r1 - r0
    out = np.full((rows_n, x1 - x0), fill, np.int32)
    error = False
    for a, b in zip(keys[0::2].tolist(), keys[1::2].tolist()):
        ga, gb = a // (W + 1), b // (W + 1)
        label = ga // rows_n
        if a < 0 or ga != gb or label > MAX_LABEL:
            error = True
            continue
        row, ca, cb = ga - label * rows_n, a - ga * (W + 1), b - gb * (W + 1)
        lo, hi = max(ca, x0), min(cb, x1)
        if lo < hi:
            np.maximum(out[row, lo - x0:hi - x0], label, out=out[row, lo - x0:hi - x0])
    return out, error


def read(ring_ptr, xy_fixed, ring_label, H, W, box, fill=-1) -> np.ndarray:
    """RingSource.read(y0, y1, x0, x1): the spec."""
    y0, y1, x0, x1 = box
    keys = band_keys(ring_ptr, xy_fixed, ring_label, H, W, y0, y1)
    if keys.size % 2:
        raise RuntimeError("rings not closed")
    out, error = fill_window(keys, y0, y1, W, x0, x1, fill)
    if error:
        raise RuntimeError("rings not closed")
    return out


def tile_grid(H, W, tile):
    th, tw = (tile, tile) if isinstance(tile, int) else tile
    return [(y, min(H, y + th), x, min(W, x + tw)) for y in range(0, H, th) for x in range(0, W, tw)]


def rasterize_tiled(ring_ptr, xy_fixed, ring_label, H, W, tile, fill=-1) -> np.ndarray:
    """scene.rasterize_rings: the spec.  One sort per row of tiles, one fill per tile."""
    out = np.empty((H, W), np.int32)
    band, keys = None, None
    for y0, y1, x0, x1 in tile_grid(H, W, tile):
        if band != (y0, y1):
            band, keys = (y0, y1), band_keys(ring_ptr, xy_fixed, ring_label, H, W, y0, y1)
        out[y0:y1, x0:x1], error = fill_window(keys, y0, y1, W, x0, x1, fill)
        if error:
            raise RuntimeError("rings not closed")
    return out


def translated(ring_ptr, xy_fixed, ring_label, box, fill=-1) -> np.ndarray:
    """The box from rasterize_ref.rasterize on the rings moved by whole pixels: defined for any scene size."""
    y0, y1, x0, x1 = box
    moved = np.asarray(xy_fixed, np.int64).reshape(-1, 2) - np.array([SUBPIXEL * x0, SUBPIXEL * y0], np.int64)
    return Z.rasterize(ring_ptr, moved, ring_label, y1 - y0, x1 - x0, fill)


# ---- fixtures the host and the GPU tests share ----------------------------------------------------------------------------------------------
TILES = ((3, 64), (64, 3), (37, 41), (1 << 12, 1 << 12))          # the last: one tile larger than the scene


def tilings(H, W):
    return TILES + (((1, 1),) if H <= 16 and W <= 16 else ())


def boxes(H, W, n=6, seed=0):
    """Unaligned boxes inside H x W, one-pixel boxes and the whole raster among them."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    out = [(0, H, 0, W), (H - 1, H, W - 1, W), (0, 1, 0, 1), (H // 2, H // 2 + 1, W // 3, W // 3 + 1)]
    for _ in range(n):
        ya, xa = int(rng.integers(0, H)), int(rng.integers(0, W))
        out.append((ya, int(rng.integers(ya + 1, H + 1)), xa, int(rng.integers(xa + 1, W + 1))))
    return out


def big_scene():
    """H = W = 2^20, beyond rag.rasterize's range: rings with fractional coordinates near 2^20, two long diagonals from (-2^20, -2^20)
    to (2^20, 2^20) that bound a thin band along the main diagonal, the label 2^31 - 2; and the boxes to read: the far corner, the
    middle, one on the diagonal away from both.  Returns ((ring_ptr, xy float64, ring_label), H, W, boxes)."""
    S = 1 << 20
    f = float(S)
    polys = [
        (7, [(-f, -f), (f, f), (f, f - 40.25), (-f + 40.25, -f)]),                                     # above-right of the diagonal
        (3, [(-f, -f), (-f, -f + 33.5), (f - 33.5, f), (f, f)]),                                       # below-left of it
        ((1 << 31) - 2, [(f - 60.25, f - 70.5), (f - 10.5, f - 66.125), (f - 3.75, f - 5.25), (f - 50.0, f - 20.0)]),
        (11, [(f - 100.5, f - 30.25), (f, f - 90.0), (f, f), (f - 80.75, f)]),                         # reaches the scene's corner
        (5, [(S / 2 - 20.25, S / 2 - 30.5), (S / 2 + 70.125, S / 2 - 10.0), (S / 2 + 30.0, S / 2 + 60.75)]),
        (5, [(S / 2 + 5.0, S / 2 - 5.0), (S / 2 + 25.0, S / 2 - 2.5), (S / 2 + 20.0, S / 2 + 15.0)]),  # a hole in it
    ]
    bx = [(S - 96, S, S - 112, S), (S // 2 - 40, S // 2 + 56, S // 2 - 50, S // 2 + 62), (300000, 300096, 299950, 300062),
          (S - 1, S, S - 1, S), (0, 96, 0, 112)]
    return Z.pack(polys), S, S, bx


def window_cases():
    """name -> (rings = (ring_ptr, xy float64, ring_label), H, W, tiles): where a band or a window can go wrong."""
    sq = Z._square
    diamond = lambda cx, top, bottom, half: [(cx, top), (cx + half, (top + bottom) / 2), (cx, bottom), (cx - half, (top + bottom) / 2)]
    out = {
        # the left edge lies in tile column 0: for columns 1 and 2 the crossing outside the window must toggle the parity inside
        "three_columns": ([(4, [(2.3, 1.2), (140.6, 4.9), (131.2, 27.7), (9.8, 22.1)])], 30, 150, ((30, 50), (7, 50), (30, 1))),
        "hole_straddles_seams": ([(2, sq(5, 5, 95, 75)), (2, sq(40.25, 30.5, 60.75, 50.5))], 80, 100, ((40, 50), (35, 45))),
        # crossings at X = 50.5 and X = 50.0 both give cx = 50: the x1 of column 0 and the x0 of column 1; X = 100.5 gives cx = 100
        "events_on_window_edges": ([(1, sq(10.5, 3, 50.5, 20)), (2, sq(50.5, 25, 100.5, 35)), (3, sq(50.0, 38, 100.0, 44)),
                                    (4, sq(0, 46, 50.0, 48))], 50, 150, ((16, 50), (50, 50))),
        "span_misses_window": ([(0, sq(3, 3, 9, 9)), (1, sq(120.5, 2.5, 149.5, 11.5))], 12, 150, ((12, 50), (5, 30))),
        # th = 8: row centres 7.5 (band 0's last row), 8.5 and 15.5 (band 1's first and last), 16.5 (band 2's first)
        "vertices_on_band_edge_rows": ([(0, diamond(20, 8.5, 15.5, 9.25)), (1, diamond(45, 7.5, 16.5, 9.25)), (2, diamond(70, 0.5, 23.5, 9.25)),
                                        (3, sq(80, 7.5, 90, 8.5)), (4, sq(80, 15.5, 90, 16.5))], 24, 100, ((8, 100), (8, 33))),
        "overlap_ab_across_seam": ([(3, sq(30, 1, 70, 17)), (5, sq(40.5, 9.5, 90, 25))], 30, 100, ((15, 50),)),
        "overlap_ba_across_seam": ([(5, sq(40.5, 9.5, 90, 25)), (3, sq(30, 1, 70, 17))], 30, 100, ((15, 50),)),
        # spans longer than FILL_CHUNK = 1024 that start at x0 != 0
        "long_spans": ([(6, [(1.3, 0.2), (2498.7, 0.4), (2490.1, 4.9), (7.6, 4.6)]), (9, sq(1100.0, 1, 2300.5, 4))], 5, 2500,
                       ((5, 2500), (2, 1100))),
        "band_without_event": ([(1, sq(2, 1, 30, 10))], 40, 36, ((16, 36), (16, 10))),
        "no_rings": ([], 9, 11, ((4, 5),)),
        "empty_rings": ([(0, []), (3, []), (1, [(3.0, 3.0)])], 9, 11, ((4, 5),)),
        "outside_on_all_sides": ([(2, [(-20.5, 15.0), (30.25, -15.5), (90.75, 12.0), (35.5, 60.25)]), (1, sq(-5, -5, 75, 45))], 40, 70,
                                 ((16, 24), (40, 70))),
    }
    return {name: (Z.pack(polys), H, W, tiles) for name, (polys, H, W, tiles) in out.items()}
