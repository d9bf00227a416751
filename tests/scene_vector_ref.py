"""Spec (numpy, integers only) of the per-tile dart records behind scene.trace_labels (csrc/dm_scene_vector.hip).

The rule is tests/vector_ref.py's, read through a window: a tile of a scene is a core box and its window, the core grown by one
pixel on every side and clipped to the scene.  Only the core's pixels own darts.  Outside the window counts as outside the raster
(label -1); for a core dart that is only ever asked where the window's edge is the scene's edge.  A record is
  id          4 ((y + oy) W + (x + ox)) + side: the dart's scene-wide id (W: the scene's width, (ox, oy): the window's first pixel)
  succ        the scene-wide id of its successor, whose pixel may be an apron pixel
  lab, other  the pixel's label and the label across the side (-1 outside)
  succ_flags  the flags of the SUCCESSOR: 1 if its side differs from this dart's (vertex dart), 2 if its `other` differs (break dart)
Slow and plain on purpose.
"""
from __future__ import annotations

import numpy as np

import vector_ref as V


def tile_records(window: np.ndarray, core, origin, scene_w: int):
    """Records of the core (cy0, cy1, cx0, cx1) of `window` (both in window coordinates), the window's first pixel at origin =
    (oy, ox) of a scene `scene_w` wide.  Returns a dict of arrays in ascending id: id, succ int64; lab, other int32; succ_flags uint8."""
    L = np.asarray(window)
    cy0, cy1, cx0, cx1 = core
    oy, ox = int(origin[0]), int(origin[1])
    W = int(scene_w)
    rows = []
    for y in range(cy0, cy1):
        for x in range(cx0, cx1):
            l = int(L[y, x])
            for s in range(4):
                o = V._label(L, x + V.DY[s], y - V.DX[s])
                if o == l:
                    continue
                arx, ary = x + V.DX[s], y + V.DY[s]                # ahead-right
                alx, aly = arx + V.DY[s], ary - V.DX[s]             # ahead-left
                if V._label(L, arx, ary) != l:
                    qx, qy, t = x, y, (s + 1) & 3
                elif V._label(L, alx, aly) != l:
                    qx, qy, t = arx, ary, s
                else:
                    qx, qy, t = alx, aly, (s + 3) & 3
                across = V._label(L, qx + V.DY[t], qy - V.DX[t])
                rows.append((4 * ((y + oy) * W + (x + ox)) + s, 4 * ((qy + oy) * W + (qx + ox)) + t, l, o, (t != s) | ((across != o) << 1)))
    cols = list(zip(*rows)) if rows else [[]] * 5
    return {"id": np.asarray(cols[0], np.int64), "succ": np.asarray(cols[1], np.int64), "lab": np.asarray(cols[2], np.int32),
            "other": np.asarray(cols[3], np.int32), "succ_flags": np.asarray(cols[4], np.uint8)}


def scene_records(labels: np.ndarray, tile):
    """The records of every tile of `labels` cut into cores of `tile` = (th, tw), concatenated in tile order: what the join takes."""
    L = np.asarray(labels)
    H, W = L.shape
    th, tw = tile
    parts = []
    for y0 in range(0, H, th):
        for x0 in range(0, W, tw):
            y1, x1 = min(H, y0 + th), min(W, x0 + tw)
            wy0, wy1, wx0, wx1 = max(0, y0 - 1), min(H, y1 + 1), max(0, x0 - 1), min(W, x1 + 1)
            parts.append(tile_records(L[wy0:wy1, wx0:wx1], (y0 - wy0, y1 - wy0, x0 - wx0, x1 - wx0), (wy0, wx0), W))
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def raster_flags(d: dict, nxt: dict) -> dict:
    """dart id -> flags of the one-raster rule (vector_ref.successor_map's d and nxt): 1 vertex dart, 2 break dart."""
    out = {}
    for i, j in nxt.items():
        out[j] = int(d[j][2] != d[i][2]) | (int(d[j][4] != d[i][4]) << 1)
    return out
