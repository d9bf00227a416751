"""The seam stitch, restated in numpy (the rule: include/deepmerge_hip.h, "seam stitch"; csrc/dm_scene.hip).

a[i], b[i]: the scene-wide ids of the two pixels that face each other across seam position i; S: superpixels of the scene;
peri int64 [S,2]: label_stats' perimeter columns (shared with another label / on the raster border) of every tile, concatenated.
"""
import numpy as np


def seam_stitch(a, b, S, peri):
    """(edges int32 [E,2] with a < b sorted by (a, b), weights int32 [E], the perimeter after the move int64 [S,2])."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    both = (a >= 0) & (a < S) & (b >= 0) & (b < S) & (a != b)
    keys, counts = np.unique(np.minimum(a, b)[both] * S + np.maximum(a, b)[both], return_counts=True)
    edges = np.stack((keys // S, keys % S), 1).astype(np.int32).reshape(-1, 2)
    out = np.array(peri, dtype=np.int64, copy=True)
    for l, f in ((a, b), (b, a)):                                 # the pixel edge of l that faces f, as dm_label_stats sees a neighbour
        own = (l >= 0) & (l < S) & (f != -2)                      # -2: its "outside the raster" marker, the edge stays border
        np.subtract.at(out[:, 1], l[own], 1)                      # the tile counted it as raster border
        other = own & (f != l)
        np.add.at(out[:, 0], l[other], 1)                         # in the scene it faces another label
    return edges, counts.astype(np.int32), out
