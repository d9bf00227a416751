"""What the tests of the label-raster scene path share (deepmerge_amd/scene.py: sample_points, label_graph, segment_labels,
mrs_labels; csrc/dm_scene_points.hip): the key in Python integers, the two label rasters and the numpy facts about them.

The key (include/deepmerge_hip.h).  Largest score, then smallest scene linear index y * W + x: bits 56..63 the score, bits 8..55
2^48 - 1 - lin, bits 0..7 the pixel's clearance.  Positions are unique, so the clearance never decides an order.
"""
import numpy as np

import points_ref as PR

LIN_BITS = 48
LIN_MASK = (1 << LIN_BITS) - 1
MAX_PIXELS = 1 << LIN_BITS

H, W, TILE = 200, 232, (96, 112)      # the scene of tests/test_gpu_scene.py: 9 tiles, both axes end in an 8-pixel sliver
SEED_A = 9                            # 21 of its 30 regions have pixels in two tiles or more, 4 of them in four


def pack_key(score: int, lin: int, clearance: int) -> int:
    assert 0 <= score <= 255 and 0 <= clearance <= 255 and 0 <= lin < MAX_PIXELS
    return (score << 56) | ((LIN_MASK - lin) << 8) | clearance


def unpack_key(key: int):
    """(score, lin, clearance)"""
    return key >> 56, LIN_MASK - ((key >> 8) & LIN_MASK), key & 255


def tiles_of(H, W, tile):
    th, tw = tile
    return [(y, min(H, y + th), x, min(W, x + tw)) for y in range(0, H, th) for x in range(0, W, tw)]


def tile_index(y, x, W, tile):
    th, tw = tile
    return (np.asarray(y) // th) * ((W + tw - 1) // tw) + np.asarray(x) // tw


def tiles_per_label(labels, S, tile):
    """int [S]: in how many tiles every id of [0, S) has pixels."""
    Hh, Ww = labels.shape
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    t = tile_index(yy, xx, Ww, tile)
    ok = (labels >= 0) & (labels < S)
    pairs = np.unique(np.stack((labels[ok].astype(np.int64), t[ok]), 1), axis=0)
    return np.bincount(pairs[:, 0], minlength=S)


def raster_a():
    """(a) jittered Voronoi regions of cell 40: they know nothing of the tile grid."""
    return PR.voronoi_labels(H, W, 40, SEED_A)


FRAME, BLOCK, STRIPE, CORNERS, ABSENT, S_B = 0, 65, 66, (67, 68, 69, 70), 71, 72
STRIPE_ROWS = (185, 190)


def raster_b():
    """(b) the designed raster.  A grid of 25 x 29 cells (ids 1..64) under:
    id 0: a frame of width 2 and a cross (rows 180..183, columns 200..203): pixels in all nine tiles;
    id 65: a 150 x 150 block over the first seam crossing (four tiles), clearance 75 at its centre;
    id 66: a stripe of 5 rows across the full width: its centre line has clearance 3 from x = 2 to x = W - 3, a tie over three tiles;
    ids 67..70: single pixels on the four corners of the seam crossing (192, 224);
    -1 painted over the seams y = 96 and x = 224;  id 71 never occurs (nor do the cells the block covers)."""
    yy, xx = np.mgrid[0:H, 0:W]
    lab = (1 + (yy // 25) * 8 + xx // 29).astype(np.int32)
    assert lab.max() == 64
    lab[20:170, 30:180] = BLOCK
    lab[180:184, :] = FRAME
    lab[:, 200:204] = FRAME
    lab[:2, :] = FRAME
    lab[-2:, :] = FRAME
    lab[:, :2] = FRAME
    lab[:, -2:] = FRAME
    lab[STRIPE_ROWS[0]:STRIPE_ROWS[1], :] = STRIPE
    for s, (y, x) in zip(CORNERS, ((191, 223), (191, 224), (192, 223), (192, 224))):
        lab[y, x] = s
    lab[90:101, 215:229] = -1
    return lab, S_B


def scene_image():
    """Coarse colour blocks + noise, as tests/test_gpu_scene.py builds its scene."""
    rng = np.random.default_rng(12)
    base = rng.integers(0, 256, (3, 4, 4)).astype(np.uint8)
    full = np.clip(np.kron(base, np.ones((64, 64), np.uint8)).astype(np.int64) + rng.integers(-8, 9, (3, 256, 256)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(full[:, :H, :W])


def seam_pairs(labels, tile):
    """(a, b): the ids that face each other across every seam position of the grid."""
    th, tw = tile
    Hh, Ww = labels.shape
    a = [labels[:, x - 1] for x in range(tw, Ww, tw)] + [labels[y - 1, :] for y in range(th, Hh, th)]
    b = [labels[:, x] for x in range(tw, Ww, tw)] + [labels[y, :] for y in range(th, Hh, th)]
    return np.concatenate(a), np.concatenate(b)


def edge_tiles(labels, S, tile):
    """dict (a, b) -> number of sources (tiles, and 1 for all seams) in which the 4-neighbour pair a < b occurs."""
    seen = {}

    def add(p, q, src):
        ok = (p != q) & (p >= 0) & (p < S) & (q >= 0) & (q < S)
        for u, v in set(zip(np.minimum(p[ok], q[ok]).tolist(), np.maximum(p[ok], q[ok]).tolist())):
            seen.setdefault((u, v), set()).add(src)

    for i, (y0, y1, x0, x1) in enumerate(tiles_of(*labels.shape, tile)):
        c = labels[y0:y1, x0:x1]
        add(c[:, :-1].ravel(), c[:, 1:].ravel(), i)
        add(c[:-1, :].ravel(), c[1:, :].ravel(), i)
    add(*seam_pairs(labels, tile), "seam")
    return {k: len(v) for k, v in seen.items()}
