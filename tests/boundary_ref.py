"""The boundary-score rule of include/deepmerge_hip.h in plain numpy (csrc/dm_boundary.hip): canonical values,
one-pixel-thick boundary bits from shifted comparisons, the match as a maximum filter written as 2 d + 1 shifted ORs per axis, the
four counts on a box.  `brute` is the same rule as a double loop over pixels, for rasters of a few pixels."""
import math

import numpy as np

MAX_TOLERANCE = 64


def canonical(raster, n_ids, mapping=None):
    """int64 [H,W]: the id (mapping[id] with a mapping) where 0 <= id < n_ids, -1 elsewhere and for a negative mapping entry."""
    r = np.asarray(raster).astype(np.int64)
    ok = (r >= 0) & (r < n_ids)
    if mapping is None:
        return np.where(ok, r, -1)
    m = np.maximum(np.asarray(mapping).astype(np.int64), -1)
    return np.where(ok, m[np.where(ok, r, 0)], -1)


def edge_bits(v):
    """bool [H,W]: the right or the lower neighbour exists and has another value."""
    b = np.zeros(v.shape, dtype=bool)
    b[:, :-1] |= v[:, :-1] != v[:, 1:]
    b[:-1, :] |= v[:-1, :] != v[1:, :]
    return b


def dilate(b, d):
    """bool [H,W]: some set pixel within Chebyshev distance d; 2 d + 1 shifted ORs along the row, then along the column."""
    H, W = b.shape
    rows = np.zeros_like(b)
    for s in range(-d, d + 1):
        if s >= 0:
            rows[:, s:] |= b[:, :W - s] if s < W else False
        else:
            rows[:, :W + s] |= b[:, -s:] if -s < W else False
    out = np.zeros_like(b)
    for s in range(-d, d + 1):
        if s >= 0:
            out[s:, :] |= rows[:H - s, :] if s < H else False
        else:
            out[:H + s, :] |= rows[-s:, :] if -s < H else False
    return out


def counts(labels, truth, n_labels, n_truth, d, mapping=None, box=None):
    """(n_truth_b, hit_truth, n_label_b, hit_label) as Python integers."""
    assert 0 <= d <= MAX_TOLERANCE
    vl, vt = canonical(labels, n_labels, mapping), canonical(truth, n_truth)
    H, W = vl.shape
    y0, y1, x0, x1 = (0, H, 0, W) if box is None else box
    assert 0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W
    bl, bt = edge_bits(vl), edge_bits(vt)
    ml, mt = dilate(bl, d), dilate(bt, d)
    inside = np.zeros((H, W), dtype=bool)
    inside[y0:y1, x0:x1] = True
    return (int((bt & inside).sum()), int((bt & ml & inside).sum()), int((bl & ((vt >= 0) | mt) & inside).sum()),
            int((bl & mt & inside).sum()))


def brute(labels, truth, n_labels, n_truth, d, mapping=None, box=None):
    """The rule pixel by pixel: every loop is the sentence it stands for."""
    labels, truth = np.asarray(labels), np.asarray(truth)
    H, W = labels.shape
    y0, y1, x0, x1 = (0, H, 0, W) if box is None else box

    def value(raster, n, y, x, m):
        i = int(raster[y, x])
        if not 0 <= i < n:
            return -1
        return i if m is None else max(int(m[i]), -1)

    def boundary(raster, n, y, x, m):
        v = value(raster, n, y, x, m)
        return (x + 1 < W and value(raster, n, y, x + 1, m) != v) or (y + 1 < H and value(raster, n, y + 1, x, m) != v)

    def match(raster, n, y, x, m):
        return any(boundary(raster, n, yy, xx, m) for yy in range(max(0, y - d), min(H, y + d + 1))
                   for xx in range(max(0, x - d), min(W, x + d + 1)))

    n_t = h_t = n_l = h_l = 0
    for y in range(y0, y1):
        for x in range(x0, x1):
            if boundary(truth, n_truth, y, x, None):
                n_t += 1
                h_t += match(labels, n_labels, y, x, mapping)
            if boundary(labels, n_labels, y, x, mapping):
                near = match(truth, n_truth, y, x, None)
                n_l += value(truth, n_truth, y, x, None) >= 0 or near
                h_l += near
    return n_t, h_t, n_l, h_l


def scores(c):
    """recall, precision, f from the four counts; NaN where a denominator is zero."""
    n_t, h_t, n_l, h_l = c
    r = h_t / n_t if n_t else math.nan
    p = h_l / n_l if n_l else math.nan
    return {"recall": r, "precision": p, "f": 2 * p * r / (p + r) if p + r > 0 else math.nan}


def nearest_seed(H, W, n, seed):
    """int32 [H,W]: every pixel labelled by the nearest of n random seed points (squared Euclidean distance, ties to the smaller id)."""
    rng = np.random.default_rng(seed)
    sy, sx = rng.integers(0, H, n), rng.integers(0, W, n)
    y, x = np.mgrid[0:H, 0:W]
    d2 = (y[None] - sy[:, None, None]) ** 2 + (x[None] - sx[:, None, None]) ** 2
    return d2.argmin(0).astype(np.int32)


def small_pair(H, W, seed):
    """(labels, n_labels, truth, n_truth) for a raster of any size down to 1 x 1: a few regions and objects, with ids outside
    the range on both rasters."""
    S, G = min(9, H * W), min(4, H * W)
    labels, truth = nearest_seed(H, W, S, seed), nearest_seed(H, W, G, seed + 1)
    rng = np.random.default_rng(seed + 2)
    for raster, bad in ((labels, (-1, S, S + 3)), (truth, (-1, -7, G + 1))):
        for v in bad:
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            raster[y:y + 1 + H // 8, x:x + 1 + W // 6] = v
    return labels, S, truth, G


def hand_merge(S0, rounds, device):
    """A `rag.MergeResult` built by hand from its history: rounds = per round a list of (survivor, absorbed) original ids.  Only
    the fields `region_of_at` reads carry content."""
    import torch
    from deepmerge_amd import rag
    history = [(r + 1, a, b) for r, pairs in enumerate(rounds) for a, b in pairs]
    empty = torch.empty(0, dtype=torch.int32, device=device)
    res = rag.MergeResult(region_of=torch.zeros(S0, dtype=torch.int32, device=device), ptr=empty, idx=empty, edges=empty.reshape(0, 2),
                          weights=None, stats=None, pooled=empty, simi=empty, rep=empty, rounds=len(rounds),
                          history=torch.tensor(history, dtype=torch.int32, device=device).reshape(-1, 3),
                          history_simi=torch.zeros(len(history), device=device), regions_per_round=[],
                          merges_per_round=[len(p) for p in rounds])
    res.region_of = res.region_of_at(len(rounds))
    return res


def region_of_at(S0, rounds, r):
    """numpy int32 [S0]: what `MergeResult.region_of_at(r)` gives for `hand_merge(S0, rounds)`: regions numbered by their
    smallest original id."""
    parent = np.arange(S0)
    for pairs in rounds[:r]:
        for a, b in pairs:
            parent[b] = a
    for _ in range(S0):
        parent = parent[parent]
    return (np.cumsum(parent == np.arange(S0)) - 1)[parent].astype(np.int32)


def scene_pair(H=200, W=232):
    """(labels, n_labels, truth, n_truth): about 60 regions against about 12 objects with a band of unlabelled pixels."""
    labels, truth = nearest_seed(H, W, 60, 11), nearest_seed(H, W, 12, 12)
    truth[H // 2 - 9:H // 2 + 8, :] = -1
    truth[:, W // 3:W // 3 + 5] = 12 + 4                          # unlabelled by an id behind the range as well
    return labels, 60, truth, 12
