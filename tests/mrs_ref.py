"""The multiresolution region merging rule (`rag.mrs`) restated in numpy: the spec the device path is held to, bit for bit.

The rule is stated once, in include/deepmerge_hip.h (dm_region_merge_cost).  State of a round: the state of the mutual-best merge
without point lists (tests/merge_ref.py): C regions, edges int32 [E,2] (a < b, sorted, unique), weights = shared boundary length,
the five statistics of `label_stats` for nb = min(bands, 3) bands.  One round: cost per edge (below) -> `pick_edges` with
margin = float32(scale * scale) -> `fold`, both imported from tests/merge_ref.py unchanged.

All statistics are exact integers.  V = n * sumsq - sum^2 goes through Python integers and float(int), which rounds once to
nearest-even; n, l, b are converted to double one by one; every operation after that is one IEEE double operation, in the
association written in `cost`.
"""
import numpy as np

from merge_ref import STAT_KEYS, fold, pick_edges
from oracle import rag as ORAG


def _V(n, s1, s2):
    """double [R, nb] = float(n * sumsq - sum^2), the integer exact, the conversion rounded once."""
    out = np.empty(s1.shape, np.float64)
    for r in range(s1.shape[0]):
        nr = int(n[r])
        for c in range(s1.shape[1]):
            v = nr * int(s2[r, c]) - int(s1[r, c]) ** 2
            assert v >= 0
            out[r, c] = float(v)
    return out


def _box_len(box):
    box = box.astype(np.int64)
    return 2 * ((box[:, 2] - box[:, 0] + 1) + (box[:, 3] - box[:, 1] + 1))


def cost(stats, edges, weights, shape=0.1, compactness=0.5, band_weights=None):
    """float32 [E]: the merge cost of every edge."""
    st = {k: np.asarray(stats[k]) for k in STAT_KEYS}
    nb = st["sum"].shape[1]
    bw = [1.0] * nb if band_weights is None else [float(v) for v in band_weights]
    assert len(bw) == nb
    edges = np.asarray(edges, np.int32).reshape(-1, 2)
    if edges.shape[0] == 0:
        return np.zeros(0, np.float32)
    a, b = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    w = np.asarray(weights).astype(np.int64)
    n = st["count"].astype(np.int64)
    l = st["peri"][:, 0].astype(np.int64) + st["peri"][:, 1].astype(np.int64)
    n_m, l_m = n[a] + n[b], l[a] + l[b] - 2 * w
    box = st["bbox"].astype(np.int64)
    box_m = np.stack((np.minimum(box[a, 0], box[b, 0]), np.minimum(box[a, 1], box[b, 1]),
                      np.maximum(box[a, 2], box[b, 2]), np.maximum(box[a, 3], box[b, 3])), 1)
    V_r = _V(n, st["sum"], st["sumsq"])
    V_m = _V(n_m, st["sum"][a].astype(np.int64) + st["sum"][b].astype(np.int64),
             st["sumsq"][a].astype(np.int64) + st["sumsq"][b].astype(np.int64))
    f64 = np.float64
    na, nbb, nm = n[a].astype(f64), n[b].astype(f64), n_m.astype(f64)
    la, lb, lm = l[a].astype(f64), l[b].astype(f64), l_m.astype(f64)
    ba, bb, bm = _box_len(box[a]).astype(f64), _box_len(box[b]).astype(f64), _box_len(box_m).astype(f64)
    hc = np.zeros(len(a), f64)
    for c in range(nb):
        hc = hc + f64(bw[c]) * ((np.sqrt(V_m[:, c]) - np.sqrt(V_r[a, c])) - np.sqrt(V_r[b, c]))
    hcm = (lm * np.sqrt(nm) - la * np.sqrt(na)) - lb * np.sqrt(nbb)
    hsm = ((nm * lm) / bm - (na * la) / ba) - (nbb * lb) / bb
    hs = f64(compactness) * hcm + (f64(1.0) - f64(compactness)) * hsm
    f = (f64(1.0) - f64(shape)) * hc + f64(shape) * hs
    return np.where(f > 0.0, f, 0.0).astype(np.float32)


def pixel_regions_ref(tile):
    """(stats, edges, weights) of the start in which pixel (y, x) is region y * W + x, in closed form."""
    tile = np.asarray(tile, np.uint8)
    bands, H, W = tile.shape
    nb = min(bands, 3)
    p = tile[:nb].reshape(nb, H * W).T.astype(np.int64)
    ys, xs = np.mgrid[0:H, 0:W]
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    inner = (xs > 0).astype(np.int64) + (xs + 1 < W) + (ys > 0) + (ys + 1 < H)
    stats = {"count": np.ones(H * W, np.int64), "sum": p.copy(), "sumsq": p * p,
             "bbox": np.stack((xs, ys, xs, ys), 1).astype(np.int32), "peri": np.stack((inner, 4 - inner), 1).astype(np.int64)}
    E = H * (W - 1) + (H - 1) * W
    edges = np.zeros((E, 2), np.int32)
    for y in range(H):
        for x in range(W):
            a = y * W + x
            row = y * (2 * W - 1) + (2 * x if y + 1 < H else x)
            if x + 1 < W:
                edges[row] = (a, a + 1)
                row += 1
            if y + 1 < H:
                edges[row] = (a, a + W)
    return stats, edges, np.ones(E, np.int32)


def mrs_ref(tile, scale, shape=0.1, compactness=0.5, band_weights=None, labels=None, n_labels=None, max_rounds=None, min_regions=0):
    """The dict `merge_ref.merge_regions_ref` returns (pooled float32 [C,0], ptr zeros, idx empty), plus "clamped": the number
    of edge costs over the run that the clamp set to 0 while some edge of the round was a candidate."""
    tile = np.asarray(tile, np.uint8)
    if labels is None:
        stats, edges, weights = pixel_regions_ref(tile)
        S0 = tile.shape[1] * tile.shape[2]
    else:
        S0 = int(n_labels)
        stats = ORAG.label_stats(np.asarray(labels), tile, S0)
        edges, weights = ORAG.rag_edges(np.asarray(labels), S0)
    margin = np.float32(scale * scale)
    rep = np.arange(S0, dtype=np.int32)
    region_of = np.arange(S0, dtype=np.int32)
    ptr, idx = np.zeros(S0 + 1, np.int32), np.zeros(0, np.int32)
    hist, hist_simi, regions, merges, maps, matchings = [], [], [S0], [], [region_of.copy()], []
    rounds = clamped = 0
    while True:
        C = len(ptr) - 1
        simi = cost(stats, edges, weights, shape, compactness, band_weights)
        if max_rounds is not None and rounds >= max_rounds:
            break
        picked, _ = pick_edges(simi, edges, C, margin) if len(edges) else (np.zeros(0, bool), None)
        n = int(picked.sum())
        if n == 0 or C - n < min_regions:
            break
        clamped += int((simi == 0).sum())
        matchings.append(edges[picked].copy())
        hist.append(np.stack((np.full(n, rounds, np.int32), rep[edges[picked, 0]], rep[edges[picked, 1]]), 1).astype(np.int32))
        hist_simi.append(simi[picked].copy())
        new_id, ptr, idx, edges, weights, stats, rep = fold(ptr, idx, edges, weights, stats, rep, picked)
        region_of = new_id[region_of].astype(np.int32)
        rounds += 1
        regions.append(len(ptr) - 1)
        merges.append(n)
        maps.append(region_of.copy())
    return {"region_of": region_of, "ptr": ptr, "idx": idx, "edges": edges, "weights": weights, "stats": stats,
            "pooled": np.zeros((len(ptr) - 1, 0), np.float32), "simi": simi, "rep": rep, "rounds": rounds,
            "history": np.concatenate(hist).reshape(-1, 3) if hist else np.zeros((0, 3), np.int32),
            "history_simi": np.concatenate(hist_simi) if hist_simi else np.zeros(0, np.float32),
            "regions_per_round": regions, "merges_per_round": merges, "maps": maps, "matchings": matchings, "clamped": clamped}


# ---- input builders the tests share ---------------------------------------------------------------------------------------------
def quadrant_tile(H=24, W=40, bands=3, levels=(60, 120, 180, 90), seed=3, sigma=4.0):
    """uint8 [bands,H,W]: four quadrants of constant level plus normal noise, clipped."""
    base = np.empty((H, W), np.float64)
    base[:H // 2, :W // 2], base[:H // 2, W // 2:], base[H // 2:, :W // 2], base[H // 2:, W // 2:] = levels
    noise = np.random.default_rng(seed).normal(0, sigma, (bands, H, W))
    return np.clip(base[None] + noise, 0, 255).astype(np.uint8)


def big_count_stats():
    """Two regions of 2^30 pixels each and one edge: V of the regions and of the union exceeds 2^64 in every band (up to about 2^74)."""
    n = 1 << 30
    count = np.array([n, n], np.int64)
    s1 = np.array([[100 * n + 12345, 7 * n], [140 * n - 777, 250 * n - 3]], np.int64)
    s2 = np.array([[10400 * n + 999, 80 * n], [20100 * n + 31, 62600 * n]], np.int64)
    bbox = np.array([[0, 0, 32767, 32767], [32768, 0, 65535, 32767]], np.int32)
    peri = np.array([[40000, 98304], [52001, 98304]], np.int64)
    return ({"count": count, "sum": s1, "sumsq": s2, "bbox": bbox, "peri": peri}, np.array([[0, 1]], np.int32),
            np.array([32768], np.int32))
