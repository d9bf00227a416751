"""The mutual-best-neighbour merge rule restated in numpy (the spec `rag.merge_regions` is held to, bit for bit), and the
input builders its tests share.

State of a round: C regions 0..C-1, CSR point lists ptr / idx, edges int32 [E,2] (a < b, sorted, unique), optional weights,
optional statistics, rep = smallest original superpixel id of each region.  One round:
  1. score      pooled = strict_segment_mean, simi = strict_edge_similarity (oracle/sweep.py: the sweep's pinned order)
  2. best       candidate iff simi < margin (float32; NaN is none); best[r] = min over r's candidate edges of the unsigned
                64-bit key (bits(simi) << 32) | other_id
  3. match      (a, b) picked iff best[a] names b and best[b] names a; b is absorbed into a
  4. fold       dense ids in order of the surviving region's old id; points of a then of b; edges relabelled, self edges
                dropped, duplicates folded with weights added, sorted; count / sum / sumsq / border perimeter added, bbox
                min / max, inner perimeter peri_a + peri_b - 2 weight(a, b); rep' = rep[a]
  5. history    (round, rep[a], rep[b]) and simi per picked edge, in edge order
Stop when nothing is picked, after max_rounds rounds, or before a round that would leave fewer than min_regions regions.
`pooled` / `simi` of the result are the scoring of the final partition.
"""
import numpy as np

from oracle import sweep as OS

NO_BEST = np.uint64(0xFFFFFFFFFFFFFFFF)
STAT_KEYS = ("count", "sum", "sumsq", "bbox", "peri")


def score(F, ptr, idx, edges, margin):
    pooled = OS.strict_segment_mean(F, ptr, idx)
    if edges.shape[0] == 0:
        return pooled, np.zeros(0, np.float32)
    return pooled, OS.strict_edge_similarity(pooled, edges, margin)[0]


def pick_edges(simi, edges, C, margin):
    """(picked bool [E], best uint64 [C]) of steps 2 and 3."""
    a, b = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    with np.errstate(invalid="ignore"):
        cand = np.less(simi, np.float32(margin))
    hi = simi.view(np.uint32).astype(np.uint64) << np.uint64(32)
    best = np.full(C, NO_BEST, dtype=np.uint64)
    np.minimum.at(best, a[cand], hi[cand] | b[cand].astype(np.uint64))
    np.minimum.at(best, b[cand], hi[cand] | a[cand].astype(np.uint64))
    other = np.where(best == NO_BEST, -1, (best & np.uint64(0xFFFFFFFF)).astype(np.int64))
    picked = cand & (other[a] == b) & (other[b] == a)
    return picked, best


def fold(ptr, idx, edges, weights, stats, rep, picked):
    """Step 4.  Returns (new_id int64 [C], ptr', idx', edges', weights', stats', rep')."""
    C = len(ptr) - 1
    a, b = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    root = np.arange(C)
    root[b[picked]] = a[picked]
    is_root = root == np.arange(C)
    new_id = (np.cumsum(is_root) - 1)[root]
    C2 = int(is_root.sum())
    lens = np.diff(ptr).astype(np.int64)
    owner = np.repeat(new_id, lens)                              # entries in old CSR order: a's points come before b's (a < b)
    new_idx = idx[np.argsort(owner, kind="stable")].astype(np.int32)
    new_ptr = np.zeros(C2 + 1, dtype=np.int64)
    np.add.at(new_ptr, new_id + 1, lens)
    new_ptr = np.cumsum(new_ptr).astype(np.int32)
    na, nb = new_id[a], new_id[b]
    keep = na != nb
    lo, hi = np.minimum(na[keep], nb[keep]), np.maximum(na[keep], nb[keep])
    keys, inv = np.unique(lo * C2 + hi, return_inverse=True)
    new_edges = np.stack((keys // C2, keys % C2), 1).astype(np.int32).reshape(-1, 2)
    new_w = None
    if weights is not None:
        acc = np.zeros(len(keys), dtype=np.int64)
        np.add.at(acc, inv.reshape(-1), weights[keep].astype(np.int64))
        new_w = acc.astype(np.int32)
    new_stats = None
    if stats is not None:
        new_stats = {}
        for k in ("count", "sum", "sumsq", "peri"):
            acc = np.zeros((C2,) + stats[k].shape[1:], dtype=np.int64)
            np.add.at(acc, new_id, stats[k])
            new_stats[k] = acc
        new_stats["peri"][new_id[a[picked]], 0] -= 2 * weights[picked].astype(np.int64)
        box = np.empty((C2, 4), dtype=np.int32)
        box[:, :2] = np.iinfo(np.int32).max
        box[:, 2:] = -1
        for c in (0, 1):
            np.minimum.at(box[:, c], new_id, stats["bbox"][:, c])
            np.maximum.at(box[:, c + 2], new_id, stats["bbox"][:, c + 2])
        new_stats["bbox"] = box
    return new_id, new_ptr, new_idx, new_edges, new_w, new_stats, rep[is_root]


def merge_regions_ref(F, ptr, idx, edges, margin=1.0, weights=None, stats=None, max_rounds=None, min_regions=0):
    F = np.ascontiguousarray(F, np.float32)
    ptr, idx, edges = np.asarray(ptr, np.int32), np.asarray(idx, np.int32), np.asarray(edges, np.int32).reshape(-1, 2)
    S0 = len(ptr) - 1
    if stats is not None:
        stats = {k: np.asarray(stats[k]) for k in STAT_KEYS}
    rep = np.arange(S0, dtype=np.int32)
    region_of = np.arange(S0, dtype=np.int32)
    hist, hist_simi, regions, merges, maps, matchings = [], [], [S0], [], [region_of.copy()], []
    rounds = 0
    while True:
        C = len(ptr) - 1
        pooled, simi = score(F, ptr, idx, edges, margin)
        if max_rounds is not None and rounds >= max_rounds:
            break
        picked, _ = pick_edges(simi, edges, C, margin)
        n = int(picked.sum())
        if n == 0 or C - n < min_regions:
            break
        matchings.append(edges[picked].copy())
        hist.append(np.stack((np.full(n, rounds, np.int32), rep[edges[picked, 0]], rep[edges[picked, 1]]), 1).astype(np.int32))
        hist_simi.append(simi[picked].copy())
        new_id, ptr, idx, edges, weights, stats, rep = fold(ptr, idx, edges, weights, stats, rep, picked)
        region_of = new_id[region_of].astype(np.int32)
        rounds += 1
        regions.append(len(ptr) - 1)
        merges.append(n)
        maps.append(region_of.copy())
    return {"region_of": region_of, "ptr": ptr, "idx": idx, "edges": edges, "weights": weights, "stats": stats, "pooled": pooled,
            "simi": simi, "rep": rep, "rounds": rounds,
            "history": np.concatenate(hist).reshape(-1, 3) if hist else np.zeros((0, 3), np.int32),
            "history_simi": np.concatenate(hist_simi) if hist_simi else np.zeros(0, np.float32),
            "regions_per_round": regions, "merges_per_round": merges, "maps": maps, "matchings": matchings}


def region_of_at(history, merges_per_round, S0, k):
    """The map after the first k rounds, replayed from the history alone (what MergeResult.region_of_at does)."""
    parent = np.arange(S0)
    for _, ra, rb in history[:sum(merges_per_round[:k])]:
        parent[rb] = ra
    for s in range(S0):                                          # rep[a] < rep[b]: parents are resolved before their children
        parent[s] = parent[parent[s]]
    is_root = parent == np.arange(S0)
    return (np.cumsum(is_root) - 1)[parent].astype(np.int32)


# ---- input builders -------------------------------------------------------------------------------------------------------
def canonical_edges(raw, S):
    """Random endpoint pairs -> the form merge_regions takes: a < b, unique, sorted by (a, b)."""
    raw = np.asarray(raw, np.int64).reshape(-1, 2)
    raw = raw[raw[:, 0] != raw[:, 1]]
    keys = np.unique(np.minimum(raw[:, 0], raw[:, 1]) * S + np.maximum(raw[:, 0], raw[:, 1]))
    return np.stack((keys // S, keys % S), 1).astype(np.int32).reshape(-1, 2)


def random_graph(S, E, D, seed, groups=8):
    """Random graph over S regions with random CSR point lists (some regions empty); regions of one group embed alike (with 8
    groups and a mean degree of 6 to 8, the like-minded neighbours form clusters that take 5 to 40 rounds to grow)."""
    rng = np.random.default_rng(seed)
    edges = canonical_edges(rng.integers(0, S, size=(E, 2)), S) if E else np.zeros((0, 2), np.int32)
    lens = rng.integers(1, 5, size=S)
    lens[rng.random(S) < 0.02] = 0                               # (empty regions pool to 0 and so resemble each other: keep them rare)
    lens[S // 2] = 0
    if lens.sum() == 0:
        lens[0] = 1
    P = int(lens.sum())
    ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    idx = rng.permutation(P).astype(np.int32)
    group = rng.integers(0, groups, size=S)
    centres = rng.standard_normal((groups, D)).astype(np.float32) * np.float32(3.0)
    F = np.zeros((P, D), np.float32)
    F[idx] = centres[np.repeat(group, lens)] + np.float32(0.05) * rng.standard_normal((P, D)).astype(np.float32)
    weights = rng.integers(1, 50, size=edges.shape[0]).astype(np.int32)
    return F, ptr, idx, edges, weights


def superpixels(H, W, cell, seed):
    """Jittered-grid Voronoi labels (irregular, spatially coherent regions); superpixel ny * gx + nx grows from grid cell (ny, nx)."""
    rng = np.random.default_rng(seed)
    gy, gx = (H + cell - 1) // cell, (W + cell - 1) // cell
    cy = (np.arange(gy)[:, None] + rng.uniform(0.2, 0.8, (gy, gx))) * cell
    cx = (np.arange(gx)[None, :] + rng.uniform(0.2, 0.8, (gy, gx))) * cell
    yy, xx = np.mgrid[0:H, 0:W]
    best = np.full((H, W), np.inf, dtype=np.float32)
    lab = np.zeros((H, W), np.int32)
    by, bx = yy // cell, xx // cell
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ny, nx = np.clip(by + dy, 0, gy - 1), np.clip(bx + dx, 0, gx - 1)
            d = ((yy - cy[ny, nx]) ** 2 + (xx - cx[ny, nx]) ** 2).astype(np.float32)
            upd = d < best
            best[upd] = d[upd]
            lab[upd] = (ny * gx + nx)[upd]
    return lab, gy, gx


def points_to_csr(lab, xy, S):
    member = lab[xy[:, 1], xy[:, 0]].astype(np.int64)
    order = np.argsort(member, kind="stable")
    ptr = np.concatenate(([0], np.cumsum(np.bincount(member, minlength=S)))).astype(np.int32)
    return ptr, order.astype(np.int32)


def raster_case(H, W, cell, bands, block, D, seed, step=None, extra_ids=3):
    """Label raster + tile + sample points + features with one centre per block x block superpixels (+ 0.05 noise): merging at
    margin 1 grows every block into one region, one neighbour per round."""
    lab, gy, gx = superpixels(H, W, cell, seed)
    S = gy * gx + extra_ids                                      # a few ids that never occur
    rng = np.random.default_rng(seed + 1)
    tile = rng.integers(0, 256, (bands, H, W), dtype=np.uint8)
    step = step or max(2, cell // 2)
    ys, xs = np.mgrid[step // 2:H:step, step // 2:W:step]
    xy = np.stack((xs.reshape(-1), ys.reshape(-1)), 1).astype(np.int32)
    ptr, idx = points_to_csr(lab, xy, S)
    bw = (gx + block - 1) // block
    sp = np.arange(gy * gx)
    block_of = np.zeros(S, np.int64)
    block_of[:gy * gx] = ((sp // gx) // block) * bw + (sp % gx) // block
    centres = rng.standard_normal((int(block_of.max()) + 1, D)).astype(np.float32) * np.float32(3.0)
    member = lab[xy[:, 1], xy[:, 0]]
    F = centres[block_of[member]] + np.float32(0.05) * rng.standard_normal((xy.shape[0], D)).astype(np.float32)
    return {"labels": lab, "S": S, "tile": tile, "xy": xy, "ptr": ptr, "idx": idx, "F": np.ascontiguousarray(F, np.float32)}


def is_matching(picked_edges):
    ends = np.asarray(picked_edges).reshape(-1)
    return len(np.unique(ends)) == len(ends)
