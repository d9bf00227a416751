"""The minimum-region-area rule of the merge (`merge_regions(min_area=)`, `mrs(min_area=)`) restated in numpy: the spec the device
path is held to, bit for bit.  The rule is stated once, in include/deepmerge_hip.h; the rounds it extends are tests/merge_ref.py's.

Phase 1: merge_ref's rounds (score -> pick_edges -> fold), unchanged, until a round picks nothing.
Phase 2, only if phase 1 ended because nothing was picked (not at max_rounds, not at min_regions), and only with min_area > 0:
region r is small iff count[r] < min_area (int64).  One elimination round:
  1. score      the partition as it is (the same score as phase 1)
  2. propose    an edge is usable iff simi == simi; every small region takes best[s] = min over its usable edges of the unsigned
                64-bit key (bits(simi) << 32) | other_id; non-small regions get all-ones
  3. accept     a non-small region t takes best[t] = min of (bits(simi) << 32) | s over the small s whose best[s] names t
  4. match, fold, history: as in phase 1 -- (a, b) picked iff best[a] names b and best[b] names a
Stop when a round picks nothing, at max_rounds (which counts both phases), or before a round that would leave fewer than
min_regions regions.  Phase 2 never goes back to phase 1.
"""
import numpy as np

import merge_ref as M
import mrs_ref as R
from merge_ref import NO_BEST, STAT_KEYS


def pick_small(simi, edges, C, count, min_area):
    """(picked bool [E], best uint64 [C]) of steps 2 to 4."""
    edges = np.asarray(edges, np.int32).reshape(-1, 2)
    simi = np.asarray(simi, np.float32)
    a, b = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    small = np.asarray(count, np.int64) < np.int64(min_area)
    usable = simi == simi
    hi = simi.view(np.uint32).astype(np.uint64) << np.uint64(32)
    ka, kb = hi | b.astype(np.uint64), hi | a.astype(np.uint64)   # the key an edge offers its a side / its b side
    best = np.full(C, NO_BEST, dtype=np.uint64)
    m = usable & small[a]
    np.minimum.at(best, a[m], ka[m])
    m = usable & small[b]
    np.minimum.at(best, b[m], kb[m])
    other = np.where(best == NO_BEST, -1, (best & np.uint64(0xFFFFFFFF)).astype(np.int64))      # the proposals, final
    m = usable & small[a] & ~small[b] & (other[a] == b)
    np.minimum.at(best, b[m], kb[m])
    m = usable & small[b] & ~small[a] & (other[b] == a)
    np.minimum.at(best, a[m], ka[m])
    other = np.where(best == NO_BEST, -1, (best & np.uint64(0xFFFFFFFF)).astype(np.int64))
    picked = (other[a] == b) & (other[b] == a)
    return picked, best


def _rounds(score, margin, ptr, idx, edges, weights, stats, max_rounds, min_regions, min_area):
    """Both phases around score(ptr, idx, edges, weights, stats) -> (pooled, simi)."""
    S0 = len(ptr) - 1
    min_area = int(min_area)
    assert min_area >= 0 and (min_area == 0 or stats is not None)
    rep = np.arange(S0, dtype=np.int32)
    region_of = np.arange(S0, dtype=np.int32)
    hist, hist_simi, regions, merges, maps, matchings = [], [], [S0], [], [region_of.copy()], []
    rounds = small_rounds = 0
    small_phase = False
    while True:
        C = len(ptr) - 1
        pooled, simi = score(ptr, idx, edges, weights, stats)
        if max_rounds is not None and rounds >= max_rounds:
            break
        if len(edges) == 0:
            break
        if small_phase:
            picked, _ = pick_small(simi, edges, C, stats["count"], min_area)
        else:
            picked, _ = M.pick_edges(simi, edges, C, margin)
        n = int(picked.sum())
        if n == 0 and not small_phase and min_area > 0:
            small_phase = True                                   # the scores are those of this partition: step 1 of the first
            picked, _ = pick_small(simi, edges, C, stats["count"], min_area)           # elimination round is done
            n = int(picked.sum())
        if n == 0 or C - n < min_regions:
            break
        matchings.append(edges[picked].copy())
        hist.append(np.stack((np.full(n, rounds, np.int32), rep[edges[picked, 0]], rep[edges[picked, 1]]), 1).astype(np.int32))
        hist_simi.append(simi[picked].copy())
        new_id, ptr, idx, edges, weights, stats, rep = M.fold(ptr, idx, edges, weights, stats, rep, picked)
        region_of = new_id[region_of].astype(np.int32)
        rounds += 1
        small_rounds += int(small_phase)
        regions.append(len(ptr) - 1)
        merges.append(n)
        maps.append(region_of.copy())
    return {"region_of": region_of, "ptr": ptr, "idx": idx, "edges": edges, "weights": weights, "stats": stats, "pooled": pooled,
            "simi": simi, "rep": rep, "rounds": rounds, "small_rounds": small_rounds,
            "history": np.concatenate(hist).reshape(-1, 3) if hist else np.zeros((0, 3), np.int32),
            "history_simi": np.concatenate(hist_simi) if hist_simi else np.zeros(0, np.float32),
            "regions_per_round": regions, "merges_per_round": merges, "maps": maps, "matchings": matchings}


def merge_regions_ref(F, ptr, idx, edges, margin=1.0, weights=None, stats=None, max_rounds=None, min_regions=0, min_area=0):
    """merge_ref.merge_regions_ref's dict plus "small_rounds": the same rounds around merge_ref.score."""
    F = np.ascontiguousarray(F, np.float32)
    ptr, idx, edges = np.asarray(ptr, np.int32), np.asarray(idx, np.int32), np.asarray(edges, np.int32).reshape(-1, 2)
    if stats is not None:
        stats = {k: np.asarray(stats[k]) for k in STAT_KEYS}
    return _rounds(lambda p, i, e, w, st: M.score(F, p, i, e, margin), margin, ptr, idx, edges, weights, stats, max_rounds, min_regions,
                   min_area)


def mrs_ref(tile, scale, shape=0.1, compactness=0.5, band_weights=None, labels=None, n_labels=None, max_rounds=None, min_regions=0,
            min_area=0):
    """mrs_ref.mrs_ref's dict (without "clamped") plus "small_rounds": the same rounds around mrs_ref.cost."""
    tile = np.asarray(tile, np.uint8)
    if labels is None:
        stats, edges, weights = R.pixel_regions_ref(tile)
        S0 = tile.shape[1] * tile.shape[2]
    else:
        S0 = int(n_labels)
        stats = R.ORAG.label_stats(np.asarray(labels), tile, S0)
        edges, weights = R.ORAG.rag_edges(np.asarray(labels), S0)
    stats = {k: np.asarray(stats[k]) for k in STAT_KEYS}

    def score(ptr, idx, edges, weights, stats):
        return np.zeros((len(ptr) - 1, 0), np.float32), R.cost(stats, edges, weights, shape, compactness, band_weights)

    return _rounds(score, np.float32(scale * scale), np.zeros(S0 + 1, np.int32), np.zeros(0, np.int32), edges, weights, stats,
                   max_rounds, min_regions, min_area)


# ---- input builders the tests share ---------------------------------------------------------------------------------------------
def graph_stats(S, seed, count=None):
    """Synthetic statistics for a graph without a raster: random `count` in 1..59 (or the one given), consistent integers elsewhere."""
    rng = np.random.default_rng(seed)
    count = rng.integers(1, 60, S).astype(np.int64) if count is None else np.asarray(count, np.int64)
    s1 = rng.integers(0, 256, (S, 3)).astype(np.int64) * count[:, None]
    x0, y0 = rng.integers(0, 100, S), rng.integers(0, 100, S)
    return {"count": count, "sum": s1, "sumsq": s1 * 200,
            "bbox": np.stack((x0, y0, x0 + rng.integers(0, 9, S), y0 + rng.integers(0, 9, S)), 1).astype(np.int32),
            "peri": rng.integers(200, 400, (S, 2)).astype(np.int64)}


def add_outliers(case, share=0.15, seed=0):
    """merge_ref.raster_case's features with `share` of the superpixels moved far from every block centre, each to a place of its
    own: the leftovers a margin merge keeps (a shadow, a car, a roof patch).  Returns a copy of the features."""
    rng = np.random.default_rng(seed)
    F = case["F"].copy()
    S = case["S"]
    member = case["labels"][case["xy"][:, 1], case["xy"][:, 0]]
    out = rng.random(S) < share
    shift = (rng.standard_normal((S, F.shape[1])) * 6.0).astype(np.float32)
    F[out[member]] += shift[member[out[member]]]
    return np.ascontiguousarray(F, np.float32)
