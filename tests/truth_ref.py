"""The build's own specification of rag.label_overlap / rag.pair_flags / Overlap.coarsen / Overlap.scores (csrc/dm_truth.hip),
in numpy.

The reference trains from `positive` / `negative` polygon-pair lists made outside the program by comparing the over-segmentation
with a ground-truth map, and never scores a partition against a reference map; this is the rule the build uses for both.
Everything is integer arithmetic, so the kernels must equal this file bit for bit.

Input: labels int32 [H,W], region ids 0..S-1 (ids outside [0,S) are ignored); truth int32 [H,W], object ids 0..G-1 (any other
value is "unlabelled" and counted under the pseudo-object G).  H*W < 2^31, S*(G+1) < 2^62.

Overlap table.  n[s,g] = number of pixels with labels == s and truth column g, g in 0..G; sparse, keys s*(G+1)+g, sorted.
Row facts [S].  area = sum over all G+1 columns; owner = the g < G with the largest n[s,g] >= 1, ties to the smallest g, -1 when s
has no labelled pixel; owner_count = n[s,owner] or 0.  With the key (count << 32) | (0xFFFFFFFF - g): one unsigned 64-bit max.
Column facts [G].  size = sum over s, cover = max over s.
Pair flags.  pure(s) iff owner[s] >= 0 and 1000 owner_count[s] >= purity_pm area[s]; edge (a, b): 1 iff both pure and the owners
agree, 0 iff both pure and they differ, -1 otherwise (any endpoint outside [0,S) included).
Summary int64 [8] over the labelled columns g < G: n, sum n[s,g]^2, sum_s r_s^2 (r_s = sum_{g<G} n[s,g]), sum_g size^2,
sum owner_count, sum cover, rows with r_s > 0, columns with size > 0.
"""
import numpy as np


def _facts(keys, counts, S, G):
    """Row / column facts and summary from sorted unique keys and their counts."""
    keys, counts = np.asarray(keys, np.int64), np.asarray(counts, np.int64)
    s, g = keys // (G + 1), keys % (G + 1)
    area = np.zeros(S, np.int64)
    np.add.at(area, s, counts)
    lab = g < G
    best = np.zeros(S, np.uint64)
    np.maximum.at(best, s[lab], (counts[lab].astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - g[lab].astype(np.uint64)))
    owner_count = (best >> np.uint64(32)).astype(np.int64)
    owner = np.where(best > 0, (np.uint64(0xFFFFFFFF) - (best & np.uint64(0xFFFFFFFF))).astype(np.int64), -1)
    rows = np.zeros(S, np.int64)
    np.add.at(rows, s[lab], counts[lab])
    size, cover = np.zeros(G, np.int64), np.zeros(G, np.int64)
    np.add.at(size, g[lab], counts[lab])
    np.maximum.at(cover, g[lab], counts[lab])
    summary = np.array([counts[lab].sum(), (counts[lab] ** 2).sum(), (rows ** 2).sum(), (size ** 2).sum(), owner_count.sum(), cover.sum(),
                        (rows > 0).sum(), (size > 0).sum()], np.int64)
    return {"cells": np.stack((s, g), 1).astype(np.int32), "count": counts.astype(np.int32), "area": area, "owner": owner.astype(np.int32),
            "owner_count": owner_count.astype(np.int32), "size": size, "cover": cover.astype(np.int32), "summary": summary,
            "n_labels": S, "n_truth": G}


def label_overlap(labels, truth, S, G):
    """dict: cells int32 [K,2] = (s, g) sorted, count int32 [K], area int64 [S], owner / owner_count int32 [S], size int64 [G],
    cover int32 [G], summary int64 [8]."""
    labels, truth = np.asarray(labels), np.asarray(truth)
    assert labels.shape == truth.shape and labels.size < 2 ** 31 and S >= 1 and G >= 1 and S * (G + 1) < 2 ** 62
    l, t = labels.reshape(-1).astype(np.int64), truth.reshape(-1).astype(np.int64)
    keep = (l >= 0) & (l < S)
    col = np.where((t >= 0) & (t < G), t, G)
    keys, counts = np.unique(l[keep] * (G + 1) + col[keep], return_counts=True)
    return _facts(keys, counts, S, G)


def label_overlap_dense(labels, truth, S, G):
    """The same by brute force: one pixel at a time into a dense [S, G+1] table, the facts read off the table.  Small rasters only."""
    n = np.zeros((S, G + 1), np.int64)
    for l, t in zip(np.asarray(labels).reshape(-1).tolist(), np.asarray(truth).reshape(-1).tolist()):
        if 0 <= l < S:
            n[l, t if 0 <= t < G else G] += 1
    s, g = np.nonzero(n)
    lab = n[:, :G]
    owner = np.where(lab.max(1) > 0, lab.argmax(1), -1)            # argmax: the first (smallest g) of equal maxima
    r = lab.sum(1)
    summary = [lab.sum(), (lab ** 2).sum(), (r ** 2).sum(), (lab.sum(0) ** 2).sum(), lab.max(1).sum(), lab.max(0).sum(), (r > 0).sum(),
               (lab.sum(0) > 0).sum()]
    return {"cells": np.stack((s, g), 1).astype(np.int32), "count": n[s, g].astype(np.int32), "area": n.sum(1), "owner": owner.astype(np.int32),
            "owner_count": lab.max(1).astype(np.int32), "size": lab.sum(0), "cover": lab.max(0).astype(np.int32),
            "summary": np.array(summary, np.int64), "n_labels": S, "n_truth": G}


FIELDS = ("cells", "count", "area", "owner", "owner_count", "size", "cover", "summary")


def coarsen(ov, mapping):
    """The overlap of the partition mapping[labels] (mapping int [S] -> 0..C-1, C = max + 1), from the cells alone."""
    mapping = np.asarray(mapping, np.int64)
    S, G = ov["n_labels"], ov["n_truth"]
    assert mapping.shape == (S,) and mapping.min() >= 0
    C = int(mapping.max()) + 1
    keys = mapping[ov["cells"][:, 0]] * (G + 1) + ov["cells"][:, 1]
    uniq, inverse = np.unique(keys, return_inverse=True)
    counts = np.zeros(uniq.size, np.int64)
    np.add.at(counts, inverse.reshape(-1), ov["count"].astype(np.int64))
    return _facts(uniq, counts, C, G)


def purity_pm(min_purity):
    return int(round(float(min_purity) * 1000))


def pair_flags(edges, ov, pm):
    """int8 [E]: 1 merge, 0 do not merge, -1 ambiguous."""
    assert 0 <= pm <= 1000
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    S = ov["n_labels"]
    pure = (ov["owner"] >= 0) & (1000 * ov["owner_count"].astype(np.int64) >= pm * ov["area"])
    inside = ((edges >= 0) & (edges < S)).all(1)
    a, b = np.where(inside, edges[:, 0], 0), np.where(inside, edges[:, 1], 0)
    both = inside & pure[a] & pure[b]
    return np.where(both, (ov["owner"][a] == ov["owner"][b]).astype(np.int8), np.int8(-1)).astype(np.int8)


def scores(summary):
    """dict of the derived figures, in Python integer arithmetic until the final division (NaN where a denominator is 0)."""
    n, sq, rows, cols, oc, cv, n_regions, n_objects = (int(v) for v in summary)
    nan = float("nan")
    out = {"n": n, "n_regions": n_regions, "n_objects": n_objects, "asa": oc / n if n else nan, "coverage": cv / n if n else nan,
           "rand": nan, "adjusted_rand": nan}
    if n >= 2:
        total = n * (n - 1) // 2
        both, same_region, same_object = (sq - n) // 2, (rows - n) // 2, (cols - n) // 2       # sum C(x, 2) = (sum x^2 - n) / 2
        out["rand"] = (total + 2 * both - same_region - same_object) / total
        num = 2 * (both * total - same_region * same_object)
        den = (same_region + same_object) * total - 2 * same_region * same_object
        out["adjusted_rand"] = num / den if den else 1.0
    return out


def pair_counts_brute(labels, truth, S, G):
    """O(n^2): over all pairs of labelled pixels (label in [0,S), truth in [0,G)), how many share a region, an object, both."""
    l, t = np.asarray(labels).reshape(-1).astype(np.int64), np.asarray(truth).reshape(-1).astype(np.int64)
    keep = (l >= 0) & (l < S) & (t >= 0) & (t < G)
    l, t = l[keep], t[keep]
    iu = np.triu_indices(l.size, 1)
    same_l, same_t = (l[:, None] == l[None, :])[iu], (t[:, None] == t[None, :])[iu]
    return {"total": int(same_l.size), "both": int((same_l & same_t).sum()), "same_region": int(same_l.sum()), "same_object": int(same_t.sum()),
            "neither": int((~same_l & ~same_t).sum())}

