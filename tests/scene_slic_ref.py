"""The specification of scene.slic_labels in numpy, on top of tests/slic_ref.py.

Steps 1-3 of the SLIC rule are per pixel against one scene-wide table of centres, so they are slic_ref.iterate on the whole raster
whatever the tiling.  This file restates what follows, as the scene form does it: per core the tile-local components of the
assigned raster with provisional ids, first pixels, areas, edges and border lines; unions across seams where the two facing pixels
hold the same centre id; numbering by scene-wide first pixel; the absorption rounds on the folded graph only; one relabel pass.
The claim the tests check: the result equals slic_ref.slic of the whole raster in labels, n and rounds, whatever the tiling.
"""
import numpy as np

import slic_ref as R


def cores_of(H, W, tile):
    th, tw = tile
    return [(y, min(H, y + th), x, min(W, x + tw)) for y in range(0, H, th) for x in range(0, W, tw)]


def fold_graph(mapping, n_new, area, a, b, w):
    """Areas add; edge keys are mapped, self edges dropped, the weights of equal keys added.  Returns (area, a, b, w), a < b sorted."""
    area = np.bincount(mapping, weights=area, minlength=n_new).astype(np.int64)
    a, b = mapping[a], mapping[b]
    keep = a != b
    a, b, w = a[keep], b[keep], w[keep]
    keys, inverse = np.unique(np.minimum(a, b) * n_new + np.maximum(a, b), return_inverse=True)
    w = np.bincount(inverse.reshape(-1), weights=w, minlength=keys.size).astype(np.int64)
    return area, keys // n_new, keys % n_new, w


def absorb_round_graph(n, area, a, b, w, min_size):
    """One round of step 5 on the graph: (mapping int64 [n] or None, n_new, who, pick) -- slic_ref.absorb_round without the raster."""
    src, dst, ww = np.concatenate((a, b)), np.concatenate((b, a)), np.concatenate((w, w))
    small = area[src] < min_size
    src, dst, ww = src[small], dst[small], ww[small]
    if src.size == 0:
        return None, n, src, dst
    best = np.zeros(n, np.uint64)
    np.maximum.at(best, src, (ww.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - dst.astype(np.uint64)))
    who = np.nonzero(best)[0]
    pick = (np.uint64(0xFFFFFFFF) - (best[who] & np.uint64(0xFFFFFFFF))).astype(np.int64)
    root = R._unite(n, who, pick)
    is_root = root == np.arange(n)
    dense = np.cumsum(is_root) - 1                                # keeps the order: a union's first pixel is its smallest member's
    return dense[root], int(is_root.sum()), who, pick


def components_and_absorption(assigned, tile, min_size, info=None):
    """Stages 3-7 on the assigned raster int [H,W] in cores of `tile` = (th, tw): (labels int32 [H,W], n, rounds).
    info: a dict that receives what the tests' preconditions ask about."""
    H, W = assigned.shape
    cores = cores_of(H, W, tile)
    nx = sum(1 for c in cores if c[0] == 0)
    ny = len(cores) // nx
    prov = np.empty((H, W), np.int64)
    core_of_pixel = np.empty((H, W), np.int64)
    base, first, area, ea, eb, ew = 0, [], [], [], [], []
    for t, (y0, y1, x0, x1) in enumerate(cores):
        comp, n = R.connected_labels(assigned[y0:y1, x0:x1])
        flat = comp.reshape(-1)
        _, local_first = np.unique(flat, return_index=True)       # ids are 0..n-1 in first-pixel order
        w = x1 - x0
        first.append((local_first // w + y0) * W + (local_first % w + x0))
        area.append(np.bincount(flat, minlength=n).astype(np.int64))
        a, b, wt = R.region_edges(comp, n)
        ea.append(a + base); eb.append(b + base); ew.append(wt)
        prov[y0:y1, x0:x1] = comp.astype(np.int64) + base
        core_of_pixel[y0:y1, x0:x1] = t
        base += n
    P = base
    first, area = np.concatenate(first), np.concatenate(area)
    # seams: the facing pixels of every vertical and horizontal seam
    ys = [c[1] for c in cores[::nx]][:-1]                         # rows below which a horizontal seam runs
    xs = [c[3] for c in cores[:nx]][:-1]
    pa = np.concatenate([prov[:, x - 1] for x in xs] + [prov[y - 1, :] for y in ys] + [np.empty(0, np.int64)])
    pb = np.concatenate([prov[:, x] for x in xs] + [prov[y, :] for y in ys] + [np.empty(0, np.int64)])
    ca = np.concatenate([assigned[:, x - 1] for x in xs] + [assigned[y - 1, :] for y in ys] + [np.empty(0, np.int64)])
    cb = np.concatenate([assigned[:, x] for x in xs] + [assigned[y, :] for y in ys] + [np.empty(0, np.int64)])
    same = ca == cb
    root = R._unite(P, pa[same], pb[same])
    keys, counts = np.unique(np.minimum(pa[~same], pb[~same]) * P + np.maximum(pa[~same], pb[~same]), return_counts=True)
    ea.append(keys // P); eb.append(keys % P); ew.append(counts.astype(np.int64))
    # numbering: a component is a union's root, its first pixel the minimum over its members
    first_of = np.full(P, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(first_of, root, first)
    roots = np.nonzero(root == np.arange(P))[0]
    order = np.argsort(first_of[roots], kind="stable")
    rank = np.empty(P, np.int64)
    rank[roots[order]] = np.arange(roots.size)
    mapping = rank[root]
    n = int(roots.size)
    comp_first = first_of[roots[order]]                           # per component, ascending
    area, a, b, w = fold_graph(mapping, n, area, np.concatenate(ea), np.concatenate(eb), np.concatenate(ew))
    if info is not None:
        info.update(provisional=P, components=n, seam_unions=int(np.unique(pa[same] * P + pb[same]).size),
                    rank_differs=bool((order != np.arange(roots.size)).any()), cross_core_pick=False, picks=[])
    rounds = 0
    while True:
        step, n_new, who, pick = absorb_round_graph(n, area, a, b, w, min_size)
        if step is None:
            break
        if info is not None:
            core = core_of_pixel.reshape(-1)[comp_first]
            info["cross_core_pick"] |= bool((core[who] != core[pick]).any())
            info["picks"].append(int(who.size))
        new_first = np.full(n_new, np.iinfo(np.int64).max, np.int64)
        np.minimum.at(new_first, step, comp_first)
        comp_first = new_first
        area, a, b, w = fold_graph(step, n_new, area, a, b, w)
        mapping = step[mapping]
        n, rounds = n_new, rounds + 1
    labels = mapping[prov].astype(np.int32)                       # the one relabel pass
    if info is not None:
        flat, cores_flat = labels.reshape(-1), core_of_pixel.reshape(-1)
        lo = np.full(n, len(cores), np.int64); hi = np.full(n, -1, np.int64)
        np.minimum.at(lo, flat, cores_flat); np.maximum.at(hi, flat, cores_flat)
        info["region_in_two_cores"] = bool((lo != hi).any())
    return labels, n, rounds


def slic(tile_image, tiling, cell=29, compactness=10, iters=10, min_size=None, info=None):
    """(labels int32 [H,W], n, rounds): the scene form of slic_ref.slic in cores of `tiling` = (th, tw)."""
    min_size = R.default_min_size(cell) if min_size is None else min_size
    assigned, _ = R.iterate(np.asarray(tile_image), cell, compactness, iters)
    return components_and_absorption(assigned, tiling, min_size, info)
