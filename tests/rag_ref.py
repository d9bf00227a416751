"""A second statement of the label-raster chain's spec, and the cases that pin it at its edges (tests/test_rag_host.py,
tests/test_gpu_rag_pins.py).

`brute_rag` restates the docstring of oracle/rag.py one pixel and four neighbours at a time, in Python ints and Python floats
(IEEE double), so it shares no vectorised code with the oracle; `components_ref`, `points_to_csr_ref` and `merge_partition_ref`
restate the docstrings of rag.merge_components / points_to_csr / merge_partition as loops over Python lists.  All of it is slow:
rasters of a few thousand pixels, graphs of a few hundred thousand edges.
"""
import math

import numpy as np

from test_gpu_rag import offset_view, superpixels          # noqa: F401  (re-exported for the GPU file; not copied)

INT_MAX = 2 ** 31 - 1
OUTSIDE = -2                                                # reserved id: counted as "outside the raster" by its neighbours


# ---- the raster pass, by brute force ------------------------------------------------------------------------------------------
def brute_rag(labels, tile, S):
    """(edges int32 [E,2], weights int32 [E], stats dict, features float32 [S,15]): what OR.rag_edges, OR.label_stats and
    OR.designed_features return."""
    lab = np.asarray(labels).tolist()
    H, W = len(lab), len(lab[0])
    nb = min(len(tile), 3)
    px = [np.asarray(tile[b]).tolist() for b in range(nb)]
    count = [0] * S
    sums = [[0] * nb for _ in range(S)]
    sumsq = [[0] * nb for _ in range(S)]
    bbox = [[INT_MAX, INT_MAX, -1, -1] for _ in range(S)]
    peri = [[0, 0] for _ in range(S)]
    weight = {}
    for y in range(H):
        for x in range(W):
            l = lab[y][x]
            if not 0 <= l < S:
                continue
            count[l] += 1
            for b in range(nb):
                v = px[b][y][x]
                sums[l][b] += v
                sumsq[l][b] += v * v
            box = bbox[l]
            box[0], box[1], box[2], box[3] = min(box[0], x), min(box[1], y), max(box[2], x), max(box[3], y)
            for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
                ny, nx = y + dy, x + dx
                inside = 0 <= ny < H and 0 <= nx < W
                other = lab[ny][nx] if inside else OUTSIDE
                if other == OUTSIDE:
                    peri[l][1] += 1
                elif other != l:
                    peri[l][0] += 1
                    if 0 <= other < S and l < other:       # every shared pixel edge is met from both sides: count it from the smaller
                        weight[(l, other)] = weight.get((l, other), 0) + 1
    keys = sorted(weight)
    edges = np.array(keys, np.int32).reshape(-1, 2)
    weights = np.array([weight[k] for k in keys], np.int32)
    stats = {"count": np.array(count, np.int64), "sum": np.array(sums, np.int64).reshape(S, nb),
             "sumsq": np.array(sumsq, np.int64).reshape(S, nb), "bbox": np.array(bbox, np.int32), "peri": np.array(peri, np.int64)}
    feats = np.zeros((S, 15), np.float32)
    for s in range(S):
        if count[s] == 0:
            continue
        area = float(count[s])
        pin, pbd = float(peri[s][0]), float(peri[s][1])
        per = pin + pbd
        bw, bh = float(bbox[s][2] - bbox[s][0] + 1), float(bbox[s][3] - bbox[s][1] + 1)
        mean, std = [0.0] * 3, [0.0] * 3
        for b in range(nb):
            m = float(sums[s][b]) / area
            var = float(sumsq[s][b]) / area - m * m
            mean[b], std[b] = m, math.sqrt(var if var > 0.0 else 0.0)
        row = [area, per, max(bw, bh), min(bw, bh), per / (2.0 * (bw + bh)), std[0], std[1], std[2], mean[0], mean[1], mean[2],
               per / (4.0 * math.sqrt(area)), area / (bw * bh), (mean[0] + mean[1] + mean[2]) / float(nb), pin]
        feats[s] = [np.float32(v) for v in row]
    return edges, weights, stats, feats


STAT_KEYS = ("count", "sum", "sumsq", "bbox", "peri")


def dirty(labels, S, rng, share=0.03):
    """A copy of `labels` with that share of the pixels (at least one) set to ids outside [0, S)."""
    bad = np.array([-1, -7, S, S + 7, 2 ** 31 - 1, -2 ** 31], np.int64)
    out = np.array(labels, np.int32, copy=True)
    n = max(1, int(round(share * out.size)))
    where = rng.choice(out.size, size=n, replace=False)
    out.reshape(-1)[where] = rng.choice(bad, size=n).astype(np.int32)
    return out


# ---- raster cases ---------------------------------------------------------------------------------------------------------
WIDTHS = (1, 2, 15, 16, 17, 31, 32, 48, 63, 64, 65, 80, 127, 128, 129)
HEIGHTS = (1, 2, 63, 64, 65, 66)

# id -2 inside the raster: its four neighbours count that side as raster border, not as inner perimeter
RESERVED = np.array([[0, 0, 1, 1],
                     [0, -2, 1, 1],
                     [2, 2, 2, 1]], np.int32)
RESERVED_S = 3
RESERVED_COUNT = [3, 5, 3]
RESERVED_PERI = [[2, 6], [3, 7], [3, 5]]                    # with "a different id is inner" it would be [4, 4], [4, 6], [4, 4]
RESERVED_EDGES = [[0, 1], [0, 2], [1, 2]]
RESERVED_WEIGHTS = [1, 1, 2]


def width_case(H, W, bands=3):
    """Superpixels of cell 5 with three ids that never occur, 3 % of the pixels outside [0, S), `bands` random bands."""
    rng = np.random.default_rng(1000 * H + W)
    lab, S = superpixels(H, W, 5, 1000 * H + W)
    S += 3
    return dirty(lab, S, rng), S, rng.integers(0, 256, (bands, H, W), dtype=np.uint8)


def one_label_case(H, W):
    """Label 0 on every pixel, band 0 all 255: 255^2 H W passes 2^32 from H W = 66052 pixels on."""
    rng = np.random.default_rng(H + W)
    tile = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    tile[0] = 255
    return np.zeros((H, W), np.int32), 2, tile


def noise_case(H, W, S):
    """Per-pixel noise labels: far more labels and pairs in a 64x64 tile than its LDS tables hold."""
    lab = np.random.default_rng(4).integers(0, S, (H, W)).astype(np.int32)
    return lab, S, np.random.default_rng(5).integers(0, 256, (3, H, W), dtype=np.uint8)


def max_per_tile(lab, S):
    """(most distinct labels, most distinct 4-neighbour pairs) whose first pixel lies in one 64x64 tile."""
    H, W = lab.shape
    L = lab.astype(np.int64)
    most_l = most_p = 0
    for y0 in range(0, H, 64):
        for x0 in range(0, W, 64):
            t = L[y0:y0 + 64, x0:x0 + 64]
            most_l = max(most_l, np.unique(t).size)
            right = L[y0:y0 + 64, x0 + 1:x0 + 65]
            below = L[y0 + 1:y0 + 65, x0:x0 + 64]
            a = np.concatenate((t[:, :right.shape[1]].reshape(-1), t[:below.shape[0]].reshape(-1)))
            b = np.concatenate((right.reshape(-1), below.reshape(-1)))
            keep = a != b
            most_p = max(most_p, np.unique(np.minimum(a, b)[keep] * S + np.maximum(a, b)[keep]).size)
    return most_l, most_p


BIG_S = 1 << 24


def big_key_case():
    """32x48 raster of 8x8 blocks with ids spread over [0, 2^24): keys a * S + b beyond 2^32."""
    ids = [(k * 699051 + BIG_S - 1) % BIG_S for k in range(24)]
    ids[0], ids[1] = BIG_S - 1, 0
    blocks = np.array(ids, np.int32).reshape(4, 6)
    return np.repeat(np.repeat(blocks, 8, axis=0), 8, axis=1), BIG_S


def refusal_case():
    """48x48 raster of 6x6 blocks with ids 0..63: 2 * 8 * 7 = 112 edges."""
    blocks = np.arange(64, dtype=np.int32).reshape(8, 8)
    return np.repeat(np.repeat(blocks, 6, axis=0), 6, axis=1), 64


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def components_ref(edges, merge, S):
    """int64 [S]: the smallest id of every node's component in the graph of the edges with merge[e] set (rows with a negative
    endpoint must not be flagged)."""
    parent = list(range(S))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    flagged = np.asarray(edges).reshape(-1, 2)[np.asarray(merge).reshape(-1).astype(bool)]
    for a, b in flagged.tolist():
        assert 0 <= a < S and 0 <= b < S
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)              # the root is the smallest member, by induction
    return np.array([find(s) for s in range(S)], np.int64)


def bit_reverse(p, bits):
    r = 0
    for _ in range(bits):
        r, p = (r << 1) | (p & 1), p >> 1
    return r


def path_graph(k, order, seed=0):
    """A path of 2^k nodes, edge list shuffled, every 37th edge unflagged.  The node at position p has id
    p (identity), the next of 0, n-1, 1, n-2, ... (zigzag), or the bit reversal of p (bitrev: neighbours on the path lie far
    apart in id at every scale, so a round can only halve the number of roots)."""
    n = 1 << k
    pos = np.arange(n)
    if order == "identity":
        ids = pos
    elif order == "zigzag":
        ids = np.where(pos % 2 == 0, pos // 2, n - 1 - pos // 2)
    elif order == "bitrev":
        ids = np.array([bit_reverse(int(p), k) for p in pos])
    else:
        raise ValueError(order)
    assert sorted(ids.tolist()) == list(range(n))
    edges = np.stack((ids[:-1], ids[1:]), 1).astype(np.int32)
    merge = (np.arange(n - 1) % 37) != 36
    perm = np.random.default_rng(seed + k).permutation(n - 1)
    return edges[perm], merge[perm], n


def star_graph(centre_is_largest, leaves=300):
    n = leaves + 1
    centre = n - 1 if centre_is_largest else 0
    others = np.array([i for i in range(n) if i != centre], np.int32)
    edges = np.stack((np.full(leaves, centre, np.int32), others), 1)
    edges[::2] = edges[::2, ::-1]                          # the centre on either side
    return edges, np.ones(leaves, bool), n


def random_graph(S, E, frac, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, S, size=(E, 2)).astype(np.int32), rng.random(E) < frac, S


def with_junk(edges, merge, S, seed=1):
    """10 % more rows of each kind that must change nothing: flagged self loops, copies of existing rows with their flags,
    unflagged [-1, b] rows; all shuffled in."""
    rng = np.random.default_rng(seed)
    n = max(1, len(edges) // 10)
    loops = np.repeat(rng.integers(0, S, size=(n, 1)), 2, axis=1).astype(np.int32)
    pick = rng.integers(0, len(edges), size=n)
    dead = np.stack((np.full(n, -1), rng.integers(0, S, size=n)), 1).astype(np.int32)
    e = np.concatenate((edges, loops, edges[pick], dead))
    m = np.concatenate((merge, np.ones(n, bool), merge[pick], np.zeros(n, bool)))
    perm = rng.permutation(len(e))
    return e[perm], m[perm], S


# ---- point lists and the merged partition -------------------------------------------------------------------------------------
def points_to_csr_ref(labels, xy, S):
    """(ptr [S+1], idx [P]): the points of superpixel s are idx[ptr[s]:ptr[s+1]], in their order in `xy` = rows of (x, y)."""
    lab = np.asarray(labels).tolist()
    members = [[] for _ in range(S)]
    for p, (x, y) in enumerate(np.asarray(xy).tolist()):
        members[lab[y][x]].append(p)
    ptr, idx = [0], []
    for m in members:
        idx += m
        ptr.append(len(idx))
    return np.array(ptr, np.int32), np.array(idx, np.int32)


def merge_partition_ref(ptr, idx, edges, root):
    """(new_id [S], ptr' [C+1], idx', edges' [E',2]): regions numbered in order of their smallest member (= root); a region's
    points are its members' lists in ascending old id, each in its old order; edges between two regions, a < b, once each,
    sorted; rows with a negative endpoint and rows inside one region are dropped."""
    ptr, idx, root = (np.asarray(v).tolist() for v in (ptr, idx, root))
    S = len(root)
    roots = sorted(set(root))
    assert all(root[r] == r for r in roots)
    rank = {r: i for i, r in enumerate(roots)}
    new_id = [rank[root[s]] for s in range(S)]
    lists = [[] for _ in roots]
    for s in range(S):
        lists[new_id[s]] += idx[ptr[s]:ptr[s + 1]]
    new_ptr, new_idx = [0], []
    for l in lists:
        new_idx += l
        new_ptr.append(len(new_idx))
    pairs = set()
    for a, b in np.asarray(edges).reshape(-1, 2).tolist():
        if a < 0 or b < 0:
            continue
        a, b = new_id[a], new_id[b]
        if a != b:
            pairs.add((min(a, b), max(a, b)))
    return (np.array(new_id, np.int32), np.array(new_ptr, np.int32), np.array(new_idx, np.int32),
            np.array(sorted(pairs), np.int32).reshape(-1, 2))
