"""numpy restatement of the per-epoch pair draw (csrc/dm_epoch.hip): Philox4x32-10, the Feistel + cycle-walk
shuffle and the keyed per-pair point draw, vectorised over positions.  The GPU tests compare dm_pair_epoch_draw against it bit for bit."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: 4 uint32 arrays (broadcastable), key: 2 uint32 values -> 4 uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint32) for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint32(key[0]), np.uint32(key[1])
    with np.errstate(over="ignore"):
        for r in range(10):
            if r:
                k0, k1 = np.uint32(k0 + W0), np.uint32(k1 + W1)
            p0 = c[0].astype(np.uint64) * M0
            p1 = c[2].astype(np.uint64) * M1
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & MASK32).astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & MASK32).astype(np.uint32)
            c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return c


def seed_key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def feistel_bits(n):
    b = 2
    while (1 << b) < n:
        b += 2
    return b


def epoch_perm(n, seed, epoch):
    """src[j] = perm_epoch(j) for j in [0, n)."""
    key = seed_key(seed)
    h = feistel_bits(n) // 2
    mask = np.uint32((1 << h) - 1)
    x = np.arange(n, dtype=np.uint32)
    todo = np.ones(n, dtype=bool)
    while todo.any():
        v = x[todo]
        L, R = v >> np.uint32(h), v & mask
        for r in range(4):
            f = philox4x32_10((R, epoch, 2, r), key)[0] & mask
            L, R = R, L ^ f
        v = (L << np.uint32(h)) | R
        x[todo] = v
        todo[todo] = v >= n
    return x.astype(np.int64)


def umulhi(a, b):
    return ((np.asarray(a, dtype=np.uint64) * np.asarray(b, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)


def epoch_draw(pairs, pair_flag, poly_off, poly_pts, seed, epoch, batch):
    """-> (left point ids [N], right point ids [N], flags [N], src [N]) in POSITION order."""
    pairs, poly_off, poly_pts = np.asarray(pairs, np.int64), np.asarray(poly_off, np.int64), np.asarray(poly_pts, np.int64)
    n = pairs.shape[0]
    src = epoch_perm(n, seed, epoch)
    r = philox4x32_10((src.astype(np.uint32), epoch, 1, 0), seed_key(seed))
    pl, pr = pairs[src, 0], pairs[src, 1]
    left = poly_pts[poly_off[pl] + umulhi(r[0], poly_off[pl + 1] - poly_off[pl])]
    right = poly_pts[poly_off[pr] + umulhi(r[1], poly_off[pr + 1] - poly_off[pr])]
    return left, right, np.asarray(pair_flag)[src], src


def blocked_rows(n, batch):
    """(left row, right row) of every position in the per-step blocked layout."""
    j = np.arange(n, dtype=np.int64)
    s = j // batch
    b_s = np.minimum(batch, n - s * batch)
    left = s * batch + j
    return left, left + b_s


def epoch_table(pts, pairs, pair_flag, poly_off, poly_pts, seed, epoch, batch):
    """The whole epoch table as the kernel writes it: dict of numpy columns (tile_id, xy, inner, obj, region, flag, point_id).
    pts: dict with tile [n], xy [n, 2], inner [n], obj [n], region [n, 15]."""
    n = len(pairs)
    left, right, flag, _ = epoch_draw(pairs, pair_flag, poly_off, poly_pts, seed, epoch, batch)
    rl, rr = blocked_rows(n, batch)
    point_id = np.empty(2 * n, dtype=np.int64)
    point_id[rl], point_id[rr] = left, right
    return {"point_id": point_id.astype(np.int32), "tile_id": np.asarray(pts["tile"])[point_id].astype(np.int32),
            "xy": np.asarray(pts["xy"])[point_id].astype(np.int32), "inner": np.asarray(pts["inner"])[point_id].astype(np.int32),
            "obj": np.asarray(pts["obj"])[point_id].astype(np.int32), "region": np.asarray(pts["region"], np.float32)[point_id],
            "flag": np.asarray(flag, np.float32)}
