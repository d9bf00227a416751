"""numpy / Python-integer restatement of weighted pair sampling (csrc/dm_epoch.hip): the select on counter word 5,
the position-keyed point draw, orientation and radiometric streams on counter words 17 / 19 / 20, the blocked layout with M draws in
place of N pairs, and the fp32 sequence of dataset.hardness_weights -- on top of tests/train_smt_ref.py's Philox and
tests/radiometric_ref.py's `sym`.  The GPU tests compare the kernels and the public path against it bit for bit."""
import math

import numpy as np

import radiometric_ref as RR
import train_smt_ref as R

WORD_SELECT, WORD_DRAW, WORD_ORIENT, WORD_RADIO = 5, 17, 19, 20
MAX_TOTAL = 1 << 62


def cumsum(w):
    """The inclusive prefix sums as Python ints (exact at any size)."""
    out, t = [], 0
    for v in np.asarray(w).reshape(-1).tolist():
        if v < 0:
            raise ValueError("negative weight")
        t += int(v)
        out.append(t)
    if not 1 <= t < MAX_TOTAL:
        raise ValueError(f"total weight {t} outside 1 .. 2^62 - 1")
    return out


def select_u(total: int, m: int, seed: int, epoch: int) -> np.ndarray:
    """uint64 [m]: u[j] = umul64hi(R_j, T), R_j = r[0] << 32 | r[1], r = philox((j, epoch, 5, 0), key) -- the high 64 bits of the
    128-bit product from 32-bit limbs (T < 2^62, so no partial sum overflows uint64).  tests/test_sampling_host.py checks it against
    Python integers."""
    total = int(total)
    if not 1 <= total < MAX_TOTAL:
        raise ValueError(f"total weight {total} outside 1 .. 2^62 - 1")
    r = R.philox4x32_10((np.arange(m, dtype=np.uint32), epoch, WORD_SELECT, 0), R.seed_key(seed))
    a, b = r[0].astype(np.uint64), r[1].astype(np.uint64)
    t1, t0, s32, m32 = np.uint64(total >> 32), np.uint64(total & 0xFFFFFFFF), np.uint64(32), np.uint64(0xFFFFFFFF)
    at0, bt1, bt0 = a * t0, b * t1, b * t0
    carry = ((at0 & m32) + (bt1 & m32) + (bt0 >> s32)) >> s32
    return a * t1 + (at0 >> s32) + (bt1 >> s32) + carry


def select(w, m: int, seed: int, epoch: int) -> np.ndarray:
    """int32 [m]: src[j] = #{i : cum[i] <= u[j]}, the smallest i with cum[i] > u[j]."""
    cum = cumsum(w)
    return np.searchsorted(np.asarray(cum, dtype=np.uint64), select_u(cum[-1], m, seed, epoch), side="right").astype(np.int32)


def blocked_rows(m: int, batch: int):
    return R.blocked_rows(m, batch)


def draw_table(pts, pairs, pair_flag, poly_off, poly_pts, src, seed: int, epoch: int, batch: int):
    """dm_pair_epoch_draw_src's table: dict of numpy columns (tile_id, xy, inner, obj, region, flag, point_id) over m = len(src)
    positions.  pts as in train_smt_ref.epoch_table.  An src entry outside [0, N): point id -1, tile id -1, zeros, flag 0."""
    pairs, poly_off, poly_pts = np.asarray(pairs, np.int64), np.asarray(poly_off, np.int64), np.asarray(poly_pts, np.int64)
    src = np.asarray(src, np.int64)
    m, n = len(src), len(pairs)
    ok = (src >= 0) & (src < n)
    s = np.where(ok, src, 0)
    r = R.philox4x32_10((np.arange(m, dtype=np.uint32), epoch, WORD_DRAW, 0), R.seed_key(seed))
    pl, pr = pairs[s, 0], pairs[s, 1]
    left = poly_pts[poly_off[pl] + R.umulhi(r[0], poly_off[pl + 1] - poly_off[pl])]
    right = poly_pts[poly_off[pr] + R.umulhi(r[1], poly_off[pr + 1] - poly_off[pr])]
    left, right = np.where(ok, left, -1), np.where(ok, right, -1)
    rl, rr = blocked_rows(m, batch)
    pid = np.empty(2 * m, np.int64)
    pid[rl], pid[rr] = left, right
    good = pid >= 0
    q = np.where(good, pid, 0)
    col = lambda a, fill: np.where(good.reshape((-1,) + (1,) * (np.asarray(a).ndim - 1)), np.asarray(a)[q], fill)
    return {"point_id": pid.astype(np.int32), "tile_id": col(pts["tile"], -1).astype(np.int32), "xy": col(pts["xy"], 0).astype(np.int32),
            "inner": col(pts["inner"], 0).astype(np.int32), "obj": col(pts["obj"], 0).astype(np.int32),
            "region": col(np.asarray(pts["region"], np.float32), np.float32(0)).astype(np.float32),
            "flag": np.where(ok, np.asarray(pair_flag)[s], 0).astype(np.float32)}


def epoch_orient(m: int, seed: int, epoch: int, batch: int, mask: int) -> np.ndarray:
    """int32 [2 m]: position j gets philox((j, epoch, 19, 0), key)[0] & mask on both of its rows."""
    if mask not in (3, 7):
        raise ValueError(f"mask {mask}: 3 (flips) or 7 (d4)")
    o = (R.philox4x32_10((np.arange(m, dtype=np.uint32), epoch, WORD_ORIENT, 0), R.seed_key(seed))[0] & np.uint32(mask)).astype(np.int32)
    rl, rr = blocked_rows(m, batch)
    out = np.empty(2 * m, np.int32)
    out[rl], out[rr] = o, o
    return out


def position_radio(m: int, seed: int, epoch: int, bands: int, gain_span: int, band_span: int, offset_span: int) -> np.ndarray:
    """int32 [m, bands, 2]: radiometric_ref.pair_radio's arithmetic keyed by the position on counter word 20."""
    if not (0 <= gain_span <= RR.MAX_SPANS[0] and 0 <= band_span <= RR.MAX_SPANS[1] and 0 <= offset_span <= RR.MAX_SPANS[2] and 1 <= bands <= 16):
        raise ValueError("span or band count outside its limits")
    key, j = R.seed_key(seed), np.arange(m, dtype=np.uint32)
    a = R.philox4x32_10((j, epoch, WORD_RADIO, 0), key)
    g0, b0 = 256 + RR.sym(a[0], gain_span), RR.sym(a[1], offset_span)
    out = np.empty((m, bands, 2), np.int32)
    for c in range(bands):
        gain = g0 + RR.sym(R.philox4x32_10((j, epoch, WORD_RADIO, 1 + c // 4), key)[c % 4], band_span)
        out[:, c, 0], out[:, c, 1] = gain, b0 - 128 * (gain - 256)
    return out


def epoch_radio(m: int, seed: int, epoch: int, batch: int, bands: int, gain_span: int, band_span: int, offset_span: int) -> np.ndarray:
    t = position_radio(m, seed, epoch, bands, gain_span, band_span, offset_span)
    rl, rr = blocked_rows(m, batch)
    out = np.empty((2 * m, bands, 2), np.int32)
    out[rl], out[rr] = t, t
    return out


def epoch_table(pts, pairs, pair_flag, poly_off, poly_pts, w, m: int, seed: int, epoch: int, batch: int):
    """PairDataset.epoch(weights=w, draws=m): select, then the draw; the table gains the `src` column."""
    src = select(w, m, seed, epoch)
    return dict(draw_table(pts, pairs, pair_flag, poly_off, poly_pts, src, seed, epoch, batch), src=src)


def balance_class_weights(n_pos: int, n_neg: int, share: float):
    """(w_pos, w_neg) in Python ints: P n_neg and (65536 - P) n_pos over their gcd, P = round(65536 share)."""
    P = int(round(65536 * share))
    a, b = P * n_neg, (65536 - P) * n_pos
    g = math.gcd(a, b)
    return a // g, b // g


def hardness(term, floor_share: float = 1.0 / 16.0, cap: float = 1.0) -> np.ndarray:
    """int64 [n]: scale = 255.0f / (float)cap; x = term * scale (fp32); NaN -> 0; x = min(255, max(0, x)); h = 1 + trunc(x);
    h = max(h, F), F = min(256, max(1, round(256 floor_share)))."""
    f32 = np.float32
    scale = f32(255.0) / f32(cap)
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.asarray(term, f32) * scale
    x = np.where(np.isnan(x), f32(0), x)
    x = np.minimum(f32(255), np.maximum(f32(0), x))
    h = 1 + x.astype(np.int32).astype(np.int64)
    return np.maximum(h, min(256, max(1, int(round(256 * floor_share)))))
