"""numpy restatement of the feed's dihedral augmentation: the orientation applied to the zero-padded crop
between `cut_image` and the resize, composed from oracle/patches.py, and the per-epoch orientation draw on top of
tests/train_smt_ref.py's Philox and permutation.  The GPU tests compare dm_pair_batch_gather_oriented and dm_pair_epoch_orient
against it bit for bit."""
import numpy as np

import train_smt_ref as R
from oracle import patches as OP

MASKS = {"flips": 3, "d4": 7}


def orient_crop(crop: np.ndarray, o: int) -> np.ndarray:
    """The rule, in its slicing form: [..., L, L] -> [..., L, L]."""
    if not 0 <= o <= 7:
        raise ValueError(f"orientation {o} outside 0..7")
    c = crop
    if o & 2:
        c = c[..., ::-1, :]
    if o & 1:
        c = c[..., :, ::-1]
    if o & 4:
        c = np.swapaxes(c, -1, -2)
    return np.ascontiguousarray(c)


def orient_crop_indexed(crop: np.ndarray, o: int) -> np.ndarray:
    """The same as an index map: crop'[j][i] = crop[fy(a)][fx(b)], (a, b) = (i, j) if bit 2 is set and (j, i) otherwise."""
    L = crop.shape[-1]
    j, i = np.meshgrid(np.arange(L), np.arange(L), indexing="ij")
    a, b = (i, j) if o & 4 else (j, i)
    fy = L - 1 - a if o & 2 else a
    fx = L - 1 - b if o & 1 else b
    return np.ascontiguousarray(crop[..., fy, fx])


def oriented_patch(img: np.ndarray, x: int, y: int, L: int, t: int, o: int, resize: str = "opencv") -> np.ndarray:
    """float32 [bands, t, t]: crop (zero-padded) -> orientation o -> resize on uint8 -> / 255.0 (oracle.patches.patch_pyramid with
    the transform in the middle)."""
    x0, y0 = OP.top_left(x, y, L)
    win = orient_crop(OP.cut_image(img, x0, y0, L), o)
    fn = OP.RESIZE_RULES[resize]
    return np.stack([fn(win[b], t) for b in range(win.shape[0])]).astype(np.float32) / 255.0


def patch_rows(patch: np.ndarray, grid: int) -> np.ndarray:
    """[bands, t, t] -> the patch-embed rows [grid * grid, bands * ps * ps]: row py * grid + px, column (c * ps + dy) * ps + dx
    (the im2col order of Conv2d(k = ps, stride = ps))."""
    bands, t, _ = patch.shape
    ps = t // grid
    return np.ascontiguousarray(patch.reshape(bands, grid, ps, grid, ps).transpose(1, 3, 0, 2, 4).reshape(grid * grid, bands * ps * ps))


def window_side(inner: int, obj: int, scale_index: int) -> int:
    return OP.get_scales(int(inner), int(obj))[0][scale_index]


def designed_row(region: np.ndarray, inner: int, obj: int) -> np.ndarray:
    """[15 attributes | 4 scale factors] in float32 -- no orientation enters it."""
    windows = np.asarray(OP.get_scales(int(inner), int(obj))[0], np.float32)
    return np.concatenate((np.asarray(region, np.float32), windows / np.asarray(OP.CONFIG_SCALES, np.float32)))


def gather(tiles: np.ndarray, tile_id, xy, inner, obj, orient, scale_index: int, target: int, max_window: int, resize: str = "opencv"):
    """dm_pair_batch_gather_oriented for planar fp32 output: (float32 [P, bands, target, target], flagged).  A sample whose tile id,
    window side or orientation is out of range is zeros and raises the flag."""
    P, bands = len(xy), tiles.shape[1]
    out = np.zeros((P, bands, target, target), np.float32)
    flagged = False
    for p in range(P):
        L = window_side(inner[p], obj[p], scale_index)
        if not (1 <= L <= max_window and 0 <= tile_id[p] < tiles.shape[0] and 0 <= orient[p] <= 7):
            flagged = True
            continue
        out[p] = oriented_patch(tiles[int(tile_id[p])], int(xy[p][0]), int(xy[p][1]), L, target, int(orient[p]), resize)
    return out, flagged


def epoch_orient(n: int, seed: int, epoch: int, batch: int, mask: int) -> np.ndarray:
    """int32 [2 n]: the pair at position j with src = perm(j) gets philox((src, epoch, 3, 0), key)[0] & mask on both of its rows."""
    if mask not in (3, 7):
        raise ValueError(f"mask {mask}: 3 (flips) or 7 (d4)")
    src = R.epoch_perm(n, seed, epoch)
    o = (R.philox4x32_10((src.astype(np.uint32), epoch, 3, 0), R.seed_key(seed))[0] & np.uint32(mask)).astype(np.int32)
    rl, rr = R.blocked_rows(n, batch)
    out = np.empty(2 * n, np.int32)
    out[rl], out[rr] = o, o
    return out
