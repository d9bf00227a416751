"""numpy restatement of the feed's radiometric jitter: the per-(sample, band) affine rule applied to the
zero-padded crop before tests/augment_ref.py's orientation and oracle/patches.py's resize, the fp32 sequence that moves the designed
row with it, and the per-epoch table draw on top of tests/train_smt_ref.py's Philox and permutation.  The GPU tests compare
dm_pair_batch_gather_augmented and dm_pair_epoch_radiometric against it bit for bit."""
import numpy as np

import augment_ref as A
import train_smt_ref as R
from oracle import patches as OP

GAIN_MAX, OFFSET_MAX = 1023, 65535                       # gain: Q8 in 0 .. GAIN_MAX (256 = 1.0); offset: 1/256 grey levels, |.| <= OFFSET_MAX
MAX_SPANS = (128, 64, 16320)                             # limits of (gain_span, band_span, offset_span)
IDENTITY = (256, 0)
STD0, MEAN0, BRIGHT = 5, 8, 13                           # oracle/rag.py's attribute order: std at 5..7, means at 8..10, bright at 13


def in_range(radio) -> bool:
    r = np.asarray(radio, np.int64).reshape(-1, 2)
    return bool(((r[:, 0] >= 0) & (r[:, 0] <= GAIN_MAX) & (np.abs(r[:, 1]) <= OFFSET_MAX)).all())


def pixel(v, gain: int, offset: int) -> np.ndarray:
    """The rule on pixel values: min(255, max(0, (gain v + offset + 128) >> 8)), the shift arithmetic (floor)."""
    s = int(gain) * np.asarray(v, np.int64) + int(offset) + 128
    assert (np.abs(s) < 1 << 19).all()
    return np.clip(s >> 8, 0, 255).astype(np.uint8)


def radio_crop(img: np.ndarray, x0: int, y0: int, L: int, radio) -> np.ndarray:
    """uint8 [bands, L, L]: cut_image with the rule applied to every pixel inside the raster; the padding stays 0."""
    crop = OP.cut_image(img, x0, y0, L)
    inside = OP.cut_image(np.ones_like(img), x0, y0, L).astype(bool)
    radio = np.asarray(radio).reshape(img.shape[0], 2)
    out = np.zeros_like(crop)
    for c in range(img.shape[0]):
        out[c] = np.where(inside[c], pixel(crop[c], radio[c, 0], radio[c, 1]), 0)
    return out


def augmented_patch(img: np.ndarray, x: int, y: int, L: int, t: int, o: int, radio, resize: str = "opencv") -> np.ndarray:
    """float32 [bands, t, t]: crop (zero-padded) -> radiometric rule -> orientation o -> resize on uint8 -> / 255.0."""
    x0, y0 = OP.top_left(x, y, L)
    win = A.orient_crop(radio_crop(img, x0, y0, L, radio), o)
    fn = OP.RESIZE_RULES[resize]
    return np.stack([fn(win[b], t) for b in range(win.shape[0])]).astype(np.float32) / 255.0


def gather(tiles: np.ndarray, tile_id, xy, inner, obj, orient, radio, scale_index: int, target: int, max_window: int, resize: str = "opencv"):
    """dm_pair_batch_gather_augmented for planar fp32 output: (float32 [P, bands, target, target], flagged).  orient None: every
    orientation 0.  A sample whose tile id, window side, orientation or any band's (gain, offset) is out of range is zeros and
    raises the flag."""
    P, bands = len(xy), tiles.shape[1]
    radio = np.asarray(radio).reshape(P, bands, 2)
    out = np.zeros((P, bands, target, target), np.float32)
    flagged = False
    for p in range(P):
        L = A.window_side(inner[p], obj[p], scale_index)
        o = 0 if orient is None else int(orient[p])
        if not (1 <= L <= max_window and 0 <= tile_id[p] < tiles.shape[0] and 0 <= o <= 7 and in_range(radio[p])):
            flagged = True
            continue
        out[p] = augmented_patch(tiles[int(tile_id[p])], int(xy[p][0]), int(xy[p][1]), L, target, o, radio[p], resize)
    return out, flagged


def designed_row(region: np.ndarray, inner: int, obj: int, radio, bands: int) -> np.ndarray:
    """[15 attributes | 4 scale factors] in float32 with the first nb = min(bands, 3) standard deviations and means and `bright` moved
    by the sample's table: every operation a float32 one, rounded to nearest, in the order written.  A table out of range leaves the
    row as augment_ref.designed_row writes it."""
    row = A.designed_row(region, inner, obj)
    radio = np.asarray(radio).reshape(bands, 2)
    if not in_range(radio):
        return row
    f32 = np.float32
    nb = min(bands, 3)
    total = None
    out = row.copy()
    for c in range(nb):
        gf, bf = f32(radio[c, 0]) / f32(256), f32(radio[c, 1]) / f32(256)
        mean = row[MEAN0 + c]
        m = f32(f32(gf * mean) + bf)
        m = f32(0) if m < 0 else m
        m = f32(255) if m > 255 else m
        out[MEAN0 + c] = m
        out[STD0 + c] = f32(gf * row[STD0 + c])
        d = f32(m - mean)
        total = d if total is None else f32(total + d)
    out[BRIGHT] = f32(row[BRIGHT] + f32(total / f32(nb)))
    return out


def sym(r, s: int) -> np.ndarray:
    """(int32)umulhi(r, 2 s + 1) - s: uniform on -s .. s, 0 when s = 0."""
    return (R.umulhi(r, 2 * int(s) + 1) - int(s)).astype(np.int32)


def pair_radio(src, seed: int, epoch: int, bands: int, gain_span: int, band_span: int, offset_span: int) -> np.ndarray:
    """int32 [len(src), bands, 2]: the table of the pairs `src`, a function of (seed, epoch, pair) alone (counter word 4)."""
    if not (0 <= gain_span <= MAX_SPANS[0] and 0 <= band_span <= MAX_SPANS[1] and 0 <= offset_span <= MAX_SPANS[2] and 1 <= bands <= 16):
        raise ValueError("span or band count outside its limits")
    key = R.seed_key(seed)
    src = np.asarray(src).astype(np.uint32)
    a = R.philox4x32_10((src, epoch, 4, 0), key)
    g0 = 256 + sym(a[0], gain_span)
    b0 = sym(a[1], offset_span)
    out = np.empty((len(src), bands, 2), np.int32)
    for c in range(bands):
        b = R.philox4x32_10((src, epoch, 4, 1 + c // 4), key)[c % 4]
        gain = g0 + sym(b, band_span)
        out[:, c, 0] = gain
        out[:, c, 1] = b0 - 128 * (gain - 256)
    return out


def epoch_radio(n: int, seed: int, epoch: int, batch: int, bands: int, gain_span: int, band_span: int, offset_span: int) -> np.ndarray:
    """int32 [2 n, bands, 2]: the pair at position j with src = perm(j) gets pair_radio(src) on both of its rows."""
    t = pair_radio(R.epoch_perm(n, seed, epoch), seed, epoch, bands, gain_span, band_span, offset_span)
    rl, rr = R.blocked_rows(n, batch)
    out = np.empty((2 * n, bands, 2), np.int32)
    out[rl], out[rr] = t, t
    return out


def spans(contrast: float = 0.2, brightness: float = 0.1, colour: float = 0.05):
    """ops.Radiometric(contrast, brightness, colour).spans(): (gain_span, band_span, offset_span)."""
    return int(round(256 * contrast)), int(round(256 * colour)), int(round(255 * 256 * brightness))
