"""Device-resident stand-in for the reference's training dataset `MergingSegmensPairDataset` (MyUtils1.py:18-37, :225-296) with the
same tensor contract and no GDAL / OGR: the caller hands over, per training image, what one positive / negative pair list, its
polygon and point shapefiles and its GeoTIFF hold, as arrays.

The unit of data is a POLYGON PAIR (a line `x,left_polygon_id,right_polygon_id[,...]` of a pair list, MyUtils1.py:225-235).  Every
epoch the reference rebuilds the dataset, drawing one sample point uniformly from each polygon's `PointID` list (:275-293), and
shuffles it (DataLoader(shuffle=True), Train_SMT.py:218-220).  Here one dm_pair_epoch_draw launch does both, keyed by (seed, epoch)
(DESIGN.md 3.9), and writes the epoch's table in the per-step blocked layout feed.PairFeed reads: each step's feed.PairTable is a
set of views, no `cat`.

All ids are checked once, on the host, when the dataset is built (`build_host`, no GPU needed); the upload follows.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops, rag
from .feed import PairTable
from .patches import geo_to_pixel

MAX_WINDOW = 384        # the gather's LDS staging limit (csrc/dm_patches.hip MAX_WINDOW)
MAX_WEIGHT_TOTAL = 1 << 62   # the sum of an epoch's pair weights stays below this (dm_pair_epoch_select)
MAX_HARDNESS = 256           # hardness_weights' values are 1 .. MAX_HARDNESS


def read_pair_list(path: str) -> np.ndarray:
    """A pair list of the reference (`x,left_polygon_id,right_polygon_id[,...]` per line; only columns 1 and 2 are read,
    MyUtils1.py:225-235) -> int32 [k, 2]."""
    rows = []
    with open(path, "r") as f:
        for line in f.readlines():
            line = line.strip("\n")
            if not line.strip():
                continue
            cols = line.split(",")
            rows.append((int(cols[1]), int(cols[2])))
    return np.asarray(rows, dtype=np.int32).reshape(-1, 2)


def window_sides(inner: np.ndarray, obj: np.ndarray, n_scales: int) -> np.ndarray:
    """(inner, obj, obj + interval, obj + 2 interval)[:n_scales] per point (MyUtils1.py:130-156) -> int64 [n, n_scales]."""
    inner, obj = np.asarray(inner, np.int64), np.asarray(obj, np.int64)
    interval = obj - inner
    return np.stack((inner, obj, obj + interval, obj + 2 * interval), axis=1)[:, :n_scales]


def _point_lists(polys, where: str) -> List[np.ndarray]:
    out = []
    for k, p in enumerate(polys):
        if isinstance(p, str):        # the raw `PointID` field: space-separated point fids (MyUtils1.py:264-268)
            p = [int(t) for t in p.split()]
        try:
            out.append(np.asarray(p, dtype=np.int64).reshape(-1))
        except (TypeError, ValueError) as e:
            raise ValueError(f"{where}: polygon {k}: point list is not a list of integer point ids ({e})") from e
    return out


@dataclass
class HostPairs:
    """The dataset as host arrays (what `PairDataset` uploads).  Ids are global: polygon ids index poly_off, point ids the point table."""
    tiles: np.ndarray           # uint8 [T, bands, Hmax, Wmax] (zero padded right / bottom)
    pairs: np.ndarray           # int32 [N, 2] global polygon ids: all positives image by image, then all negatives
    flag: np.ndarray            # int32 [N]
    poly_off: np.ndarray        # int32 [n_poly + 1]
    poly_pts: np.ndarray        # int32 [poly_off[-1]]
    pt_tile: np.ndarray         # int32 [n_pts]
    pt_xy: np.ndarray           # int32 [n_pts, 2] pixel coordinates
    pt_inner: np.ndarray        # int32 [n_pts]
    pt_obj: np.ndarray          # int32 [n_pts]
    pt_region: np.ndarray       # float32 [n_pts, 15]
    positive_pair_number: int
    negative_pair_number: int
    n_scales: int
    max_windows: List[int]      # per scale, over every point a pair can draw


def build_host(images: Sequence[Dict], n_scales: int = 3) -> HostPairs:
    """Validate and join the per-image arrays (see PairDataset.from_arrays).  Raises ValueError naming the image and pair of the
    first polygon id out of range, polygon without points, point id out of range or window side outside 1..384 at any of the first
    `n_scales` scales, or when there are no pairs at all.  CPU only."""
    if not 1 <= n_scales <= 4:
        raise ValueError("n_scales: 1..4 (the reference's get_scales derives four window sides)")
    if len(images) == 0:
        raise ValueError("PairDataset: no images")
    tiles, bands = [], None
    poly_lists, pts = [], {"tile": [], "xy": [], "inner": [], "obj": [], "region": []}
    pos, neg = [], []
    n_pts = n_poly = 0
    for i, im in enumerate(images):
        where = f"image {i}"
        tile = np.asarray(im["tile"])
        if tile.dtype != np.uint8 or tile.ndim != 3:
            raise ValueError(f"{where}: tile must be uint8 [bands, H, W], got {tile.dtype} {tile.shape}")
        if bands is not None and tile.shape[0] != bands:
            raise ValueError(f"{where}: {tile.shape[0]} bands, image 0 has {bands}")
        bands = tile.shape[0]
        if "xy" in im:
            xy = np.asarray(im["xy"], dtype=np.int64).reshape(-1, 2)
        else:
            g = np.asarray(im["geo"], dtype=np.float64).reshape(-1, 2)
            xy = geo_to_pixel(list(im["geotransform"]), torch.from_numpy(g[:, 0]), torch.from_numpy(g[:, 1])).numpy().astype(np.int64)
        n = xy.shape[0]
        inner, obj = np.asarray(im["inner"], np.int64).reshape(-1), np.asarray(im["obj"], np.int64).reshape(-1)
        region = np.asarray(im["region"], dtype=np.float32).reshape(-1, 15) if n else np.zeros((0, 15), np.float32)
        if not (inner.shape[0] == obj.shape[0] == region.shape[0] == n):
            raise ValueError(f"{where}: {n} points, but {inner.shape[0]} inner, {obj.shape[0]} obj and {region.shape[0]} region rows")
        polys = _point_lists(im["polygon_points"], where)
        windows = window_sides(inner, obj, n_scales)
        bad_poly = {}                          # polygon id -> why a pair may not reference it (checked once per polygon)
        for p, ids in enumerate(polys):
            if ids.size == 0:
                bad_poly[p] = "the polygon has no sample points"
                continue
            bad = ids[(ids < 0) | (ids >= n)]
            if bad.size:
                bad_poly[p] = f"point id {int(bad[0])} out of range (the image has {n} points)"
                continue
            w = windows[ids]
            q, sc = np.nonzero((w < 1) | (w > MAX_WINDOW))
            if q.size:
                bad_poly[p] = f"point {int(ids[q[0]])} has window side {int(w[q[0], sc[0]])} at scale {int(sc[0])}, outside 1..{MAX_WINDOW}"
        for kind, lst in (("positive", pos), ("negative", neg)):
            pr = np.asarray(im.get(kind, np.zeros((0, 2))), dtype=np.int64).reshape(-1, 2)
            out = (pr < 0) | (pr >= len(polys))
            flagged = out | np.isin(pr, np.fromiter(bad_poly, dtype=np.int64, count=len(bad_poly)))
            if flagged.any():
                k, side = (int(v[0]) for v in np.nonzero(flagged))
                p = int(pr[k, side])
                what = f"{where}, {kind} pair {k} ({pr[k, 0]}, {pr[k, 1]}), {('left', 'right')[side]} polygon {p}"
                why = f"polygon id out of range (the image has {len(polys)} polygons)" if out[k, side] else bad_poly[p]
                raise ValueError(f"{what}: {why}")
            lst.append(pr + n_poly)
        for p in polys:
            poly_lists.append(p + n_pts)
        pts["tile"].append(np.full(n, i, np.int64)); pts["xy"].append(xy); pts["inner"].append(inner); pts["obj"].append(obj)
        pts["region"].append(region)
        tiles.append(tile)
        n_pts += n
        n_poly += len(polys)
    n_pos, n_neg = sum(len(p) for p in pos), sum(len(p) for p in neg)
    N = n_pos + n_neg
    if N == 0:
        raise ValueError("PairDataset: empty dataset (no positive and no negative pairs)")
    if n_pts >= 2 ** 31 or N > 2 ** 30:
        raise ValueError("PairDataset: too many points or pairs for int32 ids")
    Hm, Wm = max(t.shape[1] for t in tiles), max(t.shape[2] for t in tiles)
    canvas = np.zeros((len(tiles), bands, Hm, Wm), dtype=np.uint8)
    for i, t in enumerate(tiles):          # zero padding right / bottom is exact: cut_image zero-fills outside the image (MyUtils1.py:160-189)
        canvas[i, :, :t.shape[1], :t.shape[2]] = t
    counts = np.asarray([p.size for p in poly_lists], dtype=np.int64)
    poly_off = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    poly_pts = np.concatenate(poly_lists).astype(np.int32) if poly_lists else np.zeros(0, np.int32)
    pairs = np.concatenate(pos + neg).astype(np.int32).reshape(-1, 2)
    used = np.unique(np.concatenate([poly_lists[p] for p in np.unique(pairs)]))
    inner_all, obj_all = np.concatenate(pts["inner"]), np.concatenate(pts["obj"])
    max_windows = window_sides(inner_all[used], obj_all[used], n_scales).max(axis=0)
    return HostPairs(tiles=canvas, pairs=pairs, flag=np.concatenate((np.ones(n_pos, np.int32), np.zeros(n_neg, np.int32))),
                     poly_off=poly_off, poly_pts=poly_pts, pt_tile=np.concatenate(pts["tile"]).astype(np.int32),
                     pt_xy=np.concatenate(pts["xy"]).astype(np.int32).reshape(-1, 2), pt_inner=inner_all.astype(np.int32),
                     pt_obj=obj_all.astype(np.int32), pt_region=np.concatenate(pts["region"]).astype(np.float32).reshape(-1, 15),
                     positive_pair_number=n_pos, negative_pair_number=n_neg, n_scales=n_scales,
                     max_windows=[int(m) for m in max_windows])


def holdout_hash(seed: int, image: int, a, b) -> np.ndarray:
    """uint64 hash of (seed, image, a, b) per pair (a, b int arrays): the key of from_rasters' train / validation split.  Fixed
    integer arithmetic (the 64-bit finaliser of MurmurHash3 over the packed fields), the same on every machine."""
    m = (1 << 64) - 1
    base = ((int(seed) * 0x9E3779B97F4A7C15) ^ ((int(image) + 1) * 0xC2B2AE3D27D4EB4F)) & m
    k = np.uint64(base) ^ ((np.asarray(a).astype(np.uint64) << np.uint64(32)) | (np.asarray(b).astype(np.uint64) & np.uint64(0xFFFFFFFF)))
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(33); k *= np.uint64(0xff51afd7ed558ccd)
        k ^= k >> np.uint64(33); k *= np.uint64(0xc4ceb9fe1a85ec53)
        k ^= k >> np.uint64(33)
    return k


def balance_class_weights(n_pos: int, n_neg: int, positive_share: float) -> Tuple[int, int]:
    """(weight of a positive pair, weight of a negative pair), Python ints, such that a weighted draw is positive with probability
    exactly P / 65536, P = round(65536 positive_share): P n_neg and (65536 - P) n_pos, both divided by their gcd.  Raises ValueError
    when P is outside 1 .. 65535, a class is empty, or the total weight n_pos w_pos + n_neg w_neg would reach 2^62."""
    share = float(positive_share)
    P = int(round(65536 * share)) if math.isfinite(share) else 0
    if not 1 <= P <= 65535:
        raise ValueError(f"positive_share must round to 1/65536 .. 65535/65536, got {positive_share!r}")
    n_pos, n_neg = int(n_pos), int(n_neg)
    if n_pos < 1 or n_neg < 1:
        raise ValueError(f"balance needs pairs of both classes, got {n_pos} positive and {n_neg} negative")
    w_pos, w_neg = P * n_neg, (65536 - P) * n_pos
    g = math.gcd(w_pos, w_neg)
    w_pos, w_neg = w_pos // g, w_neg // g
    if n_pos * w_pos + n_neg * w_neg >= MAX_WEIGHT_TOTAL:
        raise ValueError(f"balance: the total weight of {n_pos} positive and {n_neg} negative pairs reaches 2^62")
    return w_pos, w_neg


def balance_weights(flag, positive_share: float) -> torch.Tensor:
    """int64 [N] pair weights (on flag's device) for PairDataset.epoch(weights=) under which a draw is a positive pair (flag 1) with
    probability exactly round(65536 positive_share) / 65536, whatever the list's own ratio; see `balance_class_weights`.  flag: the
    pairs' 0 / 1 flags, a tensor or an array (the class counts are one host read when it lives on the device)."""
    f = flag if isinstance(flag, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(flag))
    f = f.reshape(-1)
    n_pos = int((f == 1).sum())
    w_pos, w_neg = balance_class_weights(n_pos, f.numel() - n_pos, positive_share)
    return torch.where(f == 1, w_pos, w_neg).to(torch.int64)


def hardness_weights(term: torch.Tensor, floor_share: float = 1.0 / 16.0, cap: float = 1.0,
                     class_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 [N] pair weights from the per-pair loss terms (PairDataset.pair_terms): an integer hardness h in 1 .. 256, linear in the
    term and saturating at `cap`, by a fixed fp32 sequence (tests/sampling_ref.py pins it; term fp32, every step an fp32 one):
      scale = 255.0f / (float)cap         x = term * scale         x = 0 where x is NaN         x = min(255.0f, max(0.0f, x))
      h = 1 + (int32)x  (truncation)      h = max(h, F),  F = min(256, max(1, round(256 floor_share)))
    so a term of 0 (or -0, a negative one, NaN) gives the floor and a term >= cap gives 256.  floor_share in (0, 1]: the least
    weight as a share of the greatest -- pairs the model already separates keep being seen.  class_weights: int64 [N] (e.g.
    balance_weights') to compose with by multiplication, w = class_w h; refused (one host read) when sum(class_w) * 256 reaches 2^62,
    a bound that does not depend on the terms.  No kernel: elementwise torch on the terms' device."""
    cap32 = np.float32(cap)
    if not (np.isfinite(cap32) and cap32 > 0):
        raise ValueError(f"hardness_weights: cap must be a finite number > 0 in float32, got {cap!r}")
    if not 0.0 < float(floor_share) <= 1.0:
        raise ValueError(f"hardness_weights: floor_share must be in (0, 1], got {floor_share!r}")
    if term.dtype != torch.float32 or term.dim() != 1:
        raise ValueError(f"hardness_weights: term must be a float32 [N] tensor, got {term.dtype} {tuple(term.shape)}")
    floor = min(MAX_HARDNESS, max(1, int(round(MAX_HARDNESS * float(floor_share)))))
    scale = float(np.float32(255.0) / cap32)                 # fp32 quotient; exact as a Python float, and exact again as an fp32 scalar
    x = term * torch.tensor(scale, dtype=torch.float32, device=term.device)
    x = torch.where(x != x, torch.zeros_like(x), x).clamp_(0.0, 255.0)
    h = (x.to(torch.int32) + 1).clamp_(min=floor).to(torch.int64)
    if class_weights is None:
        return h
    if class_weights.dtype != torch.int64 or tuple(class_weights.shape) != tuple(term.shape):
        raise ValueError(f"hardness_weights: class_weights must be int64 {tuple(term.shape)}, got {class_weights.dtype} {tuple(class_weights.shape)}")
    lo, total = (int(v) for v in torch.stack((class_weights.min(), class_weights.sum())).cpu())
    if lo < 0 or not 0 < total < MAX_WEIGHT_TOTAL // MAX_HARDNESS:
        raise ValueError(f"hardness_weights: class_weights must be >= 0 with 0 < sum * {MAX_HARDNESS} < 2^62, got min {lo}, sum {total}")
    return class_weights * h


class EpochTable:
    """One epoch's sample table on the device, in the per-step blocked layout: `len()` steps, step s is a feed.PairTable of
    b_s = min(batch, N - s batch) pairs made of views (rows [2 s batch, 2 s batch + 2 b_s), flags [s batch, s batch + b_s)).
    A sampled epoch (PairDataset.epoch(weights=)) has n_pairs = its number of draws and a `src` column: the pair of each position."""

    def __init__(self, cols: Dict[str, torch.Tensor], n_pairs: int, batch: int, epoch: int):
        self.cols, self.n_pairs, self.batch, self.epoch = cols, n_pairs, batch, epoch

    def __len__(self):
        return -(-self.n_pairs // self.batch)

    def pairs_in_step(self, s: int) -> int:
        return min(self.batch, self.n_pairs - s * self.batch)

    def step(self, s: int) -> PairTable:
        if not 0 <= s < len(self):
            raise IndexError(f"step {s} of {len(self)}")
        lo, b = 2 * s * self.batch, self.pairs_in_step(s)
        c = self.cols
        return PairTable(tile_id=c["tile_id"][lo:lo + 2 * b], xy=c["xy"][lo:lo + 2 * b], inner=c["inner"][lo:lo + 2 * b],
                         obj=c["obj"][lo:lo + 2 * b], region=c["region"][lo:lo + 2 * b],
                         flag=c["flag"][s * self.batch:s * self.batch + b],
                         orient=c["orient"][lo:lo + 2 * b] if "orient" in c else None,
                         radio=c["radio"][lo:lo + 2 * b] if "radio" in c else None)

    def __iter__(self):
        return (self.step(s) for s in range(len(self)))


class PairDataset:
    """`MergingSegmensPairDataset` on the device.  `epoch(e, batch)` draws epoch e's table (one launch) into buffers the dataset
    keeps and reuses: a later call overwrites the previous table."""

    def __init__(self, host: HostPairs, seed: int = 0, device="cuda:0"):
        self.host, self.seed, self.device = host, int(seed), torch.device(device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.tiles = up(host.tiles)
        self.pairs, self.flag = up(host.pairs), up(host.flag)
        self.poly_off, self.poly_pts = up(host.poly_off), up(host.poly_pts)
        self.pt_tile, self.pt_xy, self.pt_inner, self.pt_obj, self.pt_region = (up(host.pt_tile), up(host.pt_xy), up(host.pt_inner),
                                                                                up(host.pt_obj), up(host.pt_region))
        N, dev = len(host.pairs), self.device
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        self._cols = {"tile_id": i32(2 * N), "xy": i32(2 * N, 2), "inner": i32(2 * N), "obj": i32(2 * N),
                      "region": torch.empty((2 * N, 15), dtype=torch.float32, device=dev),
                      "flag": torch.empty((N,), dtype=torch.float32, device=dev), "point_id": i32(2 * N)}
        self._orient = None         # int32 [2N], allocated by the first epoch(augment=...) and kept
        self._radio = None          # int32 [2N, bands, 2], allocated by the first epoch(radiometric=...) and kept
        self._sampled = None        # the sampled epoch's own columns (2 draws rows + src), allocated by the first epoch(weights=...)
        self._sampled_rows = 0      # ... and reallocated only when `draws` grows
        self._terms = None          # pair_terms' own columns and arange, allocated by its first call
        self._term_feeds = {}       # ... and its feeds, per (model input form, batch)

    @classmethod
    def from_arrays(cls, images: Sequence[Dict], seed: int = 0, n_scales: int = 3, device="cuda:0") -> "PairDataset":
        """images: one dict per training image (one pair list + its shapefiles + its GeoTIFF upstream):
          tile            uint8 [bands, H, W]
          xy              int [n, 2] pixel coordinates of the sample points, or
          geo + geotransform   float [n, 2] map coordinates and the GDAL geotransform (converted like MyUtils1.py:67-73)
          inner, obj      int [n] window sides (the `inner` / `object` fields), region float [n, 15] (the designed attributes)
          polygon_points  per polygon, an int array of point ids or the raw `PointID` string ("3 17 42")
          positive, negative   int [k, 2] polygon id pairs (read_pair_list), either may be missing
        seed: the key of the per-epoch draw -- a resumed run that uses the same seed sees the same epochs.
        n_scales: how many of the four window sides are checked against the gather's 1..384 (the model's scale count)."""
        return cls(build_host(images, n_scales), seed=seed, device=device)

    @classmethod
    def from_rasters(cls, images: Sequence[Dict], k: int = 3, min_purity: float = 0.6, n_scales: int = 3, max_window: int = MAX_WINDOW,
                     holdout: float = 0.0, seed: int = 0, device="cuda:0"):
        """A dataset from tiles, their over-segmentations and ground-truth maps alone -- no pair lists, no shapefiles.
        images: one dict per training image:
          tile            uint8 [bands, H, W]
          labels, n_labels   int32 [H, W] superpixel ids 0..n_labels-1 (others ignored); without a `labels` key the tile is
                             segmented with rag.slic(tile, **im.get("slic", {})) (slic: a dict of its keyword arguments)
          truth, n_truth     int32 [H, W] object ids 0..n_truth-1 (any other value: unlabelled)
        (arrays or tensors).  Per image, on the device: rag.label_stats -> designed_features -> rag_edges -> sample_points(k,
        max_window) -> label_overlap -> pair_flags(min_purity); the points become xy / inner / obj / polygon_points, the designed
        attributes `region`, the edges flagged 1 / 0 `positive` / `negative` (ambiguous edges are no training pairs), and
        `build_host` takes it from there.  holdout in [0, 1): 0 returns one dataset; otherwise (train, val), where a pair of image t
        goes to val iff holdout_hash(seed, t, a, b) % 10^6 < round(holdout * 10^6) -- disjoint, reproducible, the form
        train(val_dataset=) takes.  Raises ValueError naming the image that yields no unambiguous pair."""
        if not 0.0 <= float(holdout) < 1.0:
            raise ValueError(f"holdout must be in [0, 1), got {holdout}")
        dev = torch.device(device)
        cut = int(round(float(holdout) * 1000000))
        up = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(dev)
        train, val = [], []
        with torch.cuda.device(dev):
            for t, im in enumerate(images):
                tile, truth = up(im["tile"]), up(im["truth"])
                if "labels" in im:
                    labels, S = up(im["labels"]), int(im["n_labels"])
                else:
                    labels, S = rag.slic(tile, **im.get("slic", {}))
                designed = rag.designed_features(rag.label_stats(labels, tile, S))
                edges, _ = rag.rag_edges(labels, S)
                pts = rag.sample_points(labels, S, k=k, max_window=max_window)
                flags = rag.pair_flags(edges, rag.label_overlap(labels, truth, S, int(im["n_truth"])), min_purity).cpu().numpy()
                edges = edges.cpu().numpy()
                if not (flags >= 0).any():
                    raise ValueError(f"image {t}: no unambiguous pair among {len(edges)} edges at min_purity = {min_purity} "
                                     f"(does the truth raster overlap the labels?)")
                ptr = pts.ptr.cpu().numpy()
                base = {"tile": np.asarray(im["tile"].cpu() if isinstance(im["tile"], torch.Tensor) else im["tile"]),
                        "xy": pts.xy.cpu().numpy(), "inner": pts.inner.cpu().numpy(), "obj": pts.obj.cpu().numpy(),
                        "region": pts.region_features(designed).cpu().numpy(),
                        "polygon_points": [np.arange(ptr[s], ptr[s + 1]) for s in range(S)]}
                to_val = holdout_hash(seed, t, edges[:, 0], edges[:, 1]) % np.uint64(1000000) < np.uint64(cut)
                for part, lst in ((~to_val, train), (to_val, val)):
                    lst.append(dict(base, positive=edges[part & (flags == 1)], negative=edges[part & (flags == 0)]))
        if float(holdout) == 0.0:
            return cls(build_host(train, n_scales), seed=seed, device=device)
        return cls(build_host(train, n_scales), seed=seed, device=device), cls(build_host(val, n_scales), seed=seed, device=device)

    def __len__(self):
        return len(self.host.pairs)

    @property
    def positive_pair_number(self) -> int:
        return self.host.positive_pair_number

    @property
    def negative_pair_number(self) -> int:
        return self.host.negative_pair_number

    def max_window(self, n_scales: int) -> List[int]:
        """Per-scale bounds of the window sides a draw can produce (PairFeed's max_window)."""
        if n_scales > self.host.n_scales:
            raise ValueError(f"the dataset was validated for {self.host.n_scales} scales, not {n_scales}")
        return self.host.max_windows[:n_scales]

    def _draw_inputs(self):
        return (self.pairs, self.flag, self.poly_off, self.poly_pts, self.pt_tile, self.pt_xy, self.pt_inner, self.pt_obj, self.pt_region)

    def _empty_cols(self, rows: int, **extra) -> Dict[str, torch.Tensor]:
        """Uninitialised table columns for `rows` positions (2 rows samples)."""
        dev = self.device
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        cols = {"tile_id": i32(2 * rows), "xy": i32(2 * rows, 2), "inner": i32(2 * rows), "obj": i32(2 * rows),
                "region": torch.empty((2 * rows, 15), dtype=torch.float32, device=dev),
                "flag": torch.empty((rows,), dtype=torch.float32, device=dev), "point_id": i32(2 * rows)}
        cols.update(extra)
        return cols

    def _epoch_sampled(self, e: int, batch: int, augment, radiometric, weights: torch.Tensor, draws: Optional[int]) -> EpochTable:
        N = len(self)
        M = N if draws is None else int(draws)
        if not 1 <= M <= 2 ** 30:
            raise ValueError(f"draws must be in 1 .. 2^30, got {draws}")
        if not isinstance(weights, torch.Tensor) or weights.dtype != torch.int64 or tuple(weights.shape) != (N,) or weights.device != self.device:
            raise ValueError(f"weights must be an int64 [{N}] tensor on {self.device}, got "
                             f"{getattr(weights, 'dtype', type(weights).__name__)} {tuple(getattr(weights, 'shape', ()))}")
        bands = int(self.tiles.shape[1])
        cum = torch.cumsum(weights.contiguous(), 0)
        # the one readback of a sampled epoch.  A sum that wraps int64 leaves a negative prefix behind (each weight is < 2^63)
        lo, cum_lo, total = (int(v) for v in torch.stack((weights.min(), cum.min(), cum[-1])).cpu())
        if lo < 0:
            raise ValueError(f"weights must be >= 0, the smallest is {lo}")
        if cum_lo < 0 or not 0 < total < MAX_WEIGHT_TOTAL:
            raise ValueError("weights: the total must be in 1 .. 2^62 - 1" + (" (every weight is 0)" if total == 0 and cum_lo == 0 else
                                                                               f", got {total if cum_lo >= 0 else 'an int64 overflow'}"))
        with torch.cuda.device(self.device):
            if M > self._sampled_rows:
                i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=self.device)
                self._sampled = self._empty_cols(M, src=i32(M), orient=i32(2 * M), radio=i32(2 * M, bands, 2))
                self._sampled_rows = M
            c = {k: v[:(M if k in ("flag", "src") else 2 * M)] for k, v in self._sampled.items()}
            orient, radio = c.pop("orient"), c.pop("radio")
            ops.pair_epoch_select(cum, self.seed, e, c["src"])
            ops.pair_epoch_draw(*self._draw_inputs(), self.seed, e, batch, c["tile_id"], c["xy"], c["inner"], c["obj"], c["region"], c["flag"],
                                point_id=c["point_id"], src=c["src"])
            if augment is not None:
                ops.pair_epoch_orient(self.seed, e, M, batch, ops.ORIENT_MASKS[augment], orient, by_position=True)
                c["orient"] = orient
            if radiometric is not None:
                ops.pair_epoch_radiometric(self.seed, e, M, batch, bands, *radiometric.spans(), radio, by_position=True)
                c["radio"] = radio
        return EpochTable(c, M, batch, e)

    def epoch(self, e: int, batch: int, augment: Optional[str] = None, radiometric=None, *, weights: Optional[torch.Tensor] = None,
              draws: Optional[int] = None) -> EpochTable:
        """Draw epoch e (one launch, nothing read back); the table's `point_id` column holds the drawn global point ids.
        augment: None, "flips" or "d4" -- with one more launch, every pair of the epoch also draws a dihedral orientation keyed by
        (seed, epoch, pair) ("flips": the four without the transposition), the table's `orient` column, which
        PairFeed.fill applies to both of the pair's crops.  None: the tables carry orient=None.
        radiometric: None, an ops.Radiometric or a (contrast, brightness, colour) triple -- with one more launch, every pair also
        draws a gain and an offset per band keyed by (seed, epoch, pair), the table's `radio` column, applied by
        PairFeed.fill to both of the pair's crops and designed rows.  Independent of `augment`.  None: radio=None.
        weights: None, or an int64 [N] device tensor of pair weights (>= 0, total in 1 .. 2^62 - 1; `balance_weights`,
        `hardness_weights`) -- the epoch is then `draws` (default N) pairs sampled WITH replacement, pair i with probability
        w_i / sum(w), by dm_pair_epoch_select: a function of (seed, e, position, weights), with the point draw,
        orientation and jitter keyed by the position, so a pair drawn twice is seen at two samples.  The weights are checked on the
        host with one readback per call; the table has n_pairs = draws and a `src` column, and lives in buffers of its own (sized by
        the largest `draws` so far), so the unweighted table of an earlier call stays as it was.  draws without weights: ValueError."""
        if batch < 1:
            raise ValueError("batch must be >= 1")
        if augment is not None and augment not in ops.ORIENT_MASKS:
            raise ValueError(f"augment must be None, 'flips' or 'd4', got {augment!r}")
        radiometric = ops.Radiometric.of(radiometric)
        if weights is None and draws is not None:
            raise ValueError("draws needs weights: an unweighted epoch is every pair exactly once")
        if weights is not None:
            return self._epoch_sampled(e, batch, augment, radiometric, weights, draws)
        c = self._cols
        with torch.cuda.device(self.device):
            ops.pair_epoch_draw(self.pairs, self.flag, self.poly_off, self.poly_pts, self.pt_tile, self.pt_xy, self.pt_inner, self.pt_obj,
                                self.pt_region, self.seed, e, batch, c["tile_id"], c["xy"], c["inner"], c["obj"], c["region"], c["flag"],
                                point_id=c["point_id"])
            if augment is not None:
                if self._orient is None:
                    self._orient = torch.empty((2 * len(self),), dtype=torch.int32, device=self.device)
                ops.pair_epoch_orient(self.seed, e, len(self), batch, ops.ORIENT_MASKS[augment], self._orient)
                c = dict(c, orient=self._orient)
            if radiometric is not None:
                bands = int(self.tiles.shape[1])
                if self._radio is None:
                    self._radio = torch.empty((2 * len(self), bands, 2), dtype=torch.int32, device=self.device)
                ops.pair_epoch_radiometric(self.seed, e, len(self), batch, bands, *radiometric.spans(), self._radio)
                c = dict(c, radio=self._radio)
        return EpochTable(c, len(self), batch, e)

    def pair_terms(self, net, batch: int, margin: float, key: int = 0) -> torch.Tensor:
        """fp32 [N] (a new tensor): the contrastive loss term of every pair IN PAIR ORDER under `net` as it stands -- what
        `hardness_weights` turns into mining weights.  The pairs are fed through the sampled draw with src = arange(N)
        (dm_pair_epoch_draw_src: position = pair id, epoch word = `key`, so the sample points are a function of (seed, key, pair)),
        without augmentation, `batch` pairs per eval-mode forward under no_grad, then ops.contrastive_terms at `margin`.  Its table
        columns and feeds are its own: neither epoch()'s tables nor a training feed are touched, and no RNG is read."""
        from .feed import PairFeed
        from .trainer import stacked_pair_inputs
        N, B = len(self), int(batch)
        if B < 1:
            raise ValueError("batch must be >= 1")
        scales = [int(s) for s in getattr(net, "input_image_scales", ())]
        if not scales:
            raise ValueError(f"{type(net).__name__} has no input_image_scales: pair_terms feeds patch pyramids")
        rows, numerics = stacked_pair_inputs(net), getattr(net, "numerics", ops.get_numerics())
        term = torch.empty(N, dtype=torch.float32, device=self.device)
        d2 = torch.empty(N, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            if self._terms is None:
                self._terms = self._empty_cols(N, src=torch.arange(N, dtype=torch.int32, device=self.device))
            c = self._terms
            ops.pair_epoch_draw(*self._draw_inputs(), self.seed, key, B, c["tile_id"], c["xy"], c["inner"], c["obj"], c["region"], c["flag"],
                                point_id=c["point_id"], src=c["src"])
            table = EpochTable({k: v for k, v in c.items() if k != "src"}, N, B, int(key))
            feeds = []
            for b in sorted({table.pairs_in_step(0), table.pairs_in_step(len(table) - 1)}):
                k = (tuple(scales), bool(rows), str(numerics), b)
                if k not in self._term_feeds:
                    self._term_feeds[k] = PairFeed(self.tiles, scales, b, self.max_window(len(scales)), rows=rows, numerics=numerics)
                feeds.append(self._term_feeds[k])
            by_size = {f.pairs: f for f in feeds}
            was_training = net.training
            net.eval()
            try:
                with torch.no_grad():
                    for s in range(len(table)):
                        b, off = table.pairs_in_step(s), s * B
                        feed = by_size[b]
                        _, _, _, _, flag = feed.fill(table.step(s))
                        F = net(feed.both, feed.dboth)
                        if not (isinstance(F, torch.Tensor) and F.dim() == 2 and F.shape[0] == 2 * b and F.dtype == torch.float32):
                            raise ValueError(f"the model's eval output must be a float32 [{2 * b}, D] tensor, got "
                                             f"{getattr(F, 'dtype', type(F).__name__)} {tuple(getattr(F, 'shape', ()))}")
                        F = F.contiguous()
                        ops.contrastive_terms(F[:b], F[b:], flag, float(margin), d2=d2[off:off + b], term=term[off:off + b])
            finally:
                net.train(was_training)
            for f in feeds:
                f.check()
        return term
