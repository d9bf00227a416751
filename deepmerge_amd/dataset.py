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

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops, rag
from .feed import PairTable
from .patches import geo_to_pixel

MAX_WINDOW = 384        # the gather's LDS staging limit (csrc/dm_patches.hip MAX_WINDOW)


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


class EpochTable:
    """One epoch's sample table on the device, in the per-step blocked layout: `len()` steps, step s is a feed.PairTable of
    b_s = min(batch, N - s batch) pairs made of views (rows [2 s batch, 2 s batch + 2 b_s), flags [s batch, s batch + b_s))."""

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

    def epoch(self, e: int, batch: int, augment: Optional[str] = None, radiometric=None) -> EpochTable:
        """Draw epoch e (one launch, nothing read back); the table's `point_id` column holds the drawn global point ids.
        augment: None, "flips" or "d4" -- with one more launch, every pair of the epoch also draws a dihedral orientation keyed by
        (seed, epoch, pair) ("flips": the four without the transposition), the table's `orient` column, which
        PairFeed.fill applies to both of the pair's crops.  None: the tables carry orient=None.
        radiometric: None, an ops.Radiometric or a (contrast, brightness, colour) triple -- with one more launch, every pair also
        draws a gain and an offset per band keyed by (seed, epoch, pair), the table's `radio` column, applied by
        PairFeed.fill to both of the pair's crops and designed rows.  Independent of `augment`.  None: radio=None."""
        if batch < 1:
            raise ValueError("batch must be >= 1")
        if augment is not None and augment not in ops.ORIENT_MASKS:
            raise ValueError(f"augment must be None, 'flips' or 'd4', got {augment!r}")
        radiometric = ops.Radiometric.of(radiometric)
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
