"""Scenes larger than one tile: tile stream, seam stitch, one merge.

Everything from image to merged partition elsewhere in this package works on one tile resident in HBM.  A real scene has 10^9 to
10^10 pixels: it fits neither the raster kernels' index range (2^31 pixels) nor, with its intermediates, the device.  This
module streams the scene through the device tile by tile and runs ONE merge over the scene's graph.

The definition.  Superpixels are made per tile and never cross a seam.  Everything after that is, bit for bit, what the one-tile
pipeline (`FeatureIO.merge_tile`) computes on the whole scene given the assembled seam-cut label raster with scene-wide ids:
statistics, designed features, edges and boundary lengths, sample points and window fields, the crops the encoder sees, the
merge.  What the per-tile passes cannot see -- the RAG edges whose two pixels lie in different tiles, and the pixel edges a tile
counted as "raster border" although another label faces them -- is added by one `rag.seam_stitch` launch over all seams
(csrc/dm_scene.hip).  The encoder's crops reach across seams: every tile is read with a halo of (max_window + 1) // 2 pixels.
(The encoder's rows are bit-equal to the whole-scene call's as far as the encoder itself does not depend on which points share
a batch: the batches of a scene break at tile boundaries.)

Known consequence: where the learned merge does not join two superpixels across a seam, a straight boundary stays on the seam
line; superpixels that cross seams avoid it: brought along as a label raster, or made here by `slic_labels` (both below;
`segment_scene(..., cross_seams=True)`).  Out of scope: a pixel-start `rag.mrs` on a scene; overlapping the copy of the next tile
with compute.

Superpixels from a label raster.  `segment_labels` (`segment_scene(..., labels=, n_labels=)`) takes the scene's
superpixels as an int32 raster on the host whose regions know nothing of the tile grid -- those of external GIS software, or an
earlier merge's result -- and returns what `FeatureIO.merge_tile` returns on the whole scene, bit for bit, whatever the tile size.
Statistics and edges are folded over the tiles a region lies in (`label_graph`), the seam stitch meets equal ids on both sides of
a seam, and the sample points are a scene-wide per-region maximum over k passes (`sample_points`, csrc/dm_scene_points.hip).
`mrs_labels` runs the classical baseline `rag.mrs` on the same graph.

Superpixels that cross seams, made here.  `slic_labels` is `rag.slic` on a scene, bit for bit, whatever the tile
size: one scene-wide table of centres, the assignment passes streamed core by core (csrc/dm_scene_slic.hip), components and
absorption finished on the component graph.  `slic_assign` is its steps 1-3.

Rings and arcs.  `trace_labels` traces a scene's label raster -- the merged raster through
`SceneResult.trace` -- into the rings and arcs `rag._trace` gives on the whole raster, array for array and bit for bit, whatever
the tile size: every tile is read with one pixel of its neighbours' labels, its core's darts get scene-wide 64-bit ids
(csrc/dm_scene_vector.hip), the tiles' tables are joined by one sort, and the jumping rounds run once over the scene's table.
`SceneResult.save_shapefiles` writes them as `polygons.shp` and `lines.shp`.

Simplified rings and arcs.  `simplify_labels` is `rag.simplify` on a scene, bit for bit: the same tile stream
also yields the scene's nodes (csrc/dm_scene_simplify.hip), and the keep flag per pixel corner becomes two sorted node lists, one
byte per stored arc vertex and the sorted kept set.  `SceneResult.simplified` and `save_shapefiles(..., tolerance=)` go through it.
Out of scope: `PointsGCS.shp` for a scene; overlapping the next tile's read with compute.

Topology-safe simplification.  `simplify_labels_topology` is `rag.simplify(..., topology=True)` on a
scene, bit for bit: the detection and repair rounds of 3.5.12 run on the byte per stored arc vertex, over a grid whose cell side
grows with the scene (csrc/dm_scene_simplify_topology.hip); `simplify_conflicts` lists what the plain call breaks.

Polygon rings as a label source.  `RingSource` stands for `rag.rasterize` of a scene's rings without building
the raster: a read sorts the events of its band of rows once and fills its window of columns (csrc/dm_scene_rasterize.hip), bit
for bit the whole-raster call's pixels, for any H, W < 2^31.  It goes wherever a label or truth source goes; `rasterize_rings`
and `labels_from_shapefile` write the host raster tile by tile.

Boundary scores.  `boundary_scores` is `rag.boundary_scores` on a scene: every core read with a halo of the
tolerance plus one pixel, the counts taken on the core and added over the cores, equal to the whole-raster call's whatever the
tile size (csrc/dm_boundary.hip).  `SceneResult.boundary_scores` scores the scene's merged partition, or a round of it.

Memory.  The scene's pixels are never on the device as a whole: one halo window at a time.  What is resident for the whole scene
is per superpixel and per sample point: the statistics, the graph, the points and the [P,100] feature rows.  The scene-wide
label raster lives on the host (`labels_out`, a numpy array or a memmap).  Every tile is read twice: once for the graph, once
for the encode, because the designed features the encoder takes need the statistics of ALL tiles' seams first; the alternative
(encode in the first pass once a tile's four neighbours are known) saves the second read at the price of per-tile bookkeeping.
"""
from __future__ import annotations

import ctypes
import time
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib, rag
from .ops import _stream, check

Core = Tuple[int, int, int, int]          # y0, y1, x0, x1


class ArraySource:
    """A scene held in a numpy array, an `np.memmap` or a CPU tensor ([bands,H,W] uint8 for an image, [H,W] int32 for a truth
    raster): `.shape` and `.read(y0, y1, x0, x1)`, the two things `segment_scene` asks of a source."""

    def __init__(self, array):
        if isinstance(array, torch.Tensor):
            if array.is_cuda:
                raise ValueError("ArraySource wraps host memory (the scene is never on the device as a whole)")
            array = array.numpy()
        if not isinstance(array, np.ndarray) or array.ndim not in (2, 3):
            raise ValueError("ArraySource takes a numpy array, an np.memmap or a CPU tensor of 2 or 3 dimensions")
        self.array = array
        self.shape = tuple(int(v) for v in array.shape)

    def read(self, y0: int, y1: int, x0: int, x1: int) -> np.ndarray:
        return np.ascontiguousarray(self.array[..., y0:y1, x0:x1])


def halo_of(max_window: int) -> int:
    """Pixels a tile's window is grown by on every side: the crop of a window of side L <= max_window around (mx, my) starts at
    (2 mx - L) / 2 >= mx - (max_window + 1) // 2 and ends before mx + L / 2 + 1."""
    return (int(max_window) + 1) // 2


def window_of(core: Core, H: int, W: int, halo: int) -> Core:
    """The core grown by `halo` on every side, clipped to the scene."""
    y0, y1, x0, x1 = core
    return max(0, y0 - halo), min(H, y1 + halo), max(0, x0 - halo), min(W, x1 + halo)


@dataclass(frozen=True)
class _Grid:
    """The tile grid of one call, built once by `_Grid.of(H, W, tile)`: an H x W scene in ny x nx tiles of th x tw pixels (tile: an
    int or (th, tw)), the last row and column ragged, down to 1 pixel; cores: the tiles' (y0, y1, x0, x1), row-major."""
    H: int
    W: int
    th: int
    tw: int
    ny: int
    nx: int
    cores: List[Core]

    @classmethod
    def of(cls, H: int, W: int, tile) -> "_Grid":
        th, tw = (tile, tile) if isinstance(tile, int) else tuple(tile)
        th, tw, H, W = int(th), int(tw), int(H), int(W)
        if th < 1 or tw < 1:
            raise ValueError(f"tile must be >= 1, got {tile}")
        if H < 1 or W < 1:
            raise ValueError(f"the scene must have at least one pixel, got {H} x {W}")
        cores = [(y, min(H, y + th), x, min(W, x + tw)) for y in range(0, H, th) for x in range(0, W, tw)]
        return cls(H, W, th, tw, -(-H // th), -(-W // tw), cores)

    def __len__(self) -> int:
        return len(self.cores)

    def window(self, i: int, halo: int) -> Tuple[Core, Core, Tuple[int, int]]:
        """Tile i's window (`window_of` its core), the core's box in window coordinates, and the window's origin (oy, ox)."""
        y0, y1, x0, x1 = self.cores[i]
        wy0, wy1, wx0, wx1 = box = window_of(self.cores[i], self.H, self.W, halo)
        return box, (y0 - wy0, y1 - wy0, x0 - wx0, x1 - wx0), (wy0, wx0)

    def max_window(self, halo: int) -> Tuple[int, int]:
        """(side_y, side_x): the largest height and width among the grid's windows.  A window's height depends on its tile row only
        and its width on its column only; along either axis the windows grow while the halo is still clipped at the scene's start
        (tile q with q t <= halo) and never after, so two tiles decide: the first two when halo < t."""
        def side(n: int, t: int, count: int) -> int:
            q = min(halo // t, count - 1)
            return max(min(n, (r + 1) * t + halo) - max(0, r * t - halo) for r in (q, min(q + 1, count - 1)))
        return side(self.H, self.th, self.ny), side(self.W, self.tw, self.nx)

    def tile_of(self, xy: torch.Tensor) -> torch.Tensor:
        """int64 [P]: the index in `cores` of the tile whose core holds every point (x, y) of xy [P,2]."""
        return torch.div(xy[:, 1].long(), self.th, rounding_mode="floor") * self.nx + torch.div(xy[:, 0].long(), self.tw, rounding_mode="floor")


def point_tiles(xy: torch.Tensor, W: int, tile) -> torch.Tensor:
    """int64 [P]: the row-major index in `tile_grid(H, W, tile)` of the tile whose core holds every point (x, y) of xy [P,2]."""
    return _Grid.of(1, W, tile).tile_of(xy)                      # (the index does not depend on H: one row of tiles will do)


def tile_grid(H: int, W: int, tile) -> List[Core]:
    """The row-major list of (y0, y1, x0, x1) cores that cover an H x W scene in tiles of `tile` (an int or (th, tw)); the last
    row and column are ragged, down to 1 pixel."""
    return _Grid.of(H, W, tile).cores


def _as_source(source):
    return source if hasattr(source, "read") and hasattr(source, "shape") else ArraySource(source)


def _read(source, box: Core, dtype: torch.dtype, ndim: int, device) -> torch.Tensor:
    y0, y1, x0, x1 = box
    got = source.read(y0, y1, x0, x1)
    t = got if isinstance(got, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(got))
    if t.dtype != dtype or t.dim() != ndim or tuple(t.shape[-2:]) != (y1 - y0, x1 - x0):
        raise ValueError(f"source.read({y0}, {y1}, {x0}, {x1}) must return {dtype} with trailing shape [{y1 - y0},{x1 - x0}] and "
                         f"{ndim} dimensions, got {t.dtype} {list(t.shape)}")
    return t.to(device)


class _Clock:
    """Seconds per stage into a dict (tools/mb_scene.py); synchronises at every stage boundary, so only when asked for."""

    def __init__(self, into: Optional[dict], device):
        self.into, self.device = into, device
        self.t = self._now()

    def _now(self):
        if self.into is None:
            return 0.0
        torch.cuda.synchronize(self.device)
        return time.perf_counter()

    def lap(self, stage: str):
        if self.into is not None:
            now = self._now()
            self.into[stage] = self.into.get(stage, 0.0) + now - self.t
            self.t = now


# ---- the limits the pipelines share: each a ValueError before any read ------------------------------------------------------------------
def _image_shape(source) -> Tuple[int, int, int]:
    shape = tuple(source.shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"source.shape must be (bands, H, W) with bands, H, W >= 1, got {shape}")
    return tuple(int(v) for v in shape)


def _label_shape(source, name: str) -> Tuple[int, int]:
    shape = tuple(source.shape)
    if len(shape) != 2 or min(shape) < 1:
        raise ValueError(f"{name}.shape must be (H, W) with H, W >= 1, got {shape}")
    return tuple(int(v) for v in shape)


def _out_raster(out, H: int, W: int, name: str) -> np.ndarray:
    """`out`, allocated if None: the host raster a call writes into."""
    if out is None:
        return np.empty((H, W), dtype=np.int32)
    if not isinstance(out, np.ndarray) or out.dtype != np.int32 or out.shape != (H, W) or not out.flags.writeable:
        raise ValueError(f"{name} must be a writable int32 [{H},{W}] numpy array or memmap")
    return out


def _halo_grid(H: int, W: int, tile, max_window: int) -> Tuple[_Grid, int]:
    """(grid, halo) of a call whose windows hold the encoder's crops: max_window, the tile, then every window below 2^31 pixels."""
    if not 1 <= int(max_window) <= rag.MAX_WINDOW:
        raise ValueError(f"max_window must be in 1..{rag.MAX_WINDOW}, got {max_window}")
    grid, halo = _Grid.of(H, W, tile), halo_of(max_window)
    side_y, side_x = grid.max_window(halo)
    if side_y * side_x >= 1 << 31:
        raise ValueError(f"a tile's window (core + halo of {halo}) must have fewer than 2^31 pixels, got {side_y} x {side_x}")
    return grid, halo


def _check_scene(source, tile, max_window: int, labels_out):
    """Returns (bands, H, W, grid, halo, labels_out)."""
    bands, H, W = _image_shape(source)
    grid, halo = _halo_grid(H, W, tile, max_window)
    return bands, H, W, grid, halo, _out_raster(labels_out, H, W, "labels_out")


def _border(raster: torch.Tensor) -> Tuple[torch.Tensor, ...]:
    """The (top, bottom, left, right) lines of a tile's raster, cloned: what `_seam_pairs` takes of it."""
    return raster[0].clone(), raster[-1].clone(), raster[:, 0].clone(), raster[:, -1].clone()


def _seam_pairs(strips: list, nx: int, ny: int, dev) -> Tuple[torch.Tensor, ...]:
    """All seams of the scene, concatenated: for every seam position the entries of the two facing pixels (left / right of every
    vertical seam, above / below every horizontal one), per field of the strips (strips[i] = a tuple of fields of tile i, each a
    `_border`).  Returns (a, b) per field."""
    fields = len(strips[0])
    sa, sb = [[] for _ in range(fields)], [[] for _ in range(fields)]
    for r in range(ny):
        for c in range(nx):
            for f in range(fields):
                top, bottom, left, right = strips[r * nx + c][f]
                if c + 1 < nx:
                    sa[f].append(right); sb[f].append(strips[r * nx + c + 1][f][2])
                if r + 1 < ny:
                    sa[f].append(bottom); sb[f].append(strips[(r + 1) * nx + c][f][0])
    empty = torch.empty(0, dtype=torch.int32, device=dev)
    return tuple((torch.cat(sa[f]), torch.cat(sb[f])) if sa[f] else (empty, empty) for f in range(fields))


def _scene_graph(source, tile=4096, segmenter: Optional[Callable] = None, k: int = 3, max_window: int = rag.MAX_WINDOW,
                 labels_out=None, device="cuda:0", stage_times: Optional[dict] = None) -> dict:
    """The first pass of `segment_scene`, everything but the encoder and the merge: per tile segment, statistics, edges, points;
    then the seam stitch, the edge sort and the designed features.  Returns the fields of a SceneResult that do not need a net."""
    source = _as_source(source)
    bands, H, W, grid, halo, labels_out = _check_scene(source, tile, max_window, labels_out)
    segmenter = rag.slic if segmenter is None else segmenter
    dev, i32, tiles = torch.device(device), torch.int32, grid.cores
    clock = _Clock(stage_times, dev)
    offsets, point_offsets = [0], [0]
    stats_parts: Dict[str, list] = {key: [] for key in rag._STAT_KEYS}
    edge_parts, weight_parts, strips = [], [], []
    pt_parts: Dict[str, list] = {f: [] for f in ("xy", "label", "inner", "obj", "ptr", "bbox", "round")}
    nb = min(bands, 3)
    # (the first pass needs the core only; the halo is what the encoder's crops reach into, in the second pass)
    for i, (y0, y1, x0, x1), core_tile, _, _ in _windows(source, grid, 0, torch.uint8, 3, dev, clock):
        labels, n = segmenter(core_tile)
        n = int(n)
        if labels.dtype != i32 or tuple(labels.shape) != (y1 - y0, x1 - x0) or n < 1:
            raise ValueError(f"segmenter must return (labels int32 [{y1 - y0},{x1 - x0}], n >= 1) for tile {i}, got "
                             f"{labels.dtype} {list(labels.shape)}, n = {n}")
        off = offsets[-1]
        if off + n > rag.MAX_REGIONS:
            raise ValueError(f"the scene has more than 2^24 superpixels ({off + n} after tile {i} of {len(tiles)}): one merge takes "
                             f"at most {rag.MAX_REGIONS} regions; use larger superpixels")
        inside = (labels >= 0) & (labels < n)
        local = torch.where(inside, labels, torch.full_like(labels, -1)).contiguous()      # ids outside [0, n): "no superpixel"
        clock.lap("segment")
        st = rag.label_stats(local, core_tile, n)
        e, w = rag.rag_edges(local, n)
        pts = rag.sample_points(local, n, k=k, max_window=max_window)
        # tile ids / positions -> scene ids / positions
        shift = torch.tensor([x0, y0, x0, y0], dtype=i32, device=dev)
        for key in rag._STAT_KEYS:
            stats_parts[key].append(st[key] if key != "bbox" else torch.where(st["bbox"][:, 2:3] >= 0, st["bbox"] + shift, st["bbox"]))
        edge_parts.append(e + off)
        weight_parts.append(w)
        pt_parts["xy"].append(pts.xy + shift[:2])
        pt_parts["label"].append(pts.label + off)
        pt_parts["inner"].append(pts.inner)
        pt_parts["obj"].append(pts.obj)
        pt_parts["round"].append(pts.round)
        pt_parts["ptr"].append(pts.ptr[:-1] + point_offsets[-1])
        pt_parts["bbox"].append(torch.where(pts.bbox[:, 2:3] >= 0, pts.bbox + shift, pts.bbox))
        glob = torch.where(inside, local + off, local)
        strips.append((_border(glob),))
        offsets.append(off + n)
        point_offsets.append(point_offsets[-1] + pts.xy.shape[0])
        clock.lap("graph")
        labels_out[y0:y1, x0:x1] = glob.cpu().numpy()
        clock.lap("write")
    S, P = offsets[-1], point_offsets[-1]
    stats = {key: torch.cat(stats_parts[key]).contiguous() for key in rag._STAT_KEYS}
    stats["bands"] = nb
    (a, b), = _seam_pairs(strips, grid.nx, grid.ny, dev)
    # (a seam position adds at most one distinct pair: the table is sized for the seams, not for the scene)
    seam_edges, seam_weights = rag.seam_stitch(a, b, S, stats["peri"], max_edges=max(1024, min(8 * S, int(a.numel()))))
    clock.lap("stitch")
    edges, weights = torch.cat(edge_parts + [seam_edges]), torch.cat(weight_parts + [seam_weights])
    order = torch.argsort(edges[:, 0].long() * S + edges[:, 1].long())       # the two sets are disjoint: one sort, nothing to fold
    edges, weights = edges[order].contiguous(), weights[order].contiguous()
    designed = rag.designed_features(stats)                      # only now: `peri` and `border` need the seam fix
    ptr = torch.cat(pt_parts["ptr"] + [torch.tensor([P], dtype=i32, device=dev)])
    points = rag.PointSamples(xy=torch.cat(pt_parts["xy"]), label=torch.cat(pt_parts["label"]), inner=torch.cat(pt_parts["inner"]),
                              obj=torch.cat(pt_parts["obj"]), ptr=ptr, idx=torch.arange(P, dtype=i32, device=dev),
                              bbox=torch.cat(pt_parts["bbox"]), round=torch.cat(pt_parts["round"]))
    clock.lap("graph")
    return dict(n_labels=S, tiles=tiles, offsets=offsets, point_offsets=point_offsets, stats=stats, designed=designed, edges=edges,
                weights=weights, points=points, labels=labels_out, halo=halo, n_seam=int(a.numel()), n_seam_edges=int(seam_edges.shape[0]),
                source=source, device=dev, grid=grid)


@dataclass
class SceneResult:
    """What `segment_scene` leaves.  result: the MergeResult of the one merge over the scene; n_labels: superpixels of the scene;
    tiles: the cores (y0, y1, x0, x1), row-major; offsets [T+1]: tile i owns the scene-wide ids offsets[i] .. offsets[i+1]-1, or
    None when the superpixels come from a label raster whose regions cross seams (`segment_labels`: no tile owns an id);
    stats / designed / edges / weights: `label_stats`, `designed_features` and `rag_edges` of the scene; points: a PointSamples in
    scene coordinates; features [P,100]: the encoder's rows; labels: the scene-wide superpixel raster on the host (`labels_out`,
    or what `segment_labels` was given: an array, or anything with `.shape` and `.read`)."""
    result: "rag.MergeResult"
    n_labels: int
    tiles: List[Core]
    offsets: Optional[List[int]]
    stats: Dict[str, torch.Tensor]
    designed: torch.Tensor
    edges: torch.Tensor
    weights: torch.Tensor
    points: "rag.PointSamples"
    features: torch.Tensor
    labels: np.ndarray

    def _tile_labels(self, i: int) -> torch.Tensor:
        return _read(_as_source(self.labels), self.tiles[i], torch.int32, 2, self.edges.device)

    def merged_tile(self, i: int) -> torch.Tensor:
        """int32 [th,tw] on the device: tile i of the merged raster, `relabel_raster` of its superpixels with `result.region_of`."""
        return rag.relabel_raster(self._tile_labels(i), self.result.region_of)

    def write_merged(self, out=None) -> np.ndarray:
        """Streams every tile of the merged raster into `out`, a writable int32 [H,W] numpy array or memmap (allocated if None)."""
        out = _out_raster(out, *(int(v) for v in self.labels.shape), "out")
        for i, (y0, y1, x0, x1) in enumerate(self.tiles):
            out[y0:y1, x0:x1] = self.merged_tile(i).cpu().numpy()
        return out

    def _tile(self) -> Tuple[int, int]:
        y0, y1, x0, x1 = self.tiles[0]
        return y1 - y0, x1 - x0

    def trace(self, merged=None, tile=None, stats: Optional[dict] = None) -> Tuple["rag.Polygons", "rag.Arcs"]:
        """The merged regions as polygon rings and boundary arcs in scene coordinates, regions that cross seams in one piece:
        `trace_labels` of the merged raster.  merged: the host raster as `write_merged` returns it (computed if None); tile: the
        tracing tile, default the scene's own.  `Arcs.edge` is the row of (right, left) in `result.edges`.  Equals
        `MergeResult.polygons / boundary_arcs` on the assembled raster."""
        merged = self.write_merged() if merged is None else merged
        C = int(self.result.rep.numel())
        polys, arcs = trace_labels(merged, C, tile=self._tile() if tile is None else tile, stats=stats, device=self.edges.device)
        return polys, rag._attach_edges(arcs, C, self.result.edges)

    def polygons(self, merged=None, tile=None) -> "rag.Polygons":
        return self.trace(merged, tile)[0]

    def boundary_arcs(self, merged=None, tile=None) -> "rag.Arcs":
        return self.trace(merged, tile)[1]

    def simplified(self, tolerance: float, merged=None, tile=None, stats: Optional[dict] = None) -> Tuple["rag.Polygons", "rag.Arcs"]:
        """The rings and arcs of `trace`, simplified to `tolerance` pixels once per stretch of shared boundary:
        `simplify_labels` of the merged raster, `Arcs.edge` attached as `trace` does.  Equals `MergeResult.simplified` on the
        assembled raster."""
        return self._simplified(simplify_labels, tolerance, merged, tile, stats=stats)

    def simplified_topology(self, tolerance: float, merged=None, tile=None, stats: Optional[dict] = None,
                            max_rounds: int = 64) -> Tuple["rag.Polygons", "rag.Arcs"]:
        """`simplified` with what plain simplification breaks repaired: `simplify_labels_topology` of the merged raster.  Equals
        `MergeResult.simplified(..., topology=True)` on the assembled raster."""
        return self._simplified(simplify_labels_topology, tolerance, merged, tile, stats=stats, max_rounds=max_rounds)

    def _simplified(self, call, tolerance, merged, tile, **kw):
        merged = self.write_merged() if merged is None else merged
        C = int(self.result.rep.numel())
        polys, arcs = call(merged, C, tolerance, tile=self._tile() if tile is None else tile, device=self.edges.device, **kw)
        return polys, rag._attach_edges(arcs, C, self.result.edges)

    def save_shapefiles(self, folder: str, geotransform=None, merged=None, tile=None, tolerance: Optional[float] = None,
                        topology: bool = False) -> Tuple[str, str]:
        """Write the merged regions as the two layers of `FeatureIO.save_shapefiles` that a scene has: `polygons.shp` (one record
        per merged region: the 15 designed fields of `designed_features(result.stats)` and `PointID` from `result.ptr / idx`) and
        `lines.shp` (one record per boundary arc: LEFT_FID, RIGHT_FID, simi = `result.simi` of the arc's edge, 0.0 on the scene's
        frame), through the same writer.  tolerance: None writes the traced pixel staircase; a number writes the rings and arcs of
        `simplified(tolerance)`, or of `simplified_topology(tolerance)` with topology=True, so the two layers share every vertex; topology=True also repairs collapsed
        islands and boundaries that cross, so a GIS takes the layer as it is.  Without a tolerance `topology` has no effect, as in
        `FeatureIO.save_shapefiles`: the traced staircase has no conflict to repair.  No `PointsGCS.shp`: out of scope for a scene.
        Returns the two paths."""
        from .ExtractFeatures import write_polygon_and_line_layers
        simplified = self.simplified_topology if topology else self.simplified
        polys, arcs = self.trace(merged, tile) if tolerance is None else simplified(tolerance, merged, tile)
        r = self.result
        return tuple(write_polygon_and_line_layers(folder, polys, arcs, int(r.rep.numel()), r.ptr, r.idx, rag.designed_features(r.stats),
                                                   edges=r.edges, simi=r.simi, geotransform=geotransform))

    def overlap(self, truth_source, n_truth: int) -> "rag.Overlap":
        """The `Overlap` of the scene's superpixels with a ground-truth raster (int32 [H,W]: an array, a memmap, a CPU tensor, or
        anything with `.read(y0, y1, x0, x1)` returning int32 [y1-y0, x1-x0]), for `result.scores(...)`: per tile one
        `rag.label_overlap` with tile-local ids (so that every table is sized for one tile), keys shifted to scene-wide ids and
        concatenated, then the facts of the whole table.  Equals `rag.label_overlap` on the assembled rasters field by field.
        Without `offsets` (regions cross seams) the tile-local ids come from compacting the ids present in the tile, and a cell
        that several tiles hold is folded, counts added."""
        truth_source = _as_source(truth_source)
        G, dev = int(n_truth), self.edges.device
        keys, counts = [], []
        for i, core in enumerate(self.tiles):
            truth = _read(truth_source, core, torch.int32, 2, dev)
            glob = self._tile_labels(i)
            if self.offsets is None:
                local, ids = _compact_ids(glob, self.n_labels)
                if ids.numel() == 0:
                    continue
                ov = rag.label_overlap(local, truth, int(ids.numel()), G)
                keys.append(ids[ov.cells[:, 0].long()] * (G + 1) + ov.cells[:, 1].long())
            else:
                off, n = self.offsets[i], self.offsets[i + 1] - self.offsets[i]
                local = torch.where(glob >= 0, glob - off, glob)
                ov = rag.label_overlap(local, truth, n, G)
                keys.append((ov.cells[:, 0].long() + off) * (G + 1) + ov.cells[:, 1].long())
            counts.append(ov.count)
        if self.offsets is not None:
            return rag._overlap_facts(torch.cat(keys), torch.cat(counts), self.n_labels, G)    # sorted: offsets ascend
        empty = torch.empty(0, dtype=torch.int64, device=dev)
        uniq, inverse = torch.unique(torch.cat(keys + [empty]), return_inverse=True)           # sorted
        folded = torch.zeros(uniq.numel(), dtype=torch.int32, device=dev).index_add_(0, inverse, torch.cat(counts + [empty.to(torch.int32)]))
        return rag._overlap_facts(uniq, folded, self.n_labels, G)

    def boundary_scores(self, truth_source, n_truth: int, tolerance=2, round: Optional[int] = None):
        """The boundaries of the scene's merged partition (round None), or of the partition after `round` rounds, scored against
        a ground-truth source at `tolerance` pixels: `boundary_scores` of the superpixel raster with mapping = `result.region_of`
        or `result.region_of_at(round)`, on the scene's own tile.  Equals `MergeResult.boundary_scores` on the assembled rasters."""
        mapping = self.result.region_of if round is None else self.result.region_of_at(round)
        return boundary_scores(self.labels, truth_source, self.n_labels, n_truth, tolerance=tolerance, tile=self._tile(),
                               mapping=mapping, device=self.edges.device)


def segment_scene(fio, source, tile=4096, segmenter: Optional[Callable] = None, k: int = 3, margin: float = 1.0,
                  max_window: int = rag.MAX_WINDOW, batch_size: int = 2000, labels_out=None, stage_times: Optional[dict] = None,
                  labels=None, n_labels: Optional[int] = None, cross_seams: bool = False, slic: Optional[dict] = None,
                  **merge_kwargs) -> SceneResult:
    """From a scene of any size to its merged partition (the module docstring states the definition).

    fio: a FeatureIO; source: `.shape == (bands, H, W)` and `.read(y0, y1, x0, x1) -> uint8 [bands, y1-y0, x1-x0]` (a numpy
    array or a CPU tensor), or an array / memmap / CPU tensor, which is wrapped in an ArraySource; tile: core side, an int or
    (th, tw); segmenter(core_tile uint8 [bands,th,tw] on the device) -> (labels int32 [th,tw], n), default `rag.slic` with its
    defaults (ids outside [0, n) are written as -1, "no superpixel"); k, max_window: as `rag.sample_points` takes them; margin,
    merge_kwargs: as `rag.merge_regions` takes them (max_rounds, min_regions, min_area; they reach the one merge on every path
    below); labels_out: a writable int32 [H,W] numpy array or memmap for the scene-wide superpixel raster, allocated if None;
    stage_times: a dict that receives seconds per stage (synchronises at stage boundaries).
    labels, n_labels: the scene's superpixels brought along as a label raster on the host, whose regions may cross seams: the call
    is `segment_labels(fio, source, labels, n_labels, ...)` (no segmenter and no labels_out go with it: ValueError).
    cross_seams=True makes the superpixels here and lets them cross the seams: `slic_labels(source, tile, **(slic or {}),
    labels_out=labels_out)`, then `segment_labels` on that raster; slic: its keywords (cell, compactness, iters, min_size,
    resident_bytes).  It takes no segmenter and no labels= (ValueError); the default, False, is the per-tile path above.
    Limits: at most 2^24 superpixels in the scene, every window (core + halo) below 2^31 pixels."""
    if cross_seams:
        if segmenter is not None or labels is not None or n_labels is not None:
            raise ValueError("cross_seams=True makes the scene's superpixels itself (slic_labels): it takes neither a segmenter nor labels=")
        made, n_made = slic_labels(source, tile, **(slic or {}), labels_out=labels_out, device=fio.device, stage_times=stage_times)
        return segment_labels(fio, source, made, n_made, tile=tile, k=k, margin=margin, max_window=max_window, batch_size=batch_size,
                              stage_times=stage_times, **merge_kwargs)
    if slic is not None:
        raise ValueError("slic= holds the keywords of slic_labels: it goes with cross_seams=True")
    if labels is not None:
        if segmenter is not None or labels_out is not None:
            raise ValueError("labels= brings the scene's superpixels along: it takes neither a segmenter nor labels_out")
        if n_labels is None:
            raise ValueError("n_labels must be given with labels")
        return segment_labels(fio, source, labels, n_labels, tile=tile, k=k, margin=margin, max_window=max_window, batch_size=batch_size,
                              stage_times=stage_times, **merge_kwargs)
    if n_labels is not None:
        raise ValueError("n_labels goes with labels")
    g = _scene_graph(source, tile, segmenter, k, max_window, labels_out, device=fio.device, stage_times=stage_times)
    clock = _Clock(stage_times, g["device"])
    _need_points(g["points"])
    offs = g["point_offsets"]
    rows = [slice(lo, hi) if hi > lo else None for lo, hi in zip(offs, offs[1:])]
    return _encode_and_merge(fio, g, rows, clock, margin, batch_size, merge_kwargs)


def _need_points(pts: "rag.PointSamples"):
    if pts.xy.shape[0] < 1:
        raise ValueError("the scene has no sample point (no pixel carries a superpixel id)")


def _encode_and_merge(fio, g: dict, rows: list, clock: _Clock, margin: float, batch_size: int, merge_kwargs: dict) -> SceneResult:
    """What `segment_scene` and `segment_labels` end in: the encoder over every tile's halo window, then the one merge.  g: the
    graph dict; rows[i]: the rows of tile i's points in the points' tables, a slice or an index tensor, None for a tile without
    points (it is not read)."""
    dev, pts = g["device"], g["points"]
    features = torch.empty((pts.xy.shape[0], 100), dtype=torch.float32, device=dev)
    only = [i for i, r in enumerate(rows) if r is not None]
    for i, _, window, _, (oy, ox) in _windows(g["source"], g["grid"], g["halo"], torch.uint8, 3, dev, clock, only):
        r = rows[i]
        origin = torch.tensor([ox, oy], dtype=torch.int32, device=dev)
        features[r] = fio.extract_features_from_tile(window, pts.xy[r] - origin, pts.inner[r], pts.obj[r], g["designed"][pts.label[r].long()],
                                                     batch_size=batch_size)
        clock.lap("encode")
    fio.features = features
    result = rag.merge_regions(features, pts.ptr, pts.idx, g["edges"], margin=margin, weights=g["weights"], stats=g["stats"], **merge_kwargs)
    clock.lap("merge")
    return SceneResult(result=result, n_labels=g["n_labels"], tiles=g["tiles"], offsets=g["offsets"], stats=g["stats"], designed=g["designed"],
                       edges=g["edges"], weights=g["weights"], points=pts, features=features, labels=g["labels"])


def _windows(source, grid: _Grid, halo: int, dtype: torch.dtype, ndim: int, dev, clock: _Clock, only=None):
    """The halo-window stream of every pipeline: per tile (i, core, window on the device, the core's box in window coordinates, the
    window's origin (oy, ox) in the scene), the window being the core and `halo` pixels of its neighbours, clipped to the scene.
    dtype, ndim: what the source must deliver; only: the tiles to read, default all."""
    for i in range(len(grid)) if only is None else only:
        wbox, box, origin = grid.window(i, halo)
        window = _read(source, wbox, dtype, ndim, dev)
        clock.lap("read + copy")
        yield i, grid.cores[i], window, box, origin


# ---- a scene from a label raster whose regions cross tile seams (csrc/dm_scene_points.hip) ------------------------
MAX_POINT_SCENE = 1 << 48             # DM_SCENE_POINTS_MAX_PIXELS: the key keeps 2^48 - 1 - (y W + x) in 48 bits
MAX_SCENE_SIDE = (1 << 31) - 1        # points and boxes are int32


def _check_labels(labels, n_labels, k, max_window, tile, like: Optional[tuple] = None):
    """The limits of the calls below, each a ValueError before any device work.  labels: the label source; like: the (H, W) the
    raster must have (the image's).  Returns (H, W, S, k, grid, halo)."""
    H, W = _label_shape(labels, "labels")
    if like is not None and (H, W) != tuple(like):
        raise ValueError(f"labels must cover the scene: labels.shape = ({H}, {W}), the source has {like[0]} x {like[1]} pixels")
    if H > MAX_SCENE_SIDE or W > MAX_SCENE_SIDE or H * W > MAX_POINT_SCENE:
        raise ValueError(f"the scene must have H, W < 2^31 and at most 2^48 pixels (the points' 64-bit key), got {H} x {W}")
    S = int(n_labels)
    if not 1 <= S <= rag.MAX_REGIONS:
        raise ValueError(f"n_labels must be in 1..2^24, got {n_labels}")
    if not 1 <= int(k) <= rag.MAX_POINTS:
        raise ValueError(f"k must be in 1..{rag.MAX_POINTS}, got {k}")
    return (H, W, S, int(k), *_halo_grid(H, W, tile, max_window))


def _compact_ids(labels: torch.Tensor, n_labels: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(local int32 like labels, ids int64 [n] ascending): the ids of [0, n_labels) present in `labels` numbered 0..n-1 in
    ascending order, every other id -1 ("no superpixel"), so that the per-tile tables are sized for the tile, not for the scene."""
    u, inverse = torch.unique(labels, return_inverse=True)
    ok = (u >= 0) & (u < n_labels)
    local_of = torch.where(ok, torch.cumsum(ok, 0) - 1, torch.full_like(u, -1, dtype=torch.int64)).to(torch.int32)
    return local_of[inverse].contiguous(), u[ok].long()


def sample_points(labels, n_labels: int, k: int = 3, max_window: int = rag.MAX_WINDOW, tile=4096, device="cuda:0",
                  stage_times: Optional[dict] = None) -> "rag.PointSamples":
    """`rag.sample_points` on a scene's label raster, equal in every field whatever the tile size, although a region's pixels lie in
    several tiles (csrc/dm_scene_points.hip; the rule: include/deepmerge_hip.h).

    labels: int32 [H, W] on the host -- an array, an `np.memmap`, a CPU tensor, or anything with `.shape == (H, W)` and
    `.read(y0, y1, x0, x1) -> int32 [y1-y0, x1-x0]`; ids outside [0, n_labels) get no points.  The tables (best, points, counts,
    boxes: 8 + 12 k + 20 bytes per superpixel) stay on the device; per round every tile's halo window of labels is read, its
    clearance taken and its core's candidates folded in, then the round's scene-wide winners are committed: k passes over the
    label raster, because round j + 1 scores against round j's winners.  Limits, each a ValueError before any device work: H, W <
    2^31 and H W <= 2^48; n_labels in 1..2^24; k in 1..16; max_window in 1..384; every window below 2^31 pixels."""
    source = _as_source(labels)
    H, W, S, k, grid, halo = _check_labels(source, n_labels, k, max_window, tile)
    dev, lib, i32 = torch.device(device), _lib.lib(), torch.int32
    clock = _Clock(stage_times, dev)
    best = torch.empty(S, dtype=torch.int64, device=dev)
    pts = torch.empty((S, k, 2), dtype=i32, device=dev)
    pclr = torch.empty((S, k), dtype=i32, device=dev)
    cnt = torch.empty(S, dtype=i32, device=dev)
    bbox = torch.empty((S, 4), dtype=i32, device=dev)
    for j in range(k):
        for i, _, window, box, (oy, ox) in _windows(source, grid, halo, i32, 2, dev, clock):
            window = window.contiguous()
            clr = rag.clearance(window, max_window)
            if i == 0 and j == 0:                                # (behind the first read: a source of the wrong kind fails before any launch)
                check(lib.dm_scene_point_init(best.data_ptr(), cnt.data_ptr(), bbox.data_ptr(), S, _stream()), "dm_scene_point_init")
            check(lib.dm_scene_point_select(window.data_ptr(), clr.data_ptr(), *window.shape, *box, oy, ox, H, W, S, k, j, pts.data_ptr(),
                                            cnt.data_ptr(), best.data_ptr(), bbox.data_ptr(), _stream()), "dm_scene_point_select")
            clock.lap(f"points round {j}")
        check(lib.dm_scene_point_commit(best.data_ptr(), H, W, S, k, pts.data_ptr(), pclr.data_ptr(), cnt.data_ptr(), _stream()),
              "dm_scene_point_commit")
        clock.lap(f"points round {j}")
    cap = S * k
    ptr = torch.empty(S + 1, dtype=i32, device=dev)
    xy = torch.empty((cap, 2), dtype=i32, device=dev)
    label, inner, obj, rnd = (torch.empty(cap, dtype=i32, device=dev) for _ in range(4))
    check(lib.dm_point_emit(cnt.data_ptr(), pts.data_ptr(), pclr.data_ptr(), bbox.data_ptr(), S, k, int(max_window), cap, ptr.data_ptr(),
                            xy.data_ptr(), label.data_ptr(), inner.data_ptr(), obj.data_ptr(), rnd.data_ptr(), _stream()), "dm_point_emit")
    P = int(ptr[S])                                            # the one readback: sizes the views below
    clock.lap("points emit")
    return rag.PointSamples(xy=xy[:P], label=label[:P], inner=inner[:P], obj=obj[:P], ptr=ptr, idx=torch.arange(P, dtype=i32, device=dev),
                            bbox=bbox, round=rnd[:P])


def label_graph(source, labels, n_labels: int, tile=4096, k: int = 3, max_window: int = rag.MAX_WINDOW, device="cuda:0",
                stage_times: Optional[dict] = None, points: bool = True) -> dict:
    """The net-free pass of `segment_labels`: the dict `_scene_graph` returns, with `offsets` and `point_offsets` None, for
    superpixels that come as a label raster on the host and may cross seams.  Per core the ids present are compacted
    (`torch.unique`), `label_stats` and `rag_edges` run on the tile-local ids and are folded into the scene's tables (counts, sums
    and perimeters add, boxes take min / max, the empty box folds to whatever it meets); then one `rag.seam_stitch` over all seams
    (equal ids facing each other lose the border edge: a region that crosses the seam), one sort of the edge keys with the
    weights of equal keys added (a pair can occur in several tiles and on seams), the designed features, and `sample_points`
    (points=False leaves it out: `mrs_labels`).  `n_edge_parts` is the number of edge rows before the fold."""
    source, lsource = _as_source(source), _as_source(labels)
    bands, *like = _image_shape(source)
    H, W, S, k, grid, halo = _check_labels(lsource, n_labels, k, max_window, tile, like=tuple(like))
    dev, i32, i64, tiles = torch.device(device), torch.int32, torch.int64, grid.cores
    nb = min(bands, 3)
    clock = _Clock(stage_times, dev)
    stats = {"count": torch.zeros(S, dtype=i64, device=dev), "sum": torch.zeros((S, nb), dtype=i64, device=dev),
             "sumsq": torch.zeros((S, nb), dtype=i64, device=dev), "peri": torch.zeros((S, 2), dtype=i64, device=dev),
             "bbox": torch.tensor([(1 << 31) - 1, (1 << 31) - 1, -1, -1], dtype=i32, device=dev).repeat(S, 1)}
    key_parts, weight_parts, strips = [], [], []
    for i, core in enumerate(tiles):
        y0, y1, x0, x1 = core
        lab = _read(lsource, core, i32, 2, dev)                  # (the labels first: a source of the wrong kind fails before any copy)
        core_tile = _read(source, core, torch.uint8, 3, dev)
        clock.lap("read + copy")
        local, ids = _compact_ids(lab, S)
        n = int(ids.numel())
        glob = torch.where(local >= 0, lab, local)               # ids outside [0, S): "no superpixel"
        clock.lap("compact")
        if n:
            st = rag.label_stats(local, core_tile, n)
            e, w = rag.rag_edges(local, n)
            for key in ("count", "sum", "sumsq", "peri"):
                stats[key].index_add_(0, ids, st[key])
            box = st["bbox"] + torch.tensor([x0, y0, x0, y0], dtype=i32, device=dev)       # every local id has pixels: no empty box
            seen = stats["bbox"][ids]
            stats["bbox"][ids] = torch.cat((torch.minimum(seen[:, :2], box[:, :2]), torch.maximum(seen[:, 2:], box[:, 2:])), 1)
            key_parts.append(ids[e[:, 0].long()] * S + ids[e[:, 1].long()])               # ids ascend: a < b stays a < b
            weight_parts.append(w)
        strips.append((_border(glob),))
        clock.lap("graph")
    stats["bands"] = nb
    (a, b), = _seam_pairs(strips, grid.nx, grid.ny, dev)
    seam_edges, seam_weights = rag.seam_stitch(a, b, S, stats["peri"], max_edges=max(1024, min(8 * S, int(a.numel()))))
    clock.lap("stitch")
    keys = torch.cat(key_parts + [seam_edges[:, 0].long() * S + seam_edges[:, 1].long()])
    uniq, inverse = torch.unique(keys, return_inverse=True)      # sorted by (a, b); equal keys of several tiles and seams fold
    weights = torch.zeros(uniq.numel(), dtype=i32, device=dev).index_add_(0, inverse, torch.cat(weight_parts + [seam_weights]))
    edges = torch.stack((uniq // S, uniq % S), 1).to(i32).contiguous()
    designed = rag.designed_features(stats)                      # only now: `peri` and `border` need the seam fix
    clock.lap("graph")
    pts = sample_points(lsource, S, k=k, max_window=max_window, tile=tile, device=dev, stage_times=stage_times) if points else None
    return dict(n_labels=S, tiles=tiles, offsets=None, point_offsets=None, stats=stats, designed=designed, edges=edges, weights=weights,
                points=pts, labels=labels if isinstance(labels, np.ndarray) else lsource, halo=halo, n_seam=int(a.numel()),
                n_seam_edges=int(seam_edges.shape[0]), n_edge_parts=int(keys.numel()), source=source, device=dev, grid=grid)


def segment_labels(fio, source, labels, n_labels: int, tile=4096, k: int = 3, margin: float = 1.0, max_window: int = rag.MAX_WINDOW,
                   batch_size: int = 2000, stage_times: Optional[dict] = None, **merge_kwargs) -> SceneResult:
    """`segment_scene` for superpixels that are brought along: from a scene and its label raster (int32 [H, W] on the host, ids
    0..n_labels-1, anything else "no superpixel"; regions may cross tile seams, as those of external GIS software or of an earlier
    merge do) to the merged partition.  Returns, bit for bit and layer by layer, what `FeatureIO.merge_tile(whole scene, whole
    raster, n_labels, ...)` returns, whatever the tile size (the encoder's rows at equal batch shapes).

    source, tile, k, margin, max_window, batch_size, stage_times, merge_kwargs: as `segment_scene` takes them; labels: as
    `sample_points` takes it.  A point is encoded with the tile whose core holds it, from that tile's halo window; the rows go back
    by index, so the points stay sorted by (superpixel, round) scene-wide.  The result's `offsets` is None.  Limits: those of
    `sample_points`; an id that never occurs has count 0, the empty box and no points."""
    g = label_graph(source, labels, n_labels, tile=tile, k=k, max_window=max_window, device=fio.device, stage_times=stage_times)
    clock = _Clock(stage_times, g["device"])
    _need_points(g["points"])
    tile_of = g["grid"].tile_of(g["points"].xy)
    order = torch.argsort(tile_of, stable=True)                  # within a tile the rows keep their (superpixel, round) order
    ends = torch.cumsum(torch.bincount(tile_of, minlength=len(g["tiles"])), 0).tolist()
    rows = [order[lo:hi] if hi > lo else None for lo, hi in zip([0] + ends, ends)]
    return _encode_and_merge(fio, g, rows, clock, margin, batch_size, merge_kwargs)


def mrs_labels(source, labels, n_labels: int, scale: float, shape: float = 0.1, compactness: float = 0.5, band_weights=None,
               max_rounds: Optional[int] = None, min_regions: int = 0, tile=4096, device="cuda:0",
               stage_times: Optional[dict] = None, min_area: int = 0) -> "rag.MergeResult":
    """The classical baseline on a scene's graph: `rag.mrs(whole scene, scale, labels=whole raster, n_labels=n_labels, ...)` bit
    for bit, whatever the tile size -- `label_graph` without points, then `rag.mrs_graph`.  Every id in [0, n_labels) must occur
    (the same ValueError).  min_area: as `rag.mrs` takes it.  A pixel start on a scene stays out of scope: a merge takes at most
    2^24 regions."""
    min_area = rag._check_min_area(min_area)
    shape3 = tuple(_as_source(source).shape)
    rag._mrs_check(scale, min(int(shape3[0]), 3) if len(shape3) == 3 and shape3[0] >= 1 else 1, shape, compactness, band_weights, max_rounds)
    g = label_graph(source, labels, n_labels, tile=tile, k=1, device=device, stage_times=stage_times, points=False)
    return rag.mrs_graph(g["stats"], g["edges"], g["weights"], scale, shape, compactness, band_weights, max_rounds, min_regions,
                         min_area=min_area)


# ---- rings and arcs across tile seams (csrc/dm_scene_vector.hip) ---------------------------------------------------
MAX_TRACE_SIDE = (1 << 31) - 1        # DM_SCENE_VECTOR_MAX_SIDE: H, W below it, so every corner fits int32
MAX_TRACE_SCENE = 1 << 60             # DM_SCENE_VECTOR_MAX_PIXELS: dart ids 4 (y W + x) + side stay below 2^62
MAX_DARTS = 1 << 31                   # slots are int32


def _check_trace(source, n_labels, tile) -> Tuple[int, int, int, _Grid]:
    H, W = _label_shape(source, "source")
    if H >= MAX_TRACE_SIDE or W >= MAX_TRACE_SIDE:
        raise ValueError(f"H and W must be below 2^31 - 1, got {H} x {W}")
    if H * W > MAX_TRACE_SCENE:
        raise ValueError(f"the scene must have at most 2^60 pixels (64-bit dart ids), got {H} x {W}")
    S = int(n_labels)
    if not 1 <= S < 1 << 31:
        raise ValueError(f"n_labels must be in 1..2^31-1, got {n_labels}")
    grid = _Grid.of(H, W, tile)
    side_y, side_x = grid.max_window(1)
    if side_y * side_x > rag.MAX_TRACE_PIXELS:
        raise ValueError(f"a tile's window (core + 1 pixel on every side) must have at most 2^28 pixels, got {side_y} x {side_x}")
    return H, W, S, grid


def _check_darts(total: int, i: int, n_tiles: int):
    if total >= MAX_DARTS:
        raise ValueError(f"the scene has 2^31 darts or more ({total} after tile {i} of {n_tiles}): slots are 32-bit; trace a coarser "
                         f"partition or the scene in parts")


def _tile_darts(window: torch.Tensor, box: Core, origin: Tuple[int, int], H: int, W: int):
    """The dart records of one tile (dm_scene_vector_count, dm_vector_emit, dm_scene_vector_link).  window int32 [wh,ww] on the
    device: the core `box` = (cy0, cy1, cx0, cx1) in window coordinates and its apron; origin (oy, ox): the window's first pixel in
    the H x W scene.  Returns (id int64, succ int64, lab, other, succ_flags uint8), each [D], in the tile's slot order; None when
    the core has no dart."""
    rag._need_cuda(window)
    lib, dev, i32 = _lib.lib(), window.device, torch.int32
    window = window.contiguous()
    wh, ww = window.shape
    cy0, cy1, cx0, cx1 = box
    new = lambda n, dt: torch.empty(n, dtype=dt, device=dev)
    n_tiles = ((wh + 63) // 64) * ((ww + 63) // 64)
    mask, core_mask, tile_off, meta = new(wh * ww, torch.uint8), new(wh * ww, torch.uint8), new(n_tiles + 1, i32), new(1, i32)
    check(lib.dm_scene_vector_count(window.data_ptr(), wh, ww, cy0, cy1, cx0, cx1, mask.data_ptr(), core_mask.data_ptr(), tile_off.data_ptr(),
                                    meta.data_ptr(), _stream()), "dm_scene_vector_count")
    D = int(meta[0])
    if D == 0:
        return None
    first_slot, dart = new(wh * ww, i32), new(D, i32)
    check(lib.dm_vector_emit(core_mask.data_ptr(), tile_off.data_ptr(), wh, ww, first_slot.data_ptr(), dart.data_ptr(), _stream()),
          "dm_vector_emit")
    ids, succ = new(D, torch.int64), new(D, torch.int64)
    lab, other, sflags = new(D, i32), new(D, i32), new(D, torch.uint8)
    check(lib.dm_scene_vector_link(window.data_ptr(), mask.data_ptr(), dart.data_ptr(), wh, ww, D, int(origin[0]), int(origin[1]), H, W,
                                   ids.data_ptr(), succ.data_ptr(), lab.data_ptr(), other.data_ptr(), sflags.data_ptr(), _stream()),
          "dm_scene_vector_link")
    return ids, succ, lab, other, sflags


def _join(ids: torch.Tensor, succ: torch.Tensor, lab: torch.Tensor, other: torch.Tensor, succ_flags: torch.Tensor):
    """The tiles' concatenated records as one linked table: one sort by scene dart id (slot order = id order), next = the slot of
    every successor, the returned flags scattered to it (the successor map is a permutation: nothing collides), key = slot << 32 |
    slot.  Returns (dart int64, next int32, lab, other, flags uint8, key int64).  Table arithmetic in torch, as rag._trace does its
    own between the kernels."""
    D = int(ids.numel())
    dart, order = torch.sort(ids)
    succ = succ[order]
    nxt = torch.searchsorted(dart, succ)
    if not bool((dart[nxt.clamp(max=D - 1)] == succ).all()):
        raise RuntimeError("a dart's successor is not a dart of the scene: the tiles' records do not cover one label raster")
    flags = torch.empty(D, dtype=torch.uint8, device=ids.device)
    flags[nxt] = succ_flags[order]
    slot = torch.arange(D, dtype=torch.int64, device=ids.device)
    return dart, nxt.to(torch.int32), lab[order], other[order], flags, (slot << 32) | slot


def _scene_table(source, grid: _Grid, S: int, dev, clock: _Clock, nodes: Optional[list] = None):
    """One stream of the scene's windows (the core and one pixel of apron, ids checked) into the joined dart table
    `rag._trace_table` takes.  nodes: a list that receives every tile's node records (`_tile_nodes`) from the same windows, so
    that the scene is read once."""
    H, W = grid.H, grid.W
    parts, total, n_nodes = [], 0, 0
    for i, _, window, box, origin in _windows(source, grid, 1, torch.int32, 2, dev, clock):
        lo, hi = (int(v) for v in torch.aminmax(window))
        if lo < 0 or hi >= S:
            (oy, ox), (wh, ww) = origin, window.shape
            raise ValueError(f"labels must be in 0..n_labels-1 = 0..{S - 1}: the window of tile {i} (rows {oy}..{oy + wh - 1}, columns "
                             f"{ox}..{ox + ww - 1}) holds {lo}..{hi}")
        got = _tile_darts(window, box, origin, H, W)
        if got is not None:
            total += int(got[0].numel())
            _check_darts(total, i, len(grid))
            parts.append(got)
        if nodes is not None:
            own = _tile_nodes(window, box, origin, H, W)
            if own is not None:
                n_nodes += int(own.numel())
                _check_nodes(n_nodes, i, len(grid))
                nodes.append(own)
        clock.lap("per-tile passes")
    ids, succ, lab, other, sflags = (torch.cat([p[k] for p in parts]) for k in range(5))
    del parts
    table = _join(ids, succ, lab, other, sflags)
    del ids, succ, lab, other, sflags
    clock.lap("sort + join")
    return table


_TRACE_STAGE = {"head rounds": "rounds", "rank rounds": "rounds"}


def trace_labels(source, n_labels: int, tile=4096, stats: Optional[dict] = None, device="cuda:0") -> Tuple["rag.Polygons", "rag.Arcs"]:
    """A scene's label raster traced into polygon rings and boundary arcs across tile seams: array for array and bit for bit what
    `rag._trace(L, n_labels)` returns on the whole raster L, in scene coordinates, whatever the tile size.

    source: int32 [H, W] with ids 0..n_labels-1 -- a numpy array, an `np.memmap`, a CPU tensor, or anything with `.shape == (H, W)`
    and `.read(y0, y1, x0, x1) -> int32 [y1-y0, x1-x0]`; it is read window by window and never modified.  tile: core side, an int
    or (th, tw).  stats: a dict that receives the darts, rings, arcs, rounds and seconds per stage (synchronises at stage
    boundaries).  Limits, each a ValueError: H, W < 2^31 - 1 and H W <= 2^60; every window (core + 1 pixel) at most 2^28 pixels;
    ids outside 0..n_labels-1 (-1 included) name their tile; fewer than 2^31 darts in the scene.
    Memory: one window's rasters at a time; 25 bytes per dart of the scene while the tiles stream."""
    polys, arcs, _, _, _, _, info, n_tiles = _scene_tables(source, n_labels, tile, device, stats, with_nodes=False)
    if stats is not None:
        stats.update(D=info["D"], rings=info["R"], arcs=info["A"], vertices=info["V"], arc_vertices=int(info["arc_xy"].shape[0]),
                     head_rounds=info["head_rounds"], rank_rounds=info["rank_rounds"], tiles=n_tiles)
    return polys, arcs


# ---- shared-boundary Douglas-Peucker across tile seams (csrc/dm_scene_simplify.hip) -------------------------------
MAX_NODES = 1 << 31                   # positions in the sorted node lists are counted in int32 ranges per run
MAX_ARC_EXTENT = rag.MAX_SIMPLIFY_SIDE        # DM_SIMPLIFY_MAX_SIDE: an arc's bounding box, so that every |cross| stays below 2^31


def _check_nodes(total: int, i: int, n_tiles: int):
    if total >= MAX_NODES:
        raise ValueError(f"the scene has 2^31 nodes or more ({total} after tile {i} of {n_tiles}): simplify a coarser partition or the "
                         f"scene in parts")


def _tile_nodes(window: torch.Tensor, box: Core, origin: Tuple[int, int], H: int, W: int) -> Optional[torch.Tensor]:
    """The node records of one tile (dm_scene_simplify_node_count / node_emit): int64 [N], the scene corner ids y (W + 1) + x of the
    nodes among the corners the core owns, in no particular order; None when it owns none.  Arguments as `_tile_darts` takes them."""
    rag._need_cuda(window)
    lib, dev, i32 = _lib.lib(), window.device, torch.int32
    window = window.contiguous()
    wh, ww = window.shape
    blocks = ((wh + 64) // 64) * ((ww + 64) // 64)                # 64 x 64 blocks of the (wh + 1) x (ww + 1) corners
    tile_off, meta = torch.empty(blocks + 1, dtype=i32, device=dev), torch.empty(1, dtype=i32, device=dev)
    place = (window.data_ptr(), wh, ww, *box, int(origin[0]), int(origin[1]), H, W)
    check(lib.dm_scene_simplify_node_count(*place, tile_off.data_ptr(), meta.data_ptr(), _stream()), "dm_scene_simplify_node_count")
    N = int(meta[0])
    if N == 0:
        return None
    node = torch.empty(N, dtype=torch.int64, device=dev)
    check(lib.dm_scene_simplify_node_emit(*place, tile_off.data_ptr(), N, node.data_ptr(), _stream()), "dm_scene_simplify_node_emit")
    return node


def _check_arc_extents(arcs: "rag.Arcs"):
    """Every arc's bounding box at most 32768 on each side (one reduction, one readback): within a chain the rule's cross products
    are taken from the chain's first vertex and must stay below 2^31, which `rag.simplify` gets from H, W <= 32768."""
    A, Va, dev = arcs.left.numel(), arcs.xy.shape[0], arcs.xy.device
    arc_of = (torch.searchsorted(arcs.arc_ptr, torch.arange(Va, dtype=torch.int64, device=dev), right=True) - 1).clamp(0, A - 1)
    index = arc_of[:, None].expand(-1, 2)
    lo = torch.full((A, 2), (1 << 31) - 1, dtype=torch.int32, device=dev).scatter_reduce_(0, index, arcs.xy, "amin")
    hi = torch.full((A, 2), -(1 << 31), dtype=torch.int32, device=dev).scatter_reduce_(0, index, arcs.xy, "amax")
    extent = hi.long() - lo.long()
    worst = torch.argmax(extent.amax(1))
    w, h, left, right, a = torch.stack((extent[worst, 0], extent[worst, 1], arcs.left[worst].long(), arcs.right[worst].long(), worst)).tolist()
    if max(w, h) > MAX_ARC_EXTENT:
        raise ValueError(f"arc {a} between (left, right) = ({left}, {right}) spans {w} x {h} pixels: an arc's bounding box must be at most "
                         f"{MAX_ARC_EXTENT} on each side (the rule's cross products stay below 2^31); simplify the scene in parts")


MAX_TOPOLOGY_CELLS = 1 << 22          # DM_SCENE_SIMPLIFY_TOPOLOGY_MAX_CELLS: 32 bytes of counts and offsets per cell, 128 MB at the cap
MAX_TOPOLOGY_ARCS = 1 << 30           # the segment table's tag is 2 arc + skip in an int32
MAX_TOPOLOGY_ARC_VERTICES = 1 << 30   # as rag.simplify(topology=True): the refine stack is 2 Va int64


def topology_cells(H: int, W: int, cell_log2: int) -> int:
    """Cells of the topology grid of an H x W scene at cells of 2^cell_log2 corners: corner coordinates run to H and W included."""
    return ((int(H) >> cell_log2) + 1) * ((int(W) >> cell_log2) + 1)


def topology_cell_log2(H: int, W: int) -> int:
    """The cell side `simplify_labels_topology` uses, as its log2: the smallest value >= 5 (the one-raster grid's) at which the
    grid has at most MAX_TOPOLOGY_CELLS cells.  Pure arithmetic: 5 up to 65535 x 65535, 6 up to 131071 x 131071, 20 for the widest scene `trace_labels` takes."""
    log2 = 5
    while topology_cells(H, W, log2) > MAX_TOPOLOGY_CELLS:
        log2 += 1
    return log2


class _SceneTopologyRounds(rag._TopologyRounds):
    """`rag._TopologyRounds` on the scene form of its entries (csrc/dm_scene_simplify_topology.hip): the keep flags are `arc_keep`,
    one byte per stored arc vertex, and the grid's cell side is the struct's `cell_log2`.  The rounds are the base class's."""
    STRUCT, PREFIX, KEEP = _lib.DmSceneSimplifyTopology, "dm_scene_simplify_topology_", "arc_keep"

    def _cells(self, cell_log2: int) -> int:
        return topology_cells(self.H, self.W, cell_log2)

    def _arc_count(self):
        a = self.arcs
        check(self.lib.dm_scene_simplify_arc_count(a.xy.data_ptr(), a.arc_ptr.data_ptr(), self.A, self.Va, self.H, self.W, self.keep.data_ptr(),
                                                   self.count.data_ptr(), _stream()), "dm_scene_simplify_arc_count")


def _check_topology(H: int, W: int, A: int, Va: int, max_rounds: int, cell_log2: Optional[int]) -> int:
    """The limits `simplify_labels_topology` adds, each a ValueError naming its quantity, before any round; returns the cell side's log2."""
    if int(max_rounds) < 1:
        raise ValueError(f"max_rounds must be at least 1, got {max_rounds}")
    if A >= MAX_TOPOLOGY_ARCS:
        raise ValueError(f"topology=True takes fewer than 2^30 arcs, got {A}: simplify a coarser partition or the scene in parts")
    if Va > MAX_TOPOLOGY_ARC_VERTICES:
        raise ValueError(f"topology=True takes at most 2^30 arc vertices, got {Va}: simplify a coarser partition or the scene in parts")
    least = topology_cell_log2(H, W)
    if cell_log2 is None:
        return least
    if not least <= int(cell_log2) <= 24:
        raise ValueError(f"_cell_log2 must be in {least}..24 for a scene of {H} x {W} (at most 2^22 cells), got {cell_log2}")
    return int(cell_log2)


def _chain_flags(arcs: "rag.Arcs", node_row: torch.Tensor, H: int, W: int, q: int, mark=lambda stage: None):
    """The chain pass of `_simplify_tables`: (node_col, ids, arc_keep) -- the nodes by column, the corner id y (W + 1) + x of every
    stored arc vertex, and one keep byte per stored arc vertex (2 node, 1 kept by the chain pass, 0 dropped)."""
    lib, dev = _lib.lib(), arcs.xy.device
    A, Va = arcs.left.numel(), arcs.xy.shape[0]
    Nn = int(node_row.numel())
    if max(H, W) > MAX_ARC_EXTENT:                               # within 32768 x 32768 no arc can be wider
        _check_arc_extents(arcs)
    ny = torch.div(node_row, W + 1, rounding_mode="floor")
    node_col = torch.sort((node_row - ny * (W + 1)) * (H + 1) + ny).values
    ids = arcs.xy[:, 1].long() * (W + 1) + arcs.xy[:, 0].long()
    at = torch.searchsorted(node_row, ids).clamp(max=Nn - 1)
    arc_keep = ((node_row[at] == ids).to(torch.uint8) * 2).contiguous()
    del at, ny
    mark("node lists + arc_keep")
    stack = torch.empty(Va, dtype=torch.int64, device=dev)       # one entry per arc vertex: the bound of the depth-first walk
    check(lib.dm_scene_simplify_chains(arcs.xy.data_ptr(), arcs.arc_ptr.data_ptr(), A, Va, H, W, q, arc_keep.data_ptr(), stack.data_ptr(), _stream()),
          "dm_scene_simplify_chains")
    del stack
    mark("chains")
    return node_col, ids, arc_keep


def _simplify_tables(polys: "rag.Polygons", arcs: "rag.Arcs", node_row: torch.Tensor, H: int, W: int, q: int, mark=lambda stage: None,
                     stats: Optional[dict] = None, topology: bool = False, max_rounds: int = 64,
                     cell_log2: Optional[int] = None) -> Tuple["rag.Polygons", "rag.Arcs", torch.Tensor]:
    """From a scene's traced rings and arcs and its nodes (node_row int64, the corner ids y (W + 1) + x, ascending) to the simplified
    rings and arcs and `arc_keep`: the sparse form of `rag._simplify`.  Table arithmetic in torch between the
    kernels: node_col, arc_keep's 2s, the kept set, the scans.  Readbacks: the arc extents, the kept set's size, the totals.
    topology: the repair rounds of `_SceneTopologyRounds` run on arc_keep between the chain pass and the kept set (DESIGN.md 3.5.13;
    one readback per round).  A restored vertex is a stored vertex of its arc, so it is a turn of the ring or a node, and the ring
    pass, which reads only the kept set and the node lists, runs unchanged on the repaired flags."""
    lib, dev, i32, i64 = _lib.lib(), arcs.xy.device, torch.int32, torch.int64
    rag._need_cuda(arcs.xy)
    new = lambda n, dt: torch.empty(n, dtype=dt, device=dev)
    A, Va = arcs.left.numel(), arcs.xy.shape[0]
    R, V = polys.ring_label.numel(), polys.xy.shape[0]
    Nn = int(node_row.numel())
    if topology:
        cell_log2 = _check_topology(H, W, A, Va, max_rounds, cell_log2)
    node_col, ids, arc_keep = _chain_flags(arcs, node_row, H, W, q, mark)
    if topology:
        rounds = _SceneTopologyRounds(arcs, arc_keep, H, W, q, cell_log2=cell_log2)
        flagged = rounds.repair(int(max_rounds), stats is not None)
        mark("topology rounds")
    kept_row = torch.sort(torch.cat((node_row, ids[arc_keep == 1]))).values
    del ids
    mark("kept set")
    arc_count, ring_count, status = new(A, i32), new(V, i32), new(1, i32)
    check(lib.dm_scene_simplify_arc_count(arcs.xy.data_ptr(), arcs.arc_ptr.data_ptr(), A, Va, H, W, arc_keep.data_ptr(), arc_count.data_ptr(),
                                          _stream()), "dm_scene_simplify_arc_count")
    mark("arc_count")
    vert_ring = (torch.searchsorted(polys.ring_ptr, torch.arange(V, dtype=i64, device=dev), right=True) - 1).to(i32)
    t = _lib.DmSceneSimplifyRings()
    for name, tensor in (("xy", polys.xy), ("ring_ptr", polys.ring_ptr), ("vert_ring", vert_ring), ("node_row", node_row), ("node_col", node_col),
                         ("kept_row", kept_row), ("status", status)):
        setattr(t, name, tensor.data_ptr())
    t.n_nodes, t.n_kept, t.scene_h, t.scene_w, t.V, t.R = Nn, int(kept_row.numel()), H, W, V, R
    check(lib.dm_scene_simplify_ring_count(ctypes.byref(t), ring_count.data_ptr(), _stream()), "dm_scene_simplify_ring_count")
    mark("ring_count")
    arc_ptr, scan = torch.zeros(A + 1, dtype=i64, device=dev), torch.zeros(V + 1, dtype=i64, device=dev)
    torch.cumsum(arc_count, 0, dtype=i64, out=arc_ptr[1:])
    torch.cumsum(ring_count, 0, dtype=i64, out=scan[1:])
    ring_ptr = scan[polys.ring_ptr]
    Van, Vn, unsorted = (int(v) for v in torch.stack((arc_ptr[-1], scan[-1], status[0].long())).tolist())       # the vertex totals
    if unsorted:
        raise RuntimeError("dm_scene_simplify_ring_count: the node lists are not sorted")
    mark("scans + readback of the totals")
    arc_xy, xy, area2 = new((Van, 2), i32), new((Vn, 2), i32), new(R, i64)
    check(lib.dm_scene_simplify_arc_emit(arcs.xy.data_ptr(), arcs.arc_ptr.data_ptr(), arc_ptr.data_ptr(), A, Va, Van, H, W, arc_keep.data_ptr(),
                                         arc_xy.data_ptr(), _stream()), "dm_scene_simplify_arc_emit")
    mark("arc_emit")
    check(lib.dm_scene_simplify_ring_emit(ctypes.byref(t), scan.data_ptr(), ring_ptr.data_ptr(), Vn, xy.data_ptr(), area2.data_ptr(), _stream()),
          "dm_scene_simplify_ring_emit")
    mark("ring_emit + area")
    out_polys = rag.Polygons(region_ptr=polys.region_ptr, ring_ptr=ring_ptr, xy=xy, ring_label=polys.ring_label, ring_area2=area2)
    out_arcs = rag.Arcs(arc_ptr=arc_ptr, xy=arc_xy, left=arcs.left, right=arcs.right)
    if stats is not None:
        stats.update(q=q, nodes=Nn, kept=int(kept_row.numel()), arcs=A, rings=R, arc_vertices=Va, vertices=V, kept_arc_vertices=Van,
                     kept_vertices=Vn, longest_arc=int((arcs.arc_ptr[1:] - arcs.arc_ptr[:-1]).max()))
        if topology:
            stats.update(topology_rounds=len(flagged) - 1, topology_flagged=flagged, topology_stage_ms=rounds.stage_ms,
                         topology_segments=rounds.n_segments, topology_cell_entries=rounds.cell_entries, topology_cell_log2=cell_log2)
    return out_polys, out_arcs, arc_keep


def _scene_tables(source, n_labels: int, tile, device, stats: Optional[dict], with_nodes: bool = True):
    """What `trace_labels`, `simplify_labels` and `simplify_conflicts` share: one stream of the scene into its traced rings and arcs
    and (with_nodes) its sorted node list.  Returns (polys, arcs, node_row, H, W, clock, info, number of tiles)."""
    source = _as_source(source)
    H, W, S, grid = _check_trace(source, n_labels, tile)
    dev = torch.device(device)
    clock = _Clock(None if stats is None else stats.setdefault("stage_s", {}), dev)
    nodes: Optional[List[torch.Tensor]] = [] if with_nodes else None
    table = _scene_table(source, grid, S, dev, clock, nodes)
    polys, arcs, info = rag._trace_table(*table, W, S, mark=lambda stage: clock.lap(_TRACE_STAGE.get(stage, "emit")), wide=True)
    del table
    node_row = torch.sort(torch.cat(nodes)).values if with_nodes else None
    del nodes
    return polys, arcs, node_row, H, W, clock, info, len(grid)


def _simplify_scene(source, n_labels: int, tolerance: float, tile, stats: Optional[dict], device, topology: bool, max_rounds: int = 64,
                    cell_log2: Optional[int] = None) -> Tuple["rag.Polygons", "rag.Arcs"]:
    """`simplify_labels` (topology=False) and `simplify_labels_topology` (topology=True): one tile stream, one `_simplify_tables`."""
    q = rag._quantise_tolerance(tolerance)
    if topology and int(max_rounds) < 1:
        raise ValueError(f"max_rounds must be at least 1, got {max_rounds}")
    polys, arcs, node_row, H, W, clock, info, n_tiles = _scene_tables(source, n_labels, tile, device, stats)
    sizes = None if stats is None else {}
    out_polys, out_arcs, _ = _simplify_tables(polys, arcs, node_row, H, W, q, mark=lambda stage: clock.lap("simplify: " + stage), stats=sizes,
                                              topology=topology, max_rounds=max_rounds, cell_log2=cell_log2)
    if stats is not None:
        stats.update(sizes, D=info["D"], head_rounds=info["head_rounds"], rank_rounds=info["rank_rounds"], tiles=n_tiles)
    return out_polys, out_arcs


def simplify_labels(source, n_labels: int, tolerance: float, tile=4096, stats: Optional[dict] = None,
                    device="cuda:0") -> Tuple["rag.Polygons", "rag.Arcs"]:
    """A scene's label raster traced and simplified across tile seams: array for array and bit for bit what
    `rag.simplify(L, n_labels, tolerance)` returns on the whole raster L (where `rag.simplify` takes it), in scene coordinates,
    whatever the tile size.  Shared boundaries stay shared and nodes stay put, across seams as within a tile.  Two different
    boundaries may cross or land on each other and an island may collapse, as with `rag.simplify`: `simplify_conflicts` lists where,
    `simplify_labels_topology` repairs it.

    source, n_labels, tile, device: as `trace_labels` takes them; the scene is read once, the same windows yield the darts and the
    nodes.  tolerance: pixels, finite, >= 0, at most 4096, quantised to 1/256 pixel.  stats: a dict that receives the sizes and the
    seconds per stage (synchronises at stage boundaries).  Limits, each a ValueError: every limit of `trace_labels`; the tolerance
    (checked before any device work); fewer than 2^31 nodes; every arc's bounding box at most 32768 on each side.
    Memory: what `trace_labels` holds, plus 8 bytes per node twice, 9 bytes per arc vertex (keep byte, depth-first stack) and 8 bytes
    per kept vertex; no raster of corners."""
    return _simplify_scene(source, n_labels, tolerance, tile, stats, device, topology=False)


def simplify_labels_topology(source, n_labels: int, tolerance: float, tile=4096, stats: Optional[dict] = None, device="cuda:0",
                             max_rounds: int = 64, _cell_log2: Optional[int] = None) -> Tuple["rag.Polygons", "rag.Arcs"]:
    """`simplify_labels` with its conflicts repaired: array for array and bit for bit what `rag.simplify(L, n_labels, tolerance,
    topology=True)` returns on the whole raster L, whatever the tile size (DESIGN.md 3.5.12, 3.5.13;
    csrc/dm_scene_simplify_topology.hip; spec tests/simplify_topology_ref.py).  The rule and the rounds are `rag.simplify`'s: only
    dropped vertices come back, so shared boundaries stay shared and every ring keeps a non-zero area of its traced sign; without a
    conflict the result is `simplify_labels`'s bit for bit after one detection round.  (A function of its own and not a keyword of
    `simplify_labels`, whose parameter list is pinned.)

    Arguments and limits as `simplify_labels`.  The rounds work on the byte per stored arc vertex and a grid of cells of 2^cell_log2
    corners, the smallest side >= 32 at which the grid has at most 2^22 cells (`topology_cell_log2`); the result does not depend on
    the side (`_cell_log2` forces a coarser one, for tests).  Further limits, each a ValueError before the rounds start: fewer than
    2^30 arcs, at most 2^30 arc vertices, max_rounds >= 1.  RuntimeError past `max_rounds` and when no flagged segment has a vertex
    left to restore.  One readback per round.  stats also receives `topology_rounds`, `topology_flagged` (per round; the last is 0),
    `topology_stage_ms` (per round: stage -> ms), `topology_segments`, `topology_cell_entries`, `topology_cell_log2` and the stage
    "simplify: topology rounds".  Further memory while the rounds run: per arc vertex 16 bytes of segment table, 4 of kind, 8 of
    fixed points, 16 of refine stack and 8 of cell list (4 bytes an entry, sized for two entries per arc vertex, growing when a round
    needs more); per arc 12 bytes of counts and offsets; per grid cell 32 bytes of counts, fill counters and offsets (128 MB at 2^22
    cells)."""
    return _simplify_scene(source, n_labels, tolerance, tile, stats, device, topology=True, max_rounds=max_rounds, cell_log2=_cell_log2)


def simplify_conflicts(source, n_labels: int, tolerance: float, tile=4096, device="cuda:0") -> "rag.Conflicts":
    """The segments of `simplify_labels(source, n_labels, tolerance, tile)` that break the layer's topology: a `rag.Conflicts`,
    bit-equal (`arc`, `xy`, `kind`, `n_segments`) to `rag.simplify_conflicts` on the whole raster and to
    tests/simplify_topology_ref.py, whatever the tile size.  Empty means the plain result is safe and `topology=True` would return
    it unchanged.  One detection round on the plain flags; limits as `simplify_labels_topology`."""
    q = rag._quantise_tolerance(tolerance)
    polys, arcs, node_row, H, W, _, _, _ = _scene_tables(source, n_labels, tile, device, None)
    cell_log2 = _check_topology(H, W, arcs.left.numel(), arcs.xy.shape[0], 1, None)
    _, _, arc_keep = _chain_flags(arcs, node_row, H, W, q)
    return _SceneTopologyRounds(arcs, arc_keep, H, W, q, cell_log2=cell_log2).conflicts()


# ---- SLIC superpixels across tile seams (csrc/dm_scene_slic.hip, csrc/dm_slic_pass.h) -----------------------------
MAX_SLIC_SIDE = (1 << 31) - 1         # H, W are int32 (the centres' positions too)
MAX_SLIC_CENTRES = 1 << 31            # centre ids are int32
MAX_SLIC_COMPONENTS = (1 << 31) - 1   # provisional ids are int32 in the raster, in dm_merge_round and in dm_slic_absorb_pick
MAX_SLIC_EDGES = (1 << 31) - 1        # dm_slic_absorb_pick's and dm_merge_round's E
MAX_SLIC_WEIGHT = 1 << 31             # a shared boundary's length is int32 in dm_slic_absorb_pick


def _check_scene_slic(source, tile, cell, compactness, iters, min_size, out, out_name: str, resident_bytes):
    """The limits of `slic_assign` / `slic_labels`, each a ValueError before any device work.  Returns (bands, H, W, K, min_size,
    grid, out)."""
    bands, H, W = _image_shape(source)
    if H > MAX_SLIC_SIDE or W > MAX_SLIC_SIDE:
        raise ValueError(f"the scene must have H, W < 2^31, got {H} x {W}")
    min_size = rag._slic_params(cell, compactness, iters, min_size)
    if not 1 <= min_size < 1 << 31:
        raise ValueError(f"min_size must be in 1..2^31-1, got {min_size}")
    if int(resident_bytes) < 0:
        raise ValueError(f"resident_bytes must be >= 0, got {resident_bytes}")
    cell = int(cell)
    K = ((H + cell - 1) // cell) * ((W + cell - 1) // cell)
    if K >= MAX_SLIC_CENTRES:
        raise ValueError(f"the scene's grid must have fewer than 2^31 centres, got {K} (cell = {cell}); use a larger cell")
    grid = _Grid.of(H, W, tile)
    th, tw = grid.max_window(0)                                  # the largest core
    if th * tw >= 1 << 31:
        raise ValueError(f"a core must have fewer than 2^31 pixels, got {th} x {tw}")
    return bands, H, W, K, min_size, grid, _out_raster(out, H, W, out_name)


class _Cores:
    """The scene's cores as uint8 [nb,h,w] on the device (nb = min(bands, 4): what the rule uses), for several passes: they stay on
    the device between passes while their total is within `budget` bytes, otherwise every pass reads them again from the source.
    Iterating yields (i, (y0, y1, x0, x1), core)."""

    def __init__(self, source, grid: _Grid, bands: int, budget: int, dev, clock: _Clock):
        self.source, self.tiles, self.nb, self.dev, self.clock = source, grid.cores, min(bands, 4), dev, clock
        self.resident = self.nb * grid.H * grid.W <= int(budget)
        self.held: Dict[int, torch.Tensor] = {}
        self.reads = 0

    def __iter__(self):
        for i, core in enumerate(self.tiles):
            t = self.held.get(i)
            if t is None:
                t = _read(self.source, core, torch.uint8, 3, self.dev)[:self.nb].contiguous()
                rag._need_cuda(t)
                self.reads += 1
                if self.resident:
                    self.held[i] = t
            self.clock.lap("read + copy")
            yield i, core, t


def _assigned_cores(cores: _Cores, H: int, W: int, K: int, cell: int, compactness: int, iters: int, clock: _Clock):
    """Steps 1-3 on the scene: init over every core, `iters` rounds of (assignment pass with sums over every core, one update), then
    the last pass, which yields (i, core, assigned int32 [h,w] on the device) per core; `centres` int32 [K,6] is yielded first.  No
    readback."""
    lib, dev = _lib.lib(), cores.dev
    centres = torch.empty((K, 6), dtype=torch.int32, device=dev)
    sums = torch.empty((K, 7), dtype=torch.int64, device=dev)
    place = lambda t, c: (t.data_ptr(), cores.nb, c[1] - c[0], c[3] - c[2], c[0], c[2], H, W, cell)
    for i, c, t in cores:                                        # every centre before any assignment
        check(lib.dm_scene_slic_init(*place(t, c), centres.data_ptr(), sums.data_ptr(), _stream()), "dm_scene_slic_init")
        clock.lap("assignment passes")
    for _ in range(iters):
        for i, c, t in cores:
            check(lib.dm_scene_slic_pass(*place(t, c), compactness, centres.data_ptr(), sums.data_ptr(), None, _stream()), "dm_scene_slic_pass")
            clock.lap("assignment passes")
        check(lib.dm_scene_slic_update(K, centres.data_ptr(), sums.data_ptr(), _stream()), "dm_scene_slic_update")
    yield centres
    for i, c, t in cores:
        assigned = torch.empty((c[1] - c[0], c[3] - c[2]), dtype=torch.int32, device=dev)
        check(lib.dm_scene_slic_pass(*place(t, c), compactness, centres.data_ptr(), None, assigned.data_ptr(), _stream()), "dm_scene_slic_pass")
        clock.lap("assignment passes")
        yield i, c, assigned


def slic_assign(source, tile=4096, cell: int = 29, compactness: int = 10, iters: int = 10, assigned_out=None,
                resident_bytes: int = 8 << 30, device="cuda:0", stage_times: Optional[dict] = None) -> Tuple[np.ndarray, torch.Tensor]:
    """Steps 1-3 of the SLIC rule on a scene: (assigned int32 [H,W] on the host: the centre id of every pixel; centres int32 [K,6]
    on the device), both equal to `rag.slic_assign(whole scene)` whatever the tile size.  Arguments as `slic_labels` takes them;
    assigned_out: a writable int32 [H,W] array or memmap, allocated if None."""
    source = _as_source(source)
    bands, H, W, K, _, grid, out = _check_scene_slic(source, tile, cell, compactness, iters, None, assigned_out, "assigned_out", resident_bytes)
    dev = torch.device(device)
    clock = _Clock(stage_times, dev)
    stream = _assigned_cores(_Cores(source, grid, bands, resident_bytes, dev, clock), H, W, K, int(cell), int(compactness), int(iters), clock)
    centres = next(stream)
    for i, (y0, y1, x0, x1), assigned in stream:
        out[y0:y1, x0:x1] = assigned.cpu().numpy()
        clock.lap("relabel + write")
    return out, centres


def _components(assigned: torch.Tensor) -> Tuple[torch.Tensor, int, torch.Tensor]:
    """`rag.connected_labels(assigned)` and, from the same call's parent table, first int64 [n]: the linear index in the raster of
    every component's first pixel (a component's root is its first pixel; the roots in raster order are the ids in order)."""
    labels, n, parent = rag._connected_labels(assigned, None)
    first = torch.nonzero(parent == torch.arange(parent.numel(), dtype=torch.int32, device=parent.device)).view(-1)
    return labels, n, first


def _fold_graph(mapping: torch.Tensor, n_new: int, area: torch.Tensor, edges: torch.Tensor, weights: torch.Tensor):
    """The graph under a union: mapping int64 [n] -> 0..n_new-1; areas add, the edge keys are mapped, self edges dropped and the
    weights of equal keys added.  area int64, edges int64 [E,2], weights int64 [E]; returns the same three, edges sorted by (a, b)."""
    dev = mapping.device
    area = torch.zeros(n_new, dtype=torch.int64, device=dev).index_add_(0, mapping, area)
    a, b = mapping[edges[:, 0]], mapping[edges[:, 1]]
    keep = a != b
    a, b, weights = a[keep], b[keep], weights[keep]
    uniq, inverse = torch.unique(torch.minimum(a, b) * n_new + torch.maximum(a, b), return_inverse=True)
    weights = torch.zeros(uniq.numel(), dtype=torch.int64, device=dev).index_add_(0, inverse, weights)
    if uniq.numel() > MAX_SLIC_EDGES:
        raise ValueError(f"the component graph has 2^31 edges or more ({uniq.numel()}): edge counts are 32-bit")
    if weights.numel() and int(weights.max()) >= MAX_SLIC_WEIGHT:
        raise ValueError(f"two regions share a boundary of 2^31 pixel edges or more ({int(weights.max())}): weights are 32-bit")
    return area, torch.stack((uniq // n_new, uniq % n_new), 1), weights


def slic_labels(source, tile=4096, cell: int = 29, compactness: int = 10, iters: int = 10, min_size: Optional[int] = None,
                labels_out=None, resident_bytes: int = 8 << 30, device="cuda:0", stage_times: Optional[dict] = None,
                stats: Optional[dict] = None) -> Tuple[np.ndarray, int]:
    """SLIC superpixels of a scene larger than one tile, regions crossing the tile seams: (labels int32 [H,W] on the host, n_labels),
    equal to `rag.slic(whole scene, cell, compactness, iters, min_size)` bit for bit, whatever the tile size -- the raster
    `segment_labels` takes (`segment_scene(..., cross_seams=True)` chains the two).

    source: what `segment_scene` takes: uint8 [bands,H,W] as an array, an `np.memmap`, a CPU tensor, or anything with `.shape` and
    `.read(y0, y1, x0, x1)`; tile: core side, an int or (th, tw); cell, compactness, iters, min_size: as `rag.slic` takes them;
    labels_out: a writable int32 [H,W] array or memmap, allocated if None; resident_bytes: a budget -- the cores (uint8, the first
    four bands) stay on the device between the passes while their total is within it, otherwise every pass reads them again from
    the source (the image is read once, or iters + 2 times); the result does not depend on it; stage_times: seconds per stage
    (synchronises at stage boundaries); stats: receives `provisional` (tile-local components), `seam_unions` (distinct pairs united
    across seams), `components` (step 4's count), `rounds` (absorption rounds), `picks` (picked edges per round), `image_reads`.

    One scene-wide table of centres; per round an assignment pass over every core and one update; in the last pass per core the
    assigned raster, its tile-local components with provisional ids, their first pixels, areas, edges and border lines; then on
    the component graph only: unions across seams where both sides hold the same centre id, numbering by scene-wide first pixel,
    the absorption rounds on folded areas and edges; one relabel pass applies the composed mapping.
    Limits, each a ValueError: H, W < 2^31; fewer than 2^31 centres; a core below 2^31 pixels, with at most 2^25 components
    (`rag.rag_edges`' table of 32 slots per component ends at 2^30); fewer than 2^31 provisional components and fewer than 2^31
    graph edges in the scene; a shared boundary below 2^31 pixel edges.  Areas are folded in 64 bits."""
    source = _as_source(source)
    bands, H, W, K, min_size, grid, out = _check_scene_slic(source, tile, cell, compactness, iters, min_size, labels_out, "labels_out",
                                                            resident_bytes)
    dev, i32, i64, tiles = torch.device(device), torch.int32, torch.int64, grid.cores
    clock = _Clock(stage_times, dev)
    cores = _Cores(source, grid, bands, resident_bytes, dev, clock)
    stream = _assigned_cores(cores, H, W, K, int(cell), int(compactness), int(iters), clock)
    next(stream)                                                 # the centres: not needed here
    base, first_parts, area_parts, edge_parts, weight_parts, strips = 0, [], [], [], [], []
    for i, (y0, y1, x0, x1), assigned in stream:
        comp, n, first = _components(assigned)
        if base + n > MAX_SLIC_COMPONENTS:
            raise ValueError(f"the scene has 2^31 tile-local components or more ({base + n} after tile {i} of {len(tiles)}): ids are "
                             f"32-bit; use fewer, larger tiles or segment the scene in parts")
        w = x1 - x0
        first_parts.append((torch.div(first, w, rounding_mode="floor") + y0) * W + (first % w + x0))       # scene-wide, 64-bit
        area_parts.append(rag.label_area(comp, n).long())
        e, wgt = rag.rag_edges(comp, n)
        edge_parts.append(e.long() + base)
        weight_parts.append(wgt.long())
        prov = comp + base
        strips.append((_border(assigned), _border(prov)))
        base += n
        clock.lap("components + graph")
        out[y0:y1, x0:x1] = prov.cpu().numpy()
        clock.lap("relabel + write")
    P = base
    # seams: equal centre ids on both sides unite the two provisional components; different ones are an edge of the graph
    (ca, cb), (pa, pb) = _seam_pairs(strips, grid.nx, grid.ny, dev)
    same = ca == cb
    pairs = torch.unique(pa[same].long() * P + pb[same].long())
    if pairs.numel():
        united = torch.stack((pairs // P, pairs % P), 1).to(i32).contiguous()
        root = rag.merge_components(united, torch.ones(united.shape[0], dtype=torch.uint8, device=dev), P).long()
    else:
        root = torch.arange(P, dtype=i64, device=dev)
    # (counted here, not by rag.seam_stitch: its ids end at 2^24, and a scene has more fragments than that before the absorption;
    #  the seam positions are a perimeter, not an area)
    da, db = pa[~same].long(), pb[~same].long()
    seam_keys, seam_weights = torch.unique(torch.minimum(da, db) * P + torch.maximum(da, db), return_counts=True)
    seam_edges = torch.stack((seam_keys // P, seam_keys % P), 1)
    # numbering: a component is a union's root, its first pixel the minimum over its members
    first = torch.full((P,), (1 << 63) - 1, dtype=i64, device=dev).scatter_reduce_(0, root, torch.cat(first_parts), "amin")
    roots = torch.nonzero(root == torch.arange(P, dtype=i64, device=dev)).view(-1)
    n = int(roots.numel())
    rank = torch.empty(P, dtype=i64, device=dev)
    rank[roots[torch.argsort(first[roots])]] = torch.arange(n, dtype=i64, device=dev)
    mapping = rank[root]                                         # provisional id -> component, composed with every round below
    area, edges, weights = _fold_graph(mapping, n, torch.cat(area_parts), torch.cat(edge_parts + [seam_edges]),
                                       torch.cat(weight_parts + [seam_weights]))
    components = n
    clock.lap("seams")
    # absorption on the graph only: the rounds of rag.absorb_small, the raster untouched
    picks = []
    while n > 1:                                                 # (`< min_size` survives the clamp of the 64-bit areas)
        got = rag._absorb_round(edges.to(i32).contiguous(), weights.to(i32), area.clamp(max=(1 << 31) - 1).to(i32), n, min_size)
        if got is None:
            break
        step, n, picked = got
        picks.append(picked)
        area, edges, weights = _fold_graph(step, n, area, edges, weights)
        mapping = step[mapping]
    clock.lap("absorption rounds")
    # one relabel pass over the provisional raster
    mapping = mapping.to(i32).contiguous()
    for y0, y1, x0, x1 in tiles:
        prov = torch.from_numpy(np.ascontiguousarray(out[y0:y1, x0:x1])).to(dev)
        clock.lap("read + copy")
        out[y0:y1, x0:x1] = rag.relabel_raster(prov, mapping).cpu().numpy()
        clock.lap("relabel + write")
    if stats is not None:
        stats.update(provisional=P, seam_unions=int(pairs.numel()), components=components, rounds=len(picks), picks=picks,
                     image_reads=cores.reads // len(tiles), resident=cores.resident, tiles=len(tiles), n_labels=n)
    return out, n


# ---- polygon rings as a scene's label source (csrc/dm_scene_rasterize.hip) ----------------------------------------
MAX_WINDOW_PIXELS = 1 << 31           # a window's raster is indexed in int32, as every raster pass here


class RingSource:
    """Polygon rings as the label raster of an H x W scene that is never built: `.shape == (H, W)` and `.read(y0, y1, x0, x1)`,
    so it goes wherever a scene call takes a label or truth source (`segment_scene(labels=)`, `label_graph`, `sample_points`,
    `trace_labels`, `simplify_labels*`, `SceneResult.overlap`).

    rings: a `rag.Rings` (float64, quantised once, here) or a `rag.Polygons` (int32 corners; what `trace_labels` returns), in
    scene coordinates.  `read` returns the int32 device tensor [y1-y0, x1-x0] that is rows y0..y1-1, columns x0..x1-1 of
    `rag.rasterize(rings, H, W, fill)`, bit for bit, also where H W >= 2^31 and that raster cannot exist (the rule in its band
    and window form: include/deepmerge_hip.h, tests/scene_rasterize_ref.py).  `n_labels` is the largest label + 1.

    The constructor makes `rag.rasterize`'s checks with its messages (one readback) and keeps the quantised vertices on the
    device; the inputs are not modified.  A read counts, scans, emits and sorts the events of the band of rows [y0, y1) -- all V
    edges are visited per band -- and fills the window from the band's sorted keys; the keys of the LAST band are kept, so the
    scene loops, which are row-major and whose windows' rows depend on the tile row only, pay one event pass per row of tiles and
    one fill per tile.  Readbacks per read: the band's event count (a new band only) and the error flag.
    Limits, each a ValueError: coordinates within +-2^20 pixels; H, W < 2^31; a window below 2^31 pixels; at most 2^30 events per
    band; (largest label + 1) (y1 - y0) (W + 1) < 2^63.  Rings that are not closed in a band raise RuntimeError for every box of
    that band."""

    def __init__(self, rings, H: int, W: int, fill: int = -1, device="cuda:0"):
        dev = torch.device(device)
        moved = rag.Rings(rings.ring_ptr.to(dev), rings.xy.to(dev), rings.ring_label.to(dev))
        self.ring_ptr, xy, self.ring_label, self.R, self.V = rag._ring_tensors(moved)
        H, W, fill = int(H), int(W), int(fill)
        if H < 1 or W < 1 or H >= 1 << 31 or W >= 1 << 31:
            raise ValueError(f"need 1 <= H, W < 2^31, got {H} x {W}")
        if not -(1 << 31) <= fill < 0:
            raise ValueError(f"fill must be a negative int32, got {fill}")
        if self.V > rag.MAX_EVENTS:
            raise ValueError(f"rasterize takes at most 2^30 vertices, got {self.V}")
        self.n_labels = rag._check_ring_values(self.ring_ptr, xy, self.ring_label, self.R, self.V)
        self.shape, self.fill, self.device = (H, W), fill, dev
        self.q, self.vert_ring = rag._quantised(self.ring_ptr, xy, self.V) if self.R and self.V else (None, None)
        self._band, self._keys = None, None
        self.events: Dict[Tuple[int, int], int] = {}             # band -> its event count, for every band passed so far
        self.clock = _Clock(None, dev)                           # `rasterize_rings(stats=)` puts its own here

    def _event_pass(self, y0: int, y1: int) -> Optional[torch.Tensor]:
        """The sorted keys of the band [y0, y1), None when it has no event."""
        H, W = self.shape
        if self.n_labels * (y1 - y0) * (W + 1) >= 1 << 63:
            raise ValueError(f"(largest label + 1) * rows * (W + 1) must be below 2^63, got {self.n_labels} * {y1 - y0} * {W + 1}")
        N = 0
        if self.q is not None:
            lib, V, R = _lib.lib(), self.V, self.R
            count = torch.empty(V, dtype=torch.int32, device=self.device)
            check(lib.dm_rasterize_count_rows(self.q.data_ptr(), self.ring_ptr.data_ptr(), self.vert_ring.data_ptr(), V, R, H, W, y0, y1,
                                              count.data_ptr(), _stream()), "dm_rasterize_count_rows")
            scan = torch.zeros(V + 1, dtype=torch.int64, device=self.device)
            torch.cumsum(count, 0, dtype=torch.int64, out=scan[1:])
            N = int(scan[-1])
            self.clock.lap("count + scan")
        self.events[(y0, y1)] = N
        if N > rag.MAX_EVENTS:
            raise ValueError(f"the rings cross {N} pixel-row centres in rows {y0}..{y1 - 1}; a band takes at most 2^30: use a lower tile")
        if N == 0:
            return None
        keys = torch.empty(N, dtype=torch.int64, device=self.device)
        check(lib.dm_rasterize_emit_rows(self.q.data_ptr(), self.ring_ptr.data_ptr(), self.vert_ring.data_ptr(), self.ring_label.data_ptr(),
                                         scan.data_ptr(), V, R, N, H, W, y0, y1, self.n_labels, keys.data_ptr(), _stream()),
              "dm_rasterize_emit_rows")
        self.clock.lap("emit")
        keys = torch.sort(keys).values
        self.clock.lap("sort")
        return keys

    def read(self, y0: int, y1: int, x0: int, x1: int) -> torch.Tensor:
        H, W = self.shape
        y0, y1, x0, x1 = int(y0), int(y1), int(x0), int(x1)
        if not (0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W):
            raise ValueError(f"the box must lie inside the scene: rows {y0}..{y1}, columns {x0}..{x1} of {H} x {W}")
        if (y1 - y0) * (x1 - x0) >= MAX_WINDOW_PIXELS:
            raise ValueError(f"a window must have fewer than 2^31 pixels, got {y1 - y0} x {x1 - x0}")
        with torch.cuda.device(self.device):
            if self._band != (y0, y1):
                self._band, self._keys = None, None              # (a pass that raises leaves no band behind)
                self._keys = self._event_pass(y0, y1)
                self._band = (y0, y1)
            if self._keys is None:
                return torch.full((y1 - y0, x1 - x0), self.fill, dtype=torch.int32, device=self.device)
            out = torch.empty((y1 - y0, x1 - x0), dtype=torch.int32, device=self.device)
            error = torch.empty(1, dtype=torch.int32, device=self.device)
            check(_lib.lib().dm_rasterize_fill_window(self._keys.data_ptr(), int(self._keys.numel()), H, W, y0, y1, x0, x1, self.fill,
                                                      out.data_ptr(), error.data_ptr(), _stream()), "dm_rasterize_fill_window")
            if int(error):
                raise RuntimeError(f"rasterize: a pair of sorted events of rows {y0}..{y1 - 1} disagrees in (label, row): the rings are "
                                   f"not closed (an odd number of crossings in a row)")
            self.clock.lap("pre-set + fill")
        return out


def rasterize_rings(rings, H: int, W: int, tile=4096, fill: int = -1, labels_out=None, stats: Optional[dict] = None,
                    device="cuda:0") -> np.ndarray:
    """`rag.rasterize(rings, H, W, fill)` of a scene on the host, tile by tile: int32 [H,W], equal to the whole-raster call bit for
    bit, whatever the tile size, and defined for H W >= 2^31 too.  rings: a `rag.Rings` or a `rag.Polygons` (or a `RingSource` of
    H x W, whose own fill and device then hold); tile: an int or
    (th, tw), a tile below 2^31 pixels; labels_out: a writable int32 [H,W] array or memmap, allocated if None; stats: receives the
    seconds per stage (synchronises at stage boundaries), `events` (band -> event count) and `tiles`.  One event pass per row of
    tiles, one fill per tile (`RingSource`); limits and errors as there."""
    source = rings if isinstance(rings, RingSource) else RingSource(rings, H, W, fill, device)
    if source.shape != (int(H), int(W)):
        raise ValueError(f"the source has {source.shape[0]} x {source.shape[1]} pixels, not {H} x {W}")
    H, W = source.shape
    grid = _Grid.of(H, W, tile)
    side_y, side_x = grid.max_window(0)
    if side_y * side_x >= MAX_WINDOW_PIXELS:
        raise ValueError(f"a tile must have fewer than 2^31 pixels, got {side_y} x {side_x}")
    out = _out_raster(labels_out, H, W, "labels_out")
    before, source.clock = source.clock, _Clock(stats, source.device)
    try:
        for y0, y1, x0, x1 in grid.cores:
            out[y0:y1, x0:x1] = source.read(y0, y1, x0, x1).cpu().numpy()
            source.clock.lap("copy + write")
    finally:
        source.clock = before
    if stats is not None:
        stats.update(events=dict(source.events), tiles=len(grid), vertices=source.V, rings=source.R)
    return out


def labels_from_shapefile(path: str, H: int, W: int, geotransform=None, label_field: Optional[str] = None, fill: int = -1, tile=4096,
                          labels_out=None, device="cuda:0", as_source: bool = False):
    """`rag.labels_from_shapefile` on a scene: (labels int32 [H,W] on the host, n_labels) from a polygon shapefile, through
    `shpstore._read_rings` and `rasterize_rings`.  Record i is label i (n_labels = the record count), or the value of the integer
    field `label_field` (n_labels = the largest + 1); geotransform: the six GDAL terms of the scene (None: X = x, Y = -y).
    as_source=True: no host raster; the `RingSource` stands in its place, (source, n_labels), for the scene calls to read."""
    from . import shpstore
    ring_ptr, xy, ring_label, n_labels = shpstore._read_rings(path, geotransform, label_field)
    source = RingSource(rag.Rings(*(torch.from_numpy(a) for a in (ring_ptr, xy, ring_label))), H, W, fill, device)
    if as_source:
        return source, n_labels
    return rasterize_rings(source, H, W, tile=tile, labels_out=labels_out), n_labels


# ---- boundary recall / precision / F of a scene (csrc/dm_boundary.hip) ---------------------------------------------
def boundary_scores(labels_source, truth_source, n_labels: int, n_truth: int, tolerance=2, tile=4096,
                    mapping: Optional[torch.Tensor] = None, device="cuda:0", stage_times: Optional[dict] = None):
    """`rag.boundary_scores` on a scene: the four counts, and so every figure, equal the whole-raster call's on the assembled
    rasters, whatever the tile size (the rule: include/deepmerge_hip.h).

    labels_source, truth_source: int32 [H,W] on the host -- an array, an `np.memmap`, a CPU tensor, or anything with `.shape ==
    (H, W)` and `.read(y0, y1, x0, x1) -> int32 [y1-y0, x1-x0]`, a `RingSource` included: a truth `polygons.shp` is scored with no
    host raster.  tolerance: an integer, or a list or tuple of them (a list is returned); mapping int32 [n_labels] on the device:
    as in `rag.boundary_scores`.  Every core is read with a halo of max(tolerance) + 1 pixels: the tolerance for the match, and
    one more so that every pixel within the tolerance of the core has its right and lower neighbour in the window; the bits of
    both windows are made once, the counts are taken on the core's box for every tolerance and added over the cores on the
    device.  One readback (the counts).  Limits, each a ValueError before any device work: H, W < 2^31; tolerance in 0..64; every
    window below 2^31 pixels."""
    labels_source, truth_source = _as_source(labels_source), _as_source(truth_source)
    H, W = _label_shape(labels_source, "labels_source")
    if _label_shape(truth_source, "truth_source") != (H, W):
        raise ValueError(f"truth_source must cover the scene: its shape is {tuple(truth_source.shape)}, the labels have {H} x {W} pixels")
    if H > MAX_SCENE_SIDE or W > MAX_SCENE_SIDE:
        raise ValueError(f"the scene must have H, W < 2^31, got {H} x {W}")
    if not 1 <= int(n_labels) < 1 << 31 or not 1 <= int(n_truth) < 1 << 31:
        raise ValueError(f"n_labels and n_truth must be in 1..2^31-1, got {n_labels}, {n_truth}")
    ds, single = rag._tolerances(tolerance)
    rag._check_mapping(mapping, n_labels)
    grid, halo = _Grid.of(H, W, tile), max(ds) + 1
    side_y, side_x = grid.max_window(halo)
    if side_y * side_x >= MAX_WINDOW_PIXELS:
        raise ValueError(f"a tile's window (core + halo of {halo}) must have fewer than 2^31 pixels, got {side_y} x {side_x}")
    dev, i32 = torch.device(device), torch.int32
    if mapping is not None:
        mapping = mapping.to(dev).contiguous()
    clock = _Clock(stage_times, dev)
    counts = torch.zeros((len(ds), 4), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        for (_, _, lab, box, _), (_, _, tru, _, _) in zip(_windows(labels_source, grid, halo, i32, 2, dev, clock),
                                                          _windows(truth_source, grid, halo, i32, 2, dev, clock)):
            wh, ww = lab.shape
            label_edge, _ = rag.boundary_bits(lab.contiguous(), n_labels, mapping)
            truth_edge, truth_valid = rag.boundary_bits(tru.contiguous(), n_truth, valid=True)
            clock.lap("bits")
            rag.boundary_counts(label_edge, truth_edge, truth_valid, wh, ww, ds, box, counts)
            clock.lap("counts")
        out = [rag.boundary_scores_of(d, c) for d, c in zip(ds, counts.tolist())]     # the one readback
    clock.lap("readback")
    return out[0] if single else out
