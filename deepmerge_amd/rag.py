"""Region-adjacency graph and designed features from a label raster, on the device.

The reference consumes a RAG edge list and 15 per-superpixel attributes that external GIS software wrote into
shapefiles (`lines.shp` LEFT_FID / RIGHT_FID, MyUtils2.py:155-193; attribute order MyUtils1.py:79-114).  This module
derives both from the segmentation's label raster and the image tile with three HIP kernels (csrc/dm_rag.hip), which
makes the ExtractFeatures pipeline self-contained on the GPU.  Definitions: oracle/rag.py (the build's own spec).
The sample points, their `inner` / `object` window fields and point lists, which the reference reads from a point shapefile,
come from the label raster as well (csrc/dm_points.hip: `clearance`, `sample_points`; spec tests/points_ref.py).
Against a ground-truth raster, `label_overlap` counts the overlap table once; `pair_flags` labels the RAG edges for training and
`Overlap.coarsen(...).scores()` scores any merged partition (csrc/dm_truth.hip; spec tests/truth_ref.py).
`boundary_scores` adds what region scores hide: boundary recall, precision and F at a pixel tolerance, from one bit per pixel
(csrc/dm_boundary.hip; spec tests/boundary_ref.py).
`polygons` and `boundary_arcs` trace a label raster into closed rings and boundary arcs, the geometry of the reference's polygon
layer and `lines.shp` (csrc/dm_vector.hip; spec tests/vector_ref.py); deepmerge_amd/shpstore.py writes them as shapefiles.
`rasterize` is the way back, for any polygon: rings to a label raster (csrc/dm_rasterize.hip; spec tests/rasterize_ref.py), and
`labels_from_shapefile` reads the rings from a polygon shapefile, the form the reference's users have their data in.
`simplify` is Douglas-Peucker on the traced geometry, once per shared boundary, so neighbours keep sharing every vertex
(csrc/dm_simplify.hip; spec tests/simplify_ref.py); `simplify_conflicts` finds where that breaks a polygon and `simplify(topology=True)`
repairs it (csrc/dm_simplify_topology.hip; spec tests/simplify_topology_ref.py).
`mrs` is multiresolution segmentation, the classical baseline of the learned merge and a second source of superpixels: the rounds of
`merge_regions` scored by the colour / shape heterogeneity cost of the regions' statistics, from single pixels or from a label raster
(csrc/dm_mrs.hip; spec tests/mrs_ref.py).
"""
from __future__ import annotations

import ctypes
import math
import operator
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from .ops import _need_cuda, _stream, check

FEATURE_NAMES = ("area", "peri", "len", "width", "smooth", "std0", "std1", "std2", "mean0", "mean1", "mean2",
                 "shapeness", "compact", "bright", "border")          # MyUtils1.py:79-114


def label_stats(labels: torch.Tensor, tile: torch.Tensor, n_labels: int) -> Dict[str, torch.Tensor]:
    """Exact integer statistics per superpixel: count, per-band sum / sum of squares (first three bands), bounding box,
    perimeter (shared with other labels / on the raster border)."""
    _need_cuda(labels, tile)
    if labels.dtype != torch.int32 or tile.dtype != torch.uint8 or tile.dim() != 3 or labels.shape != tile.shape[1:]:
        raise ValueError("labels must be int32 [H,W] and tile uint8 [bands,H,W] over the same raster")
    labels, tile = labels.contiguous(), tile.contiguous()
    bands, H, W = tile.shape
    nb, dev = min(bands, 3), labels.device
    out = {"count": torch.empty(n_labels, dtype=torch.int64, device=dev),
           "sum": torch.empty((n_labels, nb), dtype=torch.int64, device=dev),
           "sumsq": torch.empty((n_labels, nb), dtype=torch.int64, device=dev),
           "bbox": torch.empty((n_labels, 4), dtype=torch.int32, device=dev),
           "peri": torch.empty((n_labels, 2), dtype=torch.int64, device=dev)}
    check(_lib.lib().dm_label_stats(labels.data_ptr(), tile.data_ptr(), bands, H, W, n_labels, out["count"].data_ptr(),
                                    out["sum"].data_ptr(), out["sumsq"].data_ptr(), out["bbox"].data_ptr(), out["peri"].data_ptr(),
                                    _stream()), "dm_label_stats")
    out["bands"] = nb
    return out


def designed_features(stats: Dict[str, torch.Tensor]) -> torch.Tensor:
    """float32 [S,15] in the reference's attribute order (FEATURE_NAMES)."""
    S = stats["count"].numel()
    feat = torch.empty((S, 15), dtype=torch.float32, device=stats["count"].device)
    check(_lib.lib().dm_label_features(stats["count"].data_ptr(), stats["sum"].data_ptr(), stats["sumsq"].data_ptr(),
                                       stats["bbox"].data_ptr(), stats["peri"].data_ptr(), S, stats["bands"], feat.data_ptr(), _stream()),
          "dm_label_features")
    return feat


def _count_keys(dev, n_labels: int, max_out: int, what: str, noun: str, call) -> Tuple[torch.Tensor, torch.Tensor]:
    """One pass that counts 64-bit keys in a device hash table (csrc/dm_raster.h): sizes the table for at most max_out distinct
    keys (0: max(1024, 8 n_labels)), runs call(table keys, table counts, log2 of the slots, out keys, out counts, max_out, n,
    overflow) -- the eight arguments dm_rag_edges and dm_label_overlap share, as data pointers and ints -- and returns (keys int64
    [n], counts int32 [n]) sorted by key.  One readback (n, overflow)."""
    max_out = int(max_out) or max(1024, 8 * n_labels)
    log2 = max(10, (4 * max_out - 1).bit_length())               # load factor <= 1/4
    if log2 > 30:
        raise ValueError(f"max_{noun} = {max_out} needs a table of more than 2^30 slots")
    tk = torch.empty(1 << log2, dtype=torch.int64, device=dev)
    tc = torch.empty(1 << log2, dtype=torch.int32, device=dev)
    ok = torch.empty(max_out, dtype=torch.int64, device=dev)
    oc = torch.empty(max_out, dtype=torch.int32, device=dev)
    meta = torch.empty(2, dtype=torch.int32, device=dev)
    call(tk.data_ptr(), tc.data_ptr(), log2, ok.data_ptr(), oc.data_ptr(), max_out, meta.data_ptr(), meta[1:].data_ptr())
    n, overflow = (int(v) for v in meta.tolist())
    if overflow or n > max_out:
        raise RuntimeError(f"{what} has more than max_{noun}={max_out} {noun} (found {n}, table overflow={bool(overflow)}); "
                           f"pass a larger max_{noun}")
    order = torch.argsort(ok[:n])                                # canonical order; keys are unique
    return ok[:n][order], oc[:n][order]


def rag_edges(labels: torch.Tensor, n_labels: int, max_edges: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(edges int32 [E,2] with a < b, sorted by (a, b); shared boundary length int32 [E] in pixel edges).  max_edges (default
    max(1024, 8 n_labels): a planar graph has E <= 3 S - 6, and 8 S leaves room for raster artefacts) bounds the number of edges."""
    _need_cuda(labels)
    if labels.dtype != torch.int32 or labels.dim() != 2:
        raise ValueError("labels must be int32 [H,W]")
    labels = labels.contiguous()
    H, W = labels.shape
    k, w = _count_keys(labels.device, n_labels, max_edges, "RAG", "edges", lambda *table: check(
        _lib.lib().dm_rag_edges(labels.data_ptr(), H, W, n_labels, *table, _stream()), "dm_rag_edges"))
    edges = torch.stack((k // n_labels, k % n_labels), 1).to(torch.int32)
    return edges, w


def seam_stitch(a: torch.Tensor, b: torch.Tensor, n_labels: int, peri: torch.Tensor, max_edges: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """What lies between the tiles of a scene (csrc/dm_scene.hip; the rule: include/deepmerge_hip.h).

    a, b int32 [n]: the scene-wide superpixel ids of the two pixels that face each other across every seam position, all seams
    concatenated; peri int64 [n_labels,2]: `label_stats`' "peri" of every tile, concatenated.  Returns (edges int32 [E,2] with
    a < b, sorted by (a, b); shared boundary length int32 [E]) of the pairs that face each other across a seam, as `rag_edges`
    returns those inside a raster (max_edges as there), and UPDATES `peri` IN PLACE: every seam pixel edge leaves the "raster
    border" column for the column `label_stats` on the assembled scene puts it in.  n == 0 (a scene of one tile) returns empty
    tensors without a launch.  One readback, as `rag_edges`."""
    _need_cuda(a, b, peri)
    if a.dtype != torch.int32 or b.dtype != torch.int32 or a.dim() != 1 or a.shape != b.shape:
        raise ValueError("a and b must be int32 [n], one entry per seam position")
    S = int(n_labels)
    if not 1 <= S <= MAX_REGIONS:
        raise ValueError(f"n_labels must be in 1..2^24, got {n_labels}")
    if peri.dtype != torch.int64 or tuple(peri.shape) != (S, 2) or not peri.is_contiguous():
        raise ValueError(f"peri must be contiguous int64 [{S},2] (label_stats' 'peri' of every tile, concatenated)")
    if a.device != b.device or a.device != peri.device:
        raise ValueError("a, b and peri must be on one device")
    n = a.numel()
    if n == 0:
        return torch.empty((0, 2), dtype=torch.int32, device=a.device), torch.empty(0, dtype=torch.int32, device=a.device)
    a, b = a.contiguous(), b.contiguous()
    k, w = _count_keys(a.device, S, max_edges, "the seam graph", "edges", lambda *table: check(
        _lib.lib().dm_seam_stitch(a.data_ptr(), b.data_ptr(), n, S, peri.data_ptr(), *table, _stream()), "dm_seam_stitch"))
    edges = torch.stack((k // S, k % S), 1).to(torch.int32)
    return edges, w


def points_to_csr(labels: torch.Tensor, xy: torch.Tensor, n_labels: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """CSR membership (ptr int32 [S+1], idx int32 [P]) of sample points (x, y) in superpixels, the form
    rag_similarity_sweep consumes (the reference's space-separated `PointID` strings, ExtractFeatures.py:175-179).
    Points keep their order inside a superpixel."""
    lab = labels[xy[:, 1].long(), xy[:, 0].long()].long()
    order = torch.argsort(lab, stable=True)
    counts = torch.bincount(lab, minlength=n_labels)
    ptr = torch.zeros(n_labels + 1, dtype=torch.int64, device=labels.device)
    ptr[1:] = torch.cumsum(counts, 0)
    return ptr.to(torch.int32), order.to(torch.int32)


def merge_components(edges: torch.Tensor, merge: torch.Tensor, n_labels: int, max_rounds: int = 64) -> torch.Tensor:
    """Connected components of the superpixel graph restricted to the edges flagged `merge` (the step after the sweep; the
    reference hands this to external GIS tooling).  Returns int32 [S]: the smallest superpixel id of each one's component."""
    _need_cuda(edges, merge)
    edges = edges.to(torch.int32).contiguous()
    m8 = merge.to(torch.uint8).contiguous()
    if edges.numel() and int(edges.max()) >= n_labels:
        raise ValueError(f"merge_components: edge endpoint {int(edges.max())} >= n_labels {n_labels}")
    if edges.numel() and bool(((edges < 0).any(1) & (m8 != 0)).any()):
        raise ValueError("merge_components: an edge with a -1 ('no polygon') endpoint is flagged for merging")
    dev = edges.device
    parent = torch.empty(n_labels, dtype=torch.int32, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    for r in range(max_rounds):
        check(_lib.lib().dm_merge_round(edges.data_ptr(), m8.data_ptr(), edges.shape[0], n_labels, parent.data_ptr(), changed.data_ptr(),
                                        int(r == 0), _stream()), "dm_merge_round")
        if int(changed.item()) == 0:
            return parent
    raise RuntimeError(f"merge_components did not converge in {max_rounds} rounds")


def merge_partition(ptr: torch.Tensor, idx: torch.Tensor, edges: torch.Tensor, root: torch.Tensor):
    """Apply a component labelling: merged CSR point lists (members in ascending old id, their points in the old order) and
    the edge list between the merged regions (self edges dropped, duplicates folded, sorted).
    Returns (new_id int32 [S] dense 0..C-1 in order of the component's smallest member, ptr', idx', edges')."""
    S = root.numel()
    root = root.long()
    is_root = root == torch.arange(S, device=root.device)
    dense = torch.cumsum(is_root.to(torch.int64), 0) - 1               # id of a root among the roots
    new_id = dense[root]
    C = int(is_root.sum())
    counts = (ptr[1:] - ptr[:-1]).long()
    owner = torch.repeat_interleave(new_id, counts)                    # new region of every entry of idx (old CSR order)
    order = torch.argsort(owner, stable=True)
    new_idx = idx.long()[order].to(torch.int32)
    new_ptr = torch.zeros(C + 1, dtype=torch.int64, device=root.device)
    new_ptr[1:] = torch.cumsum(torch.bincount(owner, minlength=C), 0)
    live = (edges >= 0).all(1)                                         # -1 = "no polygon" (MyUtils2.py:184-186): never relabelled
    edges = edges[live]
    if edges.numel() and int(edges.max()) >= S:
        raise ValueError(f"edge endpoint {int(edges.max())} is not a superpixel id (S = {S})")
    a, b = new_id[edges[:, 0].long()], new_id[edges[:, 1].long()]
    keep = a != b
    lo, hi = torch.minimum(a[keep], b[keep]), torch.maximum(a[keep], b[keep])
    keys = torch.unique(lo * C + hi)
    new_edges = torch.stack((keys // C, keys % C), 1).to(torch.int32)
    return new_id.to(torch.int32), new_ptr.to(torch.int32), new_idx, new_edges


# ---- mutual-best-neighbour merging (csrc/dm_merge.hip; the rule: include/deepmerge_hip.h) --------------------
_STAT_KEYS = ("count", "sum", "sumsq", "bbox", "peri")


@dataclass
class MergeResult:
    """What `merge_regions` leaves: the final partition in the form it took as input, and how it got there.

    region_of int32 [S0]: final region of every original superpixel; ptr / idx / edges / weights / stats: the final partition
    (weights / stats None when none were given); pooled [C,D], simi [E]: the scoring of the final partition; rep int32 [C]: the
    smallest original superpixel id of each region (regions are numbered in that order); rounds: rounds applied; history int32
    [M,3] = (round, rep of the surviving region, rep of the absorbed one) with history_simi float32 [M], in merge order;
    regions_per_round: region count before round 1 and after every applied round (rounds + 1 entries); small_rounds: how many of
    the rounds, the last ones, were elimination rounds (`min_area`): the margin rounds ended after `rounds - small_rounds`, and
    history / history_simi / regions_per_round / merges_per_round run on through both kinds (an elimination round's history_simi
    may be >= margin)."""
    region_of: torch.Tensor
    ptr: torch.Tensor
    idx: torch.Tensor
    edges: torch.Tensor
    weights: Optional[torch.Tensor]
    stats: Optional[Dict[str, torch.Tensor]]
    pooled: torch.Tensor
    simi: torch.Tensor
    rep: torch.Tensor
    rounds: int
    history: torch.Tensor
    history_simi: torch.Tensor
    regions_per_round: List[int]
    merges_per_round: List[int] = field(default_factory=list)
    small_rounds: int = 0

    def labels(self, raster: torch.Tensor) -> torch.Tensor:
        """Merged label raster: out[y,x] = region_of[raster[y,x]] (int32 [H,W]; ids outside [0, S0) are copied through)."""
        return relabel_raster(raster, self.region_of)

    def region_of_at(self, round: int) -> torch.Tensor:
        """int32 [S0]: the map from original superpixels to regions after the first `round` rounds, replayed from `history`
        (region ids dense, in order of the region's smallest original id, as every round numbers them)."""
        if not 0 <= round <= self.rounds:
            raise ValueError(f"round must be in 0..{self.rounds}, got {round}")
        S0 = self.region_of.numel()
        m = sum(self.merges_per_round[:round])
        parent = torch.arange(S0, dtype=torch.int64, device=self.region_of.device)
        if m:
            h = self.history[:m].long()
            parent[h[:, 2]] = h[:, 1]                      # every region is absorbed at most once
            for _ in range(max(1, S0.bit_length())):       # pointer doubling: a chain of absorptions is at most S0 long
                parent = parent[parent]
        dense = torch.cumsum((parent == torch.arange(S0, device=parent.device)).to(torch.int64), 0) - 1
        return dense[parent].to(torch.int32)

    def polygons(self, raster: torch.Tensor) -> "Polygons":
        """The merged regions as polygon rings: `polygons(self.labels(raster), number of merged regions)`."""
        return polygons(self.labels(raster), self.rep.numel())

    def boundary_arcs(self, raster: torch.Tensor) -> "Arcs":
        """The boundaries between the merged regions, `edge` = row of `self.edges`: `boundary_arcs(self.labels(raster), ...)`."""
        return boundary_arcs(self.labels(raster), self.rep.numel(), edges=self.edges)

    def simplified(self, raster: torch.Tensor, tolerance: float, topology: bool = False) -> Tuple["Polygons", "Arcs"]:
        """The merged regions' rings and boundary arcs simplified to `tolerance` pixels, `Arcs.edge` = row of `self.edges`:
        `simplify(self.labels(raster), number of merged regions, tolerance, edges=self.edges, topology=topology)`."""
        return simplify(self.labels(raster), self.rep.numel(), tolerance, edges=self.edges, topology=topology)

    def scores(self, overlap: "Overlap", round: Optional[int] = None) -> "PartitionScores":
        """The partition scored against a ground-truth map: `overlap` = label_overlap(superpixel raster, truth, S0, G), coarsened by
        the final map (round None) or the map after `round` rounds.  No pass over the raster."""
        return overlap.coarsen(self.region_of if round is None else self.region_of_at(round)).scores()

    def boundary_scores(self, raster: torch.Tensor, truth: torch.Tensor, n_truth: int, tolerance: int = 2,
                        rounds=None) -> List["BoundaryScores"]:
        """One BoundaryScores per round of `rounds` (default 0..self.rounds, every round `region_of_at` accepts): the partition
        after that round scored against the truth raster, the curve to pick a round or a margin from, next to `scores`.  raster:
        the superpixel raster the merge started from.  The truth's bits are made once; every round is one pass over `raster` with
        mapping = region_of_at(r), no relabelled raster is built; one readback (the counts of all rounds)."""
        _need_cuda(raster, truth)
        S0 = self.region_of.numel()
        _check_boundary_raster(raster, S0, "raster")
        _check_boundary_raster(truth, n_truth, "truth")
        if raster.shape != truth.shape:
            raise ValueError("raster and truth must cover the same raster")
        (d,), _ = _tolerances([tolerance])
        rounds = list(range(self.rounds + 1)) if rounds is None else [int(r) for r in rounds]
        maps = [self.region_of_at(r).contiguous() for r in rounds]           # (raises for a round outside 0..self.rounds)
        H, W = raster.shape
        raster = raster.contiguous()
        truth_edge, truth_valid = boundary_bits(truth.contiguous(), n_truth, valid=True)
        counts = torch.zeros((len(rounds), 4), dtype=torch.int64, device=raster.device)
        for i, mapping in enumerate(maps):
            label_edge, _ = boundary_bits(raster, S0, mapping)
            boundary_counts(label_edge, truth_edge, truth_valid, H, W, [d], (0, H, 0, W), counts[i:i + 1])
        return [boundary_scores_of(d, c) for c in counts.tolist()]


def relabel_raster(raster: torch.Tensor, mapping: torch.Tensor) -> torch.Tensor:
    """out[y,x] = mapping[raster[y,x]] for an int32 raster (dm_relabel_raster); ids outside [0, len(mapping)) stay as they are."""
    _need_cuda(raster, mapping)
    if raster.dtype != torch.int32 or raster.dim() != 2 or mapping.dtype != torch.int32 or mapping.dim() != 1 or mapping.numel() < 1:
        raise ValueError("raster must be int32 [H,W] and mapping int32 [S], S >= 1")
    raster, mapping = raster.contiguous(), mapping.contiguous()
    out = torch.empty_like(raster)
    if raster.numel():
        check(_lib.lib().dm_relabel_raster(raster.data_ptr(), mapping.data_ptr(), out.data_ptr(), raster.numel(), mapping.numel(),
                                           _stream()), "dm_relabel_raster")
    return out


_INPUT_ERRORS = ("ptr must start at 0, be non-decreasing and end at len(idx)",
                 "idx must index rows of features",
                 "an edge has a negative endpoint (-1 = 'no polygon' edges cannot be relabelled: filter them with "
                 "edges[(edges >= 0).all(1)])",
                 "edge endpoints must be region ids with a < b",
                 "edges must be sorted by (a, b) and unique")


def _check_merge_inputs(features, ptr, idx, edges, S0):
    """One device check (one readback) before round 1: an id out of range would be an out-of-bounds access on the device."""
    dev = ptr.device
    flags = [((ptr[1:] < ptr[:-1]).any() | (ptr[0] != 0) | (ptr[-1] != idx.numel()))]
    flags.append(((idx < 0) | (idx >= features.shape[0])).any() if idx.numel() else torch.zeros((), dtype=torch.bool, device=dev))
    if edges.shape[0]:
        a, b = edges[:, 0].long(), edges[:, 1].long()
        key = a * S0 + b
        flags += [(edges < 0).any(), ((a >= b) | (b >= S0)).any(), (key[1:] <= key[:-1]).any()]
    code = sum(f.to(torch.int32) << i for i, f in enumerate(flags))
    code = int(code)
    for i, msg in enumerate(_INPUT_ERRORS):
        if code >> i & 1:
            raise ValueError(f"merge_regions: {msg}")


def _check_min_area(min_area, have_stats: bool = True) -> int:
    """`min_area` of `merge_regions`, `mrs` and `mrs_graph`: a ValueError before any device work."""
    try:
        area = operator.index(min_area)
    except TypeError:
        raise ValueError(f"min_area must be an integer number of pixels, got {min_area!r}") from None
    if not 0 <= area < 1 << 63:
        raise ValueError(f"min_area must be >= 0 (and fit int64), got {area}")
    if area and not have_stats:
        raise ValueError("min_area needs stats: a region's area is stats['count']")
    return area


def merge_regions(features: torch.Tensor, ptr: torch.Tensor, idx: torch.Tensor, edges: torch.Tensor, *, margin: float = 1.0,
                  weights: Optional[torch.Tensor] = None, stats: Optional[Dict[str, torch.Tensor]] = None,
                  max_rounds: Optional[int] = None, min_regions: int = 0, min_area: int = 0) -> MergeResult:
    """Mutual-best-neighbour region merging on the device, from the sweep's inputs to the final partition.

    features fp32 [P,D]; ptr int32 [S0+1] / idx int32 [P']: the superpixels' point lists; edges int32 [E,2], a < b, sorted by
    (a, b), unique (as `rag_edges` returns them); weights int32 [E]: shared boundary lengths; stats: `label_stats`' dict (needs
    weights: the inner perimeter cannot be folded without them).  Per round: score the regions as they are (segment mean +
    edge similarity, the sweep's kernels), let every region choose its best neighbour among the edges with simi < margin
    (smallest simi, then smallest id), merge the pairs that chose each other, and fold point lists, edges, weights, statistics.
    Stops when a round merges nothing (then no edge has simi < margin), after `max_rounds` rounds, or before a round that would
    leave fewer than `min_regions` regions (that round is not applied, so more regions than asked may remain).
    min_area > 0 (pixels; needs stats) adds the minimum mapping unit: once a round has merged nothing -- not when max_rounds or
    min_regions ended the rounds -- elimination rounds follow, in which every region with stats["count"] < min_area proposes to the
    neighbour it resembles most (smallest simi over its edges, NaN excepted, no margin; then smallest id), every other region
    accepts the best of its proposers, and mutual choices merge as above.  They end when no small region has a scored edge left
    (or at max_rounds, which counts all rounds, or min_regions); `result.small_rounds` counts them and the history runs on through
    them.  They do not go back to the margin rule: a merge can pull a region's pooled mean below the margin to a neighbour, the
    result's `simi` shows such edges, and a caller who wants them merged calls again.  min_area = 0: no such rounds, nothing else
    changes.
    The inputs are not modified.  One small readback per round; everything else stays on the device."""
    min_area = _check_min_area(min_area, stats is not None)
    _need_cuda(features, ptr, idx, edges, weights, *((stats or {}).get(k) for k in _STAT_KEYS))
    if features.dtype != torch.float32 or features.dim() != 2 or features.shape[1] < 1:
        raise ValueError("features must be float32 [P,D]")
    if ptr.dtype != torch.int32 or ptr.dim() != 1 or ptr.numel() < 2 or idx.dtype != torch.int32 or idx.dim() != 1:
        raise ValueError("ptr must be int32 [S+1] with S >= 1 and idx int32 [P]")
    if edges.dtype != torch.int32 or edges.dim() != 2 or edges.shape[1] != 2:
        raise ValueError("edges must be int32 [E,2]")
    S0, P, E0, D = ptr.numel() - 1, idx.numel(), edges.shape[0], features.shape[1]
    if P < 1 or features.shape[0] < 1:
        raise ValueError("merge_regions needs at least one sample point")
    if S0 > 1 << 24:
        raise ValueError(f"merge_regions takes at most 2^24 regions, got {S0}")
    if weights is not None and (weights.dtype != torch.int32 or tuple(weights.shape) != (E0,)):
        raise ValueError("weights must be int32 [E]")
    if max_rounds is not None and max_rounds < 0:
        raise ValueError("max_rounds must be >= 0 or None")
    nb = 0
    if stats is not None:
        if weights is None:
            raise ValueError("stats need weights: the inner perimeter of a merged region is peri_a + peri_b - 2 weight(a, b)")
        nb = int(stats["bands"])
        want = {"count": (torch.int64, (S0,)), "sum": (torch.int64, (S0, nb)), "sumsq": (torch.int64, (S0, nb)),
                "bbox": (torch.int32, (S0, 4)), "peri": (torch.int64, (S0, 2))}
        for k, (dt, shape) in want.items():
            if stats[k].dtype != dt or tuple(stats[k].shape) != shape:
                raise ValueError(f"stats[{k!r}] must be {dt} {list(shape)} (as label_stats returns it)")
        if not 1 <= nb <= 3:
            raise ValueError("stats['bands'] must be 1..3")
    features, ptr, idx, edges = features.contiguous(), ptr.contiguous(), idx.contiguous(), edges.contiguous()
    _check_merge_inputs(features, ptr, idx, edges, S0)
    lib = _lib.lib()
    pooled = torch.empty((S0, D), dtype=torch.float32, device=ptr.device)

    def score(cur, C, E, simi, stream):                          # segment mean + edge similarity: the sweep's kernels
        check(lib.dm_segment_mean(features.data_ptr(), cur["ptr"].data_ptr(), cur["idx"].data_ptr(), pooled.data_ptr(), C, D, stream),
              "dm_segment_mean")
        if E:
            check(lib.dm_edge_similarity(pooled.data_ptr(), cur["edges"].data_ptr(), simi.data_ptr(), None, E, D, margin, stream),
                  "dm_edge_similarity")

    return _merge_loop(score, margin, pooled, ptr, idx, edges, weights, stats, nb, max_rounds, min_regions, min_area)


def _merge_loop(score, margin: float, pooled: torch.Tensor, ptr: torch.Tensor, idx: torch.Tensor, edges: torch.Tensor,
                weights: Optional[torch.Tensor], stats: Optional[Dict[str, torch.Tensor]], nb: int, max_rounds: Optional[int],
                min_regions: int, min_area: int = 0) -> MergeResult:
    """The rounds of the mutual-best merge (include/deepmerge_hip.h) around a pluggable score step, for `merge_regions` and `mrs`.
    score(cur, C, E, simi, stream) writes simi[:E] for the partition `cur` (the dict of its device arrays) and whatever it keeps of
    its own (`pooled [S0,D]`, whose first C rows go into the result); an edge is a candidate iff simi < margin.  The inputs are
    checked and contiguous.  P = len(idx) may be 0: then no point list is read or written.  min_area > 0 (checked; stats given):
    after the first round that picks nothing, the elimination rounds of the header's rule, which differ in how `best` is made."""
    S0, P, E0 = ptr.numel() - 1, idx.numel(), edges.shape[0]
    dev, lib, i32 = ptr.device, _lib.lib(), torch.int32

    def new_state():
        st = {"ptr": torch.empty(S0 + 1, dtype=i32, device=dev), "idx": torch.empty(P, dtype=i32, device=dev),
              "edges": torch.empty((E0, 2), dtype=i32, device=dev), "rep": torch.empty(S0, dtype=i32, device=dev),
              "region_of": torch.empty(S0, dtype=i32, device=dev),
              "weights": torch.empty(E0, dtype=i32, device=dev) if weights is not None else None}
        if stats is not None:
            st.update({k: torch.empty_like(stats[k]) for k in _STAT_KEYS})
        return st

    ident = torch.arange(S0, dtype=i32, device=dev)
    cur = {"ptr": ptr, "idx": idx, "edges": edges, "rep": ident, "region_of": ident,
           "weights": weights.contiguous() if weights is not None else None}
    if stats is not None:
        cur.update({k: stats[k].contiguous() for k in _STAT_KEYS})
    spare = [new_state(), new_state()] if E0 else []
    simi = torch.empty(E0, dtype=torch.float32, device=dev)
    best = torch.empty(S0, dtype=torch.int64, device=dev)
    picked = torch.empty(E0, dtype=torch.uint8, device=dev)
    root, pick, new_id, hist_rank = (torch.empty(S0, dtype=i32, device=dev) for _ in range(4))
    keys = torch.empty(E0, dtype=torch.int64, device=dev)
    meta = torch.zeros(3, dtype=i32, device=dev)                 # picked edges, new C, new E: the round's one readback
    history = torch.empty((S0, 3), dtype=i32, device=dev)
    history_simi = torch.empty(S0, dtype=torch.float32, device=dev)
    ptr_of = lambda t: (t.data_ptr() or None) if t is not None else None      # an empty tensor (no points) has no address

    C, E, rounds, n_hist = S0, E0, 0, 0
    regions, merges = [S0], []
    small, small_rounds, scored = False, 0, False                # small: the elimination rounds have begun
    while True:
        stream = _stream()
        if not scored:
            score(cur, C, E, simi, stream)
        scored = False
        if E == 0 or C <= max(min_regions, 1) or (max_rounds is not None and rounds >= max_rounds):
            break
        nxt = spare[rounds & 1]
        if small:
            args = (cur["edges"].data_ptr(), simi.data_ptr(), E, C, cur["count"].data_ptr(), min_area, best.data_ptr(), stream)
            check(lib.dm_merge_best_small(*args), "dm_merge_best_small")
            check(lib.dm_merge_accept(*args), "dm_merge_accept")
        else:
            check(lib.dm_merge_best(cur["edges"].data_ptr(), simi.data_ptr(), E, C, margin, best.data_ptr(), stream), "dm_merge_best")
        check(lib.dm_merge_match(cur["edges"].data_ptr(), best.data_ptr(), E, C, picked.data_ptr(), root.data_ptr(), pick.data_ptr(),
                                 meta.data_ptr(), stream), "dm_merge_match")
        f = _lib.DmMergeFold()
        for k in ("ptr", "idx", "edges", "rep", "region_of", "weights") + (_STAT_KEYS if stats is not None else ()):
            setattr(f, k, ptr_of(cur[k]))
        for k in ("ptr", "idx", "rep", "region_of") + (_STAT_KEYS if stats is not None else ()):
            setattr(f, "new_" + k, ptr_of(nxt[k]))
        f.root, f.pick, f.simi, f.new_id, f.hist_rank = root.data_ptr(), pick.data_ptr(), simi.data_ptr(), new_id.data_ptr(), hist_rank.data_ptr()
        f.n_regions, f.history, f.history_simi = meta[1:].data_ptr(), history.data_ptr(), history_simi.data_ptr()
        f.C, f.P, f.E, f.S0, f.bands, f.round, f.hist_base, f.hist_cap = C, P, E, S0, nb, rounds, n_hist, S0
        check(lib.dm_merge_fold_regions(ctypes.byref(f), stream), "dm_merge_fold_regions")
        check(lib.dm_merge_edge_keys(cur["edges"].data_ptr(), root.data_ptr(), new_id.data_ptr(), E, C, keys.data_ptr(), stream),
              "dm_merge_edge_keys")
        skeys, order = torch.sort(keys[:E])                      # canonical (a, b) order of the relabelled edges
        check(lib.dm_merge_fold_edges(skeys.data_ptr(), order.data_ptr(), ptr_of(cur["weights"]), E, nxt["edges"].data_ptr(),
                                      ptr_of(nxt["weights"]), meta[2:].data_ptr(), stream), "dm_merge_fold_edges")
        n_pick, C_new, E_new = meta.tolist()
        if n_pick == 0 and min_area and not small:               # the margin rounds are over: the same partition, the same scores,
            small = scored = True                                # now by the elimination rule
            continue
        if n_pick == 0 or C_new < min_regions:                   # nothing merged / the round would go too far: it is dropped whole
            break
        cur = {k: (None if v is None else v[:C_new + 1] if k == "ptr" else v[:E_new] if k in ("edges", "weights") else
                   v if k in ("idx", "region_of") else v[:C_new]) for k, v in nxt.items()}
        C, E, rounds, n_hist = C_new, E_new, rounds + 1, n_hist + n_pick
        small_rounds += small
        regions.append(C)
        merges.append(n_pick)

    out_stats = None
    if stats is not None:
        out_stats = {k: cur[k].clone() for k in _STAT_KEYS}
        out_stats["bands"] = nb
    return MergeResult(region_of=cur["region_of"].clone(), ptr=cur["ptr"].clone(), idx=cur["idx"].clone(), edges=cur["edges"].clone(),
                       weights=None if weights is None else cur["weights"].clone(), stats=out_stats, pooled=pooled[:C].clone(),
                       simi=simi[:E].clone(), rep=cur["rep"].clone(), rounds=rounds, history=history[:n_hist].clone(),
                       history_simi=history_simi[:n_hist].clone(), regions_per_round=regions, merges_per_round=merges,
                       small_rounds=small_rounds)


# ---- multiresolution region merging (csrc/dm_mrs.hip; the rule: include/deepmerge_hip.h; spec tests/mrs_ref.py) ----
MAX_REGIONS = 1 << 24     # what a merge takes (dm_merge_best's key keeps the neighbour id beside the score)


def _on_device(*ts):
    """`_need_cuda` for the entry points below, whose bad arguments are all ValueErrors."""
    try:
        _need_cuda(*ts)
    except RuntimeError as e:
        raise ValueError(str(e)) from None


def _mrs_params(nb: int, shape: float, compactness: float, band_weights) -> Tuple[float, float, List[float]]:
    shape, compactness = float(shape), float(compactness)
    if not 0.0 <= shape < 1.0:
        raise ValueError(f"shape must be in [0, 1), got {shape}")
    if not 0.0 <= compactness <= 1.0:
        raise ValueError(f"compactness must be in [0, 1], got {compactness}")
    bw = [1.0] * nb if band_weights is None else [float(v) for v in band_weights]
    if len(bw) != nb:
        raise ValueError(f"band_weights must have {nb} values (one per band that counts), got {len(bw)}")
    if not all(math.isfinite(v) and v >= 0.0 for v in bw):
        raise ValueError(f"band_weights must be finite and >= 0, got {bw}")
    return shape, compactness, bw + [1.0] * (3 - nb)


def _check_stats(stats: Dict[str, torch.Tensor], C: int) -> int:
    nb = int(stats["bands"])
    if not 1 <= nb <= 3:
        raise ValueError("stats['bands'] must be 1..3")
    want = {"count": (torch.int64, (C,)), "sum": (torch.int64, (C, nb)), "sumsq": (torch.int64, (C, nb)),
            "bbox": (torch.int32, (C, 4)), "peri": (torch.int64, (C, 2))}
    for k, (dt, shape) in want.items():
        if stats[k].dtype != dt or tuple(stats[k].shape) != shape:
            raise ValueError(f"stats[{k!r}] must be {dt} {list(shape)} (as label_stats returns it)")
    return nb


def _launch_merge_cost(lib, st, edges, weights, E: int, C: int, nb: int, bw, shape: float, compactness: float, cost, stream):
    check(lib.dm_region_merge_cost(st["count"].data_ptr(), st["sum"].data_ptr(), st["sumsq"].data_ptr(), st["bbox"].data_ptr(),
                                   st["peri"].data_ptr(), edges.data_ptr(), weights.data_ptr(), E, C, nb, bw[0], bw[1], bw[2], shape,
                                   compactness, cost.data_ptr(), stream), "dm_region_merge_cost")


def region_merge_cost(stats: Dict[str, torch.Tensor], edges: torch.Tensor, weights: torch.Tensor, shape: float = 0.1,
                      compactness: float = 0.5, band_weights=None) -> torch.Tensor:
    """float32 [E]: the multiresolution-segmentation cost of merging the two regions of every edge -- the increase of the
    Baatz-Schaepe colour heterogeneity (n sigma per band, weighted by band_weights) and shape heterogeneity (compactness
    n l / sqrt(n) and smoothness n l / b, mixed by `compactness`), mixed by `shape`, clamped at 0 -- from `label_stats`' exact
    statistics and `rag_edges`' boundary lengths.  Every region of an edge must have count > 0 (else its cost is NaN)."""
    _on_device(edges, weights, *(stats[k] for k in _STAT_KEYS))
    if edges.dtype != torch.int32 or edges.dim() != 2 or edges.shape[1] != 2:
        raise ValueError("edges must be int32 [E,2]")
    E, C = edges.shape[0], stats["count"].numel()
    if weights.dtype != torch.int32 or tuple(weights.shape) != (E,):
        raise ValueError("weights must be int32 [E]")
    nb = _check_stats(stats, C)
    if not 1 <= C <= MAX_REGIONS:
        raise ValueError(f"region_merge_cost takes 1 to 2^24 regions, got {C}")
    shape, compactness, bw = _mrs_params(nb, shape, compactness, band_weights)
    cost = torch.empty(E, dtype=torch.float32, device=edges.device)
    if E:
        _launch_merge_cost(_lib.lib(), {k: stats[k].contiguous() for k in _STAT_KEYS}, edges.contiguous(), weights.contiguous(), E, C, nb,
                           bw, shape, compactness, cost, _stream())
    return cost


def _check_tile(tile: torch.Tensor):
    _on_device(tile)
    if tile.dtype != torch.uint8 or tile.dim() != 3 or tile.shape[0] < 1 or tile.shape[1] < 1 or tile.shape[2] < 1:
        raise ValueError("tile must be uint8 [bands,H,W] with bands, H, W >= 1")


def pixel_regions(tile: torch.Tensor) -> Tuple[Dict[str, torch.Tensor], torch.Tensor, torch.Tensor]:
    """(stats, edges, weights) of the partition in which pixel (y, x) is region y * W + x: what `label_stats` and `rag_edges` give
    for an `arange` raster, bit for bit, written in closed form (no hash table).  H * W <= 2^24."""
    _check_tile(tile)
    bands, H, W = tile.shape
    if H * W > MAX_REGIONS:
        raise ValueError(f"a pixel start takes at most 2^24 pixels, got {H} x {W} = {H * W}")
    tile = tile.contiguous()
    n, nb, dev, E = H * W, min(bands, 3), tile.device, H * (W - 1) + (H - 1) * W
    stats = {"count": torch.empty(n, dtype=torch.int64, device=dev), "sum": torch.empty((n, nb), dtype=torch.int64, device=dev),
             "sumsq": torch.empty((n, nb), dtype=torch.int64, device=dev), "bbox": torch.empty((n, 4), dtype=torch.int32, device=dev),
             "peri": torch.empty((n, 2), dtype=torch.int64, device=dev)}
    edges = torch.empty((E, 2), dtype=torch.int32, device=dev)
    weights = torch.empty(E, dtype=torch.int32, device=dev)
    check(_lib.lib().dm_pixel_regions(tile.data_ptr(), bands, H, W, stats["count"].data_ptr(), stats["sum"].data_ptr(),
                                      stats["sumsq"].data_ptr(), stats["bbox"].data_ptr(), stats["peri"].data_ptr(),
                                      edges.data_ptr() or None, weights.data_ptr() or None, _stream()), "dm_pixel_regions")
    stats["bands"] = nb
    return stats, edges, weights


def mrs(tile: torch.Tensor, scale: float, shape: float = 0.1, compactness: float = 0.5, band_weights=None,
        labels: Optional[torch.Tensor] = None, n_labels: Optional[int] = None, max_rounds: Optional[int] = None,
        min_regions: int = 0, min_area: int = 0) -> MergeResult:
    """Multiresolution segmentation: mutual-best region merging by `region_merge_cost`, the classical baseline of the learned
    merge and a second source of superpixels.

    tile uint8 [bands,H,W] (the first three bands count).  Per round every region chooses its cheapest neighbour among the edges
    with cost < scale^2 (ties: smallest id), mutual choices merge, and statistics, edges and boundary lengths are folded -- the
    rounds of `merge_regions`, with the cost in place of the learned similarity and no point lists.  Starts from single pixels
    (labels None: S0 = H * W <= 2^24 and `result.region_of.view(H, W)` is the label raster) or from a label raster (labels int32
    [H,W] with every id in [0, n_labels) present: `result.labels(labels)` is the raster).  The result has pooled [C,0], ptr zeros,
    idx empty, simi = the cost of the final partition's edges; `labels()`, `polygons()`, `simplified()`, `scores()` and
    `region_of_at()` work as on any MergeResult.  Stops as `merge_regions` does; min_area > 0 (pixels) adds its elimination rounds,
    with the cost as the score: what `scale` leaves below that area (single pixels and specks from a pixel start) joins its
    cheapest neighbour.  The inputs are not modified; one small readback per round."""
    min_area = _check_min_area(min_area)
    _check_tile(tile)
    bands, H, W = tile.shape
    _mrs_check(scale, min(bands, 3), shape, compactness, band_weights, max_rounds)
    if labels is None:
        if n_labels is not None:
            raise ValueError("n_labels goes with labels")
        stats, edges, weights = pixel_regions(tile)
    else:
        _on_device(labels)
        if labels.dtype != torch.int32 or tuple(labels.shape) != (H, W):
            raise ValueError("labels must be int32 [H,W] over the tile's raster")
        if n_labels is None or not 1 <= int(n_labels) <= MAX_REGIONS:
            raise ValueError(f"n_labels must be given with labels, 1 to 2^24, got {n_labels}")
        stats = label_stats(labels, tile, int(n_labels))
        _check_no_empty_region(stats)                            # (the one readback before round 1)
        edges, weights = rag_edges(labels, int(n_labels))
    return mrs_graph(stats, edges, weights, scale, shape, compactness, band_weights, max_rounds, min_regions, min_area=min_area,
                     _checked=True)


def _mrs_check(scale, nb: int, shape, compactness, band_weights, max_rounds) -> Tuple[float, float, float, List[float]]:
    """The arguments `mrs` and `mrs_graph` share, each a ValueError before any device work."""
    scale = float(scale)
    if not (math.isfinite(scale) and scale > 0.0):
        raise ValueError(f"scale must be finite and > 0, got {scale}")
    shape, compactness, bw = _mrs_params(nb, shape, compactness, band_weights)
    if max_rounds is not None and max_rounds < 0:
        raise ValueError("max_rounds must be >= 0 or None")
    return scale, shape, compactness, bw


def _check_no_empty_region(stats: Dict[str, torch.Tensor]):
    if bool((stats["count"] == 0).any()):
        raise ValueError("mrs: every id in [0, n_labels) must occur in labels (a region without pixels has no cost)")


def mrs_graph(stats: Dict[str, torch.Tensor], edges: torch.Tensor, weights: torch.Tensor, scale: float, shape: float = 0.1,
              compactness: float = 0.5, band_weights=None, max_rounds: Optional[int] = None, min_regions: int = 0,
              min_area: int = 0, _checked: bool = False) -> MergeResult:
    """The rounds of `mrs` on a graph that is already built: stats as `label_stats` returns them (every region with count > 0,
    else ValueError), edges int32 [E,2] with a < b, sorted and unique, weights int32 [E] as `rag_edges` returns them.  `mrs` builds
    its graph from one raster and calls this; `scene.mrs_labels` builds it from a scene's label raster tile by tile.  min_area: as
    `mrs` takes it.  The inputs are not modified."""
    min_area = _check_min_area(min_area)
    _on_device(edges, weights, *(stats[k] for k in _STAT_KEYS))
    S0 = stats["count"].numel()
    nb = _check_stats(stats, S0)
    scale, shape, compactness, bw = _mrs_check(scale, nb, shape, compactness, band_weights, max_rounds)
    if not 1 <= S0 <= MAX_REGIONS:
        raise ValueError(f"mrs_graph takes 1 to 2^24 regions, got {S0}")
    if edges.dtype != torch.int32 or edges.dim() != 2 or edges.shape[1] != 2 or weights.dtype != torch.int32 or tuple(weights.shape) != (edges.shape[0],):
        raise ValueError("edges must be int32 [E,2] and weights int32 [E]")
    if not _checked:
        _check_no_empty_region(stats)
    edges, weights = edges.contiguous(), weights.contiguous()
    dev, lib = edges.device, _lib.lib()

    def score(cur, C, E, simi, stream):
        if E:
            _launch_merge_cost(lib, cur, cur["edges"], cur["weights"], E, C, nb, bw, shape, compactness, simi, stream)

    return _merge_loop(score, scale * scale, torch.empty((S0, 0), dtype=torch.float32, device=dev),
                       torch.zeros(S0 + 1, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev), edges, weights,
                       stats, nb, max_rounds, min_regions, min_area)


def mrs_segment(tile: torch.Tensor, scale: float, **kw) -> Tuple[torch.Tensor, int]:
    """(labels int32 [H,W] with dense ids 0..n-1, n): `mrs` as a segmenter, the pair `slic` returns, so that
    `FeatureIO.merge_tile(tile, *mrs_segment(tile, scale))` is the pipeline on multiresolution superpixels.  kw: `mrs`'s keywords
    (min_area among them: no superpixel below that many pixels)."""
    res = mrs(tile, scale, **kw)
    start = kw.get("labels")
    raster = res.region_of.view(tile.shape[1], tile.shape[2]).clone() if start is None else res.labels(start)
    return raster, res.rep.numel()


# ---- sample points and window sides from the label raster (csrc/dm_points.hip; the rule: include/deepmerge_hip.h) ----
MAX_WINDOW = 384          # dataset.MAX_WINDOW: the gather's LDS staging limit
MAX_POINTS = 16           # points per superpixel (csrc/dm_points.hip KMAX)


@dataclass
class PointSamples:
    """What `sample_points` leaves: one row per sample point, sorted by (superpixel, round).

    xy int32 [P,2] = (x, y) pixel position; label int32 [P]: the point's superpixel; inner / obj int32 [P]: the window fields the
    crop consumes (inner = 2 clearance - 1, obj = min(longer bounding-box side, (max_window + 2 inner) // 3)); ptr int32 [S+1] /
    idx int32 [P] = arange(P): the superpixels' point lists in the form the sweep and `merge_regions` take; bbox int32 [S,4] =
    xmin, ymin, xmax, ymax as `label_stats` writes it; round int32 [P]: the selection round that chose the point (0 = the pixel
    farthest from the superpixel's boundary)."""
    xy: torch.Tensor
    label: torch.Tensor
    inner: torch.Tensor
    obj: torch.Tensor
    ptr: torch.Tensor
    idx: torch.Tensor
    bbox: torch.Tensor
    round: torch.Tensor

    def region_features(self, designed: torch.Tensor) -> torch.Tensor:
        """[P,15]: every point's row of `designed_features` (designed[label]), as the encoder takes them."""
        if designed.dim() != 2 or designed.shape[0] != self.bbox.shape[0]:
            raise ValueError(f"designed must be [S,15] with S = {self.bbox.shape[0]} rows (as designed_features returns it)")
        return designed[self.label.long()]


def _check_raster(labels: torch.Tensor, max_window: int, what: str):
    _need_cuda(labels)
    if labels.dtype != torch.int32 or labels.dim() != 2 or labels.numel() < 1:
        raise ValueError("labels must be int32 [H,W] with at least one pixel")
    if labels.numel() >= 1 << 31:
        raise ValueError(f"{what} takes rasters of fewer than 2^31 pixels, got {labels.numel()}")
    if not 1 <= int(max_window) <= MAX_WINDOW:
        raise ValueError(f"max_window must be in 1..{MAX_WINDOW}, got {max_window}")


def clearance(labels: torch.Tensor, max_window: int = MAX_WINDOW) -> torch.Tensor:
    """uint16 [H,W]: Chebyshev distance from every pixel to the nearest pixel of another label or outside the raster, capped at
    (max_window + 1) // 2.  The largest odd square centred on the pixel inside its superpixel has side 2 c - 1."""
    _check_raster(labels, max_window, "clearance")
    labels = labels.contiguous()
    H, W = labels.shape
    dev = labels.device
    bits = torch.empty(H * ((W + 63) // 64), dtype=torch.int64, device=dev)
    row_dist = torch.empty((H, W), dtype=torch.uint8, device=dev)
    out = torch.empty((H, W), dtype=torch.uint16, device=dev)
    check(_lib.lib().dm_label_clearance(labels.data_ptr(), H, W, int(max_window), bits.data_ptr(), row_dist.data_ptr(), out.data_ptr(),
                                        _stream()), "dm_label_clearance")
    return out


def sample_points(labels: torch.Tensor, n_labels: int, k: int = 3, max_window: int = MAX_WINDOW) -> PointSamples:
    """Sample points and their window fields from the label raster alone (what the reference reads from a point shapefile).

    Every superpixel gets min(k, area) points: the pixel farthest from its boundary first, then pixels that trade clearance
    against distance to the points already chosen (the rule: include/deepmerge_hip.h).  `inner` is the largest odd square around
    the point inside the superpixel, `obj` the superpixel's longer bounding-box side, clamped so that the largest window the crop
    derives (3 obj - 2 inner) stays within max_window.  Ids outside [0, n_labels) get no points.  The input is not modified.
    One readback (the number of points); everything else stays on the device."""
    _check_raster(labels, max_window, "sample_points")
    if n_labels < 1:
        raise ValueError(f"n_labels must be >= 1, got {n_labels}")
    if not 1 <= int(k) <= MAX_POINTS:
        raise ValueError(f"k must be in 1..{MAX_POINTS}, got {k}")
    if n_labels * int(k) >= 1 << 31:
        raise ValueError(f"n_labels * k must be below 2^31, got {n_labels * int(k)}")
    labels = labels.contiguous()
    H, W = labels.shape
    S, k, dev, lib, i32 = int(n_labels), int(k), labels.device, _lib.lib(), torch.int32
    clr = clearance(labels, max_window)
    best = torch.empty(S, dtype=torch.int64, device=dev)
    pts = torch.empty((S, k, 2), dtype=i32, device=dev)
    pclr = torch.empty((S, k), dtype=i32, device=dev)
    cnt = torch.empty(S, dtype=i32, device=dev)
    bbox = torch.empty((S, 4), dtype=i32, device=dev)
    for j in range(k):
        check(lib.dm_point_select_round(labels.data_ptr(), clr.data_ptr(), H, W, S, k, j, best.data_ptr(), pts.data_ptr(), pclr.data_ptr(),
                                        cnt.data_ptr(), bbox.data_ptr(), _stream()), "dm_point_select_round")
    cap = S * k
    ptr = torch.empty(S + 1, dtype=i32, device=dev)
    xy = torch.empty((cap, 2), dtype=i32, device=dev)
    label, inner, obj, rnd = (torch.empty(cap, dtype=i32, device=dev) for _ in range(4))
    check(lib.dm_point_emit(cnt.data_ptr(), pts.data_ptr(), pclr.data_ptr(), bbox.data_ptr(), S, k, int(max_window), cap, ptr.data_ptr(),
                            xy.data_ptr(), label.data_ptr(), inner.data_ptr(), obj.data_ptr(), rnd.data_ptr(), _stream()), "dm_point_emit")
    P = int(ptr[S])                                            # the one readback: sizes the views below
    return PointSamples(xy=xy[:P], label=label[:P], inner=inner[:P], obj=obj[:P], ptr=ptr, idx=torch.arange(P, dtype=i32, device=dev),
                        bbox=bbox, round=rnd[:P])


# ---- overlap with a ground-truth raster: pair labels and partition scores (csrc/dm_truth.hip; the rule: include/deepmerge_hip.h,
# DESIGN.md 3.5.3) ----
@dataclass
class PartitionScores:
    """A partition scored against a ground-truth map, over the pixels that carry both a region id and an object id.

    The eight exact integers of the summary: n pixels, sum_cells / sum_regions / sum_objects = the sums of squared cell, region and
    object pixel counts, sum_owner = sum over regions of the pixels of their best object, sum_cover = sum over objects of the pixels
    of their best region, n_regions / n_objects = how many are non-empty.  Derived: asa = sum_owner / n (achievable segmentation
    accuracy; 1 - asa is the under-segmentation), coverage = sum_cover / n (1 - coverage is the over-segmentation), rand and
    adjusted_rand from the pair counts sum C(x, 2) = (sum x^2 - n) / 2.  NaN where a figure has no pixels (or, Rand, no pair) to
    speak of."""
    n: int
    sum_cells: int
    sum_regions: int
    sum_objects: int
    sum_owner: int
    sum_cover: int
    n_regions: int
    n_objects: int
    asa: float
    coverage: float
    rand: float
    adjusted_rand: float


def partition_scores(summary) -> PartitionScores:
    """PartitionScores from the eight summary integers (Python integer arithmetic until the final divisions)."""
    n, sq, rows, cols, oc, cv, n_regions, n_objects = (int(v) for v in summary)
    nan = float("nan")
    rand = ari = nan
    if n >= 2:
        total = n * (n - 1) // 2                                  # pixel pairs
        both, same_region, same_object = (sq - n) // 2, (rows - n) // 2, (cols - n) // 2
        rand = (total + 2 * both - same_region - same_object) / total
        num = 2 * (both * total - same_region * same_object)
        den = (same_region + same_object) * total - 2 * same_region * same_object
        ari = num / den if den else 1.0                           # den == 0: both partitions are one block, or both all singletons
    return PartitionScores(n, sq, rows, cols, oc, cv, n_regions, n_objects, oc / n if n else nan, cv / n if n else nan, rand, ari)


def _overlap_facts(keys: torch.Tensor, counts: torch.Tensor, S: int, G: int) -> "Overlap":
    """dm_overlap_reduce over sorted unique keys int64 [K] with counts int32 [K]."""
    dev, K = keys.device, keys.numel()
    keys, counts = keys.contiguous(), counts.contiguous()
    i32, i64 = torch.int32, torch.int64
    best, rows, area = (torch.empty(S, dtype=i64, device=dev) for _ in range(3))
    owner, owner_count = torch.empty(S, dtype=i32, device=dev), torch.empty(S, dtype=i32, device=dev)
    size, cover = torch.empty(G, dtype=i64, device=dev), torch.empty(G, dtype=i32, device=dev)
    summary = torch.empty(8, dtype=i64, device=dev)
    check(_lib.lib().dm_overlap_reduce(keys.data_ptr() if K else None, counts.data_ptr() if K else None, K, S, G, best.data_ptr(),
                                       rows.data_ptr(), area.data_ptr(), owner.data_ptr(), owner_count.data_ptr(), size.data_ptr(),
                                       cover.data_ptr(), summary.data_ptr(), _stream()), "dm_overlap_reduce")
    cells = torch.stack((keys // (G + 1), keys % (G + 1)), 1).to(i32)
    return Overlap(cells=cells, count=counts, area=area, owner=owner, owner_count=owner_count, size=size, cover=cover, summary=summary,
                   n_labels=S, n_truth=G)


@dataclass
class Overlap:
    """What `label_overlap` leaves: the sparse overlap table of a label raster with a ground-truth raster and the facts read off it.

    cells int32 [K,2] = (s, g) sorted by (s, g), g == n_truth is the "unlabelled" column; count int32 [K] > 0: pixels in the cell;
    area int64 [S]: pixels of every region (all columns); owner int32 [S]: the object holding most of the region's labelled pixels
    (ties to the smaller id, -1: none), owner_count int32 [S]: how many; size int64 [G]: labelled pixels of every object inside
    regions 0..S-1, cover int32 [G]: the most any single region holds of it; summary int64 [8]: see PartitionScores."""
    cells: torch.Tensor
    count: torch.Tensor
    area: torch.Tensor
    owner: torch.Tensor
    owner_count: torch.Tensor
    size: torch.Tensor
    cover: torch.Tensor
    summary: torch.Tensor
    n_labels: int
    n_truth: int

    def coarsen(self, mapping: torch.Tensor) -> "Overlap":
        """The Overlap of the partition mapping[labels] without rescanning the raster.  mapping int32 [n_labels] -> regions
        0..C-1 (C = max + 1): the `region_of` of a MergeResult, or `region_of_at(r)`.  Rows are relabelled, equal cells folded
        (counts added), the facts recomputed by dm_overlap_reduce.  One readback (C)."""
        _need_cuda(mapping, self.cells)
        if mapping.dtype != torch.int32 or tuple(mapping.shape) != (self.n_labels,):
            raise ValueError(f"mapping must be int32 [{self.n_labels}]")
        lo, hi = (int(v) for v in torch.aminmax(mapping))
        if lo < 0:
            raise ValueError("mapping must map every region id to a region id >= 0")
        G = self.n_truth
        keys = mapping.long()[self.cells[:, 0].long()] * (G + 1) + self.cells[:, 1].long()
        uniq, inverse = torch.unique(keys, return_inverse=True)   # sorted
        counts = torch.zeros(uniq.numel(), dtype=torch.int32, device=keys.device).index_add_(0, inverse, self.count)
        return _overlap_facts(uniq, counts, hi + 1, G)

    def scores(self) -> PartitionScores:
        """The partition scored against the truth (one readback: the eight integers)."""
        return partition_scores(self.summary.tolist())


def label_overlap(labels: torch.Tensor, truth: torch.Tensor, n_labels: int, n_truth: int, max_cells: int = 0) -> Overlap:
    """Overlap table of a label raster (region ids 0..n_labels-1, others ignored) with a ground-truth raster (object ids
    0..n_truth-1, any other value = unlabelled, counted in column n_truth), and the row / column facts (the rule:
    include/deepmerge_hip.h).  One pass over both rasters; one readback (number of cells, overflow).  max_cells (default
    max(1024, 8 n_labels)) bounds the number of non-empty cells; a coarse partition against a fine truth map (n_truth >> n_labels)
    needs it passed explicitly, and a table that turns out too small raises RuntimeError."""
    _need_cuda(labels, truth)
    if labels.dtype != torch.int32 or truth.dtype != torch.int32 or labels.dim() != 2 or labels.shape != truth.shape or labels.numel() < 1:
        raise ValueError("labels and truth must be int32 [H,W] over the same raster, with at least one pixel")
    if labels.numel() >= 1 << 31:
        raise ValueError(f"label_overlap takes rasters of fewer than 2^31 pixels, got {labels.numel()}")
    S, G = int(n_labels), int(n_truth)
    if S < 1 or G < 1 or G >= 1 << 31 or S * (G + 1) >= 1 << 62:
        raise ValueError(f"need n_labels >= 1, 1 <= n_truth < 2^31 and n_labels * (n_truth + 1) < 2^62, got {n_labels}, {n_truth}")
    labels, truth = labels.contiguous(), truth.contiguous()
    H, W = labels.shape
    # default max_cells: a region straddles a few objects; 8 S leaves room for ragged truth
    keys, counts = _count_keys(labels.device, S, max_cells, "the overlap table", "cells", lambda *table: check(
        _lib.lib().dm_label_overlap(labels.data_ptr(), truth.data_ptr(), H, W, S, G, *table, _stream()), "dm_label_overlap"))
    return _overlap_facts(keys, counts, S, G)


def pair_flags(edges: torch.Tensor, overlap: Overlap, min_purity: float = 0.6) -> torch.Tensor:
    """int8 [E] per edge of the region-adjacency graph: 1 = merge (both regions pure and owned by the same object), 0 = do not
    merge (both pure, different owners), -1 = ambiguous, not a training pair (a region whose best object holds less than
    min_purity of its area -- unlabelled pixels count against it -- or an endpoint outside [0, n_labels)).  min_purity in [0, 1],
    rounded to per-mille; the comparison is in integers."""
    _need_cuda(edges, overlap.area)
    if edges.dtype != torch.int32 or edges.dim() != 2 or edges.shape[1] != 2:
        raise ValueError("edges must be int32 [E,2]")
    if not 0.0 <= float(min_purity) <= 1.0:
        raise ValueError(f"min_purity must be in [0, 1], got {min_purity}")
    edges = edges.contiguous()
    E = edges.shape[0]
    flags = torch.empty(E, dtype=torch.int8, device=edges.device)
    check(_lib.lib().dm_pair_flags(edges.data_ptr() if E else None, E, overlap.area.data_ptr(), overlap.owner.data_ptr(),
                                   overlap.owner_count.data_ptr(), min(overlap.n_labels, (1 << 31) - 1), int(round(float(min_purity) * 1000)),
                                   flags.data_ptr() if E else None, _stream()), "dm_pair_flags")
    return flags


# ---- boundary recall / precision / F against a ground-truth raster (csrc/dm_boundary.hip; the rule: include/deepmerge_hip.h,
# DESIGN.md 3.5.17) ----
MAX_TOLERANCE = 64                    # DM_BOUNDARY_MAX_TOLERANCE: a dilation reaches the neighbouring 64-pixel word only


@dataclass
class BoundaryScores:
    """A partition's boundaries scored against a ground-truth map's at a tolerance of `tolerance` pixels (Chebyshev distance).

    The four exact integers: n_truth_b = the truth's boundary pixels, hit_truth = those with a boundary pixel of the partition
    within the tolerance, n_label_b = the partition's boundary pixels that lie on a labelled truth pixel or within the tolerance
    of a truth boundary, hit_label = those within the tolerance of a truth boundary.  A boundary pixel is one whose right or
    lower neighbour has another id (one pixel thick; the raster's frame is none).  Derived: recall = hit_truth / n_truth_b,
    precision = hit_label / n_label_b, f = 2 P R / (P + R); NaN where a figure has a zero denominator."""
    tolerance: int
    n_truth_b: int
    hit_truth: int
    n_label_b: int
    hit_label: int
    recall: float
    precision: float
    f: float


def boundary_scores_of(tolerance: int, counts) -> BoundaryScores:
    """BoundaryScores from the four count integers (Python integer arithmetic until the final divisions)."""
    n_t, h_t, n_l, h_l = (int(v) for v in counts)
    nan = float("nan")
    r = h_t / n_t if n_t else nan
    p = h_l / n_l if n_l else nan
    f = 2 * p * r / (p + r) if p + r > 0 else nan                # (a NaN operand compares false: f is NaN then)
    return BoundaryScores(int(tolerance), n_t, h_t, n_l, h_l, r, p, f)


def _tolerances(tolerance) -> Tuple[List[int], bool]:
    """(the tolerances as a list, whether a single one was given); each an integer in 0..MAX_TOLERANCE."""
    single = not isinstance(tolerance, (list, tuple))
    ds = [tolerance] if single else list(tolerance)
    for d in ds:
        if isinstance(d, bool) or not isinstance(d, int) or not 0 <= d <= MAX_TOLERANCE:
            raise ValueError(f"tolerance must be an integer in 0..{MAX_TOLERANCE} (or a sequence of them), got {d!r}")
    if not ds:
        raise ValueError("tolerance must not be an empty sequence")
    return ds, single


def _check_boundary_raster(raster: torch.Tensor, n_ids: int, name: str):
    if raster.dtype != torch.int32 or raster.dim() != 2 or raster.numel() < 1:
        raise ValueError(f"{name} must be int32 [H,W] with at least one pixel")
    if raster.numel() >= 1 << 31:
        raise ValueError(f"boundary_scores takes rasters of fewer than 2^31 pixels, got {raster.numel()}")
    if not 1 <= int(n_ids) < 1 << 31:
        raise ValueError(f"the number of ids of {name} must be in 1..2^31-1, got {n_ids}")


def _check_mapping(mapping: Optional[torch.Tensor], n_labels: int):
    if mapping is not None and (mapping.dtype != torch.int32 or tuple(mapping.shape) != (int(n_labels),)):
        raise ValueError(f"mapping must be int32 [{int(n_labels)}]")


def boundary_bits(raster: torch.Tensor, n_ids: int, mapping: Optional[torch.Tensor] = None, valid: bool = False):
    """(edge, valid or None): one bit per pixel of an int32 raster [H,W], int64 [H, ceil(W/64)] words, bit x % 64 of word
    (y, x // 64).  edge: the pixel's right or lower neighbour exists and has another canonical value (the id, or mapping[id],
    inside [0, n_ids), -1 otherwise); valid: the canonical value is >= 0.  One read of the raster (dm_boundary_bits)."""
    H, W = raster.shape
    WW = (W + 63) // 64
    edge = torch.empty((H, WW), dtype=torch.int64, device=raster.device)
    ok = torch.empty((H, WW), dtype=torch.int64, device=raster.device) if valid else None
    check(_lib.lib().dm_boundary_bits(raster.data_ptr(), H, W, int(n_ids), mapping.data_ptr() if mapping is not None else None,
                                      edge.data_ptr(), ok.data_ptr() if valid else None, _stream()), "dm_boundary_bits")
    return edge, ok


def boundary_counts(label_edge: torch.Tensor, truth_edge: torch.Tensor, truth_valid: torch.Tensor, H: int, W: int, tolerances,
                    box, counts: torch.Tensor):
    """counts int64 [T,4] += the four counts of `box` = (y0, y1, x0, x1) at every tolerance, from the bit planes of an H x W
    raster pair: one dm_boundary_counts launch per tolerance, no readback."""
    for t, d in enumerate(tolerances):
        check(_lib.lib().dm_boundary_counts(label_edge.data_ptr(), truth_edge.data_ptr(), truth_valid.data_ptr(), H, W, int(d),
                                            *(int(v) for v in box), counts[t].data_ptr(), _stream()), "dm_boundary_counts")


def _check_box(box, H: int, W: int):
    if box is None:
        return 0, H, 0, W
    y0, y1, x0, x1 = (int(v) for v in box)
    if not (0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W):
        raise ValueError(f"box = (y0, y1, x0, x1) must be a non-empty box inside the raster, got {tuple(box)} of {H} x {W}")
    return y0, y1, x0, x1


def boundary_scores(labels: torch.Tensor, truth: torch.Tensor, n_labels: int, n_truth: int, tolerance=2,
                    mapping: Optional[torch.Tensor] = None, box=None):
    """Boundary recall, precision and F of a label raster (region ids 0..n_labels-1) against a ground-truth raster (object ids
    0..n_truth-1, any other value = unlabelled) at a tolerance of `tolerance` pixels, 0..64 (the rule: include/deepmerge_hip.h).

    tolerance: an integer -> a BoundaryScores; a list or tuple -> a list of them (the bits of both rasters are made once, one
    count pass per tolerance).  mapping int32 [n_labels]: scores the partition mapping[labels] -- the `region_of` or
    `region_of_at(r)` of a MergeResult -- without building its raster (a negative entry means "no region").  box = (y0, y1, x0,
    x1): count the boundary pixels inside the box only; what they match may lie anywhere in the raster.  One read of each raster;
    one readback (the counts).  The inputs are not modified."""
    _need_cuda(labels, truth)
    _check_boundary_raster(labels, n_labels, "labels")
    _check_boundary_raster(truth, n_truth, "truth")
    if labels.shape != truth.shape:
        raise ValueError("labels and truth must cover the same raster")
    _check_mapping(mapping, n_labels)
    if mapping is not None:
        _need_cuda(mapping)
        mapping = mapping.contiguous()
    ds, single = _tolerances(tolerance)
    H, W = labels.shape
    box = _check_box(box, H, W)
    label_edge, _ = boundary_bits(labels.contiguous(), n_labels, mapping)
    truth_edge, truth_valid = boundary_bits(truth.contiguous(), n_truth, valid=True)
    counts = torch.zeros((len(ds), 4), dtype=torch.int64, device=labels.device)
    boundary_counts(label_edge, truth_edge, truth_valid, H, W, ds, box, counts)
    out = [boundary_scores_of(d, c) for d, c in zip(ds, counts.tolist())]         # the one readback
    return out[0] if single else out


# ---- SLIC superpixels and 4-connected components (csrc/dm_slic.hip; the rule: include/deepmerge_hip.h) ---------
def _connected_labels(raster: torch.Tensor, background: Optional[int]) -> Tuple[torch.Tensor, int, torch.Tensor]:
    """`connected_labels` and the call's parent table, int32 [H*W]: a component's root is its first pixel (scene._components)."""
    _need_cuda(raster)
    if raster.dtype != torch.int32 or raster.dim() != 2 or raster.numel() < 1:
        raise ValueError("raster must be int32 [H,W] with at least one pixel")
    if raster.numel() >= 1 << 31:
        raise ValueError(f"connected_labels takes rasters of fewer than 2^31 pixels, got {raster.numel()}")
    if background is not None and not -(1 << 31) <= int(background) < 1 << 31:
        raise ValueError(f"background must be an int32 value or None, got {background}")
    raster = raster.contiguous()
    H, W = raster.shape
    dev, i32 = raster.device, torch.int32
    parent = torch.empty(H * W, dtype=i32, device=dev)
    chunks = torch.empty((H * W + 4095) // 4096 + 1, dtype=i32, device=dev)
    labels = torch.empty((H, W), dtype=i32, device=dev)
    n = torch.empty(1, dtype=i32, device=dev)
    check(_lib.lib().dm_connected_labels(raster.data_ptr(), H, W, int(background is not None), int(background or 0), parent.data_ptr(),
                                         chunks.data_ptr(), labels.data_ptr(), n.data_ptr(), _stream()), "dm_connected_labels")
    return labels, int(n), parent


def connected_labels(raster: torch.Tensor, background: Optional[int] = None) -> Tuple[torch.Tensor, int]:
    """(labels int32 [H,W], n): the 4-connected components of equal values of an int32 raster, numbered 0..n-1 in the order of
    their first pixel in raster-scan order.  Pixels equal to `background` get -1 and belong to no component (a class raster's
    "no object" value).  The input is not modified.  One readback (n)."""
    return _connected_labels(raster, background)[:2]


def _slic_params(cell: int, compactness: int, iters: int, min_size: Optional[int]) -> int:
    """The ranges of the rule's parameters, for a tile and for a scene; returns min_size with its default, its range left to the caller."""
    if not 4 <= int(cell) <= 256:
        raise ValueError(f"cell must be in 4..256, got {cell}")
    if not 0 <= int(compactness) <= 255:
        raise ValueError(f"compactness must be in 0..255, got {compactness}")
    if int(iters) < 0:
        raise ValueError(f"iters must be >= 0, got {iters}")
    return max(1, int(cell) * int(cell) // 4) if min_size is None else int(min_size)


def _check_slic(tile: torch.Tensor, cell: int, compactness: int, iters: int, min_size: Optional[int]) -> int:
    _need_cuda(tile)
    if tile.dtype != torch.uint8 or tile.dim() != 3 or tile.numel() < 1:
        raise ValueError("tile must be uint8 [bands,H,W] with at least one band and one pixel")
    if tile.shape[1] * tile.shape[2] >= 1 << 31:
        raise ValueError(f"slic takes rasters of fewer than 2^31 pixels, got {tile.shape[1] * tile.shape[2]}")
    min_size = _slic_params(cell, compactness, iters, min_size)
    if min_size < 1:
        raise ValueError(f"min_size must be >= 1, got {min_size}")
    return min_size


def slic_assign(tile: torch.Tensor, cell: int = 29, compactness: int = 10, iters: int = 10) -> Tuple[torch.Tensor, torch.Tensor]:
    """Steps 1-3 of the SLIC rule: (centre id of every pixel int32 [H,W], final centres int32 [K,6] = y, x, band 0..3).  One call,
    no readback: assignment, then `iters` times (update, assignment)."""
    _check_slic(tile, cell, compactness, iters, None)
    tile = tile.contiguous()
    bands, H, W = tile.shape
    K = ((H + cell - 1) // cell) * ((W + cell - 1) // cell)
    dev = tile.device
    centres = torch.empty((K, 6), dtype=torch.int32, device=dev)
    sums = torch.empty((K, 7), dtype=torch.int64, device=dev)
    labels = torch.empty((H, W), dtype=torch.int32, device=dev)
    check(_lib.lib().dm_slic_iterate(tile.data_ptr(), bands, H, W, int(cell), int(compactness), int(iters), centres.data_ptr(),
                                     sums.data_ptr(), labels.data_ptr(), _stream()), "dm_slic_iterate")
    return labels, centres


def label_area(labels: torch.Tensor, n_labels: int) -> torch.Tensor:
    """int32 [n_labels]: pixels of every id 0..n_labels-1 (other ids are ignored)."""
    _need_cuda(labels)
    if labels.dtype != torch.int32 or labels.dim() != 2 or labels.numel() < 1 or labels.numel() >= 1 << 31 or n_labels < 1:
        raise ValueError("labels must be int32 [H,W] with 1 <= H*W < 2^31 pixels, and n_labels >= 1")
    labels = labels.contiguous()
    area = torch.empty(int(n_labels), dtype=torch.int32, device=labels.device)
    check(_lib.lib().dm_label_area(labels.data_ptr(), labels.shape[0], labels.shape[1], int(n_labels), area.data_ptr(), _stream()),
          "dm_label_area")
    return area


def _absorb_round(edges: torch.Tensor, weights: torch.Tensor, area: torch.Tensor, n: int, min_size: int):
    """One absorption round on a graph of n regions (int32 edges [E,2], weights [E], areas [n]): one 64-bit max per small region
    (dm_slic_absorb_pick), merge_components over the picked edges, the dense renumbering.  Returns (step int64 [n]: region ->
    0..n_new-1, n_new, picked edges), or None when nothing was picked (no edge, or no small region).  The numbering keeps the
    order: a united region's first pixel is that of its smallest member."""
    E, dev = edges.shape[0], edges.device
    if E == 0:
        return None
    best = torch.empty(n, dtype=torch.int64, device=dev)
    merge = torch.empty(E, dtype=torch.uint8, device=dev)
    picked = torch.empty(1, dtype=torch.int32, device=dev)
    check(_lib.lib().dm_slic_absorb_pick(edges.data_ptr(), weights.data_ptr(), E, area.data_ptr(), n, int(min_size), best.data_ptr(),
                                         merge.data_ptr(), picked.data_ptr(), _stream()), "dm_slic_absorb_pick")
    picked = int(picked)
    if picked == 0:
        return None
    root = merge_components(edges, merge, n).long()
    dense = torch.cumsum((root == torch.arange(n, device=dev)).to(torch.int64), 0) - 1
    return dense[root], int(dense[-1]) + 1, picked


def absorb_small(labels: torch.Tensor, n_labels: int, min_size: int, on_round=None) -> Tuple[torch.Tensor, int, int]:
    """Step 5 of the SLIC rule on a raster of connected regions 0..n_labels-1 numbered by first pixel: (labels, n, rounds).
    Per round: rag_edges, one `_absorb_round`, relabel_raster; the areas are folded, not recounted.  A few small readbacks per
    round, as merge_regions has them.
    on_round(round): called before every round (tools/mb_slic.py times the rounds with it)."""
    n, rounds, dev = int(n_labels), 0, labels.device
    area = label_area(labels, n)
    while n > 1:
        if on_round is not None:
            on_round(rounds)
        edges, weights = rag_edges(labels, n)
        got = _absorb_round(edges, weights, area, n, min_size)
        if got is None:
            break
        mapping, n, _ = got
        area = torch.zeros(n, dtype=torch.int32, device=dev).index_add_(0, mapping, area)
        labels = relabel_raster(labels, mapping.to(torch.int32))
        rounds += 1
    return labels, n, rounds


def slic(tile: torch.Tensor, cell: int = 29, compactness: int = 10, iters: int = 10, min_size: Optional[int] = None) -> Tuple[torch.Tensor, int]:
    """SLIC superpixels of an image tile (uint8 [bands,H,W], the first four bands are used): (labels int32 [H,W], n_labels), the
    label raster every other call of this module starts from.  cell: the grid step, about the side of a superpixel (4..256);
    compactness 0..255 weighs position against colour; iters: update rounds; min_size (default max(1, cell*cell // 4)): connected
    regions smaller than this are absorbed into the neighbour they share the longest boundary with.  Regions are 4-connected and
    numbered by first pixel.  Integer arithmetic throughout: the same input gives the same raster on every run (the rule:
    include/deepmerge_hip.h, restated in numpy in tests/slic_ref.py)."""
    min_size = _check_slic(tile, cell, compactness, iters, min_size)
    assigned, _ = slic_assign(tile, cell, compactness, iters)
    labels, n = connected_labels(assigned)
    labels, n, _ = absorb_small(labels, n, min_size)
    return labels, n


# ---- polygon rings and boundary arcs (csrc/dm_vector.hip; the rule: include/deepmerge_hip.h) ---------------------
MAX_TRACE_PIXELS = 1 << 28        # dart ids 4 (y W + x) + side and the packed 64-bit keys stay below 2^30


@dataclass
class Polygons:
    """What `polygons` leaves: the closed rings of every label, rings sorted by (label, smallest dart id).

    region_ptr int32 [n_labels+1]: the rings of each label (an empty range for an absent id); ring_ptr int64 [R+1] into xy;
    xy int32 [V,2]: corners (x, y), y down, a ring is not closed by repeating its first vertex; ring_label int32 [R];
    ring_area2 int64 [R]: the shoelace sum, positive for an outer ring and negative for a hole."""
    region_ptr: torch.Tensor
    ring_ptr: torch.Tensor
    xy: torch.Tensor
    ring_label: torch.Tensor
    ring_area2: torch.Tensor


@dataclass
class Arcs:
    """What `boundary_arcs` leaves: one polyline per stretch of boundary between two labels, sorted by (right, left, first dart).

    arc_ptr int64 [A+1] into xy; xy int32 [Va,2] (a closed arc repeats its first vertex at the end); right int32 [A]: the label on
    the arc's right, left int32 [A]: the label on its left, greater than `right`, or -1 for the outside of the raster; edge int32
    [A] or None: the row of (right, left) in the `edges` given (as rag_edges returns them), -1 for left == -1."""
    arc_ptr: torch.Tensor
    xy: torch.Tensor
    left: torch.Tensor
    right: torch.Tensor
    edge: Optional[torch.Tensor] = None


def _jump(call, bufs, D: int, changed: torch.Tensor, what: str, max_rounds: int = 32):
    """Pointer-jumping rounds between two buffer sets (read one, write the other) until the device flag stays 0, as
    merge_components repeats its rounds.  Returns (the set that holds the result, rounds run)."""
    for r in range(max_rounds):
        src, dst = bufs[r & 1], bufs[1 - (r & 1)]
        check(call(src[0].data_ptr(), src[1].data_ptr(), dst[0].data_ptr(), dst[1].data_ptr(), D, changed.data_ptr(), _stream()), what)
        if int(changed.item()) == 0:
            return dst, r + 1
    raise RuntimeError(f"{what} did not converge in {max_rounds} rounds")


def _trace_table(dart: torch.Tensor, nxt0: torch.Tensor, lab: torch.Tensor, other: torch.Tensor, flags: torch.Tensor, key0: torch.Tensor,
                 W: int, S: int, mark=lambda stage: None, wide: bool = False) -> Tuple[Polygons, Arcs, dict]:
    """From a linked dart table (dart ids, successor slots, labels, flags, key = head candidate << 32 | slot) to both results: the
    jumping rounds, the ring and arc tables, the two emits.  wide: the table of a scene (scene.trace_labels) -- dart int64 in
    ascending order, key = slot << 32 | slot, W up to 2^31 - 2; the emits are the 64-bit ones and an arc's first dart is known by
    its slot.  Returns (Polygons, Arcs, counts for the callers' stats)."""
    lib, dev, i32, i64, D = _lib.lib(), dart.device, torch.int32, torch.int64, int(dart.numel())
    new = lambda n, dt: torch.empty(n, dtype=dt, device=dev)
    keys, jumps = (key0, new(D, i64)), (nxt0, new(D, i32), new(D, i32))
    changed = new(1, i32)
    # heads: round 0 reads (keys[0], next) and writes (keys[1], jumps[1]); `next` itself is never written again
    check(lib.dm_vector_head_round(keys[0].data_ptr(), nxt0.data_ptr(), keys[1].data_ptr(), jumps[1].data_ptr(), D, changed.data_ptr(),
                                   _stream()), "dm_vector_head_round")
    key, head_rounds = keys[1], 1
    if int(changed.item()):
        (key, _), more = _jump(lib.dm_vector_head_round, [(keys[1], jumps[1]), (keys[0], jumps[2])], D, changed, "dm_vector_head_round")
        head_rounds += more
    del jumps
    mark("head rounds")
    # ranks
    max_rings = D // 4 + 1
    sums, nxts = (new(D, i64), new(D, i64)), (new(D, i32), new(D, i32))
    ring_key, ring_slot, n_rings = new(max_rings, i64), new(max_rings, i32), new(1, i32)
    check(lib.dm_vector_rank_init(key.data_ptr(), nxt0.data_ptr(), flags.data_ptr(), lab.data_ptr(), D, sums[0].data_ptr(), nxts[0].data_ptr(),
                                  ring_key.data_ptr(), ring_slot.data_ptr(), n_rings.data_ptr(), max_rings, _stream()), "dm_vector_rank_init")
    (total, _), rank_rounds = _jump(lib.dm_vector_rank_round, [(sums[0], nxts[0]), (sums[1], nxts[1])], D, changed, "dm_vector_rank_round")
    R = int(n_rings)
    mark("rank rounds")
    # rings in (label, head) order; the tables over rings and arcs are small next to the darts
    ring_key, order = torch.sort(ring_key[:R])
    ring_slot = ring_slot[:R][order].long()
    ring_of_slot = new(D, i32)
    ring_of_slot[ring_slot] = torch.arange(R, dtype=i32, device=dev)
    ring_total = total[ring_slot]
    ring_ptr = torch.zeros(R + 1, dtype=i64, device=dev)
    ring_ptr[1:] = torch.cumsum(ring_total >> 32, 0)
    arc_base = torch.zeros(R + 1, dtype=i64, device=dev)
    arc_base[1:] = torch.cumsum(torch.clamp(ring_total & 0xffffffff, min=1), 0)
    V, n_arcs = (int(v) for v in torch.stack((ring_ptr[-1], arc_base[-1])).tolist())
    arc_base = arc_base.to(i32)
    xy, area2 = new((V, 2), i32), new(R, i64)
    arc_first, arc_left, arc_right, arc_vstart, arc_count = (new(n_arcs, i32) for _ in range(5))
    t = _lib.DmSceneVectorTrace() if wide else _lib.DmVectorTrace()
    ring_name, arc_name = ("dm_scene_vector_ring_emit", "dm_scene_vector_arc_emit") if wide else ("dm_vector_ring_emit", "dm_vector_arc_emit")
    for name, tensor in (("dart", dart), ("next", nxt0), ("lab", lab), ("other", other), ("flags", flags), ("key", key), ("sum", total),
                         ("ring_of_slot", ring_of_slot), ("ring_ptr", ring_ptr), ("arc_base", arc_base), ("xy", xy), ("area2", area2),
                         ("arc_first", arc_first), ("arc_left", arc_left), ("arc_right", arc_right), ("arc_vstart", arc_vstart),
                         ("arc_count", arc_count)):
        setattr(t, name, tensor.data_ptr())
    t.W, t.D, t.R, t.n_arcs = W, D, R, n_arcs
    check(getattr(lib, ring_name)(ctypes.byref(t), _stream()), ring_name)
    ring_label = (ring_key >> 32).to(i32)
    region_ptr = torch.zeros(S + 1, dtype=i64, device=dev)
    region_ptr[1:] = torch.cumsum(torch.bincount(ring_label.long(), minlength=S), 0)
    polys = Polygons(region_ptr=region_ptr.to(i32), ring_ptr=ring_ptr, xy=xy, ring_label=ring_label, ring_area2=area2)
    mark("ring tables (sort, scans) + ring_emit")
    # arcs: keep one side of every boundary, order by (right, left, first dart) in two stable passes
    kept = torch.nonzero((arc_left < 0) | (arc_left > arc_right)).squeeze(1)
    # left + 1 < 2^31; one raster: dart ids < 2^30; a scene: arc_first is the slot, < 2^31, and slot order is dart-id order
    low = ((arc_left[kept].long() + 1) << (31 if wide else 30)) | arc_first[kept].long()
    by_low = torch.argsort(low)
    by_right = torch.argsort(arc_right[kept][by_low], stable=True)
    kept = kept[by_low][by_right]
    A = kept.numel()
    arc_pos = torch.full((n_arcs,), -1, dtype=i32, device=dev)
    arc_pos[kept] = torch.arange(A, dtype=i32, device=dev)
    arc_ptr = torch.zeros(A + 1, dtype=i64, device=dev)
    arc_ptr[1:] = torch.cumsum(arc_count[kept].long(), 0)
    arc_xy = new((int(arc_ptr[-1]), 2), i32)
    t.arc_pos, t.arc_ptr, t.arc_xy = arc_pos.data_ptr(), arc_ptr.data_ptr(), arc_xy.data_ptr()
    check(getattr(lib, arc_name)(ctypes.byref(t), _stream()), arc_name)
    arcs = Arcs(arc_ptr=arc_ptr, xy=arc_xy, left=arc_left[kept], right=arc_right[kept])
    mark("arc tables (two sorts, scan) + arc_emit")
    return polys, arcs, dict(D=D, R=R, A=A, V=V, head_rounds=head_rounds, rank_rounds=rank_rounds, arc_xy=arc_xy)


def _trace(labels: torch.Tensor, n_labels: int, stats: Optional[dict] = None) -> Tuple[Polygons, Arcs]:
    """One tracing run for both results.  Readbacks: the label range, the number of darts D (it sizes everything that follows, so
    there is no max_ parameter), one flag per jumping round, the numbers of rings, vertices and arcs.  stats: a dict that receives
    D, the rounds, the time per stage and the bytes of the passes (tools/mb_vector.py)."""
    _need_cuda(labels)
    if labels.dtype != torch.int32 or labels.dim() != 2 or labels.numel() < 1:
        raise ValueError("labels must be int32 [H,W] with at least one pixel")
    if labels.numel() > MAX_TRACE_PIXELS:
        raise ValueError(f"polygons / boundary_arcs take rasters of at most 2^28 pixels, got {labels.numel()}")
    S = int(n_labels)
    if not 1 <= S < 1 << 31:
        raise ValueError(f"n_labels must be in 1..2^31-1, got {n_labels}")
    labels = labels.contiguous()
    lo, hi = (int(v) for v in torch.aminmax(labels))
    if lo < 0 or hi >= S:
        raise ValueError(f"labels must be in 0..n_labels-1 = 0..{S - 1}, found {lo}..{hi}")
    H, W = labels.shape
    dev, lib, i32, i64 = labels.device, _lib.lib(), torch.int32, torch.int64
    new = lambda n, dt: torch.empty(n, dtype=dt, device=dev)
    marks = []

    def mark(stage):                                             # stage boundaries for tools/mb_vector.py; nothing when stats is None
        if stats is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((stage, e))
    mark("start")
    tiles = ((H + 63) // 64) * ((W + 63) // 64)
    mask, tile_off, meta = new(H * W, torch.uint8), new(tiles + 1, i32), new(2, i32)
    check(lib.dm_vector_count(labels.data_ptr(), H, W, mask.data_ptr(), tile_off.data_ptr(), meta.data_ptr(), _stream()), "dm_vector_count")
    D = int(meta[0])
    mark("count + scan + readback of D")
    first_slot, dart = new(H * W, i32), new(D, i32)
    check(lib.dm_vector_emit(mask.data_ptr(), tile_off.data_ptr(), H, W, first_slot.data_ptr(), dart.data_ptr(), _stream()), "dm_vector_emit")
    nxt0, lab, other, flags = new(D, i32), new(D, i32), new(D, i32), new(D, torch.uint8)
    key0 = new(D, i64)
    check(lib.dm_vector_link(labels.data_ptr(), mask.data_ptr(), first_slot.data_ptr(), dart.data_ptr(), H, W, D, nxt0.data_ptr(),
                             lab.data_ptr(), other.data_ptr(), flags.data_ptr(), key0.data_ptr(), _stream()), "dm_vector_link")
    mark("emit + link")
    polys, arcs, info = _trace_table(dart, nxt0, lab, other, flags, key0, W, S, mark)
    D, R, A, V, head_rounds, rank_rounds, arc_xy = (info[k] for k in ("D", "R", "A", "V", "head_rounds", "rank_rounds", "arc_xy"))
    if stats is not None:
        torch.cuda.synchronize()
        stats["stage_ms"] = [(b[0], a[1].elapsed_time(b[1])) for a, b in zip(marks[:-1], marks[1:])]
        # bytes read + written by the passes over the raster and over the darts (the ring and arc tables are small beside them)
        raster = H * W * (4 + 3 * 4 + 1) + H * W * (1 + 4) + 4 * D
        link = D * (17 + 25)
        rounds = (head_rounds + rank_rounds) * D * (24 + 12)
        emit = D * (33 + 30) + 8 * (V + arc_xy.shape[0])
        stats.update(D=D, rings=R, arcs=A, vertices=V, arc_vertices=int(arc_xy.shape[0]), head_rounds=head_rounds, rank_rounds=rank_rounds,
                     bytes=raster + link + rounds + emit)
    return polys, arcs


def polygons(labels: torch.Tensor, n_labels: int) -> Polygons:
    """The closed rings of every label of an int32 raster with ids 0..n_labels-1 (a label need not be connected, an id may be
    absent; any other value raises).  H*W <= 2^28.  The rule: include/deepmerge_hip.h, restated in numpy in tests/vector_ref.py; every
    array is bit-equal to it.  The input is not modified."""
    return _trace(labels, n_labels)[0]


def _attach_edges(arcs: Arcs, n_labels: int, edges: torch.Tensor) -> Arcs:
    """Arcs.edge: the row of every arc's (right, left) pair in `edges`, -1 for left == -1."""
    _need_cuda(edges)
    if edges.dtype != torch.int32 or edges.dim() != 2 or edges.shape[1] != 2:
        raise ValueError("edges must be int32 [E,2]")
    S, inner = int(n_labels), arcs.left >= 0
    edge = torch.full_like(arcs.left, -1)
    if bool(inner.any()):
        if edges.shape[0] == 0:
            raise ValueError("boundary_arcs: the raster has boundaries between labels, but `edges` is empty")
        ekeys = edges[:, 0].long() * S + edges[:, 1].long()
        akeys = arcs.right.long()[inner] * S + arcs.left.long()[inner]
        row = torch.searchsorted(ekeys, akeys).clamp(max=ekeys.numel() - 1)
        if not bool((ekeys[row] == akeys).all()):
            raise ValueError("boundary_arcs: an arc's (right, left) pair is not a row of `edges` (pass rag_edges of the same raster)")
        edge[inner] = row.to(torch.int32)
    arcs.edge = edge
    return arcs


def boundary_arcs(labels: torch.Tensor, n_labels: int, edges: Optional[torch.Tensor] = None) -> Arcs:
    """The boundary arcs of the same tracing run: every unit boundary lies in exactly one arc.  edges int32 [E,2], sorted by (a, b)
    (rag_edges of the same raster): `Arcs.edge` gets the row of every arc's (right, left) pair; a pair that is not in `edges`
    raises."""
    arcs = _trace(labels, n_labels)[1]
    return arcs if edges is None else _attach_edges(arcs, n_labels, edges)


# ---- shared-boundary Douglas-Peucker (csrc/dm_simplify.hip; the rule: include/deepmerge_hip.h) ----------------------
MAX_SIMPLIFY_SIDE = 1 << 15       # DM_SIMPLIFY_MAX_SIDE: every cross product of two corner differences stays below 2^31
MAX_SIMPLIFY_Q = 1 << 20          # DM_SIMPLIFY_MAX_Q: the tolerance in 1/256 pixel


def _quantise_tolerance(tolerance: float) -> int:
    """q = floor(256 t + 0.5) of a tolerance in pixels: finite, >= 0, at most 4096 (rag.simplify, scene.simplify_labels)."""
    t = float(tolerance)
    if not math.isfinite(t) or t < 0:
        raise ValueError(f"tolerance must be finite and >= 0, got {tolerance}")
    q = int(math.floor(t * SUBPIXEL + 0.5))
    if q > MAX_SIMPLIFY_Q:
        raise ValueError(f"tolerance must be at most {MAX_SIMPLIFY_Q // SUBPIXEL} pixels, got {tolerance}")
    return q


def _simplify(labels: torch.Tensor, n_labels: int, tolerance: float, stats: Optional[dict] = None, topology: bool = False,
              max_rounds: int = 64, conflicts_only: bool = False):
    """`simplify` and the keep flags uint8 [(H+1)(W+1)] (2 node, 1 kept chain vertex, 0 otherwise) it decided by.  topology: the
    repair rounds of `_TopologyRounds` run between the chain pass and the count.  conflicts_only: the `Conflicts` of the plain
    keep flags instead."""
    _need_cuda(labels)
    if labels.dtype != torch.int32 or labels.dim() != 2 or labels.numel() < 1:
        raise ValueError("labels must be int32 [H,W] with at least one pixel")
    H, W = labels.shape
    if H > MAX_SIMPLIFY_SIDE or W > MAX_SIMPLIFY_SIDE:
        raise ValueError(f"simplify takes rasters of at most 32768 x 32768 pixels, got {H} x {W}")
    q = _quantise_tolerance(tolerance)
    trace_stats = None if stats is None else {}
    polys, arcs = _trace(labels, n_labels, trace_stats)
    labels = labels.contiguous()
    dev, lib, i32, i64 = labels.device, _lib.lib(), torch.int32, torch.int64
    new = lambda n, dt: torch.empty(n, dtype=dt, device=dev)
    marks = []

    def mark(stage):                                             # stage boundaries for tools/mb_simplify.py; nothing when stats is None
        if stats is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((stage, e))
    mark("start")
    A, Va = arcs.left.numel(), arcs.xy.shape[0]
    R, V = polys.ring_label.numel(), polys.xy.shape[0]
    keep = new((H + 1) * (W + 1), torch.uint8)
    check(lib.dm_simplify_nodes(labels.data_ptr(), H, W, keep.data_ptr(), _stream()), "dm_simplify_nodes")
    mark("nodes")
    stack = new(Va, i64)                                         # one entry per arc vertex: the bound of the depth-first walk
    check(lib.dm_simplify_chains(arcs.xy.data_ptr(), arcs.arc_ptr.data_ptr(), A, Va, H, W, q, keep.data_ptr(), stack.data_ptr(), _stream()),
          "dm_simplify_chains")
    del stack
    mark("chains")
    if conflicts_only:
        return _TopologyRounds(arcs, keep, H, W, q).conflicts()
    if topology:
        rounds = _TopologyRounds(arcs, keep, H, W, q)
        flagged = rounds.repair(max_rounds, stats is not None)
        mark("topology rounds")
    arc_count, ring_count = new(A, i32), new(V, i32)
    check(lib.dm_simplify_arc_count(arcs.xy.data_ptr(), arcs.arc_ptr.data_ptr(), A, Va, H, W, keep.data_ptr(), arc_count.data_ptr(), _stream()),
          "dm_simplify_arc_count")
    vert_ring = (torch.searchsorted(polys.ring_ptr, torch.arange(V, dtype=i64, device=dev), right=True) - 1).to(i32)
    check(lib.dm_simplify_ring_count(polys.xy.data_ptr(), polys.ring_ptr.data_ptr(), vert_ring.data_ptr(), V, R, H, W, keep.data_ptr(),
                                     ring_count.data_ptr(), _stream()), "dm_simplify_ring_count")
    arc_ptr, scan = torch.zeros(A + 1, dtype=i64, device=dev), torch.zeros(V + 1, dtype=i64, device=dev)
    torch.cumsum(arc_count, 0, dtype=i64, out=arc_ptr[1:])
    torch.cumsum(ring_count, 0, dtype=i64, out=scan[1:])
    ring_ptr = scan[polys.ring_ptr]
    Van, Vn = (int(v) for v in torch.stack((arc_ptr[-1], scan[-1])).tolist())            # the one readback: the vertex totals
    mark("arc_count + ring_count + scans + readback of the totals")
    arc_xy, xy, area2 = new((Van, 2), i32), new((Vn, 2), i32), new(R, i64)
    check(lib.dm_simplify_arc_emit(arcs.xy.data_ptr(), arcs.arc_ptr.data_ptr(), arc_ptr.data_ptr(), A, Va, Van, H, W, keep.data_ptr(),
                                   arc_xy.data_ptr(), _stream()), "dm_simplify_arc_emit")
    check(lib.dm_simplify_ring_emit(polys.xy.data_ptr(), polys.ring_ptr.data_ptr(), vert_ring.data_ptr(), scan.data_ptr(), ring_ptr.data_ptr(), V, R,
                                    Vn, H, W, keep.data_ptr(), xy.data_ptr(), area2.data_ptr(), _stream()), "dm_simplify_ring_emit")
    mark("arc_emit + ring_emit + area")
    out_polys = Polygons(region_ptr=polys.region_ptr, ring_ptr=ring_ptr, xy=xy, ring_label=polys.ring_label, ring_area2=area2)
    out_arcs = Arcs(arc_ptr=arc_ptr, xy=arc_xy, left=arcs.left, right=arcs.right)
    if stats is not None:
        torch.cuda.synchronize()
        stats["stage_ms"] = [(b[0], a[1].elapsed_time(b[1])) for a, b in zip(marks[:-1], marks[1:])]
        stats.update(trace=trace_stats, q=q, arcs=A, rings=R, arc_vertices=Va, vertices=V, kept_arc_vertices=Van, kept_vertices=Vn,
                     longest_arc=int((arcs.arc_ptr[1:] - arcs.arc_ptr[:-1]).max()))
        if topology:
            stats.update(topology_rounds=len(flagged) - 1, topology_flagged=flagged, topology_stage_ms=rounds.stage_ms,
                         topology_segments=rounds.n_segments, topology_cell_entries=rounds.cell_entries)
    return out_polys, out_arcs, keep


@dataclass
class Conflicts:
    """The segments of a plain `simplify` that the topology rule flags, sorted by arc, then along the arc.

    arc int32 [n] (the arc of `boundary_arcs` / `simplify`); xy int32 [n,4] = the two ends (x0, y0, x1, y1) in arc order; kind
    uint8 [n]: bit 1 the segment meets another one or is degenerate, bit 2 it jumped over a fixed point; n_segments: all segments
    of the simplified scene, flagged or not."""
    arc: torch.Tensor
    xy: torch.Tensor
    kind: torch.Tensor
    n_segments: int


class _TopologyRounds:
    """The detection and repair rounds of csrc/dm_simplify_topology.hip on the keep flags of one `_simplify` call: the arrays, the
    struct the entries take, and the table arithmetic between them (the scans are torch.cumsum, as everywhere in this file).
    scene._SceneTopologyRounds binds the same rounds to the scene form of the entries: what differs is named here, once."""
    STAGES = ("segment table", "binning", "pair tests", "jump tests", "refine")
    STRUCT, PREFIX, KEEP = _lib.DmSimplifyTopology, "dm_simplify_topology_", "keep"        # the struct, its entries, its keep field

    def __init__(self, arcs: Arcs, keep: torch.Tensor, H: int, W: int, q: int, cap: Optional[int] = None, **fields):
        dev, i32, i64 = keep.device, torch.int32, torch.int64
        self.lib, self.arcs, self.keep = _lib.lib(), arcs, keep
        self.A, self.Va, self.H, self.W = arcs.left.numel(), arcs.xy.shape[0], H, W
        cells = self._cells(**fields)
        new = lambda n, dt: torch.empty(n, dtype=dt, device=dev)
        self.count, self.new_ptr = new(self.A, i32), torch.zeros(self.A + 1, dtype=i64, device=dev)
        self.point_count, self.point_fill, self.point_ptr = new(cells, i32), new(cells, i32), torch.zeros(cells + 1, dtype=i64, device=dev)
        self.point_xy = new((self.Va, 2), i32)
        self.seg, self.kind = torch.full((self.Va, 4), -1, dtype=i32, device=dev), new(self.Va, i32)
        self.cell_count, self.cell_fill, self.cell_ptr = new(cells, i32), new(cells, i32), torch.zeros(cells + 1, dtype=i64, device=dev)
        self.cell_seg = new(max(2 * self.Va, 1024) if cap is None else int(cap), i32)         # grows when a round needs more (status[2])
        self.stack, self.status = None, new(4, i32)
        self.t = self.STRUCT(arc_xy=arcs.xy.data_ptr(), arc_ptr=arcs.arc_ptr.data_ptr(), new_ptr=self.new_ptr.data_ptr(),
                             point_count=self.point_count.data_ptr(), point_fill=self.point_fill.data_ptr(),
                             point_ptr=self.point_ptr.data_ptr(), point_xy=self.point_xy.data_ptr(), seg=self.seg.data_ptr(),
                             kind=self.kind.data_ptr(), cell_count=self.cell_count.data_ptr(), cell_fill=self.cell_fill.data_ptr(),
                             cell_ptr=self.cell_ptr.data_ptr(), cell_seg=self.cell_seg.data_ptr(), stack=None,
                             status=self.status.data_ptr(), Va=self.Va, cap=self.cell_seg.numel(), A=self.A, H=H, W=W, q=q,
                             **{self.KEEP: keep.data_ptr()}, **fields)
        self.stage_ms, self.n_segments, self.cell_entries = [], 0, 0
        self._call("point_count")
        torch.cumsum(self.point_count, 0, dtype=i64, out=self.point_ptr[1:])
        self._call("point_fill")

    def _cells(self) -> int:
        return ((self.H >> 5) + 1) * ((self.W >> 5) + 1)          # DM_SIMPLIFY_TOPOLOGY_CELL_LOG2

    def _arc_count(self):
        a = self.arcs
        check(self.lib.dm_simplify_arc_count(a.xy.data_ptr(), a.arc_ptr.data_ptr(), self.A, self.Va, self.H, self.W, self.keep.data_ptr(),
                                             self.count.data_ptr(), _stream()), "dm_simplify_arc_count")

    def _call(self, name, *args):
        check(getattr(self.lib, self.PREFIX + name)(ctypes.byref(self.t), *args, _stream()), self.PREFIX + name)

    def _round(self, apply: bool, timed: bool):
        """One round on the current keep: (flagged, flagged with interior vertices).  One readback: the status words."""
        while True:
            marks = []

            def mark():
                if timed:
                    e = torch.cuda.Event(enable_timing=True)
                    e.record()
                    marks.append(e)
            mark()
            self._arc_count()
            torch.cumsum(self.count, 0, dtype=torch.int64, out=self.new_ptr[1:])
            self._call("segments")
            mark()
            self._call("bin_count")
            torch.cumsum(self.cell_count, 0, dtype=torch.int64, out=self.cell_ptr[1:])
            self._call("bin_fill")
            mark()
            self._call("pairs")
            mark()
            self._call("jumps")
            mark()
            self._call("refine", 1 if apply else 0)
            mark()
            flagged, inner, need, _ = self.status.tolist()
            if need <= self.t.cap:
                break
            self.cell_seg = torch.empty(need, dtype=torch.int32, device=self.keep.device)       # nothing was kept: the round again
            self.t.cell_seg, self.t.cap = self.cell_seg.data_ptr(), need
        if timed:                                                  # per round: stage -> ms (the readback above has synchronised)
            self.stage_ms.append({stage: e0.elapsed_time(e1) for stage, e0, e1 in zip(self.STAGES, marks[:-1], marks[1:])})
        self.cell_entries = need
        return flagged, inner

    def repair(self, max_rounds: int, timed: bool = False):
        """Rounds until no segment is flagged: the flagged-segment count of every round (the last is 0)."""
        self.stack = torch.empty(2 * self.Va, dtype=torch.int64, device=self.keep.device)
        self.t.stack = self.stack.data_ptr()
        counts = []
        while True:
            flagged, inner = self._round(True, timed)
            counts.append(flagged)
            if flagged == 0:
                self.n_segments = int(self.new_ptr[-1]) - self.A if timed else 0
                return counts
            if inner == 0:
                raise RuntimeError(f"simplify: {flagged} conflicting segments have no vertex left to restore (round {len(counts)})")
            if len(counts) > max_rounds:
                raise RuntimeError(f"simplify: conflicts remain after {max_rounds} repair rounds ({flagged} segments)")

    def conflicts(self) -> Conflicts:
        self._round(False, False)
        Vn = int(self.new_ptr[-1])
        hit = torch.nonzero(self.kind[:Vn]).reshape(-1)
        seg = self.seg[:Vn + 1]
        return Conflicts(arc=(seg[hit, 0] >> 1), xy=torch.cat((seg[hit, 2:4], seg[hit + 1, 2:4]), 1), kind=self.kind[hit].to(torch.uint8),
                         n_segments=Vn - self.A)


def simplify(labels: torch.Tensor, n_labels: int, tolerance: float, stats: Optional[dict] = None,
             edges: Optional[torch.Tensor] = None, topology: bool = False, max_rounds: int = 64) -> Tuple[Polygons, Arcs]:
    """The rings and boundary arcs of `polygons` / `boundary_arcs`, simplified by Douglas-Peucker to `tolerance` pixels (quantised to
    1/256 pixel as `rasterize` quantises coordinates; at most 4096), once per stretch of shared boundary: the two neighbours of a
    boundary get the same vertices, so the simplified polygons still tile the raster without slivers or overlaps, and `lines.shp`
    and `polygons.shp` written from the two results share every vertex.  Corners where three or more boundaries meet, and the four
    raster corners, stay put.  H, W <= 32768.

    Same rings and arcs, in the same order, as the tracing gives (`Arcs.edge` from `edges`, as `boundary_arcs` takes them); a ring
    that collapses stays, with ring_area2 == 0.  At tolerance 0 only the pixel corners inside straight runs are absent, as they are
    from the tracing, and `rasterize` of the rings is the input raster.  With topology=False two different boundaries may cross,
    land on each other or swing over a neighbour's corner, and an island may collapse, at any tolerance above 0, as with any plain
    Douglas-Peucker: `simplify_conflicts` lists where.  The rule: include/deepmerge_hip.h, restated in tests/simplify_ref.py; every
    array is bit-equal to it.  One tracing run plus the passes of csrc/dm_simplify.hip; the input is not modified; the only added
    readback is the pair of vertex totals.  stats: a dict that receives the time per stage and the sizes (tools/mb_simplify.py).

    topology=True repairs those conflicts (csrc/dm_simplify_topology.hip; spec tests/simplify_topology_ref.py): in
    rounds, every segment that meets another one or jumped over a node gets back the vertex farthest from it, and its halves are
    simplified again, until none is flagged.  Only dropped vertices come back, so shared boundaries stay shared, every removed
    vertex stays within the tolerance, and every ring keeps a non-zero area of its traced sign.  Without a conflict the result is
    bit for bit the plain one after one detection round.  One readback per round; RuntimeError past `max_rounds`.  stats also
    receives `topology_rounds`, `topology_flagged` (the flagged segments of every round; the last is 0) and `topology_stage_ms`
    (per round: stage -> ms)."""
    if max_rounds < 1:
        raise ValueError(f"max_rounds must be at least 1, got {max_rounds}")
    polys, arcs, _ = _simplify(labels, n_labels, tolerance, stats, topology=bool(topology), max_rounds=int(max_rounds))
    return polys, (arcs if edges is None else _attach_edges(arcs, n_labels, edges))


def simplify_conflicts(labels: torch.Tensor, n_labels: int, tolerance: float) -> Conflicts:
    """The segments of `simplify(labels, n_labels, tolerance)` that break the layer's topology: a `Conflicts`, bit-equal to
    tests/simplify_topology_ref.py.  Empty means the plain result is safe and `topology=True` would return it unchanged."""
    return _simplify(labels, n_labels, tolerance, conflicts_only=True)


# ---- polygon rings to a label raster (csrc/dm_rasterize.hip; the rule: include/deepmerge_hip.h) ----------------------
SUBPIXEL = 256                    # DM_RASTERIZE_SUBPIXEL: fixed-point units per pixel
MAX_COORDINATE = 1 << 20          # |coordinate| in pixels
MAX_EVENTS = 1 << 30


@dataclass
class Rings:
    """Closed polygon rings in pixel-corner space (x right, y down), as `rasterize` takes them.

    ring_ptr int64 [R+1] into xy; xy float64 [V,2]; ring_label int32 [R] in 0 .. 2^31 - 2.  The rings of one label need not be
    adjacent; a ring may repeat its first vertex at its end, need not lie inside the raster, and may be empty."""
    ring_ptr: torch.Tensor
    xy: torch.Tensor
    ring_label: torch.Tensor


def _ring_tensors(rings) -> tuple:
    """(ring_ptr, xy, ring_label, R, V) of a `Rings` or a `Polygons`, contiguous, their dtypes and shapes checked."""
    ring_ptr, xy, ring_label = rings.ring_ptr, rings.xy, rings.ring_label
    _need_cuda(ring_ptr, xy, ring_label)
    if ring_ptr.dtype != torch.int64 or ring_ptr.dim() != 1 or ring_ptr.numel() < 1:
        raise ValueError("ring_ptr must be int64 [R+1]")
    R = ring_ptr.numel() - 1
    if ring_label.dtype != torch.int32 or tuple(ring_label.shape) != (R,):
        raise ValueError(f"ring_label must be int32 [R] with R = {R}")
    if xy.dtype not in (torch.float64, torch.int32) or xy.dim() != 2 or xy.shape[1] != 2:
        raise ValueError("xy must be float64 [V,2] (or int32 [V,2] corners, as Polygons.xy)")
    return ring_ptr.contiguous(), xy.contiguous(), ring_label.contiguous(), R, xy.shape[0]


def _check_ring_values(ring_ptr: torch.Tensor, xy: torch.Tensor, ring_label: torch.Tensor, R: int, V: int) -> int:
    """The range check: one readback of (coordinates out of range or not finite, ring_ptr not 0 .. V non-decreasing, label range).
    Returns n_labels = the largest label + 1."""
    dev, i32, i64 = xy.device, torch.int32, torch.int64
    bad_xy = ~((xy >= -MAX_COORDINATE) & (xy <= MAX_COORDINATE))            # NaN compares false: refused
    bad_ptr = (ring_ptr[0] != 0) | (ring_ptr[-1] != V)
    if R:
        bad_ptr = bad_ptr | (ring_ptr[1:] < ring_ptr[:-1]).any()
        lo, hi = torch.aminmax(ring_label)
    else:
        lo = hi = torch.zeros((), dtype=i32, device=dev)
    any_bad = bad_xy.any() if V else torch.zeros((), dtype=torch.bool, device=dev)
    bad_xy_, bad_ptr_, lo, hi = torch.stack((any_bad.to(i64), bad_ptr.to(i64), lo.to(i64), hi.to(i64))).tolist()
    if bad_ptr_:
        raise ValueError(f"ring_ptr must start at 0, be non-decreasing and end at V = {V}")
    if bad_xy_:
        raise ValueError("coordinates must be finite and within +-2^20 pixels")
    if lo < 0 or hi > (1 << 31) - 2:
        raise ValueError(f"ring labels must be in 0 .. 2^31 - 2, found {lo} .. {hi}")
    return hi + 1


def _quantised(ring_ptr: torch.Tensor, xy: torch.Tensor, V: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(q int32 [V,2], vert_ring int32 [V]): the fixed-point coordinates and the ring of every vertex."""
    q = torch.floor(xy * SUBPIXEL + 0.5).to(torch.int32) if xy.dtype == torch.float64 else xy * SUBPIXEL
    vert_ring = (torch.searchsorted(ring_ptr, torch.arange(V, dtype=torch.int64, device=xy.device), right=True) - 1).to(torch.int32)
    return q, vert_ring


def rasterize(rings, H: int, W: int, fill: int = -1, stats: Optional[dict] = None) -> torch.Tensor:
    """int32 [H,W]: the label raster of polygon rings, the exact inverse of `polygons`.  rings: a `Rings` (float64 coordinates,
    quantised to 1/256 pixel: q = floor(256 v + 0.5)) or a `Polygons` (int32 corners, multiplied by 256 with no float step).

    A pixel belongs to a label iff its centre is inside that label's rings by the even-odd rule (holes need no flag), with the
    half-open tie rules of include/deepmerge_hip.h: polygons that share an edge partition the pixels along it.  A pixel inside
    several labels gets the greatest, a pixel inside none gets `fill` < 0.  Integer arithmetic throughout, bit-equal to
    tests/rasterize_ref.py.  The inputs are not modified.  Readbacks: the range check, the number of events N (it sizes the keys),
    the error flag.  stats: a dict that receives N, the time per stage and the bytes of the passes (tools/mb_rasterize.py)."""
    ring_ptr, xy, ring_label, R, V = _ring_tensors(rings)
    H, W, fill = int(H), int(W), int(fill)
    if H < 1 or W < 1 or H * W >= 1 << 31:
        raise ValueError(f"need H, W >= 1 and H * W < 2^31, got {H} x {W}")
    if not -(1 << 31) <= fill < 0:
        raise ValueError(f"fill must be a negative int32, got {fill}")
    if V > MAX_EVENTS:
        raise ValueError(f"rasterize takes at most 2^30 vertices, got {V}")
    dev, lib, i32, i64 = xy.device, _lib.lib(), torch.int32, torch.int64
    marks = []

    def mark(stage):                                             # stage boundaries for tools/mb_rasterize.py; nothing when stats is None
        if stats is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((stage, e))
    mark("start")
    n_labels = _check_ring_values(ring_ptr, xy, ring_label, R, V)
    if n_labels * H * (W + 1) >= 1 << 63:
        raise ValueError(f"(largest label + 1) * H * (W + 1) must be below 2^63, got {n_labels} * {H} * {W + 1}")
    N = 0
    if R and V:
        q, vert_ring = _quantised(ring_ptr, xy, V)
        count = torch.empty(V, dtype=i32, device=dev)
        check(lib.dm_rasterize_count(q.data_ptr(), ring_ptr.data_ptr(), vert_ring.data_ptr(), V, R, H, W, count.data_ptr(), _stream()),
              "dm_rasterize_count")
        scan = torch.zeros(V + 1, dtype=i64, device=dev)
        torch.cumsum(count, 0, dtype=i64, out=scan[1:])
        N = int(scan[-1])
        mark("quantise + count + scan + readback of N")
        if N > MAX_EVENTS:
            raise ValueError(f"the rings cross {N} pixel-row centres; rasterize takes at most 2^30")
    if N == 0:
        return torch.full((H, W), fill, dtype=i32, device=dev)
    keys = torch.empty(N, dtype=i64, device=dev)
    check(lib.dm_rasterize_emit(q.data_ptr(), ring_ptr.data_ptr(), vert_ring.data_ptr(), ring_label.data_ptr(), scan.data_ptr(), V, R, N, H, W,
                                n_labels, keys.data_ptr(), _stream()), "dm_rasterize_emit")
    mark("emit")
    keys = torch.sort(keys).values
    mark("sort")
    out = torch.empty((H, W), dtype=i32, device=dev)
    error = torch.empty(1, dtype=i32, device=dev)
    check(lib.dm_rasterize_fill(keys.data_ptr(), N, H, W, fill, out.data_ptr(), error.data_ptr(), _stream()), "dm_rasterize_fill")
    if int(error):
        raise RuntimeError("rasterize: a pair of sorted events disagrees in (label, row): the rings are not closed (an odd number of "
                           "crossings in a row)")
    mark("pre-set + fill + readback of the error flag")
    if stats is not None:
        torch.cuda.synchronize()
        stats["stage_ms"] = [(b[0], a[1].elapsed_time(b[1])) for a, b in zip(marks[:-1], marks[1:])]
        stats.update(N=N, vertices=V, rings=R)
    return out


def labels_from_shapefile(path: str, H: int, W: int, geotransform=None, label_field: Optional[str] = None, fill: int = -1,
                          device="cuda:0") -> Tuple[torch.Tensor, int]:
    """(labels int32 [H,W], n_labels) from a polygon shapefile: `shpstore.read_rings` followed by `rasterize`.  Record i is label i
    (the FID; n_labels = the record count), or the value of the integer field `label_field` (n_labels = the largest + 1).
    geotransform: the six GDAL terms of the raster the labels are for (None: X = x, Y = -y)."""
    from . import shpstore
    ring_ptr, xy, ring_label, n_labels = shpstore._read_rings(path, geotransform, label_field)
    rings = Rings(*(torch.from_numpy(a).to(device) for a in (ring_ptr, xy, ring_label)))
    return rasterize(rings, H, W, fill), n_labels
