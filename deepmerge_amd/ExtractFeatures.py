"""MI355X-native counterpart of the reference's `ExtractFeatures.py` inference sweep.

Reference flow (ExtractFeatures.py:45-86, :150-225): embed every sample point in batches of 2000
(eval forward), append the [P,100] float32 rows to an HDF5 dataset, then for each region-adjacency
edge gather the point rows of both polygons, mean-pool them and write the Euclidean distance as
`simi`.  GDAL rasters / shapefiles are out of scope (tensors in, tensors out); the HDF5 feature store exists as a writer /
reader of the same layout (deepmerge_amd/h5store.py, save_h5 / ReadFeatures below).  This module keeps the
features resident in HBM and runs the sweep as two kernels:
    dm_segment_mean      per-polygon mean over its sample points (CSR: ptr[S+1], idx[P])
    dm_edge_similarity   per-edge simi + merge = simi < margin
The arithmetic order of both is pinned (oracle/sweep_strict.c), so `merge` is bit-exact.
The reference's dense helpers `Euclidean_distance` / `MC_Lyu_2020` (ExtractFeatures.py:119-147, :228-237) run on
dm_pairwise_distance (one fused kernel: norms, product and epilogue).
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops


class FeatureIO:
    """`FeatureIO(net, checkpoint_path)` as at ExtractFeatures.py:27-43: eval mode, weights frozen."""

    def __init__(self, net: torch.nn.Module, checkpoint_path: Optional[str] = None, device: str = "cuda:0"):
        self.net = net
        if checkpoint_path is not None:
            state = torch.load(checkpoint_path, map_location="cpu")
            self.net.load_state_dict(state["net"])          # same checkpoint dict layout as Train_SMT.py:325-331
        self.net.to(device).eval()
        for p in self.net.parameters():
            p.requires_grad = False
        self.device = device
        self.features: Optional[torch.Tensor] = None

    @torch.no_grad()
    def extract_features(self, patches: Sequence[torch.Tensor], designed: torch.Tensor, batch_size: int = 2000) -> torch.Tensor:
        """Embed P sample points (per-scale patch stacks [P, C, s, s] and designed features [P,1,19]) in
        point order, `batch_size` at a time (ExtractFeatures.py:45, :58-79); returns / keeps F [P,100] fp32."""
        P = designed.shape[0]
        out = torch.empty((P, 100), dtype=torch.float32, device=self.device)
        S = len(self.net.input_image_scales)                  # the 4th 1x1 patch is dropped (:68-70)
        for s in range(0, P, batch_size):
            e = min(P, s + batch_size)
            x = [patches[i][s:e].to(self.device) for i in range(S)]
            out[s:e] = self.net(x, designed[s:e].to(self.device))
        self.features = out
        return out

    @torch.no_grad()
    def extract_features_from_tile(self, tile: torch.Tensor, points_xy: torch.Tensor, inner: torch.Tensor, obj: torch.Tensor,
                                   region_features: torch.Tensor, batch_size: int = 2000, geotransform=None,
                                   process_group=None) -> torch.Tensor:
        """`extract_features(image_path, point_path, h5_file_path, batch_size)` (ExtractFeatures.py:45-86) with the raster and the
        point table already in memory: `tile` uint8 [bands, H, W] on the GPU (what GDAL's ReadAsArray returns), one row per
        sample point in FID order -- pixel position (or geo coordinates when `geotransform` is given: the reference's own
        conversion with its +1, MyUtils1.py:67-73), the `inner` / `object` window fields and the 15 designed attributes.  The
        per-point window arithmetic, crop, resize and patch-embed operand layout run on the device (patches.point_batch_cols);
        returns / keeps F [P, 100] fp32, rows in point order, as the HDF5 `dataset` would hold them.
        The band resize follows `self.resize` ("opencv" by default: cv2.resize(..., INTER_AREA) as MyUtils1.py:202-216 calls it, restated
        branch by branch; set `FeatureIO.resize = "exact_area"` for the exact rational area average of earlier rounds)."""
        from .patches import geo_to_pixel, point_batch_cols
        import torch.distributed as dist
        if geotransform is not None:
            points_xy = geo_to_pixel(geotransform, points_xy[:, 0], points_xy[:, 1])
        world = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
        if world > 1:
            # points are independent -> contiguous equal shards per rank (the tile is replicated: 64 MiB), no exchange
            # during the encode, ONE all-gather of the [P, 100] rows (24 MB for a 4096^2 tile) before the sweep
            rank = dist.get_rank(process_group)
            P = points_xy.shape[0]
            per = (P + world - 1) // world
            lo, hi = min(P, rank * per), min(P, (rank + 1) * per)
            local = self._extract_local(tile, points_xy[lo:hi], inner[lo:hi], obj[lo:hi], region_features[lo:hi], batch_size) \
                if hi > lo else torch.empty((0, 100), dtype=torch.float32, device=self.device)
            padded = torch.zeros((per, 100), dtype=torch.float32, device=self.device)
            padded[:hi - lo] = local
            parts = [torch.empty_like(padded) for _ in range(world)]
            dist.all_gather(parts, padded, group=process_group)
            self.features = torch.cat(parts)[:P].contiguous()
            return self.features
        return self._extract_local(tile, points_xy, inner, obj, region_features, batch_size)

    @torch.no_grad()
    def merge_tile(self, tile: torch.Tensor, labels: torch.Tensor, n_labels: int, k: int = 3, margin: float = 1.0, batch_size: int = 2000,
                   **merge_kwargs):
        """From an image tile (uint8 [bands, H, W]) and its segmentation (labels int32 [H, W], ids 0..n_labels-1) to the merged
        partition: label_stats -> designed_features -> rag_edges -> sample_points -> extract_features_from_tile ->
        merge_regions(weights=, stats=), nothing else.  Returns (MergeResult, PointSamples); `result.labels(labels)` is the merged
        raster.  `merge_kwargs` go to merge_regions (max_rounds, min_regions, min_area).  Under a process group the encode is
        sharded by extract_features_from_tile and the graph stages run replicated."""
        from . import rag
        stats = rag.label_stats(labels, tile, n_labels)
        designed = rag.designed_features(stats)
        edges, weights = rag.rag_edges(labels, n_labels)
        pts = rag.sample_points(labels, n_labels, k=k)
        features = self.extract_features_from_tile(tile, pts.xy, pts.inner, pts.obj, pts.region_features(designed), batch_size=batch_size)
        result = rag.merge_regions(features, pts.ptr, pts.idx, edges, margin=margin, weights=weights, stats=stats, **merge_kwargs)
        return result, pts

    @torch.no_grad()
    def segment_tile(self, tile: torch.Tensor, cell: int = 29, compactness: int = 10, iters: int = 10, min_size: Optional[int] = None,
                     **merge_tile_kwargs):
        """From an image tile alone to the merged partition: rag.slic(tile, cell, compactness, iters, min_size) followed by
        merge_tile(tile, labels, n_labels, **merge_tile_kwargs) (min_area among them; SLIC's min_size is the other thing, the
        size below which a fragment of a superpixel is absorbed before any scoring).  Returns (MergeResult, PointSamples, labels,
        n_labels), where labels / n_labels are the SLIC superpixels the merge started from."""
        from . import rag
        labels, n_labels = rag.slic(tile, cell=cell, compactness=compactness, iters=iters, min_size=min_size)
        result, pts = self.merge_tile(tile, labels, n_labels, **merge_tile_kwargs)
        return result, pts, labels, n_labels

    @torch.no_grad()
    def segment_scene(self, source, **kw):
        """From a scene larger than one tile (anything with `.shape == (bands, H, W)` and `.read(y0, y1, x0, x1)`, or a host array
        / memmap) to the merged partition: `scene.segment_scene(self, source, **kw)`.  Returns a `scene.SceneResult`.
        `labels=, n_labels=` bring the scene's superpixels along as a label raster on the host whose regions may cross tile seams
        (`scene.segment_labels`); they go with no `segmenter`.  `cross_seams=True, slic={...}` makes such superpixels here
        (`scene.slic_labels`, then `scene.segment_labels`); it goes with neither.  `merge_regions`' keywords (max_rounds,
        min_regions, min_area) reach the scene's one merge on each of these paths."""
        from . import scene
        return scene.segment_scene(self, source, **kw)

    @torch.no_grad()
    def trace_scene(self, source, n_labels: int, **kw):
        """A scene's label raster (int32 [H, W] on the host, ids 0..n_labels-1, or anything with `.shape` and `.read`) traced
        into rings and arcs across its tiles: `scene.trace_labels(source, n_labels, device=self.device, **kw)`.  Returns
        (rag.Polygons, rag.Arcs) in scene coordinates."""
        from . import scene
        return scene.trace_labels(source, n_labels, device=self.device, **kw)

    @torch.no_grad()
    def simplify_scene(self, source, n_labels: int, tolerance: float, topology: bool = False, **kw):
        """The rings and arcs of `trace_scene`, simplified to `tolerance` pixels once per stretch of shared boundary, across the
        scene's tiles: `scene.simplify_labels(source, n_labels, tolerance, device=self.device, **kw)`.  Returns (rag.Polygons,
        rag.Arcs) in scene coordinates, bit for bit `rag.simplify` of the whole raster.  topology=True also repairs what plain
        simplification breaks: `scene.simplify_labels_topology` with the same arguments (and max_rounds), bit for bit
        `rag.simplify(..., topology=True)` of the whole raster."""
        from . import scene
        call = scene.simplify_labels_topology if topology else scene.simplify_labels
        return call(source, n_labels, tolerance, device=self.device, **kw)

    @torch.no_grad()
    def rasterize_scene(self, rings, H: int, W: int, **kw):
        """Polygon rings (a rag.Rings or a rag.Polygons in scene coordinates) rasterised into the scene's int32 [H, W] label raster
        on the host, tile by tile: `scene.rasterize_rings(rings, H, W, device=self.device, **kw)`, bit for bit `rag.rasterize` of
        the whole raster.  `scene.RingSource(rings, H, W)` hands the same pixels to the scene calls with no host raster."""
        from . import scene
        return scene.rasterize_rings(rings, H, W, device=self.device, **kw)

    @torch.no_grad()
    def _extract_local(self, tile, points_xy, inner, obj, region_features, batch_size):
        from .patches import point_batch_cols
        P = points_xy.shape[0]
        scales = list(self.net.input_image_scales)
        grid = self.net.cube_size[1]
        dtype = ops.act_dtype(getattr(self.net, "numerics", "bf16"))
        out = torch.empty((P, 100), dtype=torch.float32, device=self.device)
        xy = points_xy.to(self.device).to(torch.int32)
        feats = region_features.to(self.device)
        for s in range(0, P, batch_size):
            e = min(P, s + batch_size)
            patches, designed = point_batch_cols(tile, xy[s:e], inner[s:e], obj[s:e], feats[s:e], scales=scales, grid=grid, dtype=dtype,
                                                 resize=getattr(self, "resize", "opencv"))
            out[s:e] = self.net(patches, designed)
        self.features = out
        return out

    # -- the HDF5 feature store of the reference (ExtractFeatures.py:88-117), without h5py: deepmerge_amd/h5store.py ----------
    def save_h5(self, h5_file_path: str, batch_size: int = 2000) -> int:
        """Write the resident features as the reference's `dataset` ([P, 100] float32, first dimension unlimited, chunked),
        appended `batch_size` rows at a time like the upstream loop.  Returns the number of rows written."""
        from .h5store import H5FeatureWriter
        if self.features is None:
            raise RuntimeError("no features to save: run extract_features / extract_features_from_tile first")
        F = self.features
        with H5FeatureWriter(h5_file_path, width=F.shape[1]) as w:
            for s in range(0, F.shape[0], batch_size):
                w.append(F[s:s + batch_size].float().cpu().numpy())
        return int(F.shape[0])

    # -- the shapefiles the reference's loaders read (MyUtils1.py:60-114, MyUtils2.py:155-193), without GDAL: deepmerge_amd/shpstore.py --
    @staticmethod
    def save_shapefiles(folder: str, labels: torch.Tensor, n_labels: int, pts, designed: torch.Tensor, edges: Optional[torch.Tensor] = None,
                        simi: Optional[torch.Tensor] = None, geotransform=None, tolerance: Optional[float] = None,
                        topology: bool = False):
        """Write a label raster as the three layers the reference reads: `polygons.shp` (one record per label: the 15 FEATURE_NAMES
        fields from `designed` [n_labels,15] and `PointID`, the space-separated point indices of pts.ptr / pts.idx), `lines.shp` (one
        record per boundary arc: LEFT_FID, RIGHT_FID, -1 = outside the raster, and `simi` when given: the value of the arc's row in
        `edges`, 0.0 for LEFT_FID == -1) and `PointsGCS.shp` (one record per sample point of `pts`: inner, object).  FIDs are label,
        arc and point indices.  tolerance: None writes the traced pixel staircase; a number writes the rings and arcs of
        `rag.simplify(labels, n_labels, tolerance, topology=topology)`, so `polygons.shp` and `lines.shp` share every vertex;
        topology=True also repairs what plain simplification breaks (collapsed islands, boundaries that cross), so a GIS takes the
        layer as it is.  Returns the three paths."""
        import os
        from . import rag, shpstore
        if simi is not None and edges is None:
            raise ValueError("simi needs edges: an arc finds its value through its row in `edges`")
        if designed.dim() != 2 or tuple(designed.shape) != (n_labels, len(rag.FEATURE_NAMES)):
            raise ValueError(f"designed must be [{n_labels},{len(rag.FEATURE_NAMES)}] (as designed_features returns it)")
        if pts.ptr.numel() != n_labels + 1:
            raise ValueError(f"pts.ptr must have n_labels + 1 = {n_labels + 1} entries")
        polys, arcs = rag._trace(labels, n_labels) if tolerance is None else rag.simplify(labels, n_labels, tolerance, topology=topology)
        paths = write_polygon_and_line_layers(folder, polys, arcs, n_labels, pts.ptr, pts.idx, designed, edges, simi, geotransform)
        paths.append(shpstore.write_points(os.path.join(folder, "PointsGCS.shp"), pts.xy.cpu().numpy(),
                                           [("inner", pts.inner.cpu().numpy()), ("object", pts.obj.cpu().numpy())], geotransform))
        return tuple(paths)

    def ReadFeatures(self, h5_file_path: str):
        """Open a feature store for GetFeaturesByID (ExtractFeatures.py:103-107)."""
        from .h5store import H5FeatureReader
        self.Close()
        self.h5py_file = H5FeatureReader(h5_file_path)
        self.dataset = self.h5py_file

    def Close(self):
        if getattr(self, "h5py_file", None) is not None:
            self.h5py_file.close()
            self.h5py_file = None
            self.dataset = None

    def GetFeaturesByID(self, idx: int):
        """Row `idx` of the opened store (numpy float32 [100], as h5py returns it) or, without one, of the resident tensor."""
        if getattr(self, "dataset", None) is not None:
            if idx >= len(self.dataset):
                raise IndexError("index error!")
            return self.dataset[idx]
        if self.features is None or idx >= self.features.shape[0]:
            raise IndexError("index error!")
        return self.features[idx]


def write_polygon_and_line_layers(folder: str, polys, arcs, n_labels: int, ptr: torch.Tensor, idx: torch.Tensor, designed: torch.Tensor,
                                  edges: Optional[torch.Tensor] = None, simi: Optional[torch.Tensor] = None, geotransform=None) -> list:
    """`polygons.shp` and `lines.shp` of traced rings and arcs, as `FeatureIO.save_shapefiles` describes them: the writer both
    `FeatureIO.save_shapefiles` (one raster) and `scene.SceneResult.save_shapefiles` (a scene, traced across its tiles) go through.
    ptr / idx: the point lists behind `PointID`.  Returns the two paths."""
    import os
    from . import rag, shpstore
    if simi is not None and edges is None:
        raise ValueError("simi needs edges: an arc finds its value through its row in `edges`")
    os.makedirs(folder, exist_ok=True)
    ptr, idx = ptr.cpu().tolist(), idx.cpu().tolist()
    point_id = [" ".join(str(i) for i in idx[ptr[l]:ptr[l + 1]]) for l in range(n_labels)]
    feats = designed.float().cpu().numpy()
    fields = [(name, feats[:, i]) for i, name in enumerate(rag.FEATURE_NAMES)] + [("PointID", point_id)]
    paths = [shpstore.write_polygons(os.path.join(folder, "polygons.shp"), polys, fields, geotransform)]
    line_fields = [("LEFT_FID", arcs.left.cpu().numpy()), ("RIGHT_FID", arcs.right.cpu().numpy())]
    if simi is not None:
        if simi.numel() != edges.shape[0]:
            raise ValueError(f"simi has {simi.numel()} values for {edges.shape[0]} edges")
        row = rag._attach_edges(arcs, n_labels, edges).edge.long()
        values = torch.where(row >= 0, simi.float()[row.clamp(min=0)], torch.zeros((), dtype=torch.float32, device=row.device)) \
            if simi.numel() else torch.zeros(row.numel(), dtype=torch.float32)
        line_fields.append(("simi", values.cpu().numpy()))
    paths.append(shpstore.write_lines(os.path.join(folder, "lines.shp"), arcs, line_fields, geotransform))
    return paths


def rag_similarity_sweep(features: torch.Tensor, ptr: torch.Tensor, idx: torch.Tensor, edges: torch.Tensor,
                         margin: float = 1.0):
    """The per-edge loop of `test_for_shp` (ExtractFeatures.py:164-219) for ALL edges at once.

    features [P,D] fp32, ptr int32 [S+1], idx int32 [P'] (polygon -> its PointID list), edges int32 [E,2]
    (LEFT_FID, RIGHT_FID; -1 = no polygon, skipped as at MyUtils2.py:184-186 -> simi NaN, merge False).
    Returns (pooled [S,D], simi [E], merge [E] bool)."""
    pooled = ops.segment_mean(features.contiguous(), ptr.to(torch.int32).contiguous(), idx.to(torch.int32).contiguous())
    simi, merge = ops.edge_similarity(pooled, edges.to(torch.int32).contiguous(), margin)
    return pooled, simi, merge.bool()


def Euclidean_distance(X, Y):
    """`Euclidean_distance(X, Y)` of ExtractFeatures.py:119-147 (and Train_SMT.py:115-131): X [n,p], Y [m,p] -> D [n,m] distance
    matrix, computed on the device by one dm_pairwise_distance launch (ops.pairwise_distance).  numpy arrays and CPU tensors go to
    the current GPU and the result comes back as the input's type and dtype (float32 or float64, as the reference computes in
    the input dtype); CUDA tensors stay on their device."""
    if isinstance(X, torch.Tensor) and isinstance(Y, torch.Tensor) and X.is_cuda and Y.is_cuda:
        return ops.pairwise_distance(X, Y)
    as_numpy = not isinstance(X, torch.Tensor)
    tx = torch.as_tensor(X) if not isinstance(X, torch.Tensor) else X
    ty = torch.as_tensor(Y) if not isinstance(Y, torch.Tensor) else Y
    dev = tx.device if tx.is_cuda else (ty.device if ty.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    D = ops.pairwise_distance(tx.to(dev), ty.to(dev))
    return D.cpu().numpy() if as_numpy else D.cpu()


def MC_Lyu_2020(X, Y):
    """`MC_Lyu_2020(X, Y)` of ExtractFeatures.py:228-237: the same distance matrix as Euclidean_distance."""
    return Euclidean_distance(X, Y)


def near_margin_count(simi: torch.Tensor, margin: float = 1.0, band: float = 1e-4) -> int:
    """Edges whose similarity lies within `band` of the margin: the only merge decisions that can differ between two encoders
    whose features agree to ~1e-4 (reported next to the bit-exact `merge` comparison).  NaN (skipped edges) never counts."""
    return int(((simi - margin).abs() < band).sum())
