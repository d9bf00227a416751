"""GPU: rag.polygons / rag.boundary_arcs (csrc/dm_vector.hip) against the numpy spec tests/vector_ref.py -- every array is bit-equal
and the input is not modified --, their invariants against the device's own label_stats / rag_edges, and the chain
slic -> merge_tile -> MergeResult.polygons -> FeatureIO.save_shapefiles -> ShapeReader."""
import functools

import numpy as np
import pytest
import torch

import slic_ref as R
import vector_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _blocks(H, W, seed):
    labels, n = R.connected_labels(R.block_image(1, H, W, 37, seed, noise=0)[0].astype(np.int32))
    return labels.astype(np.int32), int(n)


@functools.lru_cache(maxsize=None)
def raster(name):
    host = V.host_cases()
    if name in host:
        return host[name]
    if name == "vec_blocks":
        return _blocks(96, 128, 3)                              # W % 16 == 0: the 16-byte loads and stores
    if name == "odd_blocks":
        return _blocks(257, 301, 5)                             # odd width, rings across the tile seams
    if name == "flat_wide":
        return _blocks(5, 700, 7)
    if name == "flat_tall":
        return _blocks(700, 6, 9)
    if name == "random_4":                                      # not connected; close to 4 darts per pixel
        return np.random.default_rng(11).integers(0, 4, (67, 70)).astype(np.int32), 4
    if name == "comb":
        return V.comb_of_combs(130), 2
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def spec(name):
    labels, n = raster(name)
    return V.trace(labels, n)


NAMES = list(V.host_cases()) + ["vec_blocks", "odd_blocks", "flat_wide", "flat_tall", "random_4", "comb"]


def assert_equals_spec(polys, arcs, want):
    pairs = (("region_ptr", polys.region_ptr, torch.int32), ("ring_ptr", polys.ring_ptr, torch.int64), ("xy", polys.xy, torch.int32),
             ("ring_label", polys.ring_label, torch.int32), ("ring_area2", polys.ring_area2, torch.int64),
             ("arc_ptr", arcs.arc_ptr, torch.int64), ("arc_xy", arcs.xy, torch.int32), ("left", arcs.left, torch.int32),
             ("right", arcs.right, torch.int32))
    for key, got, dtype in pairs:
        assert got.dtype == dtype, key
        g = got.cpu().numpy()
        assert g.shape == want[key].shape and np.array_equal(g, want[key]), key


@pytest.mark.parametrize("name", NAMES)
def test_rings_and_arcs_equal_the_spec(name):
    from deepmerge_amd import rag
    labels, n = raster(name)
    want = spec(name)
    t = dev(labels)
    polys = rag.polygons(t, n)
    arcs = rag.boundary_arcs(t, n)
    print(f"{name}: {labels.shape}, rings = {len(want['ring_label'])}, vertices = {len(want['xy'])}, arcs = {len(want['left'])}")
    assert_equals_spec(polys, arcs, want)
    assert arcs.edge is None
    assert torch.equal(t.cpu(), torch.from_numpy(labels))          # the input is not modified
    if name == "comb":
        assert int(np.diff(want["ring_ptr"]).max()) > 4096         # one ring through every tile: the jumping rounds
    if name == "random_4":
        assert int(want["ring_ptr"][-1]) > 2 * labels.size         # dense


def test_one_run_serves_both_and_two_runs_are_identical():
    from deepmerge_amd import rag
    labels, n = raster("odd_blocks")
    t = dev(labels)
    stats = {}
    polys, arcs = rag._trace(t, n, stats)
    assert_equals_spec(polys, arcs, spec("odd_blocks"))
    again = rag._trace(t, n)
    for a, b in zip((polys.xy, polys.ring_area2, arcs.xy, arcs.left), (again[0].xy, again[0].ring_area2, again[1].xy, again[1].left)):
        assert torch.equal(a, b)
    assert stats["D"] > 0 and stats["head_rounds"] >= 1 and stats["rank_rounds"] >= 1 and stats["bytes"] > 0


def test_invariants_against_label_stats_and_rag_edges():
    from deepmerge_amd import rag
    labels, n = raster("odd_blocks")
    H, W = labels.shape
    t = dev(labels)
    tile = torch.zeros((1, H, W), dtype=torch.uint8, device=DEV)
    st = rag.label_stats(t, tile, n)
    edges, weights = rag.rag_edges(t, n)
    polys = rag.polygons(t, n)
    arcs = rag.boundary_arcs(t, n, edges=edges)
    ring_label = polys.ring_label.cpu().numpy().astype(np.int64)
    area2 = np.zeros(n, np.int64)
    np.add.at(area2, ring_label, polys.ring_area2.cpu().numpy())
    assert np.array_equal(area2, 2 * st["count"].cpu().numpy())
    length = np.zeros(n, np.int64)
    np.add.at(length, ring_label, V.path_length(polys.xy.cpu().numpy(), polys.ring_ptr.cpu().numpy(), closed=True))
    assert np.array_equal(length, st["peri"].cpu().numpy().sum(1))
    left, right, edge = arcs.left.cpu().numpy(), arcs.right.cpu().numpy(), arcs.edge.cpu().numpy()
    arc_len = V.path_length(arcs.xy.cpu().numpy(), arcs.arc_ptr.cpu().numpy(), closed=False)
    per_edge = np.zeros(edges.shape[0], np.int64)
    np.add.at(per_edge, edge[left >= 0], arc_len[left >= 0])
    assert np.array_equal(per_edge, weights.cpu().numpy())
    assert arc_len[left < 0].sum() == int(st["peri"][:, 1].sum())
    assert not ((left >= 0) & (left <= right)).any()
    # Arcs.edge is the row of (right, left)
    assert arcs.edge.dtype == torch.int32 and np.array_equal(edge, V.arc_edge(left, right, edges.cpu().numpy()))
    assert np.array_equal(edges.cpu().numpy()[edge[left >= 0]], np.stack((right, left), 1)[left >= 0])


def test_input_checks():
    from deepmerge_amd import rag
    t = dev(np.zeros((4, 4), np.int32))
    with pytest.raises(ValueError):
        rag.polygons(t.long(), 1)
    with pytest.raises(ValueError):
        rag.polygons(t[0], 1)
    with pytest.raises(ValueError):
        rag.polygons(t + 1, 1)                                     # a label outside 0..n_labels-1
    with pytest.raises(ValueError):
        rag.polygons(t - 1, 1)
    with pytest.raises(ValueError):
        rag.boundary_arcs(dev(V.host_cases()["parity"][0]), 2, edges=torch.zeros((1, 2), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):                                # H * W > 2^28: refused before anything is launched
        rag.polygons(torch.empty((1, 1), dtype=torch.int32, device=DEV).expand(1 << 14, (1 << 14) + 1), 1)
    cols = dev(np.arange(8, dtype=np.int32).reshape(2, 4)).t()      # not contiguous: a contiguous copy is traced
    want = V.trace(np.arange(8, dtype=np.int32).reshape(2, 4).T.copy(), 8)
    assert_equals_spec(rag.polygons(cols, 8), rag.boundary_arcs(cols, 8), want)


def test_chain_slic_merge_polygons_shapefiles(tmp_path):
    from deepmerge_amd import rag, shpstore
    from deepmerge_amd.ExtractFeatures import FeatureIO
    from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3
    torch.manual_seed(1)
    tile = R.block_image(3, 96, 128, 37, 2)
    tt = dev(tile)
    net = ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=[32, 64, 128], depth=[1, 1, 1], in_c=3, numerics="fp32")
    fio = FeatureIO(net, None, DEV)
    labels, S = rag.slic(tt, cell=16, compactness=10, iters=3)
    result, pts = fio.merge_tile(tt, labels, S, k=3, margin=1.0, batch_size=100, max_rounds=2)
    merged = result.labels(labels)
    C = result.rep.numel()
    want = V.trace(merged.cpu().numpy(), C)
    arcs = result.boundary_arcs(labels)
    assert_equals_spec(result.polygons(labels), arcs, want)
    assert np.array_equal(arcs.edge.cpu().numpy(), V.arc_edge(want["left"], want["right"], result.edges.cpu().numpy()))
    # the merged partition as shapefiles: its own statistics, points and scores
    stats = result.stats
    designed = rag.designed_features(stats)
    mpts = rag.sample_points(merged, C, k=3)
    paths = fio.save_shapefiles(str(tmp_path), merged, C, mpts, designed, edges=result.edges, simi=result.simi)
    assert [p.rsplit("/", 1)[1] for p in paths] == ["polygons.shp", "lines.shp", "PointsGCS.shp"]
    lines = shpstore.ShapeReader(paths[1])
    got = set(zip(lines.fields["RIGHT_FID"].tolist(), lines.fields["LEFT_FID"].tolist()))
    border = {(int(l), -1) for l in np.unique(np.concatenate((merged[0].cpu().numpy(), merged[-1].cpu().numpy(), merged[:, 0].cpu().numpy(),
                                                                merged[:, -1].cpu().numpy())))}
    assert got == {(int(a), int(b)) for a, b in result.edges.cpu().numpy()} | border
    simi = result.simi.cpu().numpy()
    edge = arcs.edge.cpu().numpy()
    assert np.array_equal(lines.fields["simi"].astype(np.float32), np.where(edge >= 0, simi[np.maximum(edge, 0)], np.float32(0)))
    polys = shpstore.ShapeReader(paths[0])
    assert len(polys) == C and polys.shape_type == 5
    assert np.array_equal(polys.fields["area"].astype(np.float32), designed[:, 0].cpu().numpy())
    ptr, idx = mpts.ptr.cpu().numpy(), mpts.idx.cpu().numpy()
    assert polys.fields["PointID"] == [" ".join(str(i) for i in idx[ptr[l]:ptr[l + 1]]) for l in range(C)]
    points = shpstore.ShapeReader(paths[2])
    assert len(points) == mpts.xy.shape[0] and np.array_equal(points.fields["inner"], mpts.inner.cpu().numpy())
    assert np.array_equal(points.fields["object"], mpts.obj.cpu().numpy())
