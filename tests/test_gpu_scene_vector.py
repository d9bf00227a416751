"""GPU: a scene's label raster traced across tile seams (deepmerge_amd/scene.py trace_labels, csrc/dm_scene_vector.hip; DESIGN.md
3.5.10).  The definition is the test: whatever the tile size, every array of both results is bit-equal to `rag._trace` on the whole
raster.  The per-tile kernel and the 64-bit emits are compared with numpy at an origin where dart ids pass 2^40."""
import functools

import numpy as np
import pytest
import torch

import scene_vector_ref as SR
import slic_ref as R
import vector_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG_W = (1 << 31) - 2                                              # the widest scene: ids pass 2^40 from row 128 on


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
    if name == "flat_wide":
        return _blocks(5, 700, 7)
    if name == "flat_tall":
        return _blocks(700, 6, 9)
    if name == "comb":                                             # one ring of more than 8192 vertices through every tile
        return V.comb_of_combs(130), 2
    if name == "one_label":                                        # one ring through every tile, its head in tile 0
        return np.zeros((70, 150), np.int32), 1
    if name == "frame_hole":                                       # the hole's ring straddles the seams of every tiling below
        frame = np.zeros((80, 90), np.int32)
        frame[20:60, 25:70] = 1
        return frame, 2
    if name == "random_130":                                       # not connected; close to 4 darts per pixel
        return np.random.default_rng(11).integers(0, 5, (130, 130)).astype(np.int32), 5
    if name == "slic":
        from deepmerge_amd import rag
        tile = R.block_image(3, 257, 190, 37, 2)
        labels, n = rag.slic(dev(tile), cell=16, compactness=10, iters=3)
        return labels.cpu().numpy(), int(n)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def whole(name):
    """The reference, once per raster: rag._trace on the whole raster."""
    from deepmerge_amd import rag
    labels, n = raster(name)
    return rag._trace(dev(labels), n)


FIELDS = (("region_ptr", torch.int32), ("ring_ptr", torch.int64), ("xy", torch.int32), ("ring_label", torch.int32), ("ring_area2", torch.int64))
ARC_FIELDS = (("arc_ptr", torch.int64), ("xy", torch.int32), ("left", torch.int32), ("right", torch.int32))


def assert_same(got, want, what=""):
    for (polys, arcs), tag in ((got, "got"), (want, "want")):
        for f, dt in FIELDS:
            assert getattr(polys, f).dtype == dt, (tag, f)
        for f, dt in ARC_FIELDS:
            assert getattr(arcs, f).dtype == dt, (tag, f)
    for f, _ in FIELDS:
        assert torch.equal(getattr(got[0], f), getattr(want[0], f)), (what, "polygons", f)
    for f, _ in ARC_FIELDS:
        assert torch.equal(getattr(got[1], f), getattr(want[1], f)), (what, "arcs", f)


SMALL = list(V.host_cases())
LARGE = ["flat_wide", "flat_tall", "comb", "one_label", "frame_hole", "random_130", "slic"]
TILES = ((3, 64), (64, 3), (37, 41), (1 << 12, 1 << 12))          # the last: one tile larger than the scene


@pytest.mark.parametrize("name", SMALL + LARGE)
def test_the_tiled_trace_equals_the_one_raster_trace(name):
    from deepmerge_amd import scene
    labels, n = raster(name)
    before = labels.copy()
    want = whole(name)
    for tile in (((1, 1),) if name in SMALL else ()) + TILES:
        stats = {}
        got = scene.trace_labels(scene.ArraySource(labels), n, tile, stats=stats)
        assert_same(got, want, (name, tile))
        assert stats["tiles"] == len(scene.tile_grid(*labels.shape, tile)) and stats["D"] >= 4
    assert np.array_equal(labels, before)                          # the input is not modified
    if name == "comb":
        assert int(torch.diff(want[0].ring_ptr).max()) > 8192
    if name == "one_label":
        assert want[0].ring_ptr.tolist() == [0, 4] and want[0].xy.tolist() == [[0, 0], [150, 0], [150, 70], [0, 70]]
    if name == "frame_hole":
        assert want[0].ring_area2.tolist() == [2 * 80 * 90, -2 * 40 * 45, 2 * 40 * 45]


@pytest.mark.parametrize("tile", [(65, 1), (37, 15), (37, 16), (37, 17), (50, 63), (64, 64), (33, 65)])
def test_core_widths_across_the_strip_and_tile_edges(tile):
    """Core widths 1, 15, 16, 17, 63, 64, 65 (window widths one or two more): the 16-pixel strips, the 64-pixel tiles and both
    load paths of the tile walk are crossed."""
    from deepmerge_amd import scene
    for name in ("random_130", "comb"):
        labels, n = raster(name)
        assert_same(scene.trace_labels(labels, n, tile), whole(name), (name, tile))


@pytest.mark.parametrize("shape,core", [((40, 70), (1, 39, 1, 69)), ((66, 64), (1, 65, 0, 63)), ((3, 130), (1, 2, 1, 129)), ((1, 1), (0, 1, 0, 1))])
def test_the_tile_kernel_equals_the_spec_where_ids_pass_2_to_the_40(shape, core):
    from deepmerge_amd import scene
    rng = np.random.default_rng(shape[0])
    window = rng.integers(0, 3, shape).astype(np.int32)
    window[shape[0] // 2:, : shape[1] // 2] = 1                   # a larger piece: straight runs and left turns
    oy, ox = 300, BIG_W - shape[1] - (5 if core[3] < shape[1] else 0)      # without an apron on the right the window ends at the scene's edge
    want = SR.tile_records(window, core, (oy, ox), BIG_W)
    t = dev(window)
    got = scene._tile_darts(t, core, (oy, ox), 1000, BIG_W)
    assert torch.equal(t.cpu(), torch.from_numpy(window))
    ids, succ, lab, other, flags = got
    assert ids.dtype == succ.dtype == torch.int64 and lab.dtype == other.dtype == torch.int32 and flags.dtype == torch.uint8
    order = torch.argsort(ids)
    assert int(want["id"].min()) > 1 << 40
    for key, value in (("id", ids), ("succ", succ), ("lab", lab), ("other", other), ("succ_flags", flags)):
        assert np.array_equal(value[order].cpu().numpy(), want[key]), key


def test_a_core_without_a_dart_leaves_no_record():
    from deepmerge_amd import scene
    assert scene._tile_darts(dev(np.zeros((5, 5), np.int32)), (1, 4, 1, 4), (10, 10), 100, 100) is None


def test_the_wide_emits_equal_numpy_where_ids_pass_2_to_the_40():
    """A hand-built table: the darts of a small raster placed at (ox, oy) of the widest scene, joined and emitted by the 64-bit
    kernels.  Corners are the raster's own corners shifted by the origin; area2 is the int64 shoelace sum of the shifted corners."""
    from deepmerge_amd import rag, scene
    labels, n = raster("hole_meets_outside")
    local = V.trace(labels, n)
    for oy, ox in ((300, BIG_W - labels.shape[1]), ((1 << 20) + 1, 12345)):
        rec = SR.tile_records(labels, (0, labels.shape[0], 0, labels.shape[1]), (oy, ox), BIG_W)
        assert int(rec["id"].min()) > 1 << 40
        table = scene._join(*(dev(rec[k]) for k in ("id", "succ", "lab", "other", "succ_flags")))
        polys, arcs, _ = rag._trace_table(*table, BIG_W, n, wide=True)
        shift = np.array([ox, oy], np.int64)
        want_xy = local["xy"].astype(np.int64) + shift
        assert polys.xy.dtype == torch.int32 and np.array_equal(polys.xy.cpu().numpy(), want_xy)
        area2 = []
        for r in range(len(local["ring_label"])):
            p = want_xy[local["ring_ptr"][r]:local["ring_ptr"][r + 1]]
            q = np.roll(p, -1, 0)
            area2.append(int((p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1]).sum()))          # terms near 2^51, the sum is small
        assert polys.ring_area2.cpu().tolist() == area2 == local["ring_area2"].tolist()
        assert np.array_equal(polys.ring_ptr.cpu().numpy(), local["ring_ptr"]) and np.array_equal(polys.ring_label.cpu().numpy(), local["ring_label"])
        assert np.array_equal(arcs.xy.cpu().numpy(), local["arc_xy"].astype(np.int64) + shift)
        for f, key in (("arc_ptr", "arc_ptr"), ("left", "left"), ("right", "right")):
            assert np.array_equal(getattr(arcs, f).cpu().numpy(), local[key]), f


def test_two_calls_and_a_side_stream_agree():
    from deepmerge_amd import scene
    labels, n = raster("slic")
    first = scene.trace_labels(labels, n, (64, 96))
    assert_same(scene.trace_labels(torch.from_numpy(labels), n, (64, 96)), first)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = scene.trace_labels(labels, n, (64, 96))
    side.synchronize()
    assert_same(got, first)
    assert_same(first, whole("slic"))


def test_every_value_error_is_raised():
    from deepmerge_amd import scene
    labels, n = raster("frame_island")
    for bad, kw in ((labels.astype(np.int64), {}), (labels[None], {}), (labels, dict(tile=0)), (labels, dict(tile=(2, -1)))):
        with pytest.raises(ValueError):
            scene.trace_labels(bad, n, **kw)
    for bad_n in (0, 1 << 31):
        with pytest.raises(ValueError, match="n_labels must be in"):
            scene.trace_labels(labels, bad_n)
    # an id outside 0..n_labels-1 in the LAST tile only: the tiles before it run, the tile is named
    wrong = np.zeros((6, 8), np.int32)
    wrong[5, 7] = 2
    with pytest.raises(ValueError, match="window of tile 3 .*holds 0..2"):
        scene.trace_labels(wrong, 2, tile=(3, 4))
    wrong[5, 7] = -1
    with pytest.raises(ValueError, match="window of tile 3 .*holds -1..0"):
        scene.trace_labels(wrong, 2, tile=(3, 4))
    with pytest.raises(ValueError, match="at most 2\\^28 pixels"):
        scene.trace_labels(np.broadcast_to(np.zeros((1, 1), np.int32), (1 << 14, (1 << 14) + 1)), 1, tile=1 << 20)
    with pytest.raises(ValueError):
        scene.trace_labels(torch.zeros((4, 4), dtype=torch.int32, device=DEV), 1)     # the scene is host memory


# ---- SceneResult.trace / save_shapefiles --------------------------------------------------------------------------------------------------
H, W, TILE = 200, 232, (96, 112)                                   # tests/test_gpu_scene.py's scene: both axes end in an 8-pixel sliver


def scene_image():
    rng = np.random.default_rng(12)
    base = rng.integers(0, 256, (3, 4, 4)).astype(np.uint8)
    full = np.clip(np.kron(base, np.ones((64, 64), np.uint8)).astype(np.int64) + rng.integers(-8, 9, (3, 256, 256)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(full[:, :H, :W])


def slic24(t):
    from deepmerge_amd import rag
    return rag.slic(t, cell=24)


@pytest.fixture(scope="module")
def merged_scene():
    """The scene and the one-tile pipeline on its assembled raster (batch_size = 1 on both sides: bit-equal encoder rows)."""
    from deepmerge_amd import scene
    from deepmerge_amd.ExtractFeatures import FeatureIO
    from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3
    torch.manual_seed(1)
    net = ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=[32, 64, 128], depth=[1, 1, 1], in_c=3, numerics="fp32")
    fio = FeatureIO(net, None, DEV)
    image = scene_image()
    g = scene._scene_graph(image, tile=TILE, segmenter=slic24, k=1, device=DEV)
    S, whole_image, raster_ = g["n_labels"], dev(image), dev(g["labels"])
    first, _ = fio.merge_tile(whole_image, raster_, S, k=1, margin=1.0, batch_size=1, max_rounds=0)
    margin = float(first.simi.float().median())
    want, _ = fio.merge_tile(whole_image, raster_, S, k=1, margin=margin, batch_size=1)
    res = fio.segment_scene(image, tile=TILE, segmenter=slic24, k=1, margin=margin, batch_size=1)
    return res, want, raster_


def test_scene_result_trace_equals_merge_tile_on_the_assembled_raster(merged_scene):
    res, want, raster_ = merged_scene
    assert torch.equal(res.result.region_of, want.region_of) and torch.equal(res.result.edges, want.edges)
    merged = res.write_merged()
    across = (merged[95] == merged[96]).any() or (merged[:, 111] == merged[:, 112]).any()
    assert across                                                  # a merged region lies on both sides of a seam
    want_polys, want_arcs = want.polygons(raster_), want.boundary_arcs(raster_)
    got = res.trace()
    assert_same(got, (want_polys, want_arcs))
    assert got[1].edge.dtype == torch.int32 and torch.equal(got[1].edge, want_arcs.edge) and bool((got[1].edge >= 0).any())
    # a host raster given, another tile: the same; the two single-result calls as well
    assert_same(res.trace(merged=merged, tile=(50, 77)), (want_polys, want_arcs))
    assert torch.equal(res.polygons(merged).xy, want_polys.xy) and torch.equal(res.boundary_arcs(merged).edge, want_arcs.edge)
    # per-tile tracing, which this replaces, cuts the regions on the seams: more rings than the scene has
    from deepmerge_amd import rag
    C = int(res.result.rep.numel())
    pieces = sum(int(rag.polygons(res.merged_tile(i), C).ring_label.numel()) for i in range(len(res.tiles)))
    assert pieces > int(want_polys.ring_label.numel())


def test_scene_result_save_shapefiles_reads_back_as_the_traced_arrays(merged_scene, tmp_path):
    from deepmerge_amd import rag, shpstore
    res, _, _ = merged_scene
    r = res.result
    C = int(r.rep.numel())
    polys, arcs = res.trace()
    paths = res.save_shapefiles(str(tmp_path))
    assert [p.rsplit("/", 1)[1] for p in paths] == ["polygons.shp", "lines.shp"]
    got = shpstore.ShapeReader(paths[0])
    assert got.shape_type == 5 and len(got) == C
    region_ptr, ring_ptr, xy = polys.region_ptr.cpu().numpy(), polys.ring_ptr.cpu().numpy(), polys.xy.cpu().numpy().astype(np.float64)
    for l in range(C):
        rings = range(region_ptr[l], region_ptr[l + 1])
        assert len(got.shapes[l]) == len(rings) >= 1
        for part, ring in zip(got.shapes[l], rings):
            p = xy[ring_ptr[ring]:ring_ptr[ring + 1]]
            assert np.array_equal(part[:-1], np.stack((p[:, 0], -p[:, 1]), 1)) and np.array_equal(part[-1], part[0])
    designed = rag.designed_features(r.stats).cpu().numpy()
    for i, name in enumerate(rag.FEATURE_NAMES):
        assert np.array_equal(got.fields[name].astype(np.float32), designed[:, i]), name
    ptr, idx = r.ptr.cpu().numpy(), r.idx.cpu().numpy()
    assert got.fields["PointID"] == [" ".join(str(i) for i in idx[ptr[l]:ptr[l + 1]]) for l in range(C)]
    lines = shpstore.ShapeReader(paths[1])
    arc_ptr, arc_xy = arcs.arc_ptr.cpu().numpy(), arcs.xy.cpu().numpy().astype(np.float64)
    assert lines.shape_type == 3 and len(lines) == arcs.left.numel()
    for a, shape in enumerate(lines.shapes):
        p = arc_xy[arc_ptr[a]:arc_ptr[a + 1]]
        assert len(shape) == 1 and np.array_equal(shape[0], np.stack((p[:, 0], -p[:, 1]), 1))
    assert lines.fields["LEFT_FID"].tolist() == arcs.left.tolist() and lines.fields["RIGHT_FID"].tolist() == arcs.right.tolist()
    edge, simi = arcs.edge.cpu().numpy(), r.simi.cpu().numpy()
    assert np.array_equal(lines.fields["simi"].astype(np.float32), np.where(edge >= 0, simi[np.maximum(edge, 0)], np.float32(0)))
    assert not (tmp_path / "PointsGCS.shp").exists()
