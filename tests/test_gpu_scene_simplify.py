"""GPU: a scene's rings and arcs simplified across tile seams (deepmerge_amd/scene.py simplify_labels, csrc/dm_scene_simplify.hip;
DESIGN.md 3.5.11).  The definition is the test: whatever the tile size, every array of both results is bit-equal to `rag.simplify`
on the whole raster.  The node kernel is compared with numpy at an origin where corner ids pass 2^40, the chain, arc and ring
kernels on a set of arcs and rings translated to the far end of the widest scene."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import scene_simplify_ref as SR
import simplify_ref as S
import test_gpu_scene_vector as TV
import vector_ref as V
from test_gpu_scene_vector import assert_same, dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG_W = (1 << 31) - 2
TOLERANCES = (0, 0.5, 0.75, 1.5, 4, 4096)
SMALL = list(V.host_cases()) + list(S.drawn_cases())
LARGE = ["comb", "flat_wide", "flat_tall", "one_label", "frame_hole", "random_130", "slic"]
TILES = ((3, 64), (64, 3), (37, 41), (1 << 12, 1 << 12))          # the last: one tile larger than the scene


@functools.lru_cache(maxsize=None)
def raster(name):
    drawn, extra = S.drawn_cases(), S.extra_cases()
    if name in drawn:
        return drawn[name]
    if name in ("flat_wide", "flat_tall"):                        # 5 x 700 and 700 x 6, wavy boundaries
        return extra[name]
    if name == "random_130":
        return extra["random_4"]
    return TV.raster(name)


@functools.lru_cache(maxsize=None)
def whole(name, tol):
    """The reference, once per raster and tolerance: rag.simplify on the whole raster."""
    from deepmerge_amd import rag
    labels, n = raster(name)
    return rag.simplify(dev(labels), n, tol)


@pytest.mark.parametrize("name", SMALL + LARGE)
def test_the_tiled_simplification_equals_the_one_raster_simplification(name):
    from deepmerge_amd import scene
    labels, n = raster(name)
    before = labels.copy()
    for tile in (((1, 1),) if name in SMALL else ()) + TILES:
        for tol in TOLERANCES:
            stats = {}
            got = scene.simplify_labels(scene.ArraySource(labels), n, tol, tile, stats=stats)
            assert_same(got, whole(name, tol), (name, tile, tol))
            assert stats["tiles"] == len(scene.tile_grid(*labels.shape, tile)) and stats["nodes"] >= 4 and stats["kept"] >= stats["nodes"]
    assert np.array_equal(labels, before)                          # the input is not modified
    if name == "comb":
        assert stats["longest_arc"] > 8192                         # one chain of more than 8192 vertices through every tile
    if name == "one_label":
        assert got[0].xy.tolist() == [[0, 0], [150, 0], [150, 70], [0, 70]] and stats["nodes"] == 4
    if name == "frame_hole":                                       # the hole's arc has no node: its anchor (25, 20) is kept at every tolerance
        assert got[1].xy.tolist() == [[0, 0], [90, 0], [90, 80], [0, 80], [0, 0], [25, 20], [25, 20]]


def gpu_nodes(labels, tile):
    """The joined node records of every tile, through the driver's own tile stream."""
    from deepmerge_amd import scene
    H, W = labels.shape
    parts = []
    for _, _, window, box, origin in scene._windows(scene.ArraySource(labels), scene._Grid.of(H, W, tile), 1, torch.int32, 2, torch.device(DEV),
                                                    scene._Clock(None, DEV)):
        own = scene._tile_nodes(window, box, origin, H, W)
        if own is not None:
            assert own.dtype == torch.int64
            parts.append(own)
    return torch.sort(torch.cat(parts)).values


@pytest.mark.parametrize("tile", [(65, 1), (37, 15), (37, 16), (37, 17), (50, 63), (64, 64), (33, 65)])
def test_the_node_kernel_at_core_widths_across_the_strip_and_block_edges(tile):
    """Core widths 1, 15, 16, 17, 63, 64, 65: the 16-corner strips and the 64-corner blocks of the tile walk are crossed."""
    from deepmerge_amd import rag
    for name in ("random_130", "comb"):
        labels, n = raster(name)
        keep = rag._simplify(dev(labels), n, 0)[2]
        want = torch.nonzero(keep == 2).squeeze(1)
        assert torch.equal(gpu_nodes(labels, tile), want), (name, tile)


@pytest.mark.parametrize("shape,core", [((40, 70), (1, 39, 1, 69)), ((66, 64), (1, 65, 1, 64)), ((3, 130), (1, 3, 1, 129)), ((1, 1), (0, 1, 0, 1)),
                                        ((65, 17), (0, 64, 1, 17))])
def test_the_node_kernel_equals_the_spec_where_ids_pass_2_to_the_40(shape, core):
    """Windows at the far end of the widest scene.  A core that touches a window edge does so where the scene ends: at the right
    (x = W), the bottom (y = H) and the top; it then owns the scene's last corner column or row as well."""
    from deepmerge_amd import scene
    rng = np.random.default_rng(shape[0])
    window = rng.integers(0, 3, shape).astype(np.int32)
    window[shape[0] // 2:, : shape[1] // 2] = 1
    scene_h = 2000
    oy = 0 if core[0] == 0 else (scene_h - shape[0] if core[1] == shape[0] else 600)       # 600 (2^31 - 1) > 2^40
    ox = BIG_W - shape[1] - (5 if core[3] < shape[1] else 0)
    if shape == (1, 1):
        scene_h, oy, ox = 1, 0, 0                                  # a window without any apron is the whole scene
    scene_w = BIG_W if shape != (1, 1) else 1
    want = SR.tile_nodes(window, core, (oy, ox), scene_h, scene_w)
    t = dev(window)
    got = scene._tile_nodes(t, core, (oy, ox), scene_h, scene_w)
    assert torch.equal(t.cpu(), torch.from_numpy(window))
    assert got.dtype == torch.int64 and np.array_equal(np.sort(got.cpu().numpy()), want)
    if shape != (1, 1):
        assert len(want) > 4 and int(want.max()) > 1 << (40 if oy else 36)


def test_a_core_without_a_node_leaves_no_record():
    from deepmerge_amd import scene
    assert scene._tile_nodes(dev(np.zeros((5, 5), np.int32)), (1, 4, 1, 4), (10, 10), 100, 100) is None


# ---- the chain, arc and ring kernels far from the origin ---------------------------------------------------------------------------------
def tables(name, H, W, shift=(0, 0)):
    """rag._trace of a raster and its nodes, translated by shift = (ox, oy) into an H x W scene."""
    from deepmerge_amd import rag
    labels, n = raster(name)
    t = dev(labels)
    polys, arcs = rag._trace(t, n)
    keep = rag._simplify(t, n, 0)[2]
    at = torch.nonzero(keep == 2).squeeze(1)
    w1 = labels.shape[1] + 1
    y, x = torch.div(at, w1, rounding_mode="floor"), at % w1
    node_row = torch.sort((y + shift[1]) * (W + 1) + x + shift[0]).values
    move = torch.tensor(shift, dtype=torch.int32, device=DEV)
    polys.xy, arcs.xy = polys.xy + move, arcs.xy + move
    return polys, arcs, node_row


@pytest.mark.parametrize("name", ["random_130", "frame_hole", "slic"])
def test_the_kernels_on_a_translated_set_give_the_untranslated_answer_shifted(name):
    """The set is moved by (2^31 - 40000, 2^29 - 1000) to the far corner of a scene of 2^29 x (2^31 - 2) pixels (at most 2^60 pixels
    bound the product of the sides: 2^29 rows are all a scene this wide has).  Corner ids reach almost 2^60; arc_keep is found by
    position and does not change, the vertices are the untranslated ones shifted, and ring_area2 is the int64 shoelace sum of the
    shifted vertices."""
    from deepmerge_amd import rag, scene
    labels, n = raster(name)
    h, w = labels.shape
    H, W, shift = 1 << 29, BIG_W, ((1 << 31) - 40000, (1 << 29) - 1000)
    for tol in (0, 1.5, 4096):
        q = rag._quantise_tolerance(tol)
        near = scene._simplify_tables(*tables(name, h, w), h, w, q)
        far = scene._simplify_tables(*tables(name, H, W, shift), H, W, q)
        assert_same(near[:2], whole(name, tol), (name, tol))
        dense = rag._simplify(dev(labels), n, tol)[2]
        arcs = near[1]
        assert torch.equal(near[2], far[2]) and near[2].dtype == torch.uint8
        move = torch.tensor(shift, dtype=torch.int32, device=DEV)
        assert torch.equal(far[0].xy, near[0].xy + move) and torch.equal(far[1].xy, near[1].xy + move)
        for f in ("ring_ptr", "region_ptr", "ring_label"):
            assert torch.equal(getattr(far[0], f), getattr(near[0], f)), f
        assert torch.equal(far[1].arc_ptr, near[1].arc_ptr)
        xy, ptr = far[0].xy.cpu().numpy().astype(np.int64), far[0].ring_ptr.cpu().numpy()
        area2 = []
        for r in range(len(ptr) - 1):
            p = xy[ptr[r]:ptr[r + 1]]
            nxt = np.roll(p, -1, 0)
            area2.append(int((p[:, 0] * nxt[:, 1] - nxt[:, 0] * p[:, 1]).sum()))      # terms near 2^60; a translation leaves the sum alone
        assert far[0].ring_area2.cpu().tolist() == area2 == near[0].ring_area2.cpu().tolist()
        # arc_keep against the dense flags: wherever the chain pass looks (the positions below len), the two agree
        traced = rag._trace(dev(labels), n)[1]
        ids = traced.xy[:, 1].long() * (w + 1) + traced.xy[:, 0].long()
        written = near[2] != 0
        assert bool((dense[ids[written]] == near[2][written]).all())
        assert int((near[2] == 1).sum()) == int((dense == 1).sum())
        assert arcs.xy.shape[0] == int(whole(name, tol)[1].xy.shape[0])


def test_an_arc_wider_than_32768_raises_and_the_kernel_leaves_it_alone():
    from deepmerge_amd import _lib, rag, scene
    from deepmerge_amd.ops import _stream
    lib = _lib.lib()
    H, W = 50000, 50000
    wide = [[0, 10], [3, 10], [3, 14], [32770, 14], [32770, 20], [50000, 20]]                 # 50000 wide
    stair = [[10, 0], [10, 4], [14, 4], [14, 9], [20, 9], [20, 50000]]                        # 10 wide, 50000 tall: refused as well
    small = [[100, 0], [100, 4], [104, 4], [104, 9], [32868, 9], [32868, 20]]                 # exactly 32768 wide: simplified
    xy = dev(np.array(wide + stair + small, np.int32))
    ptr = dev(np.array([0, 6, 12, 18], np.int64))
    ends = [0, 5, 6, 11, 12, 17]
    keep = torch.zeros(18, dtype=torch.uint8, device=DEV)
    keep[ends] = 2
    stack = torch.empty(18, dtype=torch.int64, device=DEV)
    rc = lib.dm_scene_simplify_chains(xy.data_ptr(), ptr.data_ptr(), 3, 18, H, W, 0, keep.data_ptr(), stack.data_ptr(), _stream())
    assert rc == 0
    assert keep.tolist() == [2, 0, 0, 0, 0, 2] + [2, 0, 0, 0, 0, 2] + [2, 1, 1, 1, 1, 2]
    arcs = rag.Arcs(arc_ptr=ptr, xy=xy, left=dev(np.array([7, -1, 9], np.int32)), right=dev(np.array([2, 3, 4], np.int32)))
    ring = dev(np.array([[0, 0], [W, 0], [W, H], [0, H]], np.int32))
    polys = rag.Polygons(region_ptr=dev(np.array([0, 1], np.int32)), ring_ptr=dev(np.array([0, 4], np.int64)), xy=ring,
                         ring_label=dev(np.array([0], np.int32)), ring_area2=dev(np.array([2 * H * W], np.int64)))
    nodes = torch.sort(xy[ends, 1].long() * (W + 1) + xy[ends, 0].long()).values
    with pytest.raises(ValueError, match=r"between \(left, right\) = \((7, 2|-1, 3)\) spans (50000 x 10|10 x 50000) pixels"):
        scene._simplify_tables(polys, arcs, nodes, H, W, 0)


def test_an_unsorted_node_list_is_an_error_code_not_a_wild_read():
    """[[0, 0, 0], [1, 2, 2]]: label 0's run from (3, 1) to (0, 1) holds the T-junction (1, 1), id 5.  With 5 and 7 swapped in
    node_row the range found for the run holds id 7, outside the run: status is set and nothing outside the lists is read."""
    from deepmerge_amd import _lib, rag
    from deepmerge_amd.ops import _stream
    lib = _lib.lib()
    L = np.array([[0, 0, 0], [1, 2, 2]], np.int32)
    polys, _ = rag._trace(dev(L), 3)
    want = SR.simplify(L, 3, 0, (2, 3))
    V_, R_ = polys.xy.shape[0], polys.ring_label.numel()
    vert_ring = (torch.searchsorted(polys.ring_ptr, torch.arange(V_, device=DEV), right=True) - 1).to(torch.int32)
    for rows, flagged in ((want["node_row"], 0), (np.array([0, 3, 4, 7, 5, 8, 9, 11], np.int64), 1)):
        node_row, node_col, kept_row = dev(rows), dev(want["node_col"]), dev(want["kept_row"])
        status, count = torch.full((1,), 7, dtype=torch.int32, device=DEV), torch.empty(V_, dtype=torch.int32, device=DEV)
        t = _lib.DmSceneSimplifyRings()
        for f, v in (("xy", polys.xy), ("ring_ptr", polys.ring_ptr), ("vert_ring", vert_ring), ("node_row", node_row), ("node_col", node_col),
                     ("kept_row", kept_row), ("status", status)):
            setattr(t, f, v.data_ptr())
        t.n_nodes, t.n_kept, t.scene_h, t.scene_w, t.V, t.R = 8, len(want["kept_row"]), 2, 3, V_, R_
        assert lib.dm_scene_simplify_ring_count(ctypes.byref(t), count.data_ptr(), _stream()) == 0
        scan = torch.zeros(V_ + 1, dtype=torch.int64, device=DEV)
        scan[1:] = torch.cumsum(count, 0)
        Vn = int(scan[-1])
        out, area2 = torch.full((Vn, 2), -1, dtype=torch.int32, device=DEV), torch.empty(R_, dtype=torch.int64, device=DEV)
        new_ptr = scan[polys.ring_ptr]
        assert lib.dm_scene_simplify_ring_emit(ctypes.byref(t), scan.data_ptr(), new_ptr.data_ptr(), Vn, out.data_ptr(), area2.data_ptr(), _stream()) == 0
        assert int(status) == flagged
        if not flagged:
            assert np.array_equal(out.cpu().numpy(), want["xy"]) and area2.cpu().tolist() == want["ring_area2"].tolist()


def test_inputs_are_unmodified_and_two_calls_and_a_side_stream_agree():
    from deepmerge_amd import scene
    labels, n = raster("slic")
    before = labels.copy()
    first = scene.simplify_labels(labels, n, 1.5, (64, 96))
    assert_same(scene.simplify_labels(torch.from_numpy(labels), n, 1.5, (64, 96)), first)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = scene.simplify_labels(labels, n, 1.5, (64, 96))
    side.synchronize()
    assert_same(got, first)
    assert_same(first, whole("slic", 1.5))
    assert np.array_equal(labels, before)


def test_every_value_error_is_raised():
    from deepmerge_amd import scene
    labels, n = raster("frame_island")
    for tol in (-1, float("nan"), 4097):
        with pytest.raises(ValueError, match="tolerance"):
            scene.simplify_labels(labels, n, tol)
    for bad, kw in ((labels.astype(np.int64), {}), (labels[None], {}), (labels, dict(tile=0))):
        with pytest.raises(ValueError):
            scene.simplify_labels(bad, n, 1.5, **kw)
    wrong = np.zeros((6, 8), np.int32)
    wrong[5, 7] = 2
    with pytest.raises(ValueError, match="window of tile 3 .*holds 0..2"):
        scene.simplify_labels(wrong, 2, 1.5, tile=(3, 4))


# ---- SceneResult.simplified / save_shapefiles -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def merged_scene():
    """tests/test_gpu_scene_vector.py's scene (200 x 232 in tiles of 96 x 112) and the one-tile pipeline on its assembled raster."""
    from deepmerge_amd import scene
    from deepmerge_amd.ExtractFeatures import FeatureIO
    from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3
    torch.manual_seed(1)
    net = ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=[32, 64, 128], depth=[1, 1, 1], in_c=3, numerics="fp32")
    fio = FeatureIO(net, None, DEV)
    image = TV.scene_image()
    g = scene._scene_graph(image, tile=TV.TILE, segmenter=TV.slic24, k=1, device=DEV)
    S0, whole_image, raster_ = g["n_labels"], dev(image), dev(g["labels"])
    first, _ = fio.merge_tile(whole_image, raster_, S0, k=1, margin=1.0, batch_size=1, max_rounds=0)
    margin = float(first.simi.float().median())
    want, _ = fio.merge_tile(whole_image, raster_, S0, k=1, margin=margin, batch_size=1)
    res = fio.segment_scene(image, tile=TV.TILE, segmenter=TV.slic24, k=1, margin=margin, batch_size=1)
    return fio, res, want, raster_


def test_scene_result_simplified_equals_merge_tile_on_the_assembled_raster(merged_scene):
    fio, res, want, raster_ = merged_scene
    assert torch.equal(res.result.region_of, want.region_of) and torch.equal(res.result.edges, want.edges)
    merged = res.write_merged()
    assert (merged[95] == merged[96]).any() or (merged[:, 111] == merged[:, 112]).any()       # a merged region lies on both sides of a seam
    want_polys, want_arcs = want.simplified(raster_, 1.5)
    stats = {}
    got = res.simplified(1.5, stats=stats)
    assert_same(got, (want_polys, want_arcs))
    assert got[1].edge.dtype == torch.int32 and torch.equal(got[1].edge, want_arcs.edge) and bool((got[1].edge >= 0).any())
    assert stats["kept_vertices"] < stats["vertices"] and stats["tiles"] == 9
    assert_same(res.simplified(1.5, merged=merged, tile=(50, 77)), (want_polys, want_arcs))
    C = int(res.result.rep.numel())
    assert_same(fio.simplify_scene(merged, C, 1.5, tile=(50, 77)), (want_polys, want_arcs))


def test_scene_result_save_shapefiles_with_a_tolerance(merged_scene, tmp_path):
    from deepmerge_amd import shpstore
    _, res, _, _ = merged_scene
    plain = res.save_shapefiles(str(tmp_path / "plain"))
    none = res.save_shapefiles(str(tmp_path / "none"), tolerance=None)
    for a, b in zip(plain, none):
        for ext in (".shp", ".shx", ".dbf"):
            assert open(a[:-4] + ext, "rb").read() == open(b[:-4] + ext, "rb").read(), (a, ext)
    polys, arcs = res.simplified(1.5)
    paths = res.save_shapefiles(str(tmp_path / "simple"), tolerance=1.5)
    assert [p.rsplit("/", 1)[1] for p in paths] == ["polygons.shp", "lines.shp"]
    C = int(res.result.rep.numel())
    got = shpstore.ShapeReader(paths[0])
    assert got.shape_type == 5 and len(got) == C
    region_ptr, ring_ptr, xy = polys.region_ptr.cpu().numpy(), polys.ring_ptr.cpu().numpy(), polys.xy.cpu().numpy().astype(np.float64)
    for l in range(C):
        rings = range(region_ptr[l], region_ptr[l + 1])
        assert len(got.shapes[l]) == len(rings) >= 1
        for part, ring in zip(got.shapes[l], rings):
            p = xy[ring_ptr[ring]:ring_ptr[ring + 1]]
            assert np.array_equal(part[:-1], np.stack((p[:, 0], -p[:, 1]), 1)) and np.array_equal(part[-1], part[0])
    lines = shpstore.ShapeReader(paths[1])
    arc_ptr, arc_xy = arcs.arc_ptr.cpu().numpy(), arcs.xy.cpu().numpy().astype(np.float64)
    assert lines.shape_type == 3 and len(lines) == arcs.left.numel()
    for a, shape in enumerate(lines.shapes):
        p = arc_xy[arc_ptr[a]:arc_ptr[a + 1]]
        assert len(shape) == 1 and np.array_equal(shape[0], np.stack((p[:, 0], -p[:, 1]), 1))
    assert lines.fields["LEFT_FID"].tolist() == arcs.left.tolist() and lines.fields["RIGHT_FID"].tolist() == arcs.right.tolist()
    assert open(paths[0], "rb").read() != open(plain[0], "rb").read()          # the staircase is gone
    assert not (tmp_path / "simple" / "PointsGCS.shp").exists()
