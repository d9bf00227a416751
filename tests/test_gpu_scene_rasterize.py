"""GPU: polygon rings rasterised on a scene (deepmerge_amd/scene.py RingSource, rasterize_rings, labels_from_shapefile;
csrc/dm_scene_rasterize.hip).  The definition is the test: every box a RingSource reads is the slice of
`rag.rasterize` on the whole raster, bit for bit, and the numpy spec (tests/scene_rasterize_ref.py, tests/rasterize_ref.py) where the
whole raster cannot exist; the scene calls take a RingSource in place of a host raster and return what they return on that raster."""
import functools

import numpy as np
import pytest
import torch

import rasterize_ref as Z
import scene_rasterize_ref as S
import slic_ref as R
import vector_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NORTH_UP = (500000.0, 0.5, 0.0, 4100000.0, 0.0, -0.5)
CASES = Z.cases()
WINDOW_CASES = S.window_cases()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rings_of(packed):
    from deepmerge_amd import rag
    ptr, xy, label = packed
    return rag.Rings(dev(ptr), dev(xy), dev(label))


def case(name):
    return CASES[name] if name in CASES else WINDOW_CASES[name][:3]


@functools.lru_cache(maxsize=None)
def spec(name, fill=-1):
    (ptr, xy, label), H, W = case(name)
    return Z.rasterize(ptr, Z.quantise(xy), label, H, W, fill)


@functools.lru_cache(maxsize=None)
def whole(name, fill=-1):
    """The reference, once per case: rag.rasterize on the whole raster."""
    from deepmerge_amd import rag
    packed, H, W = case(name)
    return rag.rasterize(rings_of(packed), H, W, fill).cpu().numpy()


# ---- the definition ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_every_tiling_equals_the_whole_raster_and_the_spec(name):
    from deepmerge_amd import scene
    packed, H, W = CASES[name]
    rings = rings_of(packed)
    before = [t.clone() for t in (rings.ring_ptr, rings.xy, rings.ring_label)]
    assert np.array_equal(whole(name), spec(name))
    for tile in S.tilings(H, W):
        stats = {}
        got = scene.rasterize_rings(rings, H, W, tile=tile, stats=stats)
        print(f"{name} {tile}: pixels that differ = {(got != whole(name)).sum()}, events per band = {list(stats['events'].values())[:4]}")
        assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, whole(name)), (name, tile)
        grid = scene.tile_grid(H, W, tile)
        assert stats["tiles"] == len(grid) and set(stats["events"]) == {(y0, y1) for y0, y1, _, _ in grid}
        assert all(v % 2 == 0 for v in stats["events"].values())
    for a, b in zip(before, (rings.ring_ptr, rings.xy, rings.ring_label)):
        assert torch.equal(a, b)                                   # the inputs are not modified


@pytest.mark.parametrize("name", list(CASES))
def test_unaligned_boxes_equal_the_slice(name):
    from deepmerge_amd import scene
    packed, H, W = CASES[name]
    source = scene.RingSource(rings_of(packed), H, W, fill=-4)
    assert source.shape == (H, W) and source.n_labels == (int(packed[2].max()) + 1 if packed[2].size else 1)
    for box in S.boxes(H, W):
        y0, y1, x0, x1 = box
        got = source.read(*box)
        assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (y1 - y0, x1 - x0) and got.is_contiguous()
        assert np.array_equal(got.cpu().numpy(), whole(name, -4)[y0:y1, x0:x1]), (name, box)


# ---- where a window can go wrong -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(WINDOW_CASES))
def test_where_a_window_can_go_wrong(name):
    from deepmerge_amd import scene
    packed, H, W, tiles = WINDOW_CASES[name]
    rings = rings_of(packed)
    assert np.array_equal(whole(name), spec(name))
    for tile in tiles:
        got = scene.rasterize_rings(rings, H, W, tile=tile)
        print(f"{name} {tile}: pixels that differ = {(got != spec(name)).sum()}")
        assert np.array_equal(got, spec(name)), (name, tile)
    source = scene.RingSource(rings, H, W)
    for box in S.boxes(H, W, n=3):
        y0, y1, x0, x1 = box
        assert np.array_equal(source.read(*box).cpu().numpy(), spec(name)[y0:y1, x0:x1]), (name, box)


def test_overlapping_labels_across_a_seam_do_not_depend_on_ring_order():
    from deepmerge_amd import scene
    a, b = (scene.rasterize_rings(rings_of(WINDOW_CASES[n][0]), 30, 100, tile=(15, 50)) for n in ("overlap_ab_across_seam", "overlap_ba_across_seam"))
    assert np.array_equal(a, b) and a[12, 49] == 5 and a[12, 50] == 5 and a[5, 50] == 3


@pytest.mark.parametrize("name", ["hole_same_orientation", "random_300", "only_degenerate_rings", "band_without_event", "no_rings"])
def test_fill_value(name):
    from deepmerge_amd import scene
    packed, H, W = case(name)
    got = scene.rasterize_rings(rings_of(packed), H, W, tile=(7, 5) if H < 64 else (37, 41), fill=-7)
    assert np.array_equal(got, spec(name, -7)) and ((got == -7) == (spec(name) == -1)).all()
    out = np.zeros((H, W), np.int32)
    assert scene.rasterize_rings(rings_of(packed), H, W, tile=64, fill=-(1 << 31), labels_out=out) is out
    assert np.array_equal(out, spec(name, -(1 << 31)))


# ---- round trip with no host raster ----------------------------------------------------------------------------------------------------------
def _blocks(H, W, seed):
    labels, n = R.connected_labels(R.block_image(1, H, W, 37, seed, noise=0)[0].astype(np.int32))
    return labels.astype(np.int32), int(n)


@functools.lru_cache(maxsize=None)
def raster(name):                                                  # the rasters tests/test_gpu_scene_vector.py traces, by the same names
    if name == "blocks":
        return _blocks(96, 128, 3)
    if name == "comb":
        return V.comb_of_combs(130), 2
    if name == "one_label":
        return np.zeros((70, 150), np.int32), 1
    if name == "frame_hole":
        frame = np.zeros((80, 90), np.int32)
        frame[20:60, 25:70] = 1
        return frame, 2
    if name == "random_130":
        return np.random.default_rng(11).integers(0, 5, (130, 130)).astype(np.int32), 5
    if name == "slic":
        from deepmerge_amd import rag
        tile = R.block_image(3, 257, 190, 37, 2)
        labels, n = rag.slic(dev(tile), cell=16, compactness=10, iters=3)
        return labels.cpu().numpy(), int(n)
    raise KeyError(name)


RASTERS = ["blocks", "comb", "one_label", "frame_hole", "random_130", "slic"]
FIELDS = ("region_ptr", "ring_ptr", "xy", "ring_label", "ring_area2")
ARC_FIELDS = ("arc_ptr", "xy", "left", "right")


@pytest.mark.parametrize("name", RASTERS)
def test_tracing_a_ring_source_equals_tracing_the_raster(name):
    from deepmerge_amd import rag, scene
    labels, n = raster(name)
    H, W = labels.shape
    polys = rag.polygons(dev(labels), n)
    want = rag._trace(dev(labels), n)
    for tile in ((37, 41), (64, 3)) if name != "slic" else ((37, 41),):
        got = scene.trace_labels(scene.RingSource(polys, H, W), n, tile)
        for f in FIELDS:
            assert torch.equal(getattr(got[0], f), getattr(want[0], f)), (name, tile, "polygons", f)
        for f in ARC_FIELDS:
            assert torch.equal(getattr(got[1], f), getattr(want[1], f)), (name, tile, "arcs", f)


@pytest.mark.parametrize("name", RASTERS)
def test_trace_then_rasterize_with_another_tile_is_the_raster(name):
    from deepmerge_amd import scene
    labels, n = raster(name)
    H, W = labels.shape
    for a, b in (((37, 41), (64, 3)), ((3, 64), (1 << 12, 1 << 12))) if name != "slic" else (((37, 41), (50, 64)),):
        polys = scene.trace_labels(labels, n, tile=a)[0]
        got = scene.rasterize_rings(polys, H, W, tile=b)
        print(f"{name} traced in {a}, rasterised in {b}: pixels that differ = {(got != labels).sum()}")
        assert np.array_equal(got, labels), (name, a, b)


def test_label_graph_takes_a_ring_source_for_the_host_raster():
    from deepmerge_amd import rag, scene
    labels, n = raster("blocks")
    H, W = labels.shape
    image = R.block_image(3, H, W, 37, 3)
    source = scene.RingSource(rag.polygons(dev(labels), n), H, W)
    kw = dict(tile=(40, 50), k=2, max_window=32, device=DEV)
    got, want = scene.label_graph(image, source, n, **kw), scene.label_graph(image, labels, n, **kw)
    for key in ("count", "sum", "sumsq", "peri", "bbox"):
        assert torch.equal(got["stats"][key], want["stats"][key]), key
    for key in ("designed", "edges", "weights"):
        assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), key
    for f in ("xy", "label", "inner", "obj", "ptr", "idx", "bbox", "round"):
        assert torch.equal(getattr(got["points"], f), getattr(want["points"], f)), f
    assert got["labels"] is source and got["n_seam"] == want["n_seam"] and got["n_seam_edges"] == want["n_seam_edges"]
    pts = scene.sample_points(source, n, k=2, max_window=32, tile=(33, 47), device=DEV)
    assert torch.equal(pts.xy, want["points"].xy) and torch.equal(pts.label, want["points"].label)


# ---- beyond rag.rasterize's range ------------------------------------------------------------------------------------------------------------
def test_a_scene_of_2_to_the_40_pixels():
    from deepmerge_amd import rag, scene
    (ptr, xy, label), H, W, boxes = S.big_scene()
    q = Z.quantise(xy)
    rings = rings_of((ptr, xy, label))
    with pytest.raises(ValueError, match="2\\^31"):
        rag.rasterize(rings, H, W)
    source = scene.RingSource(rings, H, W)
    assert source.shape == (1 << 20, 1 << 20) and source.n_labels == (1 << 31) - 1
    seen = set()
    for box in boxes:
        want = S.translated(ptr, q, label, box)                    # (the spec's own < 2^60 asserts run here, on the CPU, first)
        got = source.read(*box).cpu().numpy()
        print(f"box {box}: labels {np.unique(want).tolist()}, pixels that differ = {(got != want).sum()}, events = {source.events[box[:2]]}")
        assert np.array_equal(got, want), box
        seen |= set(np.unique(got).tolist())
    assert seen == {-1, 3, 5, 7, 11, (1 << 31) - 2}
    with pytest.raises(ValueError, match="2\\^63"):                # (2^31 - 1) 2^12 (2^20 + 1) >= 2^63
        source.read(0, 1 << 12, 0, 16)
    with pytest.raises(ValueError, match="2\\^31 pixels"):
        source.read(0, 1 << 11, 0, 1 << 20)


# ---- errors -----------------------------------------------------------------------------------------------------------------------------------
def test_keys_that_do_not_pair_raise_for_every_box_of_their_band():
    """The rule closes every ring, so no `Rings` gives a (label, row) an odd count; the keys of an unclosed ring are made here from a
    band's sorted keys by moving one key to the next row, and put where the source keeps its band."""
    from deepmerge_amd import _lib, scene
    from deepmerge_amd.ops import _stream
    packed, H, W = (Z.pack([(1, Z._square(2, 2, 8, 8)), (2, Z._square(30, 12, 38, 18))]), 20, 40)
    source = scene.RingSource(rings_of(packed), H, W)
    good = source.read(0, 10, 0, 40)
    keys = source._keys.clone()
    assert keys.numel() == 12 and np.array_equal(good.cpu().numpy(), spec_of(packed, H, W)[0:10])
    source._keys = torch.sort(torch.cat((keys[:-1], keys[-1:] + (W + 1)))).values            # the last pair now names two rows
    for box in ((0, 10, 0, 40), (0, 10, 0, 5), (0, 10, 20, 40), (0, 10, 39, 40)):             # the last two meet no span of the band
        with pytest.raises(RuntimeError, match="not closed"):
            source.read(*box)
    assert np.array_equal(source.read(10, 20, 0, 40).cpu().numpy(), spec_of(packed, H, W)[10:20])    # another band is not affected
    assert torch.equal(source.read(0, 10, 0, 40), good)                                       # and the band is made afresh
    out, error = torch.empty((10, 5), dtype=torch.int32, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV)
    neg = torch.tensor([-1, 3], dtype=torch.int64, device=DEV)
    assert _lib.lib().dm_rasterize_fill_window(neg.data_ptr(), 2, H, W, 0, 10, 20, 25, -1, out.data_ptr(), error.data_ptr(), _stream()) == 0
    assert int(error) == 1 and bool((out == -1).all())
    assert _lib.lib().dm_rasterize_fill_window(keys.data_ptr(), 12, H, W, 0, 10, 20, 25, -1, out.data_ptr(), error.data_ptr(), _stream()) == 0
    assert int(error) == 0                                         # cleared by the call


def spec_of(packed, H, W, fill=-1):
    ptr, xy, label = packed
    return Z.rasterize(ptr, Z.quantise(xy), label, H, W, fill)


def test_every_value_error_is_raised():
    from deepmerge_amd import rag, scene
    (ptr, xy, label), H, W = CASES["fractional_triangle"]
    ok = lambda **kw: rag.Rings(dev(kw.get("ptr", ptr)), dev(kw.get("xy", xy)), dev(kw.get("label", label)))
    bad_xy, far_xy = xy.copy(), xy.copy()
    bad_xy[1, 0] = np.nan
    far_xy[0, 1] = -(2.0 ** 20) - 1
    for rings, match in ((ok(xy=bad_xy), "2\\^20"), (ok(xy=far_xy), "2\\^20"), (ok(label=np.array([-1], np.int32)), "ring labels"),
                         (ok(ptr=np.array([0, 2])), "ring_ptr"), (ok(ptr=ptr.astype(np.int32)), "ring_ptr"),
                         (ok(xy=xy.astype(np.float32)), "xy must be"), (ok(label=label.astype(np.int64)), "ring_label")):
        with pytest.raises(ValueError, match=match):
            scene.RingSource(rings, H, W)
    for kw in ({"fill": 0}, {"fill": 3}, {"fill": -(1 << 31) - 1}):
        with pytest.raises(ValueError, match="fill"):
            scene.RingSource(ok(), H, W, **kw)
    for h, w in ((0, 5), (5, 0), (1 << 31, 5), (5, 1 << 31)):
        with pytest.raises(ValueError, match="H, W"):
            scene.RingSource(ok(), h, w)
    assert scene.RingSource(ok(), (1 << 31) - 1, (1 << 31) - 1).shape == ((1 << 31) - 1, (1 << 31) - 1)
    source = scene.RingSource(ok(), H, W)
    for box in ((0, 0, 0, 5), (3, 2, 0, 5), (0, H + 1, 0, 5), (0, 5, -1, 5), (0, 5, 4, 4), (0, 5, 0, W + 1)):
        with pytest.raises(ValueError, match="inside the scene"):
            source.read(*box)
    for out in (np.zeros((H, W), np.int64), np.zeros((H, W + 1), np.int32), np.zeros(H * W, np.int32), torch.zeros((H, W), dtype=torch.int32)):
        with pytest.raises(ValueError, match="labels_out"):
            scene.rasterize_rings(ok(), H, W, labels_out=out)
    with pytest.raises(ValueError, match="tile"):
        scene.rasterize_rings(ok(), H, W, tile=0)
    with pytest.raises(ValueError, match="2\\^31 pixels"):
        scene.rasterize_rings(ok(), 1 << 20, 1 << 20, tile=(1 << 16, 1 << 15), labels_out=np.zeros((1, 1), np.int32))


# ---- the cache --------------------------------------------------------------------------------------------------------------------------------
def test_interleaved_bands_and_repeated_boxes_read_the_same_pixels():
    from deepmerge_amd import scene
    packed, H, W = CASES["random_300"]
    rings = rings_of(packed)
    before = [t.clone() for t in (rings.ring_ptr, rings.xy, rings.ring_label)]
    source = scene.RingSource(rings, H, W)
    a, b = [(10, 47, x, x + 41) for x in (0, 41, 82, 123)], [(90, 150, x, x + 50) for x in (120, 60, 0)]
    first = {box: source.read(*box).clone() for box in a + b}     # band by band: two event passes
    assert len(source.events) == 2
    for box in [v for pair in zip(a, b) for v in pair] + [a[3], a[3], b[0], b[0]]:           # interleaved, then every box twice
        got = source.read(*box)
        y0, y1, x0, x1 = box
        assert torch.equal(got, first[box]) and np.array_equal(got.cpu().numpy(), whole("random_300")[y0:y1, x0:x1]), box
    for t, u in zip(before, (rings.ring_ptr, rings.xy, rings.ring_label)):
        assert torch.equal(t, u)                                   # the ring tensors are unchanged after all reads
    q = torch.from_numpy(Z.quantise(packed[1]).astype(np.int32)).to(DEV)
    assert torch.equal(source.q, q)                                # and so are the resident vertices


# ---- shapefiles ---------------------------------------------------------------------------------------------------------------------------------
def test_shapefile_round_trip(tmp_path):
    from deepmerge_amd import rag, scene, shpstore
    labels, n = raster("blocks")
    H, W = labels.shape
    polys = scene.trace_labels(labels, n, tile=(37, 41))[0]
    path = shpstore.write_polygons(str(tmp_path / "polygons.shp"), polys, [("ID", np.arange(n, dtype=np.int32))], NORTH_UP)
    want, n_want = rag.labels_from_shapefile(path, H, W, NORTH_UP)
    got, n_got = scene.labels_from_shapefile(path, H, W, NORTH_UP, tile=(40, 50))
    assert n_got == n_want == n and isinstance(got, np.ndarray) and np.array_equal(got, want.cpu().numpy()) and np.array_equal(got, labels)
    perm = np.random.default_rng(5).permutation(n).astype(np.int32) + 4
    path = shpstore.write_polygons(str(tmp_path / "perm.shp"), polys, [("LBL", perm)], NORTH_UP)
    want, n_want = rag.labels_from_shapefile(path, H, W, NORTH_UP, label_field="LBL", fill=-3)
    out = np.zeros((H, W), np.int32)
    got, n_got = scene.labels_from_shapefile(path, H, W, NORTH_UP, label_field="LBL", fill=-3, tile=(33, 128), labels_out=out)
    assert got is out and n_got == n_want == n + 4 and np.array_equal(got, want.cpu().numpy()) and np.array_equal(got, perm[labels])
    source, n_src = scene.labels_from_shapefile(path, H, W, NORTH_UP, label_field="LBL", fill=-3, as_source=True)
    assert isinstance(source, scene.RingSource) and n_src == n + 4 and source.n_labels == n + 4 and source.shape == (H, W)
    for y0, y1, x0, x1 in S.boxes(H, W, n=3):
        assert torch.equal(source.read(y0, y1, x0, x1), want[y0:y1, x0:x1])
    with pytest.raises(ValueError, match="2\\^20"):                # read without its transform the rings lie millions of pixels away
        scene.labels_from_shapefile(path, H, W)
