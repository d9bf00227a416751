"""GPU: SLIC on a scene larger than one tile (deepmerge_amd/scene.py: slic_assign, slic_labels, segment_scene(cross_seams=True);
csrc/dm_scene_slic.hip, csrc/dm_slic_pass.h).  The definition is the test: whatever the tile size, `scene.slic_assign` returns the
centres and the assigned raster of `rag.slic_assign` on the whole scene and `scene.slic_labels` the raster and count of `rag.slic`
on the whole scene, bit for bit (`rag.slic` itself is pinned to tests/slic_ref.py by tests/test_gpu_slic.py).  Every comparison is
array equality."""
import numpy as np
import pytest
import torch

import slic_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 200, 232
TILES = ((96, 112), (200, 232), (37, 41), (64, 64))               # widths 112, 64: 16-byte strips; 232, 41 and the slivers: scalar
IMAGES = {"blocks": lambda: R.block_image(3, H, W, 23, 1), "noise": lambda: R.noise_image(3, H, W, 2)}
CELL, COMPACTNESS = 12, 10


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_whole = {}


def whole(key, img, cell, compactness, iters, min_size=None):
    """Once per case, shared and never modified: (assigned, centres, labels, n) of the one-tile calls on the whole scene, as numpy."""
    if key not in _whole:
        from deepmerge_amd import rag
        t = dev(img)
        assigned, centres = rag.slic_assign(t, cell, compactness, iters)
        labels, n = rag.slic(t, cell, compactness, iters, min_size)
        _whole[key] = (assigned.cpu().numpy(), centres.cpu().numpy(), labels.cpu().numpy(), n)
    return _whole[key]


def crosses_a_seam(labels, tile):
    """A region of `labels` has pixels in two cores of `tile`."""
    th, tw = tile
    yy, xx = np.mgrid[0:labels.shape[0], 0:labels.shape[1]]
    core = (yy // th) * (-(-labels.shape[1] // tw)) + xx // tw
    n = int(labels.max()) + 1
    lo, hi = np.full(n, 1 << 30), np.full(n, -1)
    np.minimum.at(lo, labels.reshape(-1), core.reshape(-1))
    np.maximum.at(hi, labels.reshape(-1), core.reshape(-1))
    return bool((lo != hi).any())


def check_scene(img, tile, want, cell, compactness, iters, min_size=None, **kw):
    from deepmerge_amd import scene
    assigned, centres, labels, n = want
    got_assigned, got_centres = scene.slic_assign(img, tile=tile, cell=cell, compactness=compactness, iters=iters, device=DEV, **kw)
    assert got_centres.dtype == torch.int32 and got_centres.is_cuda and np.array_equal(got_centres.cpu().numpy(), centres), tile
    assert got_assigned.dtype == np.int32 and np.array_equal(got_assigned, assigned), tile
    stats = {}
    got, m = scene.slic_labels(img, tile=tile, cell=cell, compactness=compactness, iters=iters, min_size=min_size, device=DEV, stats=stats, **kw)
    print(f"tile {tile}: n = {m}, {stats}")
    assert got.dtype == np.int32 and m == n and np.array_equal(got, labels), tile
    assert stats["provisional"] >= stats["components"] >= m == stats["n_labels"] and stats["rounds"] == len(stats["picks"])
    return stats


@pytest.mark.parametrize("iters", [0, 3])
@pytest.mark.parametrize("name", sorted(IMAGES))
def test_scene_slic_equals_the_whole_scene_for_every_tile_size(name, iters):
    img = IMAGES[name]()
    want = whole((name, iters), img, CELL, COMPACTNESS, iters)
    assert crosses_a_seam(want[2], (96, 112)) and want[3] > 4      # not vacuous: the final regions do cross seams
    for tile in TILES:
        stats = check_scene(img, tile, want, CELL, COMPACTNESS, iters)
        single = tile == (H, W)
        assert (stats["seam_unions"] == 0 and stats["provisional"] == stats["components"]) if single else stats["seam_unions"] > 0


@pytest.mark.parametrize("iters", [0, 3])
def test_tiles_smaller_than_a_cell(iters):
    img = R.block_image(3, 40, 77, 11, 5)
    want = whole(("small", iters), img, 9, COMPACTNESS, iters)
    for tile in ((5, 7), (1, 77)):
        check_scene(img, tile, want, 9, COMPACTNESS, iters)


@pytest.mark.parametrize("bands", [1, 3, 4, 5])
def test_every_band_count(bands):
    """Five bands: only the first four are used, here and in rag.slic."""
    img = R.block_image(bands, 90, 100, 17, 10 + bands, noise=30)
    want = whole(("bands", bands), img, 8, 20, 2)
    for tile in ((37, 41), (48, 64)):
        check_scene(img, tile, want, 8, 20, 2)
    if bands == 5:
        four = whole(("bands", "first four of five"), img[:4], 8, 20, 2)
        assert np.array_equal(four[2], want[2]) and np.array_equal(four[1], want[1])


def test_the_64_bit_distance_path():
    cell, comp, nb = 256, 255, 4
    assert cell * cell * (nb * 65025 + 18 * comp * comp) >= 1 << 32                 # what dm_scene_slic_pass takes the wide path on
    img = R.noise_image(4, 300, 280, 31)
    want = whole("wide", img, cell, comp, 2, 900)
    check_scene(img, (150, 140), want, cell, comp, 2, min_size=900)


def test_residency_does_not_change_the_result():
    from deepmerge_amd import scene
    img = IMAGES["blocks"]()
    want = whole(("blocks", 3), img, CELL, COMPACTNESS, 3)
    streamed = check_scene(img, (96, 112), want, CELL, COMPACTNESS, 3, resident_bytes=0)
    exact = check_scene(img, (96, 112), want, CELL, COMPACTNESS, 3, resident_bytes=3 * H * W)
    short = check_scene(img, (96, 112), want, CELL, COMPACTNESS, 3, resident_bytes=3 * H * W - 1)
    assert (streamed["resident"], exact["resident"], short["resident"]) == (False, True, False)
    assert (streamed["image_reads"], exact["image_reads"], short["image_reads"]) == (3 + 2, 1, 3 + 2)
    a, n = scene.slic_labels(img, tile=(96, 112), cell=CELL, compactness=COMPACTNESS, iters=3, device=DEV)      # the default budget
    assert n == want[3] and np.array_equal(a, want[2])


def test_sources_and_outputs_on_disk(tmp_path):
    from deepmerge_amd import scene
    img = IMAGES["noise"]()
    want = whole(("noise", 3), img, CELL, COMPACTNESS, 3)
    on_disk = np.memmap(tmp_path / "scene.u8", dtype=np.uint8, mode="w+", shape=img.shape)
    on_disk[:] = img
    on_disk.flush()

    class Reads:                                                   # a source that can only be read
        shape = img.shape

        def __init__(self):
            self.calls = 0

        def read(self, y0, y1, x0, x1):
            self.calls += 1
            return img[:, y0:y1, x0:x1].copy()

    reads = Reads()
    for k, source in enumerate((np.memmap(tmp_path / "scene.u8", dtype=np.uint8, mode="r+", shape=img.shape), reads, torch.from_numpy(img))):
        out = np.memmap(tmp_path / f"labels{k}.i32", dtype=np.int32, mode="w+", shape=(H, W))
        got, n = scene.slic_labels(source, tile=(96, 112), cell=CELL, compactness=COMPACTNESS, iters=3, labels_out=out, device=DEV)
        assert got is out and n == want[3] and np.array_equal(out, want[2])
        assigned = np.memmap(tmp_path / f"assigned{k}.i32", dtype=np.int32, mode="w+", shape=(H, W))
        got, _ = scene.slic_assign(source, tile=(96, 112), cell=CELL, compactness=COMPACTNESS, iters=3, assigned_out=assigned, device=DEV)
        assert got is assigned and np.array_equal(assigned, want[0])
    assert reads.calls == 2 * 9                                    # resident: every core read once per call
    assert np.array_equal(on_disk, img)                            # the source is untouched


@pytest.fixture(scope="module")
def fio():
    from deepmerge_amd.ExtractFeatures import FeatureIO
    from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3
    torch.manual_seed(1)
    net = ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=[32, 64, 128], depth=[1, 1, 1], in_c=3, numerics="fp32")
    return FeatureIO(net, None, DEV)


def test_segment_scene_cross_seams_equals_segment_labels_on_the_whole_scene_slic(fio):
    """Layer by layer; both sides encode in the same tiles and batches."""
    import scene_labels_ref as L
    from deepmerge_amd import rag, scene
    img, tile = L.scene_image(), (96, 112)
    labels, n = rag.slic(dev(img))
    labels = labels.cpu().numpy()
    assert crosses_a_seam(labels, tile)
    want = scene.segment_labels(fio, img, labels, n, tile=tile, k=1, margin=1.0)
    out = np.full((H, W), -7, np.int32)
    got = fio.segment_scene(img, tile=tile, cross_seams=True, labels_out=out, k=1, margin=1.0)
    assert isinstance(got, scene.SceneResult) and got.n_labels == n and got.offsets is None and got.tiles == want.tiles
    assert got.labels is out and np.array_equal(out, labels)
    for key in ("count", "sum", "sumsq", "bbox", "peri"):
        assert torch.equal(got.stats[key], want.stats[key]), key
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(got.designed), bits(want.designed))
    assert torch.equal(got.edges, want.edges) and torch.equal(got.weights, want.weights)
    for f in ("xy", "label", "inner", "obj", "ptr", "idx", "bbox", "round"):
        assert torch.equal(getattr(got.points, f), getattr(want.points, f)), f
    assert torch.equal(bits(got.features), bits(want.features))
    assert torch.equal(got.result.region_of, want.result.region_of) and torch.equal(got.result.history, want.result.history)
    assert got.result.rounds == want.result.rounds and got.result.regions_per_round == want.result.regions_per_round
    assert np.array_equal(got.write_merged(), want.write_merged())
    # slic= reaches slic_labels
    other, m = rag.slic(dev(img), cell=24, iters=2)
    got = fio.segment_scene(img, tile=tile, cross_seams=True, slic=dict(cell=24, iters=2), k=1, margin=1.0, max_rounds=0)
    assert got.n_labels == m != n and np.array_equal(got.labels, other.cpu().numpy())
    # the default is the per-tile path, untouched: its superpixels stop at the seams
    old = fio.segment_scene(img, tile=tile, k=1, margin=1.0, max_rounds=0)
    assert old.offsets is not None and not crosses_a_seam(old.labels, tile)


def test_the_new_keywords_refuse_what_does_not_go_with_them(fio):
    from deepmerge_amd import scene
    img = IMAGES["blocks"]()
    with pytest.raises(ValueError, match="cross_seams=True makes the scene's superpixels itself"):
        fio.segment_scene(img, cross_seams=True, segmenter=lambda t: None)
    with pytest.raises(ValueError, match="cross_seams=True makes the scene's superpixels itself"):
        fio.segment_scene(img, cross_seams=True, labels=np.zeros((H, W), np.int32), n_labels=1)
    with pytest.raises(ValueError, match="goes with cross_seams=True"):
        fio.segment_scene(img, slic=dict(cell=8))
    with pytest.raises(ValueError, match="cell must be in 4..256"):
        fio.segment_scene(img, cross_seams=True, slic=dict(cell=3))
    with pytest.raises(ValueError, match="resident_bytes must be >= 0"):
        scene.slic_labels(img, resident_bytes=-1, device=DEV)
    with pytest.raises(ValueError, match="labels_out must be a writable int32"):
        scene.slic_labels(img, labels_out=np.zeros((H, W), np.int64), device=DEV)
