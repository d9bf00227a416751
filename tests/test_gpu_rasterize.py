"""GPU: rag.rasterize (csrc/dm_rasterize.hip) against the input raster of rag.polygons (the exact inverse, bit for bit) and against
the numpy spec tests/rasterize_ref.py; its input checks; polygons.shp -> rag.labels_from_shapefile; truth rings -> label_overlap."""
import functools

import numpy as np
import pytest
import torch

import rasterize_ref as Z
import slic_ref as R
import vector_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NORTH_UP = (500000.0, 0.5, 0.0, 4100000.0, 0.0, -0.5)
CASES = Z.cases()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _blocks(H, W, seed):
    labels, n = R.connected_labels(R.block_image(1, H, W, 37, seed, noise=0)[0].astype(np.int32))
    return labels.astype(np.int32), int(n)


@functools.lru_cache(maxsize=None)
def raster(name):                                               # the rasters tests/test_gpu_vector.py traces, by the same names
    host = V.host_cases()
    if name in host:
        return host[name]
    return {"vec_blocks": lambda: _blocks(96, 128, 3), "odd_blocks": lambda: _blocks(257, 301, 5), "flat_wide": lambda: _blocks(5, 700, 7),
            "flat_tall": lambda: _blocks(700, 6, 9),
            "random_4": lambda: (np.random.default_rng(11).integers(0, 4, (67, 70)).astype(np.int32), 4),
            "comb": lambda: (V.comb_of_combs(130), 2)}[name]()


NAMES = list(V.host_cases()) + ["vec_blocks", "odd_blocks", "flat_wide", "flat_tall", "random_4", "comb"]


@functools.lru_cache(maxsize=None)
def spec(name, fill=-1):
    (ptr, xy, label), H, W = CASES[name]
    return Z.rasterize(ptr, Z.quantise(xy), label, H, W, fill)


def rings_of(name):
    from deepmerge_amd import rag
    (ptr, xy, label), H, W = CASES[name]
    return rag.Rings(dev(ptr), dev(xy), dev(label)), H, W


@pytest.mark.parametrize("name", NAMES)
def test_round_trip_through_polygons_is_exact(name):
    from deepmerge_amd import rag
    labels, n = raster(name)
    H, W = labels.shape
    polys = rag.polygons(dev(labels), n)
    before = [t.clone() for t in (polys.ring_ptr, polys.xy, polys.ring_label)]
    got = rag.rasterize(polys, H, W)
    assert got.dtype == torch.int32 and tuple(got.shape) == (H, W)
    g = got.cpu().numpy()
    print(f"{name}: {H} x {W}, rings = {polys.ring_label.numel()}, vertices = {polys.xy.shape[0]}, pixels that differ = {(g != labels).sum()}")
    assert np.array_equal(g, labels)
    for a, b in zip(before, (polys.ring_ptr, polys.xy, polys.ring_label)):
        assert torch.equal(a, b)                                # the inputs are not modified
    if name == "absent_ids":
        assert set(np.unique(g)) == {0, 3}                      # absent ids leave no pixel
    if name == "comb":
        assert int((polys.ring_ptr[1:] - polys.ring_ptr[:-1]).max()) > 8192
    if name == "random_4":
        assert polys.xy.shape[0] > 2 * labels.size


@pytest.mark.parametrize("name", list(CASES))
def test_general_polygons_equal_the_spec(name):
    from deepmerge_amd import rag
    rings, H, W = rings_of(name)
    before = [t.clone() for t in (rings.ring_ptr, rings.xy, rings.ring_label)]
    got = rag.rasterize(rings, H, W).cpu().numpy()
    want = spec(name)
    print(f"{name}: {H} x {W}, rings = {rings.ring_label.numel()}, pixels that differ = {(got != want).sum()}")
    assert got.dtype == np.int32 and np.array_equal(got, want)
    for a, b in zip(before, (rings.ring_ptr, rings.xy, rings.ring_label)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["hole_same_orientation", "overlap_ab", "overlap_ba", "random_300", "only_degenerate_rings"])
def test_fill_value(name):
    from deepmerge_amd import rag
    rings, H, W = rings_of(name)
    got = rag.rasterize(rings, H, W, fill=-7).cpu().numpy()
    assert np.array_equal(got, spec(name, -7)) and ((got == -7) == (spec(name) == -1)).all()


def test_overlap_does_not_depend_on_ring_order():
    from deepmerge_amd import rag
    a, b = (rag.rasterize(rings_of(n)[0], 10, 11) for n in ("overlap_ab", "overlap_ba"))
    assert torch.equal(a, b) and int(a[5, 5]) == 5 and np.array_equal(a.cpu().numpy(), spec("overlap_ab"))


def test_no_rings_and_one_pixel():
    from deepmerge_amd import rag
    i64, i32, f64 = torch.int64, torch.int32, torch.float64
    none = rag.Rings(torch.zeros(1, dtype=i64, device=DEV), torch.zeros((0, 2), dtype=f64, device=DEV), torch.zeros(0, dtype=i32, device=DEV))
    out = rag.rasterize(none, 3, 5)
    assert out.dtype == i32 and tuple(out.shape) == (3, 5) and bool((out == -1).all())
    assert bool((rag.rasterize(none, 2, 2, fill=-9) == -9).all())
    sq = rag.Rings(dev(np.array([0, 4])), dev(np.array([[0.25, 0.25], [0.75, 0.25], [0.75, 0.75], [0.25, 0.75]])), dev(np.array([6], np.int32)))
    assert rag.rasterize(sq, 1, 1).tolist() == [[6]]
    miss = rag.Rings(sq.ring_ptr, sq.xy * 0.5, sq.ring_label)    # the centre (0.5, 0.5) is outside
    assert rag.rasterize(miss, 1, 1).tolist() == [[-1]]
    top = rag.Rings(sq.ring_ptr, sq.xy, dev(np.array([(1 << 31) - 2], np.int32)))
    assert rag.rasterize(top, 1, 1).tolist() == [[(1 << 31) - 2]]
    labels, n = raster("one_pixel")
    assert rag.rasterize(rag.polygons(dev(labels), n), 1, 1).tolist() == [[0]]


def test_input_checks():
    from deepmerge_amd import rag
    (ptr, xy, label), H, W = CASES["fractional_triangle"]
    ok = lambda **kw: rag.Rings(dev(kw.get("ptr", ptr)), dev(kw.get("xy", xy)), dev(kw.get("label", label)))
    bad_xy = xy.copy()
    bad_xy[1, 0] = np.nan
    inf_xy = xy.copy()
    inf_xy[2, 1] = np.inf
    far_xy = xy.copy()
    far_xy[0, 1] = -(2.0 ** 20) - 1
    for rings, kw in ((ok(xy=bad_xy), {}), (ok(xy=inf_xy), {}), (ok(xy=far_xy), {}), (ok(), {"fill": 0}), (ok(), {"fill": 3}),
                      (ok(label=np.array([-1], np.int32)), {}), (ok(ptr=np.array([0, 2])), {}), (ok(ptr=np.array([1, 3])), {}),
                      (ok(ptr=np.array([0, 4])), {}), (ok(ptr=np.array([0, 3, 2, 3]), label=np.array([0, 1, 2], np.int32)), {}),
                      (ok(ptr=ptr.astype(np.int32)), {}), (ok(xy=xy.astype(np.float32)), {}), (ok(label=label.astype(np.int64)), {}),
                      (ok(xy=xy.reshape(-1)), {}), (ok(label=np.array([0, 1], np.int32)), {})):
        with pytest.raises(ValueError):
            rag.rasterize(rings, kw.get("H", H), kw.get("W", W), fill=kw.get("fill", -1))
    for h, w in ((0, 5), (5, 0), (1 << 16, 1 << 15)):
        with pytest.raises(ValueError):
            rag.rasterize(ok(), h, w)
    edge = xy.copy()
    edge[0] = (2.0 ** 20, -(2.0 ** 20))                          # the bound itself is allowed
    assert np.array_equal(rag.rasterize(ok(xy=edge), H, W).cpu().numpy(), Z.rasterize(ptr, Z.quantise(edge), label, H, W))


def test_shapefile_round_trip(tmp_path):
    from deepmerge_amd import rag, shpstore
    from deepmerge_amd.ExtractFeatures import FeatureIO
    labels, n = raster("vec_blocks")
    H, W = labels.shape
    t = dev(labels)
    designed = rag.designed_features(rag.label_stats(t, torch.zeros((1, H, W), dtype=torch.uint8, device=DEV), n))
    paths = FeatureIO.save_shapefiles(str(tmp_path), t, n, rag.sample_points(t, n, k=1), designed, geotransform=NORTH_UP)
    got, n_got = rag.labels_from_shapefile(paths[0], H, W, NORTH_UP)
    assert n_got == n and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), labels)
    perm = np.random.default_rng(5).permutation(n).astype(np.int32) + 4
    path = shpstore.write_polygons(str(tmp_path / "perm.shp"), rag.polygons(t, n), [("LBL", perm)], NORTH_UP)
    got, n_got = rag.labels_from_shapefile(path, H, W, NORTH_UP, label_field="LBL", fill=-3)
    assert n_got == n + 4 and np.array_equal(got.cpu().numpy(), perm[labels])
    with pytest.raises(ValueError, match="2\\^20"):              # read without its transform the rings lie millions of pixels away
        rag.labels_from_shapefile(paths[0], H, W)


def test_chain_truth_polygons_to_label_overlap():
    from deepmerge_amd import rag
    labels, n = raster("vec_blocks")                            # 96 x 128
    H, W = labels.shape
    polys = [(g, p) for g, p in Z.random_polygons(24, H, W, seed=21, n_labels=6)]
    polys += [(6, [(10.5, 8.25), (120.0, 20.0), (100.75, 90.0), (30.0, 70.5)])]
    ptr, xy, label = Z.pack(polys)
    truth = Z.rasterize(ptr, Z.quantise(xy), label, H, W)
    assert (truth >= 0).mean() > 0.3 and (truth < 0).any()
    t = dev(labels)
    got = rag.label_overlap(t, rag.rasterize(rag.Rings(dev(ptr), dev(xy), dev(label)), H, W), n, 7)
    want = rag.label_overlap(t, dev(truth), n, 7)
    assert torch.equal(got.cells, want.cells) and torch.equal(got.count, want.count) and torch.equal(got.summary, want.summary)
    cells = want.cells.cpu().numpy()
    ref = {}
    for s, g in zip(labels.reshape(-1), truth.reshape(-1)):
        ref[(int(s), int(g) if g >= 0 else 7)] = ref.get((int(s), int(g) if g >= 0 else 7), 0) + 1
    assert {(int(a), int(b)): int(c) for (a, b), c in zip(cells, got.count.cpu().numpy())} == ref
