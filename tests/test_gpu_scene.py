"""GPU: scenes larger than one tile (deepmerge_amd/scene.py, csrc/dm_scene.hip).  The definition is the test: on a scene small
enough to also run as one tile, the tile stream + seam stitch + one merge equals the one-tile pipeline on the assembled seam-cut
label raster, bit for bit, layer by layer.  Only the seam kernel has a numpy spec (tests/scene_ref.py).  Every comparison is
torch.equal / bit equality."""
import numpy as np
import pytest
import torch

import points_ref as PR
import scene_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POINT_FIELDS = ("xy", "label", "inner", "obj", "ptr", "idx", "bbox", "round")
STAT_KEYS = ("count", "sum", "sumsq", "bbox", "peri")
H, W, TILE = 200, 232, (96, 112)                                   # both axes end in an 8-pixel sliver


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def scene_image():
    """Coarse colour blocks + noise, as tests/test_gpu_points.py builds its tile: neighbours differ and resemble."""
    rng = np.random.default_rng(12)
    base = rng.integers(0, 256, (3, 4, 4)).astype(np.uint8)
    full = np.clip(np.kron(base, np.ones((64, 64), np.uint8)).astype(np.int64) + rng.integers(-8, 9, (3, 256, 256)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(full[:, :H, :W])


# ---- 1. the kernel against the spec ------------------------------------------------------------------------------------------------------
def seam(n, S, seed):
    """Runs of varying length on both sides, a == b stretches, -1 on either side and on both, -2, ids S and beyond, and the two
    largest ids (keys pass 2^32 when S = 2^24)."""
    rng = np.random.default_rng(seed)

    def side():
        runs = rng.integers(1, 40, n)
        ids = rng.integers(0, min(S, 50), n)
        big = rng.random(n) < 0.3
        ids[big] = S - 1 - rng.integers(0, min(S, 3), int(big.sum()))
        return np.repeat(ids, runs)[:n].astype(np.int32)

    a, b = side(), side()
    pick = lambda p: rng.random(n) < p
    eq = pick(0.1)
    b[eq] = a[eq]
    a[pick(0.05)] = -1
    b[pick(0.05)] = -1
    both = pick(0.03)
    a[both] = -1
    b[both] = -1
    a[pick(0.02)] = -2
    b[pick(0.02)] = S + 5
    return a, b


def run_stitch(a, b, S, peri0, max_edges=0, offset=0):
    from deepmerge_amd import rag
    if offset:                                                     # views that are not 16-byte aligned take the scalar loads
        buf_a, buf_b = (torch.zeros(a.size + 8, dtype=torch.int32, device=DEV) for _ in range(2))
        ta, tb = buf_a[offset:offset + a.size], buf_b[offset:offset + a.size]
        ta.copy_(dev(a))
        tb.copy_(dev(b))
    else:
        ta, tb = dev(a), dev(b)
    peri = dev(peri0)
    edges, weights = rag.seam_stitch(ta, tb, S, peri, max_edges=max_edges)
    assert np.array_equal(ta.cpu().numpy(), a) and np.array_equal(tb.cpu().numpy(), b)       # the inputs are untouched
    return edges, weights, peri


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024, 1025, 4097])          # 1024: positions per workgroup
def test_seam_stitch_matches_the_spec(n):
    S = 300
    rng = np.random.default_rng(n)
    peri0 = rng.integers(0, 1 << 40, (S, 2)).astype(np.int64)
    for seed, offset in ((n, 0), (n + 1, 1), (n + 2, 3)):
        a, b = seam(n, S, seed)
        edges, weights, peri = run_stitch(a, b, S, peri0, offset=offset)
        re, rw, rp = R.seam_stitch(a, b, S, peri0)
        assert edges.dtype == torch.int32 and weights.dtype == torch.int32 and tuple(edges.shape) == (len(re), 2)
        assert np.array_equal(edges.cpu().numpy(), re) and np.array_equal(weights.cpu().numpy(), rw)
        assert np.array_equal(peri.cpu().numpy(), rp)
    # one pair repeated n times: the count is n, the perimeter moves n edges on both sides
    a, b = np.full(n, 7, np.int32), np.full(n, 3, np.int32)
    edges, weights, peri = run_stitch(a, b, S, peri0)
    assert edges.tolist() == [[3, 7]] and weights.tolist() == [n]
    want = peri0.copy()
    want[[3, 7], 0] += n
    want[[3, 7], 1] -= n
    assert np.array_equal(peri.cpu().numpy(), want)
    # nothing but a == b: no edge, the border column alone loses 2 n
    edges, weights, peri = run_stitch(a, a, S, peri0)
    assert tuple(edges.shape) == (0, 2) and tuple(weights.shape) == (0,)
    want = peri0.copy()
    want[7, 1] -= 2 * n
    assert np.array_equal(peri.cpu().numpy(), want)


def test_seam_stitch_keys_pass_2_to_the_32_at_the_largest_scene():
    S, n = 1 << 24, 4097
    peri0 = np.zeros((S, 2), np.int64)
    peri0[:, 1] = 1 << 20
    a, b = seam(n, S, 99)
    a[:5], b[:5] = S - 1, S - 2                                    # the largest key of all: (S - 2) S + S - 1 > 2^47
    edges, weights, peri = run_stitch(a, b, S, peri0)
    re, rw, rp = R.seam_stitch(a, b, S, peri0)
    assert np.array_equal(edges.cpu().numpy(), re) and np.array_equal(weights.cpu().numpy(), rw)
    assert np.array_equal(peri.cpu().numpy(), rp)
    assert re[-1].tolist() == [S - 2, S - 1] and int(re[-1, 0]) * S + int(re[-1, 1]) > 1 << 32
    a, b = np.full(n, S - 1, np.int32), np.full(n, S - 2, np.int32)
    edges, weights, _ = run_stitch(a, b, S, peri0)
    assert edges.tolist() == [[S - 2, S - 1]] and weights.tolist() == [n]


def test_seam_stitch_empty_and_overflow_and_argument_checks():
    from deepmerge_amd import rag
    S = 5000
    peri = torch.zeros((S, 2), dtype=torch.int64, device=DEV)
    empty = torch.empty(0, dtype=torch.int32, device=DEV)
    edges, weights = rag.seam_stitch(empty, empty, S, peri)        # a scene of one tile: no launch
    assert tuple(edges.shape) == (0, 2) and edges.dtype == torch.int32 and tuple(weights.shape) == (0,) and weights.dtype == torch.int32
    assert not bool(peri.any())
    # a max_edges too small raises the RuntimeError rag_edges raises
    a = torch.arange(0, 200, dtype=torch.int32, device=DEV)
    b = a + 200
    with pytest.raises(RuntimeError, match=r"more than max_edges=4 edges \(found 200") as seam_err:
        rag.seam_stitch(a, b, S, peri.clone(), max_edges=4)
    noise = torch.from_numpy(np.random.default_rng(0).integers(0, S, (64, 64)).astype(np.int32)).to(DEV)
    with pytest.raises(RuntimeError, match=r"more than max_edges=4 edges \(found ") as rag_err:
        rag.rag_edges(noise, S, max_edges=4)
    assert type(seam_err.value) is type(rag_err.value)
    edges, weights = rag.seam_stitch(a, b, S, peri.clone(), max_edges=200)
    assert edges.shape[0] == 200 and bool((weights == 1).all())
    for bad in (lambda: rag.seam_stitch(a.long(), b, S, peri), lambda: rag.seam_stitch(a, b[:5], S, peri),
                lambda: rag.seam_stitch(a, b, S, peri[:10]), lambda: rag.seam_stitch(a, b, S, peri.to(torch.int32)),
                lambda: rag.seam_stitch(a, b, 0, peri), lambda: rag.seam_stitch(a, b, (1 << 24) + 1, peri),
                lambda: rag.seam_stitch(a.view(2, -1), b.view(2, -1), S, peri)):
        with pytest.raises(ValueError):
            bad()


# ---- 2. graph layer ----------------------------------------------------------------------------------------------------------------------
def slic16(t):
    from deepmerge_amd import rag
    return rag.slic(t, cell=16)


def holed(t):
    """slic with -1 painted on pixels that touch the seams (the tile's right columns, bottom rows and a stretch of its top)."""
    labels, n = slic16(t)
    labels = labels.clone()
    labels[5:40, -2:] = -1
    labels[-1:, 10:50] = -1
    labels[:2, 60:90] = -1
    return labels, n


@pytest.fixture(scope="module")
def image():
    return scene_image()


@pytest.fixture(scope="module", params=["slic", "holed"])
def graph(request, image):
    """The scene without a net (the very pass segment_scene runs first), and the whole raster on the device."""
    from deepmerge_amd import scene
    g = scene._scene_graph(image, tile=TILE, segmenter=slic16 if request.param == "slic" else holed, k=3, max_window=64, device=DEV)
    g["whole"] = dev(image)
    g["raster"] = dev(g["labels"])
    g["case"] = request.param
    return g


def test_graph_layer_equals_the_one_tile_calls_on_the_assembled_raster(graph):
    from deepmerge_amd import rag
    g, S = graph, graph["n_labels"]
    lab = g["labels"]
    assert len(g["tiles"]) == 9 and g["offsets"][0] == 0 and g["offsets"][-1] == S and S > 100
    for i, (y0, y1, x0, x1) in enumerate(g["tiles"]):              # superpixels never cross a seam; ids are scene-wide
        ids = lab[y0:y1, x0:x1]
        ids = ids[ids >= 0]
        assert ids.min() >= g["offsets"][i] and ids.max() < g["offsets"][i + 1]
    if g["case"] == "holed":
        assert (lab[:, 111] == -1).any() and (lab[95, :] == -1).any() and (lab[96, :] == -1).any() and lab.min() == -1
    else:
        assert lab.min() == 0
    st = rag.label_stats(g["raster"], g["whole"], S)
    for key in STAT_KEYS:
        assert torch.equal(st[key], g["stats"][key]), key
    assert st["bands"] == g["stats"]["bands"]
    if g["case"] == "slic":                                        # what is left in the border column is the scene's frame
        assert int(g["stats"]["peri"][:, 1].sum()) == 2 * (H + W)
    assert torch.equal(bits(rag.designed_features(st)), bits(g["designed"]))
    edges, weights = rag.rag_edges(g["raster"], S)
    assert torch.equal(edges, g["edges"]) and torch.equal(weights, g["weights"])
    tile_of = torch.bucketize(g["edges"].long(), torch.tensor(g["offsets"][1:], device=DEV), right=True)
    assert int((tile_of[:, 0] != tile_of[:, 1]).sum()) == g["n_seam_edges"] > 20      # the seam edges are in, and only the stitch brings them
    assert g["n_seam"] == 2 * W + 2 * H
    pts = rag.sample_points(g["raster"], S, k=3, max_window=64)
    for f in POINT_FIELDS:
        assert torch.equal(getattr(pts, f), getattr(g["points"], f)), f


# ---- 3. crop layer -----------------------------------------------------------------------------------------------------------------------
def test_crops_from_clipped_halo_windows_equal_the_crops_from_the_whole_scene(graph):
    from deepmerge_amd import patches, scene
    g, pts = graph, graph["points"]
    halo = g["halo"]
    assert halo == 32
    x, y = pts.xy[:, 0], pts.xy[:, 1]
    assert bool((x < halo).any()) and bool((y < halo).any()) and bool((x >= W - halo).any()) and bool((y >= H - halo).any())
    L = torch.stack((pts.inner, pts.obj, 2 * pts.obj - pts.inner), 1)                  # the three window sides of the scales in use
    assert int(L.max()) <= 64
    num = 2 * pts.xy[:, :1] - L
    assert bool(((num < 0) & (num % 2 != 0)).any())                # the truncation that is not translation invariant does occur
    shifted = 0
    for i, core in enumerate(g["tiles"]):
        lo, hi = g["point_offsets"][i], g["point_offsets"][i + 1]
        assert hi > lo
        wy0, wy1, wx0, wx1 = scene.window_of(core, H, W, halo)
        shifted += (wx0 > 0) + (wy0 > 0)
        window = g["whole"][:, wy0:wy1, wx0:wx1].contiguous()
        origin = torch.tensor([wx0, wy0], dtype=torch.int32, device=DEV)
        rows = g["designed"][pts.label[lo:hi].long()]
        args = (pts.inner[lo:hi], pts.obj[lo:hi], rows)
        got, gd = patches.point_batch_cols(window, pts.xy[lo:hi] - origin, *args, scales=[32, 64, 128], grid=8, dtype=torch.float32)
        want, wd = patches.point_batch_cols(g["whole"], pts.xy[lo:hi], *args, scales=[32, 64, 128], grid=8, dtype=torch.float32)
        assert torch.equal(bits(gd), bits(wd))
        for s in range(3):
            assert got[s].cols.shape == want[s].cols.shape and torch.equal(bits(got[s].cols), bits(want[s].cols)), (i, s)
    assert shifted >= 8                                            # most windows do not start at the scene's origin


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------------
def slic24(t):
    from deepmerge_amd import rag
    return rag.slic(t, cell=24)


@pytest.fixture(scope="module")
def fio():
    from deepmerge_amd.ExtractFeatures import FeatureIO
    from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3
    torch.manual_seed(1)
    net = ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=[32, 64, 128], depth=[1, 1, 1], in_c=3, numerics="fp32")
    return FeatureIO(net, None, DEV)


def test_scene_equals_merge_tile_on_the_assembled_raster(fio, image):
    """batch_size = 1 on both sides: every encoder call has the same shape, so the rows are bit-equal."""
    from deepmerge_amd import scene
    g = scene._scene_graph(image, tile=TILE, segmenter=slic24, k=1, device=DEV)
    S, whole, raster = g["n_labels"], dev(image), dev(g["labels"])
    # the margin inside the spread of the edge scores, so that rounds really merge and really stop
    first, _ = fio.merge_tile(whole, raster, S, k=1, margin=1.0, batch_size=1, max_rounds=0)
    margin = float(first.simi.float().median())
    want, wpts = fio.merge_tile(whole, raster, S, k=1, margin=margin, batch_size=1)
    want_features = fio.features.clone()
    res = fio.segment_scene(image, tile=TILE, segmenter=slic24, k=1, margin=margin, batch_size=1)
    assert isinstance(res, scene.SceneResult) and res.n_labels == S and np.array_equal(res.labels, g["labels"])
    assert res.tiles == g["tiles"] and res.offsets == g["offsets"]
    for f in POINT_FIELDS:
        assert torch.equal(getattr(res.points, f), getattr(wpts, f)), f
    assert torch.equal(bits(res.features), bits(want_features)) and fio.features is res.features
    got = res.result
    assert want.rounds >= 1 and 1 <= want.ptr.numel() - 1 < S
    assert torch.equal(got.region_of, want.region_of) and torch.equal(got.history, want.history)
    assert torch.equal(bits(got.history_simi), bits(want.history_simi))
    assert got.rounds == want.rounds and got.regions_per_round == want.regions_per_round
    for key in STAT_KEYS:
        assert torch.equal(got.stats[key], want.stats[key]), key
    merged = res.write_merged()
    assert merged.dtype == np.int32 and np.array_equal(merged, want.labels(raster).cpu().numpy())
    out = np.full((H, W), -7, np.int32)
    assert res.write_merged(out) is out and np.array_equal(out, merged)
    y0, y1, x0, x1 = res.tiles[4]
    assert np.array_equal(res.merged_tile(4).cpu().numpy(), merged[y0:y1, x0:x1])
    # at least one merge joins superpixels of two different tiles
    tile_of = np.searchsorted(np.asarray(res.offsets[1:]), got.history[:, 1:].cpu().numpy(), side="right")
    assert (tile_of[:, 0] != tile_of[:, 1]).any()
    with pytest.raises(ValueError, match="out must be a writable int32"):
        res.write_merged(np.zeros((H, W), np.int64))


def test_features_through_shifted_window_origins_equal_the_whole_scene_encode(fio, image):
    """max_window = 64 makes the halo 32, so most windows start inside the scene: the driver's own origin shift is under test."""
    from deepmerge_amd import scene
    res = fio.segment_scene(image, tile=TILE, segmenter=slic24, k=1, max_window=64, batch_size=1, max_rounds=0)
    assert sum((scene.window_of(c, H, W, 32)[0] > 0) + (scene.window_of(c, H, W, 32)[2] > 0) for c in res.tiles) >= 8
    pts = res.points
    want = fio.extract_features_from_tile(dev(image), pts.xy, pts.inner, pts.obj, res.designed[pts.label.long()], batch_size=1)
    assert torch.equal(bits(res.features), bits(want))


# ---- 5. overlap --------------------------------------------------------------------------------------------------------------------------
def test_overlap_equals_label_overlap_on_the_assembled_rasters(graph):
    from deepmerge_amd import rag, scene
    g, S = graph, graph["n_labels"]
    truth, G = PR.voronoi_labels(H, W, 40, 3)
    truth[20:30, 100:130] = -1                                     # unlabelled pixels, across a seam
    res = scene.SceneResult(result=None, n_labels=S, tiles=g["tiles"], offsets=g["offsets"], stats=g["stats"], designed=g["designed"],
                            edges=g["edges"], weights=g["weights"], points=g["points"], features=None, labels=g["labels"])
    want = rag.label_overlap(g["raster"], dev(truth), S, G)
    for source in (truth, scene.ArraySource(truth), torch.from_numpy(truth)):
        got = res.overlap(source, G)
        for f in ("cells", "count", "area", "owner", "owner_count", "size", "cover", "summary"):
            assert torch.equal(getattr(got, f), getattr(want, f)), f
        assert (got.n_labels, got.n_truth) == (want.n_labels, want.n_truth)
    assert got.scores() == want.scores()


# ---- 6. a scene of one tile --------------------------------------------------------------------------------------------------------------
def test_a_scene_of_one_tile_equals_segment_tile(fio, image):
    small = np.ascontiguousarray(image[:, :96, :112])
    first = fio.segment_tile(dev(small), cell=24, k=1, margin=1.0, batch_size=1, max_rounds=0)[0]
    margin = float(first.simi.float().median())
    want, wpts, wlabels, wn = fio.segment_tile(dev(small), cell=24, k=1, margin=margin, batch_size=1)
    want_features = fio.features.clone()
    res = fio.segment_scene(small, tile=4096, segmenter=slic24, k=1, margin=margin, batch_size=1)
    assert res.tiles == [(0, 96, 0, 112)] and res.offsets == [0, wn] and res.n_labels == wn
    assert np.array_equal(res.labels, wlabels.cpu().numpy())
    for f in POINT_FIELDS:
        assert torch.equal(getattr(res.points, f), getattr(wpts, f)), f
    assert torch.equal(bits(res.features), bits(want_features))
    got = res.result
    assert torch.equal(got.region_of, want.region_of) and torch.equal(got.history, want.history)
    assert torch.equal(bits(got.history_simi), bits(want.history_simi)) and got.regions_per_round == want.regions_per_round
    assert torch.equal(got.edges, want.edges) and torch.equal(got.weights, want.weights)
    assert np.array_equal(res.write_merged(), want.labels(wlabels).cpu().numpy())
