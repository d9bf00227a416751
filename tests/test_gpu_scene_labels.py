"""GPU: a scene segmented from a label raster whose regions cross tile seams (deepmerge_amd/scene.py: sample_points, label_graph,
segment_labels, mrs_labels; csrc/dm_scene_points.hip).  The definition is the test: whatever the tile size, the calls return bit
for bit what the one-raster calls (`rag.sample_points`, `label_stats`, `rag_edges`, `FeatureIO.merge_tile`, `rag.mrs`) return on
the whole scene.  Only the select kernel has a numpy spec of its own: tests/points_ref.py on the core it is given.  Every
comparison is torch.equal / bit equality.

The stripe.  One might expect rounds 1 and 2 of the stripe to land in other tiles than round 0.  The rule does not give that: the
centre line's score stays 3 at every pixel three or more columns from the points chosen so far, and ties go to the smallest scene
index, so the rounds choose x = 2, 5, 8 of row 187 (tests/points_ref.py says so, and the kernel must agree).  What the case is
there for -- a later round that scores against a winner of another tile -- is asserted on the 150 x 150 block, whose three
points do lie in different tiles, and on the Voronoi regions of raster (a)."""
import numpy as np
import pytest
import torch

import points_ref as PR
import scene_labels_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POINT_FIELDS = ("xy", "label", "inner", "obj", "ptr", "idx", "bbox", "round")
STAT_KEYS = ("count", "sum", "sumsq", "bbox", "peri")
H, W, TILE = R.H, R.W, R.TILE
TILES = (TILE, (200, 232), (37, 41))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


RASTERS = {"a": R.raster_a(), "b": R.raster_b()}


def test_the_rasters_are_not_vacuous():
    """By numpy, before any device call: regions do cross seams, the stripe's tie does span tiles, later rounds do meet winners
    of other tiles."""
    lab, S = RASTERS["a"]
    t = R.tiles_per_label(lab, S, TILE)
    assert (t >= 2).sum() >= 20 and (t >= 4).sum() >= 1
    want = PR.sample_points(lab, S, 3, 384)
    at = R.tile_index(want["xy"][:, 1], want["xy"][:, 0], W, TILE)
    assert sum(len(set(at[want["label"] == s].tolist())) >= 2 for s in range(S)) >= 3      # later rounds meet winners of other tiles (5 regions do)
    lab, S = RASTERS["b"]
    t = R.tiles_per_label(lab, S, TILE)
    assert t[R.FRAME] == 9 and t[R.BLOCK] == 4 and t[R.ABSENT] == 0 and (lab == -1).any()
    for y0, y1, x0, x1 in R.tiles_of(H, W, TILE):                  # every tile holds fewer labels than the scene
        core = lab[y0:y1, x0:x1]
        assert len(np.unique(core[(core >= 0) & (core < S)])) < (t > 0).sum()
    clr = PR.clearance(lab)
    assert clr[95, 105] == 75                                      # the block's centre: beyond any halo of a (37, 41) tile
    stripe = lab == R.STRIPE
    top = clr[stripe].max()
    ys, xs = np.nonzero(stripe & (clr == top))
    assert top == 3 and len(set(R.tile_index(ys, xs, W, TILE).tolist())) >= 2      # round 0's tie spans tiles
    want = PR.sample_points(lab, S, 3, 384, clr=clr)
    m = want["label"] == R.STRIPE
    assert want["xy"][m].tolist() == [[2, 187], [5, 187], [8, 187]]                  # smallest scene index, round after round
    m = want["label"] == R.BLOCK
    assert len(set(R.tile_index(want["xy"][m][:, 1], want["xy"][m][:, 0], W, TILE).tolist())) >= 2
    a, b = R.seam_pairs(lab, TILE)
    assert ((a == b) & (a >= 0)).sum() > 100 and ((a == -1) | (b == -1)).any()


# ---- 1. the select kernel against the spec on the core it is given -----------------------------------------------------------------------
def run_rounds(window, clr, core, origin, scene, S, k, keys_of_round0=False):
    """init, then k x (one select over `core` of the window, commit), then dm_point_emit: the tables and the emitted rows."""
    from deepmerge_amd import _lib
    from deepmerge_amd.ops import _stream, check
    lib, i32 = _lib.lib(), torch.int32
    wh, ww = window.shape
    cy0, cy1, cx0, cx1 = core
    best = torch.empty(S, dtype=torch.int64, device=DEV)
    pts, pclr = torch.empty((S, k, 2), dtype=i32, device=DEV), torch.empty((S, k), dtype=i32, device=DEV)
    cnt, bbox = torch.empty(S, dtype=i32, device=DEV), torch.empty((S, 4), dtype=i32, device=DEV)
    check(lib.dm_scene_point_init(best.data_ptr(), cnt.data_ptr(), bbox.data_ptr(), S, _stream()), "dm_scene_point_init")
    keys = None
    for j in range(k):
        check(lib.dm_scene_point_select(window.data_ptr(), clr.data_ptr(), wh, ww, cy0, cy1, cx0, cx1, origin[0], origin[1], scene[0], scene[1],
                                        S, k, j, pts.data_ptr(), cnt.data_ptr(), best.data_ptr(), bbox.data_ptr(), _stream()),
              "dm_scene_point_select")
        if j == 0 and keys_of_round0:
            keys = best.cpu().numpy().view(np.uint64).copy()
        check(lib.dm_scene_point_commit(best.data_ptr(), scene[0], scene[1], S, k, pts.data_ptr(), pclr.data_ptr(), cnt.data_ptr(), _stream()),
              "dm_scene_point_commit")
    assert not bool(best.any())                                    # the commit clears what it took
    cap = S * k
    ptr, xy = torch.empty(S + 1, dtype=i32, device=DEV), torch.empty((cap, 2), dtype=i32, device=DEV)
    label, inner, obj, rnd = (torch.empty(cap, dtype=i32, device=DEV) for _ in range(4))
    check(lib.dm_point_emit(cnt.data_ptr(), pts.data_ptr(), pclr.data_ptr(), bbox.data_ptr(), S, k, 16, cap, ptr.data_ptr(), xy.data_ptr(),
                            label.data_ptr(), inner.data_ptr(), obj.data_ptr(), rnd.data_ptr(), _stream()), "dm_point_emit")
    P = int(ptr[S])
    got = {"xy": xy[:P], "label": label[:P], "inner": inner[:P], "obj": obj[:P], "round": rnd[:P], "ptr": ptr, "bbox": bbox}
    return {f: v.cpu().numpy() for f, v in got.items()}, keys


def check_core(lab_np, core, origin, scene, S, k=3, keys=False):
    """One window, one core, all rounds == points_ref.sample_points on the core alone (the virtual raster), given the window's
    clearance there, shifted to scene coordinates: the core's raster order is the scene's linear-index order."""
    from deepmerge_amd import rag
    window = dev(lab_np)
    clr = rag.clearance(window, 16)
    cy0, cy1, cx0, cx1 = core
    got, round0 = run_rounds(window, clr, core, origin, scene, S, k, keys_of_round0=keys)
    want = PR.sample_points(lab_np[cy0:cy1, cx0:cx1], S, k, 16, clr=clr.cpu().numpy()[cy0:cy1, cx0:cx1])
    shift = np.array([origin[1] + cx0, origin[0] + cy0], np.int32)
    assert np.array_equal(got["xy"], want["xy"] + shift)
    for f in ("label", "inner", "obj", "round", "ptr"):
        assert np.array_equal(got[f], want[f]), f
    box = want["bbox"].copy()
    seen = box[:, 2] >= 0
    box[seen] += np.tile(shift, 2)
    assert np.array_equal(got["bbox"], box)
    assert np.array_equal(window.cpu().numpy(), lab_np)            # the input is untouched
    return got, want, round0


# (core width, core x0 in the window, columns right of the core, core y0, rows below the core): widths around the 64-pixel tile
# and the 16-pixel strip; x0 odd, even, and a multiple of 8 with a window width that is one too, which alone takes the 16-byte
# loads; the core inset from the window on 0 to 4 sides
CORES = [(1, 0, 0, 0, 0), (1, 3, 4, 2, 0), (63, 1, 0, 0, 3), (63, 8, 1, 1, 1), (64, 0, 0, 0, 0), (64, 8, 8, 0, 5), (64, 2, 6, 3, 0),
         (65, 5, 2, 4, 4), (65, 16, 7, 0, 0), (257, 0, 7, 1, 0), (257, 7, 0, 0, 2)]


@pytest.mark.parametrize("cw,cx0,right,cy0,below", CORES)
def test_select_rounds_equal_the_spec_on_the_core(cw, cx0, right, cy0, below):
    ch = 70                                                        # two rows of 64 x 64 tiles
    wh, ww = cy0 + ch + below, cx0 + cw + right
    lab, S = PR.voronoi_labels(wh, ww, 12, cw + cx0)               # ~ 28 labels per 64 x 64 tile: the LDS slots suffice
    lab = lab.copy()
    lab[wh // 3:wh // 3 + 4, ww // 4:ww // 4 + 9] = -1             # ids outside [0, S) are no candidates
    lab[wh // 2, ww // 2] = S + 3
    got, want, _ = check_core(lab, (cy0, cy0 + ch, cx0, cx0 + cw), (1000, 37), (3000, 5000), S)
    assert (want["ptr"][1:] - want["ptr"][:-1]).max() == 3 or cw == 1
    # every pixel of the core with a label of its own: more labels than LDS slots in every 64 x 64 tile, the global path
    own = np.full((wh, ww), -1, np.int32)
    own[cy0:cy0 + ch, cx0:cx0 + cw] = np.arange(ch * cw, dtype=np.int32).reshape(ch, cw)
    got, want, _ = check_core(own, (cy0, cy0 + ch, cx0, cx0 + cw), (1000, 37), (3000, 5000), ch * cw)
    assert len(want["label"]) == ch * cw and (want["inner"] == 1).all()


def test_select_keys_at_linear_indices_beyond_2_to_the_40():
    """The window sits at row 2^20 + 5 of a scene of 2^21 + 3 columns: lin > 2^40.  Round 0's keys, read before the commit, equal
    the key computed in Python integers from the spec's winners."""
    SH, SW = (1 << 21) + 100, (1 << 21) + 3
    oy, ox = (1 << 20) + 5, (1 << 20) + 7
    wh, ww, core = 80, 96, (3, 75, 8, 90)
    lab, S = PR.voronoi_labels(wh, ww, 12, 5)
    got, want, keys = check_core(lab, core, (oy, ox), (SH, SW), S, keys=True)
    first = want["round"] == 0
    assert first.sum() > 20
    seen = np.zeros(S, bool)
    for (x, y), s, inner in zip(want["xy"][first].tolist(), want["label"][first].tolist(), want["inner"][first].tolist()):
        c = (inner + 1) // 2                                       # in round 0 the score is the clearance
        lin = (oy + core[0] + y) * SW + ox + core[2] + x
        assert lin > 1 << 40
        assert int(keys[s]) == R.pack_key(c, lin, c), s
        seen[s] = True
    assert not keys[~seen].any()                                   # labels without a pixel in the core have no key


# ---- 2. clearance: the window's equals the scene's on the core -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("max_window", [64, 384])
def test_window_clearance_equals_the_scene_clearance_on_every_core(name, max_window):
    from deepmerge_amd import rag, scene
    lab = dev(RASTERS[name][0])
    whole = rag.clearance(lab, max_window)
    halo = scene.halo_of(max_window)
    assert halo == (32 if max_window == 64 else 192)
    inside = 0
    for core in scene.tile_grid(H, W, TILE):
        y0, y1, x0, x1 = core
        wy0, wy1, wx0, wx1 = scene.window_of(core, H, W, halo)
        inside += (wy0 > 0) + (wx0 > 0) + (wy1 < H) + (wx1 < W)
        got = rag.clearance(lab[wy0:wy1, wx0:wx1].contiguous(), max_window)
        assert torch.equal(got[y0 - wy0:y1 - wy0, x0 - wx0:x1 - wx0], whole[y0:y1, x0:x1]), core
    # windows do end inside the scene, where only the cap makes the clearance right; at halo 192 those of the last tile column do
    # (they start at x = 224 - 192) and every window spans several tiles
    assert inside >= (16 if max_window == 64 else 3)
    if name == "b":
        assert int(whole[95, 105]) == min(75, halo)


# ---- 3. points ------------------------------------------------------------------------------------------------------------------------------
_WHOLE_POINTS = {}


def whole_points(name, k, max_window):
    from deepmerge_amd import rag
    key = (name, k, max_window)
    if key not in _WHOLE_POINTS:
        lab, S = RASTERS[name]
        _WHOLE_POINTS[key] = rag.sample_points(dev(lab), S, k=k, max_window=max_window)
    return _WHOLE_POINTS[key]


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("max_window", [64, 384])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", ["a", "b"])
def test_scene_points_equal_the_points_of_the_whole_raster(name, k, max_window, tile):
    from deepmerge_amd import scene
    lab, S = RASTERS[name]
    want = whole_points(name, k, max_window)
    got = scene.sample_points(lab, S, k=k, max_window=max_window, tile=tile, device=DEV)
    for f in POINT_FIELDS:
        assert torch.equal(getattr(got, f), getattr(want, f)), f
    if name == "b":                                                # an id that never occurs: no point, the empty box
        assert int(got.ptr[R.ABSENT + 1] - got.ptr[R.ABSENT]) == 0 and got.bbox[R.ABSENT].tolist() == [2 ** 31 - 1, 2 ** 31 - 1, -1, -1]
        assert got.bbox[R.FRAME].tolist() == [0, 0, W - 1, H - 1]
        if k == 3:
            assert got.xy[got.label == R.STRIPE].tolist() == [[2, 187], [5, 187], [8, 187]]


def test_scene_points_from_a_read_only_source_and_a_tensor():
    from deepmerge_amd import scene
    lab, S = RASTERS["a"]
    want = whole_points("a", 3, 64)

    class Reads:
        shape = (H, W)

        def __init__(self):
            self.calls = 0

        def read(self, y0, y1, x0, x1):
            self.calls += 1
            return lab[y0:y1, x0:x1].copy()

    src = Reads()
    for source in (src, torch.from_numpy(lab), scene.ArraySource(lab)):
        got = scene.sample_points(source, S, k=3, max_window=64, tile=TILE, device=DEV)
        for f in POINT_FIELDS:
            assert torch.equal(getattr(got, f), getattr(want, f)), f
    assert src.calls == 3 * 9                                      # k passes over the label raster


# ---- 4. graph -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def image():
    return R.scene_image()


@pytest.mark.parametrize("name", ["a", "b"])
def test_label_graph_equals_the_one_raster_calls(name, image):
    from deepmerge_amd import rag, scene
    lab, S = RASTERS[name]
    g = scene.label_graph(image, lab, S, tile=TILE, k=3, max_window=64, device=DEV)
    assert g["offsets"] is None and g["point_offsets"] is None and g["n_labels"] == S and len(g["tiles"]) == 9 and g["halo"] == 32
    whole, raster = dev(image), dev(lab)
    st = rag.label_stats(raster, whole, S)
    for key in STAT_KEYS:
        assert g["stats"][key].dtype == st[key].dtype and torch.equal(g["stats"][key], st[key]), key
    assert g["stats"]["bands"] == st["bands"]
    assert torch.equal(bits(g["designed"]), bits(rag.designed_features(st)))
    edges, weights = rag.rag_edges(raster, S)
    assert g["edges"].dtype == torch.int32 and g["weights"].dtype == torch.int32
    assert torch.equal(g["edges"], edges) and torch.equal(g["weights"], weights)
    want = whole_points(name, 3, 64)
    for f in POINT_FIELDS:
        assert torch.equal(getattr(g["points"], f), getattr(want, f)), f
    # the fold is exercised: some pair got weight from more than one tile or seam; the stitch met equal ids across a seam
    sources = R.edge_tiles(lab, S, TILE)
    assert len(sources) == edges.shape[0] and sum(v > 1 for v in sources.values()) >= 10
    assert g["n_edge_parts"] == sum(sources.values()) > edges.shape[0]
    a, b = R.seam_pairs(lab, TILE)
    assert g["n_seam"] == a.size == 2 * W + 2 * H and ((a == b) & (a >= 0)).sum() > 100
    if name == "b":
        assert int(g["stats"]["count"][R.ABSENT]) == 0 and g["stats"]["bbox"][R.ABSENT].tolist() == [2 ** 31 - 1, 2 ** 31 - 1, -1, -1]
        assert int(g["stats"]["peri"][:, 1].sum()) == 2 * (H + W)  # what is left in the border column is the scene's frame
    # the tile size does not matter
    for tile in TILES[1:]:
        other = scene.label_graph(image, lab, S, tile=tile, max_window=64, device=DEV, points=False)
        assert other["points"] is None
        for key in STAT_KEYS:
            assert torch.equal(other["stats"][key], st[key]), (tile, key)
        assert torch.equal(other["edges"], edges) and torch.equal(other["weights"], weights)


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fio():
    from deepmerge_amd.ExtractFeatures import FeatureIO
    from deepmerge_amd.nets.ShfitScaleFormer import ShfitScaleFormer_v3
    torch.manual_seed(1)
    net = ShfitScaleFormer_v3(cube_size=[8, 8], input_image_scales=[32, 64, 128], depth=[1, 1, 1], in_c=3, numerics="fp32")
    return FeatureIO(net, None, DEV)


def equal_results(got, want):
    assert torch.equal(got.region_of, want.region_of) and torch.equal(got.history, want.history)
    assert torch.equal(bits(got.history_simi), bits(want.history_simi))
    assert got.rounds == want.rounds and got.regions_per_round == want.regions_per_round
    assert torch.equal(got.edges, want.edges) and torch.equal(got.weights, want.weights)
    for key in STAT_KEYS:
        assert torch.equal(got.stats[key], want.stats[key]), key


def test_segment_labels_equals_merge_tile_on_the_whole_raster(fio, image):
    """batch_size = 1 on both sides: every encoder call has the same shape, so the rows are bit-equal."""
    from deepmerge_amd import rag, scene
    lab, S = RASTERS["a"]
    whole, raster = dev(image), dev(lab)
    first, _ = fio.merge_tile(whole, raster, S, k=1, margin=1.0, batch_size=1, max_rounds=0)
    margin = float(first.simi.float().median())                    # inside the spread of the edge scores: rounds merge and stop
    want, wpts = fio.merge_tile(whole, raster, S, k=1, margin=margin, batch_size=1)
    want_features = fio.features.clone()

    class Reads:                                                   # a label source that can only be read
        shape = (H, W)

        def read(self, y0, y1, x0, x1):
            return lab[y0:y1, x0:x1].copy()

    for labels in (lab, Reads()):
        res = fio.segment_scene(image, tile=TILE, k=1, margin=margin, batch_size=1, labels=labels, n_labels=S)
        assert isinstance(res, scene.SceneResult) and res.n_labels == S and res.offsets is None and len(res.tiles) == 9
        for f in POINT_FIELDS:
            assert torch.equal(getattr(res.points, f), getattr(wpts, f)), f
        assert torch.equal(bits(res.features), bits(want_features)) and fio.features is res.features
        assert want.rounds >= 1 and 1 <= want.ptr.numel() - 1 < S
        equal_results(res.result, want)
        merged = res.write_merged()
        assert merged.dtype == np.int32 and np.array_equal(merged, want.labels(raster).cpu().numpy())
    y0, y1, x0, x1 = res.tiles[4]
    assert np.array_equal(res.merged_tile(4).cpu().numpy(), merged[y0:y1, x0:x1])
    # at least one merge joins two regions that both cross a seam
    crosses = R.tiles_per_label(lab, S, TILE) >= 2
    pairs = res.result.history[:, 1:].cpu().numpy()
    assert (crosses[pairs[:, 0]] & crosses[pairs[:, 1]]).any()
    # overlap: ids compacted per tile, cells of several tiles folded
    truth, G = PR.voronoi_labels(H, W, 40, 3)
    truth[20:30, 100:130] = -1
    wov = rag.label_overlap(raster, dev(truth), S, G)
    gov = res.overlap(truth, G)
    for f in ("cells", "count", "area", "owner", "owner_count", "size", "cover", "summary"):
        assert torch.equal(getattr(gov, f), getattr(wov, f)), f
    assert res.result.scores(gov) == want.scores(wov)
    # rings and arcs of the merged raster
    polys, arcs = res.trace(merged)
    wp, wa = want.polygons(raster), want.boundary_arcs(raster)
    for f in ("region_ptr", "ring_ptr", "xy", "ring_label", "ring_area2"):
        assert torch.equal(getattr(polys, f), getattr(wp, f)), f
    for f in ("arc_ptr", "xy", "left", "right", "edge"):
        assert torch.equal(getattr(arcs, f), getattr(wa, f)), f


# ---- 6. seam invariance: the new path contains the old one -----------------------------------------------------------------------------------
def slic24(t):
    from deepmerge_amd import rag
    return rag.slic(t, cell=24)


def test_the_raster_a_segmenter_assembled_gives_the_same_scene_result(fio, image):
    from deepmerge_amd import scene
    first = fio.segment_scene(image, tile=TILE, segmenter=slic24, k=1, margin=1.0, batch_size=1, max_rounds=0)
    margin = float(first.result.simi.float().median())
    old = fio.segment_scene(image, tile=TILE, segmenter=slic24, k=1, margin=margin, batch_size=1)
    new = scene.segment_labels(fio, image, old.labels, old.n_labels, tile=TILE, k=1, margin=margin, batch_size=1)
    assert old.result.rounds >= 1 and new.n_labels == old.n_labels and new.tiles == old.tiles and new.labels is old.labels
    assert old.offsets[-1] == old.n_labels and new.offsets is None
    for key in STAT_KEYS:
        assert torch.equal(new.stats[key], old.stats[key]), key
    assert torch.equal(bits(new.designed), bits(old.designed))
    assert torch.equal(new.edges, old.edges) and torch.equal(new.weights, old.weights)
    for f in POINT_FIELDS:
        assert torch.equal(getattr(new.points, f), getattr(old.points, f)), f
    assert torch.equal(bits(new.features), bits(old.features))
    equal_results(new.result, old.result)
    assert np.array_equal(new.write_merged(), old.write_merged())


# ---- 7. the classical baseline on the scene's graph ----------------------------------------------------------------------------------------
def test_mrs_labels_equals_mrs_on_the_whole_raster(image):
    from deepmerge_amd import rag, scene
    lab, S = RASTERS["a"]
    whole, raster = dev(image), dev(lab)
    st = rag.label_stats(raster, whole, S)
    edges, weights = rag.rag_edges(raster, S)
    cost = rag.region_merge_cost(st, edges, weights)
    scale = float(cost.median().sqrt())                            # inside the spread of the costs: rounds merge and stop
    assert scale > 0.0
    want = rag.mrs(whole, scale, labels=raster, n_labels=S)
    assert want.rounds >= 1 and 1 < want.rep.numel() < S
    for tile in TILES:
        got = scene.mrs_labels(image, lab, S, scale, tile=tile, device=DEV)
        equal_results(got, want)
        assert torch.equal(bits(got.simi), bits(want.simi)) and torch.equal(got.rep, want.rep)
    kw = dict(shape=0.3, compactness=0.2, band_weights=[1.0, 0.5, 2.0], max_rounds=2)
    equal_results(scene.mrs_labels(image, lab, S, scale, tile=TILE, device=DEV, **kw), rag.mrs(whole, scale, labels=raster, n_labels=S, **kw))
    # the graph form takes what the raster form builds
    equal_results(rag.mrs_graph(st, edges, weights, scale), want)
    # an id that never occurs: the ValueError of rag.mrs
    labb, Sb = RASTERS["b"]
    with pytest.raises(ValueError, match="every id in \\[0, n_labels\\) must occur") as one:
        rag.mrs(whole, scale, labels=dev(labb), n_labels=Sb)
    with pytest.raises(ValueError, match="every id in \\[0, n_labels\\) must occur") as scene_wide:
        scene.mrs_labels(image, labb, Sb, scale, tile=TILE, device=DEV)
    assert str(one.value) == str(scene_wide.value)
