"""GPU: topology-safe simplification of a scene (deepmerge_amd/scene.py simplify_labels_topology / simplify_conflicts,
csrc/dm_scene_simplify_topology.hip).  The definition is the test: whatever the tile size and the cell side of the
search grid, every array of the result is bit-equal to `rag.simplify(topology=True)` on the whole raster, and the flagged segments
of every round are the same.  Then the seams against the spec itself, the kernels far from the origin, the properties a repaired
layer has, every error, and SceneResult.simplified / save_shapefiles."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import simplify_ref as S
import simplify_topology_ref as T
import test_gpu_scene_vector as TV
import vector_ref as V
from test_gpu_scene_vector import assert_same, dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG_W = (1 << 31) - 2
CASES = T.cases()
NAMES = list(CASES)
NOISE = [name for name in NAMES if name.startswith("noise")]
TILES = ((3, 64), (64, 3), (37, 41), (4096, 4096))                # the last: one tile larger than the scene


@functools.lru_cache(maxsize=None)
def whole(name, tol, topology=True):
    """The reference, once per raster and tolerance: rag.simplify on the whole raster, and its stats."""
    from deepmerge_amd import rag
    labels, n = CASES[name]
    stats = {}
    polys, arcs = rag.simplify(dev(labels), n, tol, stats=stats, topology=topology)
    return (polys, arcs), stats


@functools.lru_cache(maxsize=None)
def traced(name):
    return V.trace(*CASES[name])


@functools.lru_cache(maxsize=None)
def spec(name, tol):
    labels, n = CASES[name]
    return T.simplify(labels, n, tol, traced(name))


def assert_equals_spec(got, want, what):
    polys, arcs = got
    for key, g in (("region_ptr", polys.region_ptr), ("ring_ptr", polys.ring_ptr), ("xy", polys.xy), ("ring_label", polys.ring_label),
                   ("ring_area2", polys.ring_area2), ("arc_ptr", arcs.arc_ptr), ("arc_xy", arcs.xy), ("left", arcs.left), ("right", arcs.right)):
        g = g.cpu().numpy()
        assert g.dtype == want[key].dtype and g.shape == want[key].shape and np.array_equal(g, want[key]), (what, key)


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_tiled_repair_equals_the_one_raster_repair(name):
    from deepmerge_amd import scene
    labels, n = CASES[name]
    before = labels.copy()
    for tol in T.TOLERANCES:
        want, want_stats = whole(name, tol)
        for tile in TILES:
            stats = {}
            got = scene.simplify_labels_topology(scene.ArraySource(labels), n, tol, tile, stats=stats)
            assert_same(got, want, (name, tile, tol))
            assert stats["topology_flagged"] == want_stats["topology_flagged"] and stats["topology_flagged"][-1] == 0, (name, tile, tol)
            assert stats["topology_rounds"] == want_stats["topology_rounds"] == len(stats["topology_flagged"]) - 1
            assert stats["topology_segments"] == want_stats["topology_segments"] and stats["topology_cell_log2"] == 5
            assert stats["topology_cell_entries"] == want_stats["topology_cell_entries"]
            assert len(stats["topology_stage_ms"]) == len(stats["topology_flagged"]) and "simplify: topology rounds" in stats["stage_s"]
        print(f"{name} t={tol}: {labels.shape}, flagged per round {want_stats['topology_flagged']}")
    assert np.array_equal(labels, before)


def test_the_cases_take_no_round_and_several_rounds():
    """So that the parity above cannot pass on data without conflicts: every case at tolerance 0 takes no repair round, and the noise
    rasters at tolerance 20 take two or more (up to 4)."""
    assert all(whole(name, 0)[1]["topology_rounds"] == 0 for name in NAMES)
    rounds = {name: whole(name, 20)[1]["topology_rounds"] for name in NOISE}
    print(rounds)
    assert max(rounds.values()) >= 2 and all(r >= 1 for r in rounds.values())
    assert whole("bay", 20)[1]["topology_rounds"] >= 1 and whole("long_bay", 20)[1]["topology_rounds"] >= 1


@pytest.mark.parametrize("tile", [(3, 31), (3, 32), (3, 33), (7, 70)])
def test_conflicts_jumps_and_refined_chains_across_a_seam_equal_the_spec(tile):
    """long_bay is 7 x 200: with tiles 31, 32 and 33 wide the seams lie beside and on the edges of the 32-corner cells, at 70 wide
    away from them.  The flagged segments, the jumped fixed points and the chains a repair refines reach over every one of them."""
    from deepmerge_amd import scene
    labels, n = CASES["long_bay"]
    for tol in T.TOLERANCES:
        want = spec("long_bay", tol)
        stats = {}
        got = scene.simplify_labels_topology(labels, n, tol, tile, stats=stats)
        assert_equals_spec(got, want, (tile, tol))
        assert stats["topology_flagged"] == want["flagged"] and stats["topology_rounds"] == want["rounds"]
    first = spec("long_bay", 20)["conflicts"]
    seams = range(tile[1], 200, tile[1])
    for bit in (T.MEETS, T.JUMPS):                                 # (70, 2) - (130, 3) meets its twin; (200, 5) - (0, 5) jumped over a node
        spans = [(min(x0, x1), max(x0, x1)) for (x0, _, x1, _), k in zip(first["xy"].tolist(), first["kind"].tolist()) if k & bit]
        assert any(lo <= s <= hi for lo, hi in spans for s in seams), bit
        assert any(lo < c < hi for lo, hi in spans for c in range(32, 200, 32)), bit
    H, W = labels.shape
    plain = S.keep_flags(labels, traced("long_bay"), S.quantise(20)).reshape(H + 1, W + 1)
    restored = np.nonzero((spec("long_bay", 20)["keep"].reshape(H + 1, W + 1) == 1) & (plain == 0))[1]
    assert len(restored) and restored.min() < tile[1] < restored.max()


@pytest.mark.parametrize("name", ["bay", "long_bay", "noise32_7", "noise24_23"])
def test_scene_simplify_conflicts_equals_the_one_raster_call_and_the_spec(name):
    from deepmerge_amd import rag, scene
    labels, n = CASES[name]
    for tol in (1, 2.5):
        want, one = spec(name, tol)["conflicts"], rag.simplify_conflicts(dev(labels), n, tol)
        for tile in ((3, 33), (4096, 4096)):
            got = scene.simplify_conflicts(labels, n, tol, tile=tile, device=DEV)
            assert isinstance(got, rag.Conflicts) and got.n_segments == one.n_segments == want["n_segments"]
            for key, dtype in (("arc", torch.int32), ("xy", torch.int32), ("kind", torch.uint8)):
                g = getattr(got, key)
                assert g.dtype == dtype and torch.equal(g, getattr(one, key)), (tol, tile, key)
                assert g.shape == want[key].shape and np.array_equal(g.cpu().numpy(), want[key]), (tol, tile, key)
        assert len(want["kind"]) > 0


@pytest.mark.parametrize("name", ["noise48_7", "long_bay", "smooth"])
def test_the_result_does_not_depend_on_the_cell_side(name):
    """Cells of 32, 64, 256 and 4096 corners.  With 4096 the whole raster is one cell: noise48_7 then has several hundred segments
    in it and the pair kernel takes more than one turn of 64 lanes."""
    from deepmerge_amd import scene
    labels, n = CASES[name]
    for tol in (1, 20):
        want, want_stats = whole(name, tol)
        for log2 in (5, 6, 8, 12):
            stats = {}
            got = scene.simplify_labels_topology(labels, n, tol, (37, 41), stats=stats, _cell_log2=log2)
            assert_same(got, want, (name, tol, log2))
            assert stats["topology_flagged"] == want_stats["topology_flagged"] and stats["topology_cell_log2"] == log2, (name, tol, log2)
        if name == "noise48_7":
            assert stats["topology_cell_entries"] == stats["topology_segments"] > 64        # one cell: every segment once
    with pytest.raises(ValueError, match="_cell_log2"):
        scene.simplify_labels_topology(labels, n, 1, _cell_log2=4)
    with pytest.raises(ValueError, match="_cell_log2"):
        scene.simplify_labels_topology(labels, n, 1, _cell_log2=25)


# ---- the kernels far from the origin ------------------------------------------------------------------------------------------------------
def tables(name, H, W, shift=(0, 0)):
    """rag._trace of a raster and its nodes, translated by shift = (ox, oy) into an H x W scene."""
    from deepmerge_amd import rag
    labels, n = CASES[name]
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


@pytest.mark.parametrize("name", ["bay", "long_bay", "noise32_7"])
def test_the_rounds_on_a_translated_set_give_the_untranslated_answer_shifted(name):
    """The set is moved by (2^31 - 40000, 2^29 - 1000) to the far corner of a scene of 2^29 x (2^31 - 2) pixels, where the cell side
    comes out 2^20 and one cell holds every segment.  arc_keep is found by position and does not change, the flagged segments of
    every round are the same, the vertices are the untranslated ones shifted, and ring_area2 is the int64 shoelace sum."""
    from deepmerge_amd import rag, scene
    labels, n = CASES[name]
    h, w = labels.shape
    H, W, shift = 1 << 29, BIG_W, ((1 << 31) - 40000, (1 << 29) - 1000)
    assert scene.topology_cell_log2(H, W) == 20
    for tol in (1, 2.5, 20):
        q = rag._quantise_tolerance(tol)
        near_stats, far_stats = {}, {}
        near = scene._simplify_tables(*tables(name, h, w), h, w, q, stats=near_stats, topology=True)
        far = scene._simplify_tables(*tables(name, H, W, shift), H, W, q, stats=far_stats, topology=True)
        assert_same(near[:2], whole(name, tol)[0], (name, tol))
        assert far_stats["topology_cell_log2"] == 20 and near_stats["topology_cell_log2"] == 5
        assert far_stats["topology_flagged"] == near_stats["topology_flagged"] == whole(name, tol)[1]["topology_flagged"]
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
    assert near_stats["topology_rounds"] >= 1


# ---- what a repaired layer has ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NOISE)
def test_properties_of_the_repaired_result(name):
    from deepmerge_amd import rag, scene
    labels, n = CASES[name]
    H, W = labels.shape
    (polys, arcs), _ = whole(name, 20)
    got = scene.simplify_labels_topology(labels, n, 20, (17, 19))
    plain = scene.simplify_labels(labels, n, 20, (17, 19))
    assert_same(got, (polys, arcs))
    area2 = got[0].ring_area2.cpu().numpy()
    assert (area2 != 0).all() and np.array_equal(np.sign(area2), np.sign(traced(name)["ring_area2"]))
    assert int(area2.sum()) == 2 * H * W
    # the kept vertices contain the plain call's, arc by arc
    for a in range(arcs.left.numel()):
        mine = {tuple(p) for p in got[1].xy[got[1].arc_ptr[a]:got[1].arc_ptr[a + 1]].tolist()}
        assert {tuple(p) for p in plain[1].xy[plain[1].arc_ptr[a]:plain[1].arc_ptr[a + 1]].tolist()} <= mine, a
    assert scene.simplify_conflicts(labels, n, 20, tile=(17, 19)).kind.numel() > 0
    # a detection round on the repaired flags reports nothing
    q = rag._quantise_tolerance(20)
    polys0, arcs0, node_row = tables(name, H, W)
    arc_keep = scene._simplify_tables(polys0, arcs0, node_row, H, W, q, topology=True)[2]
    rounds = scene._SceneTopologyRounds(arcs0, arc_keep, H, W, q, cell_log2=5)
    assert rounds._round(False, False) == (0, 0) and rounds.conflicts().kind.numel() == 0


@pytest.mark.parametrize("name", ["one_label", "frame_hole", "noise32_7", "long_bay"])
def test_without_conflicts_the_result_is_the_plain_one(name):
    from deepmerge_amd import scene
    labels, n = TV.raster(name) if name in ("one_label", "frame_hole") else CASES[name]
    for tol in ((0, 1.5, 20) if name in ("one_label", "frame_hole") else (0,)):
        stats = {}
        got = scene.simplify_labels_topology(labels, n, tol, (37, 41), stats=stats)
        assert_same(got, scene.simplify_labels(labels, n, tol, (37, 41)), (name, tol))
        assert stats["topology_rounds"] == 0 and stats["topology_flagged"] == [0]
        assert scene.simplify_conflicts(labels, n, tol, tile=(37, 41)).kind.numel() == 0


# ---- errors -----------------------------------------------------------------------------------------------------------------------------
def test_every_error_is_raised():
    from deepmerge_amd import scene
    labels, n = CASES["noise32_7"]
    assert whole("noise32_7", 2.5)[1]["topology_rounds"] == 3
    with pytest.raises(ValueError, match="max_rounds"):
        scene.simplify_labels_topology(labels, n, 2.5, max_rounds=0)
    with pytest.raises(RuntimeError, match="conflicts remain after 1 repair rounds"):
        scene.simplify_labels_topology(labels, n, 2.5, max_rounds=1)
    with pytest.raises(RuntimeError, match="repair rounds"):
        scene.simplify_labels_topology(labels, n, 2.5, max_rounds=2)
    assert_same(scene.simplify_labels_topology(labels, n, 2.5, max_rounds=3), whole("noise32_7", 2.5)[0])
    for tol in (-1, float("nan"), 4097):
        with pytest.raises(ValueError, match="tolerance"):
            scene.simplify_labels_topology(labels, n, tol)
        with pytest.raises(ValueError, match="tolerance"):
            scene.simplify_conflicts(labels, n, tol)
    for bad, kw in ((labels.astype(np.int64), {}), (labels[None], {}), (labels, dict(tile=0))):
        with pytest.raises(ValueError):
            scene.simplify_labels_topology(bad, n, 1.5, **kw)
    with pytest.raises(ValueError, match="fewer than 2\\^30 arcs"):
        scene._check_topology(100, 100, 1 << 30, 1 << 20, 64, None)
    with pytest.raises(ValueError, match="at most 2\\^30 arc vertices"):
        scene._check_topology(100, 100, 1 << 20, (1 << 30) + 1, 64, None)
    assert scene._check_topology(100, 100, (1 << 30) - 1, 1 << 30, 1, None) == 5


ENTRIES = ("point_count", "point_fill", "segments", "bin_count", "bin_fill", "pairs", "jumps", "refine")


def test_every_entry_refuses_a_bad_struct_with_an_error_code():
    from deepmerge_amd import _lib, rag, scene
    from deepmerge_amd.ops import _stream
    lib = _lib.lib()
    labels, n = CASES["bay"]
    H, W = labels.shape
    polys, arcs, node_row = tables("bay", H, W)
    arc_keep = scene._chain_flags(arcs, node_row, H, W, 256)[2]
    rounds = scene._SceneTopologyRounds(arcs, arc_keep, H, W, 256, cell_log2=5)
    rounds.stack = torch.empty(2 * rounds.Va, dtype=torch.int64, device=DEV)
    rounds.t.stack = rounds.stack.data_ptr()
    side = (1 << 31) - 2

    def call(name, **kw):
        t = _lib.DmSceneSimplifyTopology.from_buffer_copy(rounds.t)
        for k, v in kw.items():
            setattr(t, k, v)
        fn = getattr(lib, "dm_scene_simplify_topology_" + name)
        return fn(ctypes.byref(t), 1, _stream()) if name == "refine" else fn(ctypes.byref(t), _stream())

    for name in ENTRIES:
        for kw in (dict(H=65536, W=65536), dict(H=side, W=side), dict(cell_log2=4), dict(cell_log2=25), dict(A=1 << 30), dict(arc_keep=None),
                   dict(arc_xy=None), dict(H=0), dict(W=side + 1, cell_log2=24)):
            assert call(name, **kw) == -1, (name, kw)                 # DM_ERR_BAD_SHAPE
    torch.cuda.synchronize()
    assert rounds._round(False, False)[0] == int(rag.simplify_conflicts(dev(labels), n, 1).kind.numel())       # the struct itself is good


def test_a_cell_list_that_does_not_fit_keeps_nothing_and_the_retry_succeeds():
    """noise48_7 at tolerance 0.75: 1135 segments take 1180 entries of the four cells' lists, 102 of them flagged; the list is forced
    to 1024 entries."""
    from deepmerge_amd import rag, scene
    labels, n = CASES["noise48_7"]
    H, W = labels.shape
    q = rag._quantise_tolerance(0.75)
    polys, arcs, node_row = tables("noise48_7", H, W)
    want = scene._simplify_tables(polys, arcs, node_row, H, W, q, topology=True)[2]
    arc_keep = scene._chain_flags(arcs, node_row, H, W, q)[2]
    plain = arc_keep.clone()
    rounds = scene._SceneTopologyRounds(arcs, arc_keep, H, W, q, cap=1024, cell_log2=5)
    assert rounds.t.cap == 1024
    # one round by hand at the small cap: refine keeps nothing and reports the entries needed
    rounds.stack = torch.empty(2 * rounds.Va, dtype=torch.int64, device=DEV)
    rounds.t.stack = rounds.stack.data_ptr()
    rounds._arc_count()
    torch.cumsum(rounds.count, 0, dtype=torch.int64, out=rounds.new_ptr[1:])
    for entry in ("segments", "bin_count"):
        rounds._call(entry)
    torch.cumsum(rounds.cell_count, 0, dtype=torch.int64, out=rounds.cell_ptr[1:])
    for entry in ("bin_fill", "pairs", "jumps"):
        rounds._call(entry)
    rounds._call("refine", 1)
    need = int(rounds.status[2])
    assert need == 1180 and int(rounds.status[0]) > 0 and torch.equal(arc_keep, plain)
    # the driver's own loop grows the list (again in a later round: a repaired scene has more segments) and repairs
    flagged = rounds.repair(64)
    assert rounds.t.cap == rounds.cell_seg.numel() >= need and flagged[-1] == 0 and len(flagged) > 1
    assert torch.equal(arc_keep, want) and not torch.equal(arc_keep, plain)
    assert flagged == whole("noise48_7", 0.75)[1]["topology_flagged"]


def test_inputs_are_unmodified_and_two_calls_and_a_side_stream_agree():
    from deepmerge_amd import scene
    labels, n = CASES["noise48_7"]
    before = labels.copy()
    first = scene.simplify_labels_topology(labels, n, 2.5, (17, 32))
    assert_same(scene.simplify_labels_topology(torch.from_numpy(labels), n, 2.5, (17, 32)), first)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = scene.simplify_labels_topology(labels, n, 2.5, (17, 32))
        found = scene.simplify_conflicts(labels, n, 2.5, tile=(17, 32))
    side.synchronize()
    assert_same(got, first)
    assert_same(first, whole("noise48_7", 2.5)[0])
    assert torch.equal(found.kind, scene.simplify_conflicts(labels, n, 2.5).kind) and found.kind.numel() > 0
    assert np.array_equal(labels, before)


# ---- SceneResult.simplified / save_shapefiles -------------------------------------------------------------------------------------------
# The keyword's way through SceneResult and FeatureIO.  The fixture's 18 merged regions are blocks: no tolerance up to 64 pixels
# breaks them, so these calls take one detection round and no repair; FeatureIO.simplify_scene is also run where a repair takes rounds.
TOLERANCE = 4


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


def test_scene_result_simplified_with_topology_equals_merge_tile_on_the_assembled_raster(merged_scene):
    fio, res, want, raster_ = merged_scene
    merged = res.write_merged()
    want_polys, want_arcs = want.simplified(raster_, TOLERANCE, topology=True)
    stats = {}
    got = res.simplified_topology(TOLERANCE, stats=stats)
    assert stats["topology_flagged"] == [0] and stats["topology_rounds"] == 0 and stats["topology_cell_log2"] == 5
    assert_same(got, (want_polys, want_arcs))
    assert got[1].edge.dtype == torch.int32 and torch.equal(got[1].edge, want_arcs.edge) and bool((got[1].edge >= 0).any())
    assert stats["tiles"] == 9
    assert_same(res.simplified_topology(TOLERANCE, merged=merged, tile=(50, 77)), (want_polys, want_arcs))
    C = int(res.result.rep.numel())
    assert_same(fio.simplify_scene(merged, C, TOLERANCE, tile=(50, 77), topology=True), (want_polys, want_arcs))
    assert_same(res.simplified(TOLERANCE, merged=merged), want.simplified(raster_, TOLERANCE))              # the default is the plain call
    labels, n = CASES["noise48_7"]
    noisy = {}
    assert_same(fio.simplify_scene(labels, n, 2.5, tile=(17, 32), topology=True, stats=noisy), whole("noise48_7", 2.5)[0])
    assert noisy["topology_rounds"] == 3
    area2 = got[0].ring_area2
    assert bool((area2 != 0).all()) and int(area2.sum()) == 2 * merged.shape[0] * merged.shape[1]


def test_scene_result_save_shapefiles_with_topology_round_trips(merged_scene, tmp_path):
    from deepmerge_amd import shpstore
    _, res, _, _ = merged_scene
    polys, arcs = res.simplified_topology(TOLERANCE)
    paths = res.save_shapefiles(str(tmp_path / "safe"), tolerance=TOLERANCE, topology=True)
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
    # the default and topology=False write what the call wrote before it took the keyword; without a tolerance the keyword changes nothing
    plain = res.save_shapefiles(str(tmp_path / "plain"), tolerance=TOLERANCE)
    false = res.save_shapefiles(str(tmp_path / "false"), tolerance=TOLERANCE, topology=False)
    traced_ = res.save_shapefiles(str(tmp_path / "traced"))
    staircase = res.save_shapefiles(str(tmp_path / "staircase"), topology=True)
    for a, b in list(zip(plain, false)) + list(zip(traced_, staircase)):
        for ext in (".shp", ".shx", ".dbf"):
            assert open(a[:-4] + ext, "rb").read() == open(b[:-4] + ext, "rb").read(), (a, ext)
