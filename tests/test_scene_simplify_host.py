"""CPU: the host side of scene.simplify_labels.  The sparse form of `keep` without a GPU: the spec's per-tile
node records (tests/scene_simplify_ref.py), joined, are the nodes of the one-raster rule (tests/simplify_ref.py) on the assembled
raster for every tile size; arc_keep and the ring rule from the sorted lists give exactly simplify_ref.simplify; the three facts the
form rests on are asserted as such.  Then three answers worked by hand, every limit, the declaration / binding / export of the new
entry points and their validation before any launch."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import scene_simplify_ref as R
import simplify_ref as S
import vector_ref as V

TILES = ((1, 1), (3, 5), (37, 41), (1000, 1000))
TOLERANCES = (0, 0.75, 1.5, 4, 4096)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib


def cases():
    return {**V.host_cases(), **S.drawn_cases(), **S.extra_cases()}


@functools.lru_cache(maxsize=None)
def traced(name):
    labels, n = cases()[name]
    return V.trace(labels, n)


# ---- the sparse form equals the spec ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases()))
def test_the_joined_tile_node_records_are_the_nodes_of_the_assembled_raster(name):
    labels, _ = cases()[name]
    want = np.flatnonzero(S.nodes(labels).reshape(-1) == 2).astype(np.int64)
    for tile in TILES:
        if tile == (1, 1) and labels.size > 100:
            continue
        got = R.scene_nodes(labels, tile)
        assert got.dtype == np.int64 and np.array_equal(got, want), tile       # every node once: ownership is a partition


@pytest.mark.parametrize("name", list(cases()))
def test_the_sparse_form_equals_the_dense_rule_and_the_three_facts_hold(name):
    labels, n = cases()[name]
    H, W = labels.shape
    t = traced(name)
    arc_ids = t["arc_xy"].astype(np.int64)[:, 1] * (W + 1) + t["arc_xy"].astype(np.int64)[:, 0]
    below_len = np.ones(len(arc_ids), bool)                        # a closed arc's repeated end is no position of the cyclic sequence
    for a in range(len(t["left"])):
        first, end = int(t["arc_ptr"][a]), int(t["arc_ptr"][a + 1])
        if end - first >= 3 and arc_ids[first] == arc_ids[end - 1]:
            below_len[end - 1] = False
    arc_of = np.searchsorted(t["arc_ptr"], np.arange(len(arc_ids)), side="right") - 1
    for tol in TOLERANCES:
        want = S.simplify(labels, n, tol, t)
        got = R.simplify(labels, n, tol, (37, 41), t)
        for key in ("arc_ptr", "arc_xy", "left", "right", "region_ptr", "ring_ptr", "xy", "ring_label", "ring_area2"):
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (tol, key)
        keep = want["keep"]
        # fact 1: a corner with keep == 1 is a stored vertex of exactly one arc, once among its positions below len
        for corner in np.flatnonzero(keep == 1):
            at = np.flatnonzero((arc_ids == corner) & below_len)
            assert len(at) == 1 and got["arc_keep"][at[0]] == 1, (tol, corner)
        assert int((got["arc_keep"] == 1).sum()) == int((keep == 1).sum())
        # fact 2: a node that lies on an arc is a stored vertex of it -- walking every arc's unit steps meets no node between vertices
        nodes = set(np.flatnonzero(keep == 2).tolist())
        for a in range(len(t["left"])):
            pts = t["arc_xy"][t["arc_ptr"][a]:t["arc_ptr"][a + 1]].astype(np.int64)
            for (x0, y0), (x1, y1) in zip(pts[:-1], pts[1:]):
                sx, sy = np.sign(x1 - x0), np.sign(y1 - y0)
                for s in range(1, abs(x1 - x0) + abs(y1 - y0)):
                    assert (y0 + s * sy) * (W + 1) + x0 + s * sx not in nodes, (a, s)
        assert np.array_equal(got["arc_keep"][below_len] == 2, keep[arc_ids[below_len]] == 2)
        # fact 3: on a ring's run from v to its successor the kept corners are v, if kept, and exactly the nodes strictly inside
        for r in range(len(t["ring_label"])):
            pts = t["xy"][t["ring_ptr"][r]:t["ring_ptr"][r + 1]].astype(np.int64)
            for (x0, y0), (x1, y1) in zip(pts, np.roll(pts, -1, 0)):
                sx, sy = np.sign(x1 - x0), np.sign(y1 - y0)
                for s in range(1, abs(x1 - x0) + abs(y1 - y0)):
                    corner = (y0 + s * sy) * (W + 1) + x0 + s * sx
                    assert (keep[corner] != 0) == (corner in nodes), (r, corner)
        assert np.array_equal(got["kept_row"], np.flatnonzero(keep != 0))
    assert arc_of.max() == len(t["left"]) - 1


def test_an_arc_wider_than_the_limit_is_left_alone():
    xy = np.array([[0, 0], [0, 5], [9, 5], [9, 9], [0, 0], [1, 0], [1, 1]], np.int32)
    ptr = np.array([0, 4, 7], np.int64)
    node_row = np.sort(np.array([0, 9 * 100 + 9, 1 * 100 + 1], np.int64))
    assert R.arc_keep(xy, ptr, node_row, 99, 0).tolist() == [2, 1, 1, 2, 2, 1, 2]
    assert R.arc_keep(xy, ptr, node_row, 99, 0, limit=8).tolist() == [2, 0, 0, 2, 2, 1, 2]


# ---- known answers by hand ------------------------------------------------------------------------------------------------------------
def test_by_hand_a_t_junction_exactly_on_a_seam():
    """[[0, 0, 0], [1, 2, 2]] in three tiles one pixel wide: the boundary 1|2 ends at (1, 1), on the seam x = 1, inside the straight
    bottom side of label 0.  The corner belongs to the tile of pixel (1, 1), the middle one; label 0's ring gets it between (3, 1)
    and (0, 1), and the arcs 0|1 and 0|2 end there."""
    L = np.array([[0, 0, 0], [1, 2, 2]], np.int32)
    per_tile = [R.tile_nodes(L[b[0]:b[1], b[2]:b[3]], core, (b[0], b[2]), 2, 3).tolist() for core, b in R.windows(2, 3, (2, 1))]
    assert per_tile == [[0, 4, 8], [5, 9], [3, 7, 11]]             # corner id = 4 y + x; the right tile also owns corner column 3
    got = R.simplify(L, 3, 4096, (2, 1))
    assert got["node_row"].tolist() == [0, 3, 4, 5, 7, 8, 9, 11] and got["node_col"].tolist() == [0, 1, 2, 4, 5, 9, 10, 11]
    assert got["xy"][:5].tolist() == [[0, 0], [3, 0], [3, 1], [1, 1], [0, 1]] and got["ring_ptr"].tolist() == [0, 5, 9, 13]
    assert R.run_vertices((3, 1), (0, 1), got["node_row"].tolist(), got["node_col"].tolist(), got["kept_row"].tolist(), 2, 3) == [(3, 1), (1, 1)]
    assert got["ring_area2"].tolist() == [6, 2, 4]
    ends = {tuple(got["arc_xy"][i]) for a in range(len(got["left"])) for i in (got["arc_ptr"][a], got["arc_ptr"][a + 1] - 1)}
    assert (1, 1) in ends


def test_by_hand_a_node_at_a_four_tile_corner():
    """[[0, 0], [1, 2]], one tile per pixel: the T-junction (1, 1) is where the four tiles meet.  It belongs to the tile of pixel
    (1, 1) alone, whose window is the whole raster, and is in the joined list once."""
    L = S.drawn_cases()["tee"][0]
    per_tile = [R.tile_nodes(L[b[0]:b[1], b[2]:b[3]], core, (b[0], b[2]), 2, 2).tolist() for core, b in R.windows(2, 2, (1, 1))]
    assert per_tile == [[0], [2], [3, 6], [4, 5, 7, 8]]            # corner id = 3 y + x; the last tile owns corner row 2 and column 2
    assert R.scene_nodes(L, (1, 1)).tolist() == [0, 2, 3, 4, 5, 6, 7, 8]       # every corner but (1, 0), inside label 0's top side
    got = R.simplify(L, 3, 0.75, (1, 1))
    assert got["xy"][:5].tolist() == [[0, 0], [2, 0], [2, 1], [1, 1], [0, 1]]  # label 0's ring with the junction on its bottom side


def test_by_hand_a_closed_arc_whose_anchor_lies_in_another_tile_than_its_stored_start():
    """An L-shaped island of label 1 in a 6 x 6 raster of label 0, tiles of 3 x 4.  Its boundary is one closed arc without a node,
    stored from (4, 2), a corner of the tile column on the right; the vertex smallest in (y, x) is (3, 2), in the left tile column.
    The anchor is found by corner id and position alone, so the tiling does not matter: the simplified arc begins and ends at (3, 2)."""
    L = np.zeros((6, 6), np.int32)
    L[2, 3] = L[3, 2] = L[3, 3] = 1
    t = V.trace(L, 2)
    assert t["arc_xy"][5:].tolist() == [[4, 2], [3, 2], [3, 3], [2, 3], [2, 4], [4, 4], [4, 2]]
    owner = lambda x, y: (min(y, 5) // 3, min(x, 5) // 4)
    assert owner(4, 2) == (0, 1) and owner(3, 2) == (0, 0)
    got = R.simplify(L, 2, 1.5, (3, 4), t)
    assert got["node_row"].tolist() == [0, 6, 42, 48]
    assert got["arc_keep"].tolist() == [2, 2, 2, 2, 2, 0, 1, 0, 0, 1, 1, 0]
    assert got["arc_xy"][5:].tolist() == [[3, 2], [2, 4], [4, 4], [3, 2]]
    assert got["kept_row"].tolist() == [0, 6, 17, 30, 32, 42, 48]
    want = S.simplify(L, 2, 1.5, t)
    assert np.array_equal(got["xy"], want["xy"]) and np.array_equal(got["ring_area2"], want["ring_area2"])


# ---- limits ---------------------------------------------------------------------------------------------------------------------------------
class Shape:
    """A source of a given shape whose pixels are never read (the limits are checked before the first read)."""

    def __init__(self, *shape):
        self.shape = shape

    def read(self, y0, y1, x0, x1):
        raise AssertionError("read before the limits were checked")


def test_every_limit_is_a_value_error_before_any_device_work():
    from deepmerge_amd import scene
    simplify = lambda src, n=1, t=1.5, **kw: scene.simplify_labels(src, n, t, device="cpu", **kw)
    for t in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tolerance must be finite and >= 0"):
            simplify(Shape(20, 30), t=t)
    with pytest.raises(ValueError, match="tolerance must be at most 4096 pixels"):
        simplify(Shape(20, 30), t=4096.01)
    with pytest.raises(ValueError, match="tolerance must be finite"):           # the tolerance comes first: the shape is not even looked at
        simplify(Shape(3, 20, 30), t=-1)
    # every limit of trace_labels
    for shape in ((3, 20, 30), (20,), (0, 30), (20, 0)):
        with pytest.raises(ValueError, match="source.shape must be"):
            simplify(Shape(*shape))
    for shape in (((1 << 31) - 1, 4), (4, (1 << 31) - 1), (1 << 40, 4)):
        with pytest.raises(ValueError, match="H and W must be below 2\\^31 - 1"):
            simplify(Shape(*shape))
    with pytest.raises(ValueError, match="at most 2\\^60 pixels"):
        simplify(Shape((1 << 31) - 2, (1 << 31) - 2))
    for n in (0, -1, 1 << 31):
        with pytest.raises(ValueError, match="n_labels must be in"):
            simplify(Shape(20, 30), n)
    for tile in (0, -4, (8, 0)):
        with pytest.raises(ValueError, match="tile must be >= 1"):
            simplify(Shape(20, 30), tile=tile)
    with pytest.raises(ValueError, match="at most 2\\^28 pixels, got 16385 x 16385"):
        simplify(Shape(1 << 20, 1 << 20), tile=16383)
    with pytest.raises(AssertionError, match="read before"):      # a scene within every limit goes on to read
        simplify(Shape(1 << 20, 1 << 20), tile=16382, t=4096)
    L = np.zeros((6, 8), np.int32)
    L[0, 0] = 2
    with pytest.raises(ValueError, match="window of tile 0 .*holds 0..2"):
        simplify(L, 2, tile=(3, 4))
    # fewer than 2^31 nodes, counted as the tiles come in
    scene._check_nodes((1 << 31) - 1, 3, 9)
    with pytest.raises(ValueError, match="2\\^31 nodes or more .*after tile 3 of 9"):
        scene._check_nodes(1 << 31, 3, 9)
    assert scene.MAX_ARC_EXTENT == 32768 == S.MAX_SIDE


def test_the_arc_extent_limit_names_the_arc():
    """The reduction of `_check_arc_extents` is plain torch: on the CPU it names the arc, its labels and its extent."""
    from deepmerge_amd import rag, scene
    xy = torch.tensor([[5, 5], [5, 9], [40000, 9], [7, 7], [7, 32775], [8, 32775]], dtype=torch.int32)
    arcs = rag.Arcs(arc_ptr=torch.tensor([0, 3, 6]), xy=xy, left=torch.tensor([4, -1], dtype=torch.int32), right=torch.tensor([1, 3], dtype=torch.int32))
    with pytest.raises(ValueError, match=r"arc 0 between \(left, right\) = \(4, 1\) spans 39995 x 4 pixels"):
        scene._check_arc_extents(arcs)
    arcs.xy = xy.clone()
    arcs.xy[2, 0] = 32773                                          # 32768 wide: the limit itself passes
    scene._check_arc_extents(arcs)
    arcs.xy[5, 1] = 32776
    with pytest.raises(ValueError, match=r"arc 1 between \(left, right\) = \(-1, 3\) spans 1 x 32769 pixels"):
        scene._check_arc_extents(arcs)


def test_cpu_tensors_have_no_fallback():
    from deepmerge_amd import rag, scene
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene.simplify_labels(np.zeros((4, 4), np.int32), 1, 1.5, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene._tile_nodes(torch.zeros((4, 4), dtype=torch.int32), (0, 4, 0, 4), (0, 0), 4, 4)
    L = np.zeros((4, 4), np.int32)
    t = V.trace(L, 1)
    polys = rag.Polygons(*(torch.from_numpy(t[k]) for k in ("region_ptr", "ring_ptr", "xy", "ring_label", "ring_area2")))
    arcs = rag.Arcs(*(torch.from_numpy(t[k]) for k in ("arc_ptr", "arc_xy", "left", "right")))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene._simplify_tables(polys, arcs, torch.from_numpy(R.scene_nodes(L, (4, 4))), 4, 4, 0)


def test_the_public_interface_is_there():
    import inspect
    from deepmerge_amd import scene
    from deepmerge_amd.ExtractFeatures import FeatureIO
    assert list(inspect.signature(scene.simplify_labels).parameters) == ["source", "n_labels", "tolerance", "tile", "stats", "device"]
    assert inspect.signature(scene.simplify_labels).parameters["tile"].default == 4096
    assert list(inspect.signature(scene.SceneResult.simplified).parameters) == ["self", "tolerance", "merged", "tile", "stats"]
    assert inspect.signature(scene.SceneResult.save_shapefiles).parameters["tolerance"].default is None
    assert callable(FeatureIO.simplify_scene)


# ---- the library's side, without a GPU ----------------------------------------------------------------------------------------------------
NEW = ("dm_scene_simplify_node_count", "dm_scene_simplify_node_emit", "dm_scene_simplify_chains", "dm_scene_simplify_arc_count",
       "dm_scene_simplify_arc_emit", "dm_scene_simplify_ring_count", "dm_scene_simplify_ring_emit")


def test_the_entry_points_are_declared_bound_and_exported(built):
    text = re.sub(r"/\*.*?\*/", "", open(built.HEADER_PATH).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(built.SIGNATURES[name][1]), name
        assert re.search(r" T " + name + r"\b", nm), name
    assert set(NEW) <= set(built.declared_symbols())
    assert built.lib().dm_abi_version() == 7                       # additive
    rings = built.DmSceneSimplifyRings
    assert [f[0] for f in rings._fields_] == ["xy", "ring_ptr", "vert_ring", "node_row", "node_col", "kept_row", "status", "n_nodes", "n_kept",
                                              "scene_h", "scene_w", "V", "R"]
    assert ctypes.sizeof(rings) == 96 and rings.n_nodes.offset == 56 and rings.V.offset == 88
    struct = re.search(r"typedef struct DmSceneSimplifyRings \{(.*?)\}", text, flags=re.S).group(1)
    assert "const int64_t *node_row, *node_col, *kept_row;" in struct and "int64_t n_nodes, n_kept, scene_h, scene_w;" in struct


def test_the_node_entries_refuse_bad_arguments_before_any_launch(built):
    lib = built.lib()
    p = 4096                                                       # any non-null address: validation never dereferences
    big = (1 << 31) - 2
    for name, tail in (("dm_scene_simplify_node_count", dict(tile_off=p, n_nodes=p)), ("dm_scene_simplify_node_emit", dict(tile_off=p, N=5, node=p))):
        call = getattr(lib, name)
        ok = dict(labels=p, H=10, W=12, cy0=1, cy1=9, cx0=1, cx1=11, oy=7, ox=9, scene_h=100, scene_w=big, **tail)
        cases = [(dict(**{k: None}), b"null pointer") for k in ok if ok[k] == p]
        cases += [(dict(H=0), b"H*W"), (dict(W=-1), b"H*W"), (dict(H=1 << 14, W=(1 << 14) + 1), b"H*W"),
                  (dict(cy0=-1), b"must lie in the window"), (dict(cy0=2), b"must lie in the window"), (dict(cy1=11), b"must lie in the window"),
                  (dict(cy1=8), b"must lie in the window"), (dict(cx1=13), b"must lie in the window"), (dict(cy0=9, cy1=9), b"must lie in the window"),
                  (dict(scene_w=big + 1), b"must lie in a scene"), (dict(scene_h=big, scene_w=big), b"must lie in a scene"),
                  (dict(oy=-1), b"must lie in a scene"), (dict(oy=91), b"must lie in a scene"), (dict(ox=big - 11), b"must lie in a scene"),
                  # a core that touches a window edge inside the scene: an owned corner would ask for a pixel the window lacks
                  (dict(cy0=0), b"only where that is the scene's edge"), (dict(cx1=12), b"only where that is the scene's edge")]
        if "N" in tail:
            cases += [(dict(N=0), b"bad sizes"), (dict(N=-3), b"bad sizes"), (dict(N=11 * 13 + 1), b"bad sizes")]
        for change, msg in cases:
            args = {**ok, **change}
            assert call(*args.values(), None) == -1, (name, change)
            assert name.encode() in lib.dm_last_error() and msg in lib.dm_last_error(), (change, lib.dm_last_error())


def test_the_arc_entries_refuse_bad_arguments_before_any_launch(built):
    lib = built.lib()
    p = 4096
    big = (1 << 31) - 2
    calls = (("dm_scene_simplify_chains", dict(arc_xy=p, arc_ptr=p, A=3, Va=9, scene_h=big, scene_w=100, q=384, arc_keep=p, stack=p)),
             ("dm_scene_simplify_arc_count", dict(arc_xy=p, arc_ptr=p, A=3, Va=9, scene_h=big, scene_w=100, arc_keep=p, count=p)),
             ("dm_scene_simplify_arc_emit", dict(arc_xy=p, arc_ptr=p, new_ptr=p, A=3, Va=9, Vn=6, scene_h=big, scene_w=100, arc_keep=p, out_xy=p)))
    for name, ok in calls:
        call = getattr(lib, name)
        cases = [(dict(**{k: None}), b"null pointer") for k in ok if ok[k] == p]
        cases += [(dict(A=0), b"bad sizes"), (dict(A=-1), b"bad sizes"), (dict(Va=1), b"bad sizes"), (dict(Va=-9), b"bad sizes"),
                  (dict(Va=1 << 31), b"bad sizes"), (dict(scene_h=0), b"bad scene"), (dict(scene_w=-5), b"bad scene"),
                  (dict(scene_h=big + 1), b"bad scene"), (dict(scene_h=big, scene_w=big), b"bad scene")]
        if "q" in ok:
            cases += [(dict(q=-1), b"bad tolerance"), (dict(q=(1 << 20) + 1), b"bad tolerance")]
        if "Vn" in ok:
            cases += [(dict(Vn=0), b"bad sizes"), (dict(Vn=10), b"bad sizes")]
        for change, msg in cases:
            args = {**ok, **change}
            assert call(*args.values(), None) == -1, (name, change)
            assert name.encode() in lib.dm_last_error() and msg in lib.dm_last_error(), (name, change, lib.dm_last_error())


def test_the_ring_entries_refuse_bad_arguments_before_any_launch(built):
    """What the host can see of the lists is their sizes: a scene has its four corners, fewer than 2^31 nodes, and no fewer kept
    corners than nodes.  That a list is sorted is checked where it is read, on the device (status; tests/test_gpu_scene_simplify.py)."""
    lib = built.lib()
    p = 4096

    def rings(**change):
        t = built.DmSceneSimplifyRings()
        for f, _ in t._fields_[:7]:
            setattr(t, f, p)
        t.n_nodes, t.n_kept, t.scene_h, t.scene_w, t.V, t.R = 40, 90, 1 << 20, (1 << 31) - 2, 64, 3
        for k, v in change.items():
            setattr(t, k, v)
        return t

    count = lambda t, out=p: lib.dm_scene_simplify_ring_count(None if t is None else ctypes.byref(t), out, None)
    emit = lambda t, scan=p, ptr=p, Vn=70, out=p, area=p: lib.dm_scene_simplify_ring_emit(None if t is None else ctypes.byref(t), scan, ptr, Vn, out, area, None)
    for name, call in ((b"dm_scene_simplify_ring_count", count), (b"dm_scene_simplify_ring_emit", emit)):
        assert call(None) == -1 and name in lib.dm_last_error() and b"null argument struct" in lib.dm_last_error()
        for field, _ in built.DmSceneSimplifyRings._fields_[:7]:
            assert call(rings(**{field: None})) == -1, field
            assert name in lib.dm_last_error() and b"null pointer" in lib.dm_last_error(), field
        for change in (dict(V=0), dict(V=-4), dict(R=0), dict(R=65)):
            assert call(rings(**change)) == -1 and b"bad sizes" in lib.dm_last_error(), change
        for change in (dict(n_nodes=3), dict(n_nodes=-1), dict(n_nodes=1 << 31, n_kept=1 << 31), dict(n_kept=39), dict(n_kept=1 << 32)):
            assert call(rings(**change)) == -1 and b"oversized or undersized list" in lib.dm_last_error(), change
        for change in (dict(scene_h=0), dict(scene_w=(1 << 31) - 1), dict(scene_h=(1 << 31) - 2)):
            assert call(rings(**change)) == -1 and b"bad scene" in lib.dm_last_error(), change
    assert count(rings(), None) == -1 and b"null pointer" in lib.dm_last_error()
    for kw in (dict(scan=None), dict(ptr=None), dict(out=None), dict(area=None)):
        assert emit(rings(), **kw) == -1 and b"null pointer" in lib.dm_last_error(), kw
    for Vn in (0, -1, 1 << 32):
        assert emit(rings(), Vn=Vn) == -1 and b"bad sizes" in lib.dm_last_error(), Vn
