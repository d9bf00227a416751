"""CPU: the host side of scene.trace_labels.  The apron argument without a GPU: the spec's per-tile records
(tests/scene_vector_ref.py), joined by the driver's own `scene._join`, are exactly the darts, the successor map and the flags of
the one-raster rule (tests/vector_ref.py) on the assembled raster, for every tile size.  Then three answers worked by hand, every
limit, the declaration / binding / export of the new entry points and their validation before any launch."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import scene_vector_ref as R
import vector_ref as V

TILES = ((1, 1), (3, 5), (37, 41), (1000, 1000))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib


def cases():
    out = dict(V.host_cases())
    out["random_45x50"] = (np.random.default_rng(4).integers(0, 3, (45, 50)).astype(np.int32), 3)      # (37, 41) cuts it in four
    return out


def join(rec):
    from deepmerge_amd import scene
    t = lambda k: torch.from_numpy(rec[k])
    return [v.numpy() for v in scene._join(t("id"), t("succ"), t("lab"), t("other"), t("succ_flags"))]


# ---- the join equals the spec ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases()))
def test_the_joined_tile_records_are_the_one_raster_successor_map(name):
    labels, _ = cases()[name]
    d, nxt = V.successor_map(labels)
    ids = np.asarray(sorted(d), np.int64)
    slot = {int(i): k for k, i in enumerate(ids)}
    flags = R.raster_flags(d, nxt)
    for tile in TILES:
        if tile == (1, 1) and labels.size > 100:
            continue
        dart, nx, lab, other, fl, key = join(R.scene_records(labels, tile))
        assert dart.dtype == np.int64 and np.array_equal(dart, ids), tile
        assert nx.dtype == np.int32 and np.array_equal(nx, [slot[nxt[int(i)]] for i in ids]), tile
        assert lab.dtype == np.int32 and np.array_equal(lab, [d[int(i)][3] for i in ids]), tile
        assert other.dtype == np.int32 and np.array_equal(other, [d[int(i)][4] for i in ids]), tile
        assert fl.dtype == np.uint8 and np.array_equal(fl, [flags[int(i)] for i in ids]), tile
        assert key.dtype == np.int64 and np.array_equal(key, (np.arange(len(ids), dtype=np.int64) << 32) | np.arange(len(ids))), tile
        assert sorted(nx.tolist()) == list(range(len(ids)))        # a permutation: the flag scatter cannot collide


def test_a_successor_outside_the_table_is_a_runtime_error():
    rec = R.scene_records(V.host_cases()["frame_island"][0], (3, 5))
    for bad in (int(rec["id"].max()) + 7, -3):
        broken = {k: v.copy() for k, v in rec.items()}
        broken["succ"][2] = bad
        with pytest.raises(RuntimeError, match="successor is not a dart of the scene"):
            join(broken)


# ---- known answers by hand ------------------------------------------------------------------------------------------------------------
def cycles(dart, nx):
    seen, out = set(), []
    for s in range(len(dart)):
        if s in seen:
            continue
        cyc, j = [], s
        while j not in seen:
            seen.add(j)
            cyc.append(int(dart[j]))
            j = int(nx[j])
        out.append(cyc)
    return out


def test_by_hand_a_region_crossing_one_seam():
    """Two pixels of one label, one tile each (W = 2): pixel 0 has darts 0 top, 2 bottom, 3 left; pixel 1 has 4 top, 5 right, 6
    bottom.  The ring runs east along the top straight over the seam, down the right, west along the bottom straight over the seam
    again, up the left: 0 4 5 6 2 3.  The darts that go straight (4 after 0, 2 after 6) are no vertex darts; nothing breaks."""
    dart, nx, lab, other, fl, _ = join(R.scene_records(np.zeros((1, 2), np.int32), (1, 1)))
    assert dart.tolist() == [0, 2, 3, 4, 5, 6]
    assert cycles(dart, nx) == [[0, 4, 5, 6, 2, 3]]
    assert fl.tolist() == [1, 0, 1, 0, 1, 1] and set(other.tolist()) == {-1} and set(lab.tolist()) == {0}


def test_by_hand_a_region_around_a_four_tile_corner():
    """2 x 2 pixels of one label, one tile each: one ring of eight darts through all four tiles, clockwise from the top left."""
    dart, nx, _, _, fl, _ = join(R.scene_records(np.zeros((2, 2), np.int32), (1, 1)))
    assert cycles(dart, nx) == [[0, 4, 5, 13, 14, 10, 11, 3]]
    assert int((fl & 1).sum()) == 4 and int((fl & 2).sum()) == 0  # four corners


def test_by_hand_diagonal_neighbours_across_a_tile_corner_are_not_joined():
    """[[1, 0], [0, 1]], one tile each: the two pixels of label 1 touch only at the corner where the four tiles meet.  The right
    turn comes first, so every pixel is a ring of its own four darts, each a vertex dart."""
    L = np.array([[1, 0], [0, 1]], np.int32)
    dart, nx, lab, _, fl, _ = join(R.scene_records(L, (1, 1)))
    got = cycles(dart, nx)
    assert got == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15]]
    assert lab.tolist() == [1] * 4 + [0] * 8 + [1] * 4 and bool((fl & 1).all())
    want = V.trace(L, 2)
    assert len(want["ring_label"]) == 4 and want["ring_label"].tolist() == [0, 0, 1, 1]


# ---- limits ---------------------------------------------------------------------------------------------------------------------------------
class Shape:
    """A source of a given shape whose pixels are never read (the limits are checked before the first read)."""

    def __init__(self, *shape):
        self.shape = shape

    def read(self, y0, y1, x0, x1):
        raise AssertionError("read before the limits were checked")


def test_every_limit_is_a_value_error_before_any_device_work():
    from deepmerge_amd import scene
    trace = lambda src, n=1, **kw: scene.trace_labels(src, n, device="cpu", **kw)
    for shape in ((3, 20, 30), (20,), (0, 30), (20, 0)):
        with pytest.raises(ValueError, match="source.shape must be"):
            trace(Shape(*shape))
    for shape in (((1 << 31) - 1, 4), (4, (1 << 31) - 1), (1 << 40, 4)):
        with pytest.raises(ValueError, match="H and W must be below 2\\^31 - 1"):
            trace(Shape(*shape))
    with pytest.raises(ValueError, match="at most 2\\^60 pixels"):
        trace(Shape((1 << 31) - 2, (1 << 31) - 2))
    for n in (0, -1, 1 << 31):
        with pytest.raises(ValueError, match="n_labels must be in"):
            trace(Shape(20, 30), n)
    for tile in (0, -4, (8, 0)):
        with pytest.raises(ValueError, match="tile must be >= 1"):
            trace(Shape(20, 30), tile=tile)
    # every window at most 2^28 pixels: 16382 + 2 = 2^14 on both axes is the largest square core inside a larger scene
    with pytest.raises(ValueError, match="at most 2\\^28 pixels, got 16385 x 16385"):
        trace(Shape(1 << 20, 1 << 20), tile=16383)
    with pytest.raises(ValueError, match="at most 2\\^28 pixels, got 16385 x 16384"):
        trace(Shape(16385, 16384), tile=1 << 20)                   # one tile: no apron, the scene itself is the window
    with pytest.raises(AssertionError, match="read before"):      # a scene within every limit goes on to read
        trace(Shape(1 << 20, 1 << 20), tile=16382)
    # total darts < 2^31, counted as the tiles come in
    scene._check_darts((1 << 31) - 1, 3, 9)
    with pytest.raises(ValueError, match="2\\^31 darts or more .*after tile 3 of 9"):
        scene._check_darts(1 << 31, 3, 9)
    # ids in 0..n_labels-1: the window's tile is named, -1 included, before the tile's kernels run
    L = np.zeros((6, 8), np.int32)
    L[0, 0] = 2
    with pytest.raises(ValueError, match="window of tile 0 .*holds 0..2"):
        trace(L, 2, tile=(3, 4))
    L[0, 0] = -1
    with pytest.raises(ValueError, match="window of tile 0 .*holds -1..0"):
        trace(L, 2, tile=(3, 4))
    with pytest.raises(ValueError, match="source.read.* must return torch.int32"):
        trace(np.zeros((6, 8), np.int64), 1)


def test_the_default_tile_fits_and_a_raster_too_large_for_one_window_is_refused():
    from deepmerge_amd import scene
    H, W, S, tiles = scene._check_trace(Shape(30000, 30000), 5, 4096)
    assert (H, W, S, len(tiles)) == (30000, 30000, 5, 64)
    with pytest.raises(ValueError, match="at most 2\\^28 pixels"):
        scene._check_trace(Shape(30000, 30000), 5, 30000)


def test_cpu_tensors_have_no_fallback():
    from deepmerge_amd import scene
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene.trace_labels(np.zeros((4, 4), np.int32), 1, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene._tile_darts(torch.zeros((4, 4), dtype=torch.int32), (0, 4, 0, 4), (0, 0), 4, 4)


# ---- the library's side, without a GPU ----------------------------------------------------------------------------------------------------
NEW = ("dm_scene_vector_count", "dm_scene_vector_link", "dm_scene_vector_ring_emit", "dm_scene_vector_arc_emit")


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
    # DmSceneVectorTrace is DmVectorTrace with a 64-bit W (and 64-bit dart ids behind the same pointer)
    wide, narrow = built.DmSceneVectorTrace, built.DmVectorTrace
    assert [f[0] for f in wide._fields_] == [f[0] for f in narrow._fields_]
    assert wide.W.offset == narrow.W.offset == 20 * 8 and wide.W.size == 8 and narrow.W.size == 4
    assert ctypes.sizeof(wide) == 184 and wide.D.offset == 168
    struct = re.search(r"typedef struct DmSceneVectorTrace \{(.*?)\}", text, flags=re.S).group(1)
    assert "const int64_t *dart;" in struct and "int64_t W;" in struct


def test_count_and_link_refuse_bad_arguments_before_any_launch(built):
    lib = built.lib()
    p = 4096                                                       # any non-null address: validation never dereferences
    ok = dict(labels=p, H=10, W=12, cy0=1, cy1=9, cx0=1, cx1=11, mask=p, core_mask=2 * p, tile_off=p, n_darts=p)
    cases = [(dict(**{k: None}), b"null pointer") for k in ("labels", "mask", "core_mask", "tile_off", "n_darts")]
    cases += [(dict(core_mask=p), b"mask == core_mask"), (dict(H=0), b"H*W"), (dict(W=-1), b"H*W"), (dict(H=1 << 14, W=(1 << 14) + 1), b"H*W"),
              (dict(cy0=-1), b"the core"), (dict(cy0=2), b"the core"), (dict(cy1=11), b"the core"), (dict(cy1=8), b"the core"),
              (dict(cx0=2), b"the core"), (dict(cx1=13), b"the core"), (dict(cx1=10), b"the core"), (dict(cy0=9, cy1=9), b"the core")]
    for change, msg in cases:
        args = {**ok, **change}
        assert lib.dm_scene_vector_count(*args.values(), None) == -1, change
        assert b"dm_scene_vector_count" in lib.dm_last_error() and msg in lib.dm_last_error(), (change, lib.dm_last_error())
    big = (1 << 31) - 2
    ok = dict(labels=p, mask=p, dart=p, H=10, W=12, D=5, oy=7, ox=9, scene_h=100, scene_w=big, id=p, succ=p, lab=p, other=p, succ_flags=p)
    cases = [(dict(**{k: None}), b"null pointer") for k in ("labels", "mask", "dart", "id", "succ", "lab", "other", "succ_flags")]
    cases += [(dict(D=0), b"bad sizes"), (dict(D=4 * 120 + 1), b"bad sizes"), (dict(H=0), b"bad sizes"), (dict(H=1 << 14, W=(1 << 14) + 1), b"bad sizes"),
              (dict(scene_w=big + 1), b"must lie in a scene"), (dict(scene_h=big + 1), b"must lie in a scene"),
              (dict(scene_h=big, scene_w=big), b"must lie in a scene"), (dict(oy=-1), b"must lie in a scene"),
              (dict(oy=91), b"must lie in a scene"), (dict(ox=big - 11), b"must lie in a scene"), (dict(scene_h=0), b"must lie in a scene")]
    for change, msg in cases:
        args = {**ok, **change}
        assert lib.dm_scene_vector_link(*args.values(), None) == -1, change
        assert b"dm_scene_vector_link" in lib.dm_last_error() and msg in lib.dm_last_error(), (change, lib.dm_last_error())


def test_the_wide_emits_refuse_bad_arguments_before_any_launch(built):
    lib = built.lib()
    p = 4096
    for name, arcs in (("dm_scene_vector_ring_emit", False), ("dm_scene_vector_arc_emit", True)):
        call = getattr(lib, name)

        def trace(**change):
            t = built.DmSceneVectorTrace()
            for f, _ in t._fields_[:20]:
                setattr(t, f, p)
            t.W, t.D, t.R, t.n_arcs = (1 << 31) - 2, 8, 1, 1
            for k, v in change.items():
                setattr(t, k, v)
            return t

        assert call(None, None) == -1 and name.encode() in lib.dm_last_error()
        needed = ["dart", "next", "lab", "other", "flags", "key", "sum", "ring_of_slot", "arc_base", "arc_vstart"]
        needed += ["arc_pos", "arc_ptr", "arc_xy"] if arcs else ["ring_ptr", "xy", "area2", "arc_first", "arc_left", "arc_right", "arc_count"]
        for field in needed:
            assert call(ctypes.byref(trace(**{field: None})), None) == -1, field
            assert name.encode() in lib.dm_last_error() and b"null pointer" in lib.dm_last_error(), field
        for change in (dict(W=0), dict(D=3), dict(R=0), dict(n_arcs=0)):
            assert call(ctypes.byref(trace(**change)), None) == -1, change
            assert b"bad sizes" in lib.dm_last_error(), change
        assert call(ctypes.byref(trace(W=(1 << 31) - 1)), None) == -1
        assert b"W must be below 2^31-1" in lib.dm_last_error()
