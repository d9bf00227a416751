"""CPU: the host side of the label-raster scene path (deepmerge_amd/scene.py: sample_points, label_graph, segment_labels,
mrs_labels; csrc/dm_scene_points.hip) -- every limit and refusal before any device work, the declaration / binding / export of
the new entry points and their validation before any launch, the key in Python integers, the point -> tile assignment."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import points_ref as PR
import scene_labels_ref as R


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib


class Shape:
    """A source of a given shape whose pixels are never read (the limits are checked before the first read)."""

    def __init__(self, *shape):
        self.shape = shape

    def read(self, y0, y1, x0, x1):
        raise AssertionError("read before the limits were checked")


class Fio:
    device = "cpu"


NEW = ("dm_scene_point_init", "dm_scene_point_select", "dm_scene_point_commit")


# ---- limits -----------------------------------------------------------------------------------------------------------------------------
def test_every_limit_is_a_value_error_before_any_device_work():
    from deepmerge_amd import scene
    img, lab = np.zeros((3, 20, 30), np.uint8), np.zeros((20, 30), np.int32)
    calls = {
        "sample_points": lambda labels=lab, n=5, **kw: scene.sample_points(labels, n, device="cpu", **kw),
        "label_graph": lambda labels=lab, n=5, source=img, **kw: scene.label_graph(source, labels, n, device="cpu", **kw),
        "segment_labels": lambda labels=lab, n=5, source=img, **kw: scene.segment_labels(Fio(), source, labels, n, **kw),
        "segment_scene": lambda labels=lab, n=5, source=img, **kw: scene.segment_scene(Fio(), source, labels=labels, n_labels=n, **kw),
        "mrs_labels": lambda labels=lab, n=5, source=img, k=1, **kw: scene.mrs_labels(source, labels, n, 10.0, device="cpu", **kw),
    }
    for name, call in calls.items():
        # H * W > 2^48, through a source with a huge shape: 2^24 x (2^24 + 1)
        big = (1 << 24, (1 << 24) + 1)
        with pytest.raises(ValueError, match="at most 2\\^48 pixels"):
            call(labels=Shape(*big), **({} if name == "sample_points" else {"source": Shape(3, *big)}))
        with pytest.raises(ValueError, match="H, W < 2\\^31"):
            call(labels=Shape(1, 1 << 31), **({} if name == "sample_points" else {"source": Shape(3, 1, 1 << 31)}))
        for n in (0, -3, (1 << 24) + 1):
            with pytest.raises(ValueError, match="n_labels must be in 1..2\\^24"):
                call(n=n)
        if name != "mrs_labels":                                   # (no points there)
            for k in (0, -1, 17):
                with pytest.raises(ValueError, match="k must be in 1..16"):
                    call(k=k)
            for mw in (0, 385):
                with pytest.raises(ValueError, match="max_window must be in 1..384"):
                    call(max_window=mw)
        for tile in (0, (4, 0)):
            with pytest.raises(ValueError, match="tile must be >= 1"):
                call(tile=tile)
        with pytest.raises(ValueError, match="labels.shape must be \\(H, W\\)"):
            call(labels=Shape(3, 20, 30))
        if name != "sample_points":
            for shape in ((20, 31), (21, 30), (30, 20)):
                with pytest.raises(ValueError, match="labels must cover the scene"):
                    call(labels=Shape(*shape))
            with pytest.raises(ValueError, match="source.shape must be"):
                call(source=Shape(20, 30))
        # every window below 2^31 pixels
        with pytest.raises(ValueError, match="fewer than 2\\^31 pixels, got 46384 x 46384"):
            call(labels=Shape(200000, 200000), tile=46000, **({} if name == "sample_points" else {"source": Shape(3, 200000, 200000)}))
        # wrong dtype from .read: refused at the first read, before any copy or launch
        for wrong in (lab.astype(np.int64), lab.astype(np.float32)):
            with pytest.raises(ValueError, match="source.read.* must return torch.int32"):
                call(labels=wrong, tile=8)
        with pytest.raises(AssertionError, match="read before"):   # a scene within every limit goes on to read
            call(labels=Shape(20, 30), tile=8)
    # the 2^48 limit itself is taken: 2^24 x 2^24 goes on to the window check
    with pytest.raises(ValueError, match="fewer than 2\\^31 pixels"):
        scene.sample_points(Shape(1 << 24, 1 << 24), 5, tile=1 << 20, device="cpu")
    # labels together with a segmenter, or with labels_out, or without n_labels; n_labels without labels
    with pytest.raises(ValueError, match="neither a segmenter nor labels_out"):
        scene.segment_scene(Fio(), img, labels=lab, n_labels=5, segmenter=lambda t: (None, 1))
    with pytest.raises(ValueError, match="neither a segmenter nor labels_out"):
        scene.segment_scene(Fio(), img, labels=lab, n_labels=5, labels_out=np.zeros((20, 30), np.int32))
    with pytest.raises(ValueError, match="n_labels must be given with labels"):
        scene.segment_scene(Fio(), img, labels=lab)
    with pytest.raises(ValueError, match="n_labels goes with labels"):
        scene.segment_scene(Fio(), img, n_labels=5)
    # mrs_labels checks its own arguments first, as rag.mrs does
    for kw, msg in ((dict(scale=0.0), "scale must be finite"), (dict(scale=1.0, shape=1.0), "shape must be in"),
                    (dict(scale=1.0, band_weights=[1.0]), "band_weights must have 3"), (dict(scale=1.0, max_rounds=-1), "max_rounds must be")):
        with pytest.raises(ValueError, match=msg):
            scene.mrs_labels(Shape(3, 20, 30), Shape(20, 30), 5, device="cpu", **kw)


def test_cpu_tensors_have_no_fallback():
    from deepmerge_amd import scene
    lab = np.zeros((8, 8), np.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene.sample_points(lab, 1, tile=4, device="cpu")


# ---- the library's side, without a GPU ----------------------------------------------------------------------------------------------------
def test_the_new_entry_points_are_declared_bound_and_exported(built):
    text = re.sub(r"/\*.*?\*/", "", open(built.HEADER_PATH).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True).stdout
    for name, n_args in zip(NEW, (5, 20, 9)):
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert decl, name
        args = [" ".join(a.split()) for a in decl.group(1).split(",")]
        assert len(args) == n_args == len(built.SIGNATURES[name][1]), name
        assert args[-1] == "void *stream"
        # pointers bind as pointers, int64_t as 64-bit, int32_t as 32-bit integers
        for a, c in zip(args, built.SIGNATURES[name][1]):
            want = ctypes.c_void_p if "*" in a else ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_int32
            assert ctypes.sizeof(c) == ctypes.sizeof(want) and (c is ctypes.c_void_p) == ("*" in a), (name, a, c)
        assert re.search(r" T %s\b" % name, nm), name
        assert name in built.declared_symbols()
    assert re.search(r"#define\s+DM_SCENE_POINTS_MAX_PIXELS\s+\(1LL << 48\)", text)
    assert built.lib().dm_abi_version() == 7                       # additive
    from deepmerge_amd import scene
    assert scene.MAX_POINT_SCENE == R.MAX_PIXELS == 1 << 48


def test_the_new_entry_points_refuse_bad_arguments_before_any_launch(built):
    lib = built.lib()
    p = 4096                                                       # any non-null address: validation never dereferences
    assert lib.dm_scene_point_init(None, None, None, 4, None) == -1 and b"dm_scene_point_init: null pointer" in lib.dm_last_error()
    for change in (dict(best=None), dict(counts=None), dict(bbox=None), dict(S=0), dict(S=-1)):
        args = {**dict(best=p, counts=p, bbox=p, S=4), **change}
        assert lib.dm_scene_point_init(*args.values(), None) == -1, change
        assert b"dm_scene_point_init" in lib.dm_last_error()
    ok = dict(labels=p, clearance=p, wh=100, ww=120, cy0=10, cy1=90, cx0=8, cx1=100, oy=50, ox=60, scene_h=1000, scene_w=2000, S=7, k=3,
              round=0, points=p, counts=p, best=p, bbox=p)
    cases = [(dict(**{k: None}), b"null pointer") for k in ("labels", "clearance", "points", "counts", "best", "bbox")]
    cases += [(dict(labels=None, clearance=None, points=None, counts=None, best=None, bbox=None), b"null pointer"),
              (dict(wh=0), b"bad sizes"), (dict(ww=-1), b"bad sizes"), (dict(S=0), b"bad sizes"),
              (dict(wh=50000, ww=50000, cy1=50000, cx1=50000, scene_h=1 << 20, scene_w=1 << 20), b"bad sizes"),
              (dict(cy0=-1), b"outside the"), (dict(cy0=90), b"outside the"), (dict(cy1=101), b"outside the"), (dict(cx0=-1), b"outside the"),
              (dict(cx0=100), b"outside the"), (dict(cx1=121), b"outside the"),
              (dict(scene_h=0), b"bad scene"), (dict(scene_w=1 << 31), b"bad scene"), (dict(scene_h=1 << 24, scene_w=(1 << 24) + 1), b"bad scene"),
              (dict(oy=-1), b"leaves the scene"), (dict(oy=901), b"leaves the scene"), (dict(ox=1881), b"leaves the scene"),
              (dict(k=0), b"outside 1..16"), (dict(k=17), b"outside 1..16"), (dict(round=-1), b"outside 0..k-1"), (dict(round=3), b"outside 0..k-1")]
    for change, msg in cases:
        args = {**ok, **change}
        assert lib.dm_scene_point_select(*args.values(), None) == -1, change
        assert b"dm_scene_point_select" in lib.dm_last_error() and msg in lib.dm_last_error(), (change, lib.dm_last_error())
    ok = dict(best=p, scene_h=1000, scene_w=2000, S=7, k=3, points=p, point_clearance=p, counts=p)
    cases = [(dict(**{k: None}), b"null pointer") for k in ("best", "points", "point_clearance", "counts")]
    cases += [(dict(S=0), b"bad sizes"), (dict(scene_w=0), b"bad sizes"), (dict(scene_h=1 << 31), b"bad sizes"),
              (dict(scene_h=1 << 25, scene_w=1 << 24), b"bad sizes"), (dict(k=0), b"outside 1..16"), (dict(k=17), b"outside 1..16")]
    for change, msg in cases:
        args = {**ok, **change}
        assert lib.dm_scene_point_commit(*args.values(), None) == -1, change
        assert b"dm_scene_point_commit" in lib.dm_last_error() and msg in lib.dm_last_error(), (change, lib.dm_last_error())


# ---- the key ----------------------------------------------------------------------------------------------------------------------------
def test_the_key_orders_as_the_rule_does_beyond_32_bit_positions():
    rng = np.random.default_rng(3)
    lins = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) + 12345, (1 << 48) - 2, (1 << 48) - 1]
    lins += [int(v) for v in rng.integers(0, 1 << 48, 40)]
    scores = [1, 2, 3, 96, 191, 192]
    items = [(s, lin, int(rng.integers(s, 193))) for s in scores for lin in lins]       # clearance >= score, as the rule has it
    for s, lin, c in items:
        key = R.pack_key(s, lin, c)
        assert 0 < key < 1 << 64 and R.unpack_key(key) == (s, lin, c)
    # largest score first, then smallest linear index; the clearance never decides (positions are unique)
    by_key = sorted(items, key=lambda it: R.pack_key(*it), reverse=True)
    by_rule = sorted(items, key=lambda it: (-it[0], it[1]))
    assert by_key == by_rule
    assert R.pack_key(3, 1 << 32, 3) < R.pack_key(3, (1 << 32) - 1, 192) < R.pack_key(4, (1 << 48) - 1, 4)
    assert R.pack_key(3, 7, 192) > R.pack_key(3, 8, 3) and R.pack_key(3, 7, 3) > R.pack_key(3, 8, 192)
    # below 2^32 the order is points_ref's own key's order
    small = [(s, lin, s) for s in scores for lin in lins if lin < 1 << 32]
    ref_key = lambda it: (it[0] << 32) | (0xFFFFFFFF - it[1])
    assert sorted(small, key=ref_key) == sorted(small, key=lambda it: R.pack_key(*it))
    # the largest key fits: score 192 at position 0 with clearance 192; a live key is never 0 (score >= 1)
    assert R.pack_key(192, 0, 192) < 1 << 64 and R.pack_key(1, (1 << 48) - 1, 1) > 0


def test_the_rasters_of_the_gpu_tests_are_not_vacuous():
    lab, S = R.raster_a()
    t = R.tiles_per_label(lab, S, R.TILE)
    assert (t >= 2).sum() >= 20 and (t >= 4).sum() >= 1 and (t >= 1).all()
    lab, S = R.raster_b()
    t = R.tiles_per_label(lab, S, R.TILE)
    assert t[R.FRAME] == 9 and t[R.BLOCK] == 4 and t[R.STRIPE] == 3 and t[list(R.CORNERS)].tolist() == [1, 1, 1, 1] and t[R.ABSENT] == 0
    assert len({int(v) for v in R.tile_index(np.array([191, 191, 192, 192]), np.array([223, 224, 223, 224]), R.W, R.TILE)}) == 4
    assert PR.clearance(lab)[95, 105] == 75


# ---- point -> tile ----------------------------------------------------------------------------------------------------------------------
def test_every_point_belongs_to_the_one_tile_whose_core_holds_it():
    import torch
    from deepmerge_amd.scene import point_tiles, tile_grid
    for H, W, tile in ((200, 232, (96, 112)), (9, 17, (4, 8)), (7, 5, 3), (10, 20, 4096), (64, 64, 64), (100, 1, (7, 9))):
        tiles = tile_grid(H, W, tile)
        yy, xx = np.mgrid[0:H, 0:W]
        xy = torch.from_numpy(np.stack((xx.ravel(), yy.ravel()), 1).astype(np.int32))
        got = point_tiles(xy, W, tile).numpy()
        assert got.dtype == np.int64 and got.min() == 0 and got.max() == len(tiles) - 1
        want = np.full((H, W), -1, np.int64)
        for i, (y0, y1, x0, x1) in enumerate(tiles):
            assert (want[y0:y1, x0:x1] == -1).all()                # exact cover: no pixel twice
            want[y0:y1, x0:x1] = i
        assert (want >= 0).all() and np.array_equal(got, want.ravel())
    tiles = tile_grid(200, 232, (96, 112))                         # the slivers
    xy = torch.tensor([[231, 199], [224, 192], [223, 191], [0, 192], [224, 0]], dtype=torch.int32)
    assert point_tiles(xy, 232, (96, 112)).tolist() == [8, 8, 4, 6, 2]
    assert tiles[8] == (192, 200, 224, 232)


# ---- the grid and the seam walk ---------------------------------------------------------------------------------------------------------
def test_the_largest_window_of_a_grid_is_the_largest_of_its_cores_windows():
    """`max_window` looks at two tile rows and two tile columns; the brute force looks at every core, also where the halo is wider
    than a tile and the windows keep growing past the second one."""
    from deepmerge_amd.scene import _Grid, window_of
    for H, W, tile in ((200, 232, (96, 112)), (9, 17, (4, 8)), (7, 9, (3, 4)), (10, 20, 4096), (64, 64, 64), (100, 1, (7, 9)), (1000, 37, (10, 5))):
        grid = _Grid.of(H, W, tile)
        assert (grid.H, grid.W, grid.ny * grid.nx) == (H, W, len(grid.cores)) and (grid.th, grid.tw) == (tile if isinstance(tile, tuple) else (tile, tile))
        for halo in (0, 1, 2, 3, 4, 5, 9, 10, 11, 32, 192):
            windows = [window_of(c, H, W, halo) for c in grid.cores]
            assert grid.max_window(halo) == (max(w[1] - w[0] for w in windows), max(w[3] - w[2] for w in windows)), (H, W, tile, halo)
            for i, (core, w) in enumerate(zip(grid.cores, windows)):
                box, inner, origin = grid.window(i, halo)
                assert box == w and origin == (w[0], w[2])
                assert (inner[0] + w[0], inner[1] + w[0], inner[2] + w[2], inner[3] + w[2]) == core


def test_the_seam_walk_pairs_the_facing_pixels_of_every_seam_once():
    """7 x 9 pixels in tiles of (3, 4): a 3 x 3 grid whose last row and last column are 1 pixel wide.  Two fields, so that the
    walk is also checked to keep the fields apart."""
    import torch
    from deepmerge_amd.scene import _Grid, _border, _seam_pairs
    H, W = 7, 9
    raster = np.random.default_rng(5).permutation(H * W).reshape(H, W).astype(np.int32)       # every pixel its own value
    grid = _Grid.of(H, W, (3, 4))
    assert (grid.ny, grid.nx) == (3, 3) and grid.cores[-1] == (6, 7, 8, 9)
    t = torch.from_numpy(raster)
    strips = [(_border(t[y0:y1, x0:x1]), _border(t[y0:y1, x0:x1] + 100)) for y0, y1, x0, x1 in grid.cores]
    assert strips[0][0][0].data_ptr() != t.data_ptr()             # clones: a strip does not keep its tile's raster alive
    got = _seam_pairs(strips, grid.nx, grid.ny, torch.device("cpu"))
    assert len(got) == 2
    xs, ys = [c[2] for c in grid.cores[1:grid.nx]], [c[0] for c in grid.cores[grid.nx::grid.nx]]
    assert xs == [4, 8] and ys == [3, 6]
    want = [(raster[y, x - 1], raster[y, x]) for x in xs for y in range(H)] + [(raster[y - 1, x], raster[y, x]) for y in ys for x in range(W)]
    for field, (a, b) in enumerate(got):
        assert a.dtype == b.dtype == torch.int32 and len(a) == len(b) == (grid.nx - 1) * H + (grid.ny - 1) * W == 32
        pairs = sorted(zip(a.tolist(), b.tolist()))
        assert pairs == sorted((int(p) + 100 * field, int(q) + 100 * field) for p, q in want), field
    one = _Grid.of(H, W, 4096)
    got = _seam_pairs([(_border(t), _border(t + 100))], one.nx, one.ny, torch.device("cpu"))
    assert len(got) == 2
    for a, b in got:
        assert a.dtype == b.dtype == torch.int32 and a.numel() == b.numel() == 0
